"""python -m jtrace.probes end to end on the GPU, as a fresh child process: a 3 x 2 x 3 grid over
cornellbox's bounding box whose `sh` equals TraceState.probe_sh on the file's own positions bit for
bit and whose `radiance_sh` is 4 pi rgb, --points against the method, and the rejections."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT, make_params

pytestmark = pytest.mark.gpu


def _run(args):
    env = dict(os.environ, PYTHONPATH=str(ROOT / "julia-raytracer_amd"))
    return subprocess.run([sys.executable, "-m", "jtrace.probes", *args], capture_output=True, text=True, env=env,
                          cwd=str(ROOT), timeout=300)


def _state(scene, abi, lib, **kw):
    from jtrace import trace
    sa = abi.SceneABI(scene)
    return trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib),
                                  make_params(abi, traversal="near", **kw), lib)


def test_probes_cli_grid_over_the_scene(gpu, abi, lib, cornell, tmp_path):
    from jtrace.probes import grid_points, scene_bounds
    from jtrace.sh import sh_radiance
    out = tmp_path / "probes.npz"
    run = _run(["--scene", CORNELL, "--grid", "3x2x3", "--samples", "4", "--traversal", "near", "--bounces", "5", "--output", str(out)])
    assert run.returncode == 0, run.stderr
    f = np.load(out)
    position, sh, radiance_sh, grid = f["position"], f["sh"], f["radiance_sh"], f["grid"]
    assert position.shape == (18, 3) and position.dtype == np.float32 and sh.shape == (18, 9, 4) and sh.dtype == np.float32
    assert radiance_sh.shape == (18, 9, 3) and radiance_sh.dtype == np.float32 and np.array_equal(grid, [3, 2, 3])
    assert np.array_equal(position, grid_points((3, 2, 3), scene_bounds(cornell)))
    # x fastest: the first three probes differ in x only
    assert (np.diff(position[:3, 0]) > 0).all() and (position[:3, 1:] == position[0, 1:]).all()
    line = run.stdout.strip().splitlines()[-1]
    assert re.match(r"18 probes, 4 samples, [0-9.]+ ms", line), line
    st = _state(cornell, abi, lib, bounces=5)
    want = st.probe_sh(position, 0, 4)
    st.close()
    assert (want[:, 0, 3] > 0).sum() >= 9, "probes inside the box see it"
    assert np.array_equal(sh.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(radiance_sh.view(np.uint32), sh_radiance(sh).view(np.uint32))
    assert np.allclose(radiance_sh, 4 * np.pi * sh[..., :3], rtol=1e-6)
    # --bounds: a box of the caller's
    run = _run(["--scene", CORNELL, "--grid", "2x1x1", "--bounds=-0.5,0.5,-0.5,0.5,1.5,0.5", "--samples", "1", "--output", str(out)])
    assert run.returncode == 0, run.stderr
    assert np.allclose(np.load(out)["position"], [[-0.25, 1.0, 0.0], [0.25, 1.0, 0.0]])


def test_probes_cli_points_saves_what_the_context_returns(gpu, abi, lib, cornell, tmp_path):
    rng = np.random.default_rng(12)
    n = 257
    points = (rng.uniform(-0.9, 0.9, size=(n, 3)) + [0, 1, 0]).astype(np.float32)
    pts_file, out_file = tmp_path / "points.npy", tmp_path / "out.npz"
    np.save(pts_file, points)
    st = _state(cornell, abi, lib, bounces=5)
    want = st.probe_sh(points, 0, 3)
    st.close()
    assert (want[:, 0, 3] > 0).sum() > n // 2
    run = _run(["--scene", CORNELL, "--points", str(pts_file), "--traversal", "near", "--samples", "3", "--bounces", "5",
                "--output", str(out_file)])
    assert run.returncode == 0, run.stderr
    f = np.load(out_file)
    assert f["sh"].dtype == np.float32 and f["sh"].shape == (n, 9, 4) and f["grid"].shape == (0,)
    assert np.array_equal(f["position"], points)
    assert np.array_equal(f["sh"].view(np.uint32), want.view(np.uint32))
    line = run.stdout.strip().splitlines()[-1]
    assert re.match(rf"{n} probes, 3 samples, [0-9.]+ ms", line), line


def test_probes_cli_rejections(gpu, tmp_path):
    bad, good, out = tmp_path / "bad.npy", tmp_path / "good.npy", tmp_path / "probes.npz"
    np.save(bad, np.zeros((5, 6), np.float32))
    np.save(good, np.zeros((5, 3), np.float32))
    run = _run(["--scene", CORNELL, "--points", str(bad), "--output", str(out)])
    assert run.returncode != 0 and "expected shape (n, 3)" in run.stderr, (run.returncode, run.stderr)
    run = _run(["--scene", CORNELL, "--points", str(good), "--grid", "2x2x2", "--output", str(out)])
    assert run.returncode != 0 and "not both" in run.stderr, (run.returncode, run.stderr)
    run = _run(["--scene", CORNELL, "--grid", "2x0x2", "--output", str(out)])
    assert run.returncode != 0 and "at least 1" in run.stderr, (run.returncode, run.stderr)
    assert not out.exists()
