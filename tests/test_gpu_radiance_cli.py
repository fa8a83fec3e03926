"""python -m jtrace.radiance end to end on the GPU, as a fresh child process: the saved means of a ray
file on cornellbox equal TraceState.radiance, and --panorama writes an array of its shape whose
one-sample alpha is 0 or 1."""
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
    return subprocess.run([sys.executable, "-m", "jtrace.radiance", *args], capture_output=True, text=True, env=env,
                          cwd=str(ROOT), timeout=300)


def test_radiance_cli_saves_what_the_context_returns(gpu, abi, lib, cornell_abi, tmp_path):
    from jtrace import trace
    rng = np.random.default_rng(12)
    n = 257
    o = rng.uniform(-0.9, 0.9, size=(n, 3)) + [0, 1, 0]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    rays[::5, :3] += 50  # far outside: mostly misses
    ray_file, out_file = tmp_path / "rays.npy", tmp_path / "out.npy"
    np.save(ray_file, rays)

    st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib), trace.make_trace_lights(cornell_abi, lib),
                                make_params(abi, traversal="near", bounces=5), lib)
    want = st.radiance(rays, 0, 3)
    st.close()
    assert 0 < int((want[:, 3] > 0).sum()) < n

    run = _run(["--scene", CORNELL, "--rays", str(ray_file), "--traversal", "near", "--samples", "3", "--bounces", "5",
                "--output", str(out_file)])
    assert run.returncode == 0, run.stderr
    got = np.load(out_file)
    assert got.dtype == np.float32 and got.shape == (n, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    line = run.stdout.strip().splitlines()[-1]
    assert re.match(rf"{n} rays, 3 samples, [0-9.]+ ms", line), line


def test_radiance_cli_panorama(gpu, tmp_path):
    out_file = tmp_path / "pano.npy"
    run = _run(["--scene", CORNELL, "--panorama", "32x16", "--traversal", "near", "--samples", "1", "--output", str(out_file)])
    assert run.returncode == 0, run.stderr
    got = np.load(out_file)
    assert got.dtype == np.float32 and got.shape == (16, 32, 4)
    assert np.isin(got[..., 3], (0.0, 1.0)).all() and np.isfinite(got).all()
    # the camera stands in front of the open box: the centre looks into it, the far left and right out of it
    assert (got[6:10, 14:18, 3] == 1).all() and (got[..., 3] == 0).any()
