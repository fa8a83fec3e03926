"""python -m jtrace.query end to end on the GPU, as a fresh child process: the saved closest hits
and any-hit flags of a ray file on cornellbox equal TraceState.intersect / occluded."""
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
    return subprocess.run([sys.executable, "-m", "jtrace.query", *args], capture_output=True, text=True, env=env,
                          cwd=str(ROOT), timeout=300)


def test_query_cli_saves_what_the_context_returns(gpu, abi, lib, cornell_abi, tmp_path):
    from jtrace import trace
    rng = np.random.default_rng(11)
    n = 1031
    o = rng.uniform(-1.5, 1.5, size=(n, 3)) + [0, 1, 0]
    d = rng.normal(size=(n, 3))
    rays = np.concatenate([o, d], 1).astype(np.float32)
    rays[::5, :3] += 50  # far outside: mostly misses
    ray_file, hit_file, occ_file = tmp_path / "rays.npy", tmp_path / "hits.npy", tmp_path / "occ.npy"
    np.save(ray_file, rays)

    st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib), trace.make_trace_lights(cornell_abi, lib),
                                make_params(abi, traversal="near"), lib)
    want, want_occ = st.intersect(rays), st.occluded(rays)
    st.close()
    assert 0 < int(want["hit"].sum()) < n

    common = ["--scene", CORNELL, "--rays", str(ray_file), "--traversal", "near"]
    run = _run(common + ["--output", str(hit_file)])
    assert run.returncode == 0, run.stderr
    got = np.load(hit_file)
    assert got.dtype == abi.HIT_DTYPE and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    line = run.stdout.strip().splitlines()[-1]
    assert re.match(rf"{n} rays, {int(want['hit'].sum())} hits, [0-9.]+ ms", line), line

    run = _run(common + ["--output", str(occ_file), "--any", "true"])
    assert run.returncode == 0, run.stderr
    got = np.load(occ_file)
    assert got.dtype == np.bool_ and np.array_equal(got, want_occ)
    assert run.stdout.strip().splitlines()[-1].startswith(f"{n} rays, {int(want_occ.sum())} hits, ")
