"""The multi-hit queries from the command line, end to end on the GPU, each as a fresh child process:
`python -m jtrace.query --hits K` saves what TraceState.intersect_multi returns for the file's rays
(an .npz with `hits` and `counts`), `--count true` what TraceState.count_hits returns; both honour
--tmax and a bound column, and neither goes with --any, --segments or the other."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT, make_params

pytestmark = pytest.mark.gpu


def _run(args):
    env = dict(os.environ, PYTHONPATH=str(ROOT / "julia-raytracer_amd"))
    return subprocess.run([sys.executable, "-m", "jtrace.query", *args], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)


def test_query_cli_hits_and_count(gpu, abi, lib, cornell_abi, tmp_path):
    from jtrace import trace
    rng = np.random.default_rng(17)
    n = 1031
    o = rng.uniform(-0.9, 0.9, size=(n, 3)) + [0, 1, 0]
    d = rng.normal(size=(n, 3))
    rays = np.concatenate([o, d], 1).astype(np.float32)
    bounds = np.exp(rng.uniform(np.log(0.05), np.log(5.0), n)).astype(np.float32)
    bounds[::7] = np.inf
    files = {k: tmp_path / f"{k}.npy" for k in ("rays", "rays7")}
    np.save(files["rays"], rays)
    np.save(files["rays7"], np.concatenate([rays, bounds[:, None]], 1))
    npz, npy = tmp_path / "out.npz", tmp_path / "out.npy"

    st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib), trace.make_trace_lights(cornell_abi, lib),
                                make_params(abi, traversal="near"), lib)
    want = {"free": st.intersect_multi(rays, 4), "scalar": st.intersect_multi(rays, 4, tmax=0.5), "column": st.intersect_multi(rays, 4, tmax=bounds)}
    count = {"free": st.count_hits(rays), "scalar": st.count_hits(rays, tmax=0.5), "column": st.count_hits(rays, tmax=bounds)}
    st.close()
    assert (want["free"][1] >= 2).sum() > 100 and 0 < count["scalar"].sum() < count["free"].sum() and 0 < count["column"].sum() < count["free"].sum()

    common = ["--scene", CORNELL, "--traversal", "near"]
    for key, args in (("free", ["--rays", str(files["rays"])]), ("scalar", ["--rays", str(files["rays"]), "--tmax", "0.5"]),
                      ("column", ["--rays", str(files["rays7"])])):
        run = _run(common + args + ["--hits", "4", "--output", str(npz)])
        assert run.returncode == 0, (key, run.stderr)
        got = np.load(npz)
        assert sorted(got.files) == ["counts", "hits"]
        assert got["hits"].dtype == abi.HIT_DTYPE and got["hits"].shape == (n, 4) and got["counts"].dtype == np.int32
        assert np.array_equal(got["hits"].view(np.uint8), want[key][0].view(np.uint8)) and np.array_equal(got["counts"], want[key][1]), key
        assert run.stdout.strip().splitlines()[-1].startswith(f"{n} rays, {int(want[key][1].sum())} hits, "), run.stdout
        run = _run(common + args + ["--count", "true", "--output", str(npy)])
        assert run.returncode == 0, (key, run.stderr)
        got = np.load(npy)
        assert got.dtype == np.int32 and got.shape == (n,) and np.array_equal(got, count[key]), key
        assert run.stdout.strip().splitlines()[-1].startswith(f"{n} rays, {int(count[key].sum())} hits, "), run.stdout
    # turned away before a context is made
    for extra, word in ((["--rays", str(files["rays"]), "--hits", "4", "--any", "true"], "--any"),
                        (["--rays", str(files["rays"]), "--hits", "4", "--count", "true"], "--hits"),
                        (["--segments", str(files["rays"]), "--count", "true"], "--segments"),
                        (["--rays", str(files["rays"]), "--hits", "17"], "--hits")):
        run = _run(common + extra + ["--output", str(tmp_path / "never.npy")])
        assert run.returncode != 0 and word in run.stderr, (extra, run.stderr)
    assert not (tmp_path / "never.npy").exists()
