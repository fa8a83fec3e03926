"""The bounded queries and ambient occlusion from the command line, end to end on the GPU, each as
a fresh child process: `python -m jtrace.query` with --tmax, with a bound column in the rays file
and with --segments saves what TraceState.intersect / occluded (tmax=...) and visible return, and
`python -m jtrace.bake --ao-radius` on the 16 x 16 lightmap of tests/test_gpu_bake_cli.py saves
TraceState.ambient_occlusion of the file's own positions and normals, zero at uncovered texels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT, make_params

pytestmark = pytest.mark.gpu

FEATURES1 = str(ROOT / "assets" / "scenes" / "features1" / "features1.json")


def _run(module, args):
    env = dict(os.environ, PYTHONPATH=str(ROOT / "julia-raytracer_amd"))
    return subprocess.run([sys.executable, "-m", module, *args], capture_output=True, text=True, env=env, cwd=str(ROOT), timeout=300)


def _state(scene_abi, abi, lib, **kw):
    from jtrace import trace
    return trace.make_trace_state(scene_abi, trace.make_scene_bvh(scene_abi, False, lib), trace.make_trace_lights(scene_abi, lib),
                                  make_params(abi, traversal="near", **kw), lib)


def test_query_cli_bounds_and_segments(gpu, abi, lib, cornell_abi, tmp_path):
    rng = np.random.default_rng(13)
    n = 1031
    o = rng.uniform(-0.9, 0.9, size=(n, 3)) + [0, 1, 0]
    d = rng.normal(size=(n, 3))
    rays = np.concatenate([o, d], 1).astype(np.float32)
    bounds = np.exp(rng.uniform(np.log(0.05), np.log(5.0), n)).astype(np.float32)
    bounds[::7] = np.inf
    seg = np.concatenate([o, rng.uniform(-0.9, 0.9, size=(n, 3)) + [0, 1, 0]], 1).astype(np.float32)
    files = {k: tmp_path / f"{k}.npy" for k in ("rays", "rays7", "seg", "out")}
    np.save(files["rays"], rays)
    np.save(files["rays7"], np.concatenate([rays, bounds[:, None]], 1))
    np.save(files["seg"], seg)

    st = _state(cornell_abi, abi, lib)
    want = {"scalar": st.intersect(rays, tmax=0.5), "scalar_any": st.occluded(rays, tmax=0.5),
            "column": st.intersect(rays, tmax=bounds), "column_any": st.occluded(rays, tmax=bounds), "seg": st.visible(seg)}
    free = st.intersect(rays)
    st.close()
    for key in ("scalar", "column"):
        assert 0 < int(want[key]["hit"].sum()) < int(free["hit"].sum()), key
    assert 0 < int(want["seg"].sum()) < n

    common = ["--scene", CORNELL, "--traversal", "near", "--output", str(files["out"])]
    for key, args in (("scalar", ["--rays", str(files["rays"]), "--tmax", "0.5"]),
                      ("scalar_any", ["--rays", str(files["rays"]), "--tmax", "0.5", "--any", "true"]),
                      ("column", ["--rays", str(files["rays7"])]),
                      ("column_any", ["--rays", str(files["rays7"]), "--any", "true"]),
                      ("seg", ["--segments", str(files["seg"])])):
        run = _run("jtrace.query", common + args)
        assert run.returncode == 0, (key, run.stderr)
        got = np.load(files["out"])
        assert got.dtype == want[key].dtype and np.array_equal(got.view(np.uint8), want[key].view(np.uint8)), key
        line = run.stdout.strip().splitlines()[-1]
        count = int(want[key].sum()) if want[key].dtype == np.bool_ else int(want[key]["hit"].sum())
        assert line.startswith(f"{n} segments, {count} visible, " if key == "seg" else f"{n} rays, {count} hits, "), line
    # a bound given twice, and a segment file with a bound, are turned away before a context is made
    run = _run("jtrace.query", common + ["--rays", str(files["rays7"]), "--tmax", "1"])
    assert run.returncode != 0 and "--tmax" in run.stderr
    run = _run("jtrace.query", common + ["--segments", str(files["seg"]), "--tmax", "1"])
    assert run.returncode != 0 and "--segments" in run.stderr


def test_bake_cli_ambient_occlusion(gpu, abi, lib, tmp_path):
    from jtrace import sceneio
    features1 = sceneio.load_scene(FEATURES1, missing="drop")
    k = next(k for k, ins in enumerate(features1.instances)
             if len(features1.shapes[ins.shape].texcoords) and len(features1.shapes[ins.shape].quads) > 1)
    npz, png, pts_file, out_file = tmp_path / "ao.npz", tmp_path / "ao.png", tmp_path / "points.npy", tmp_path / "out.npy"
    common = ["--scene", FEATURES1, "--missing", "drop", "--samples", "8", "--traversal", "near", "--ao-radius", "0.5"]
    lightmap = [*common, "--instance", str(k), "--size", "16x16"]
    run = _run("jtrace.bake", [*lightmap, "--output", str(npz)])
    assert run.returncode == 0, run.stderr
    f = np.load(npz)
    assert "mean" not in f.files
    vis, covered, position, normal = f["visibility"], f["covered"], f["position"], f["normal"]
    assert vis.shape == (16, 16) and vis.dtype == np.float32 and covered.shape == (16, 16) and covered.dtype == bool
    n = int(covered.sum())
    assert n >= 32, n
    assert run.stdout.strip().splitlines()[-1].startswith(f"{n} points, 8 samples, ")
    points = np.concatenate([position[covered], normal[covered]], 1)
    st = _state(abi.SceneABI(features1), abi, lib)
    want = st.ambient_occlusion(points, 0.5, 0, 8)
    want_inf = st.ambient_occlusion(points[:100], np.inf, 0, 8)
    st.close()
    assert (want > 0).any() and (want < 1).any()
    assert np.array_equal(vis[covered].view(np.uint32), want.view(np.uint32))
    assert (vis[~covered].view(np.uint32) == 0).all()

    run = _run("jtrace.bake", [*lightmap, "--output", str(png)])
    assert run.returncode == 0, run.stderr
    from PIL import Image
    img = np.asarray(Image.open(png))
    assert img.shape == (16, 16, 4) and np.array_equal(img[..., 3] == 255, covered)
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()  # grey

    np.save(pts_file, points[:100])
    run = _run("jtrace.bake", ["--scene", FEATURES1, "--missing", "drop", "--samples", "8", "--traversal", "near", "--ao-radius", "inf",
                               "--points", str(pts_file), "--output", str(out_file)])
    assert run.returncode == 0, run.stderr
    got = np.load(out_file)
    assert got.shape == (100,) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want_inf.view(np.uint32))
    run = _run("jtrace.bake", [*lightmap[:-6], "--ao-radius", "0", "--points", str(pts_file), "--output", str(out_file)])
    assert run.returncode != 0 and "--ao-radius" in run.stderr
