"""Ray queries from the command line: the closest hit (jt_intersect) or the any-hit flag
(jt_occluded) of a file of rays on a scene.

    python -m jtrace.query --scene assets/scenes/cornellbox/cornellbox.json --rays rays.npy --output hits.npy

--rays is a .npy file of shape (n, 6), float32: origin and direction per ray (the direction need
not be normalised; t is in units of it). The output is a .npy file: a structured array with
jt_hit's fields (instance, element, u, v, t, hit; abi.HIT_DTYPE), or with --any true a bool array.
Bounded queries (jt_intersect_bounded, jt_occluded_bounded): --tmax X ends every ray at t = X, a hit
exactly there included, and a rays file of shape (n, 7) carries a per-ray bound in its last column.
--segments seg.npy, (n, 6) float32 = the two ends of a segment, takes the place of --rays and writes
a bool array: whether nothing lies between the ends (jt_visible).

    python -m jtrace.query --scene scene.json --rays rays.npy --tmax 2.5 --any true --output shadowed.npy
    python -m jtrace.query --scene scene.json --segments links.npy --output visible.npy
All hits along a ray (jt_intersect_multi, jt_count_hits): --hits K writes an .npz file with `hits`, (n, K)
records of jt_hit's fields, the K nearest hits of every ray ordered by (t, instance, element), and
`counts`, (n,) int32; --count true writes an (n,) int32 .npy, the primitives each ray crosses. Both
honour --tmax and an (n, 7) file; neither goes with --any or --segments, nor with the other.

    python -m jtrace.query --scene scene.json --rays rays.npy --hits 4 --output layers.npz
    python -m jtrace.query --scene scene.json --rays rays.npy --count true --output crossings.npy
The scene, camera, BVH and traversal flags are those of `python -m jtrace` (cli.py); nothing is
traced. One line is printed: rays, hits, milliseconds of the query call.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import abi
from .cli import DEFAULT_TRAVERSAL, Params, _bool
from .scene import find_camera
from .sceneio import load_scene
from .trace import make_scene_bvh, make_trace_lights, make_trace_state


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="jtrace.query", description="ray queries on a scene (jt_intersect, jt_occluded)")
    p.add_argument("--scene", type=str, required=True, help="scene filename")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--rays", type=str, help=".npy file of rays, (n, 6) float32: origin, direction; (n, 7): and a bound")
    src.add_argument("--segments", type=str, help=".npy file of segments, (n, 6) float32: the two ends; writes visible flags")
    p.add_argument("--tmax", type=float, default=None, help="one bound for all rays: hits up to t = tmax count")
    p.add_argument("--output", type=str, required=True, help=".npy file of the results")
    p.add_argument("--any", type=_bool, default=False, help="any-hit flags (jt_occluded) instead of closest hits")
    p.add_argument("--hits", type=int, default=None, help="the K nearest hits of every ray (jt_intersect_multi), K = 1 .. 16: an .npz")
    p.add_argument("--count", type=_bool, default=False, help="the number of hits of every ray (jt_count_hits): (n,) int32")
    p.add_argument("--camera", type=str, default="", help="camera name")
    p.add_argument("--highqualitybvh", type=_bool, default=False, help="enable high quality bvh")
    p.add_argument("--noparallel", type=_bool, default=False, help="disable threading")
    p.add_argument("--bvhstacksize", type=int, default=128, help="max depth of bvh exploration")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--missing", choices=["error", "drop"], default="error", help="missing scene assets: error or drop")
    p.add_argument("--traversal", choices=["reference", "near", "wide", "auto"], default=DEFAULT_TRAVERSAL,
                   help="BVH traversal of the queries, as python -m jtrace --traversal")
    return p


def run(ns, out=print) -> dict:
    segments = ns.rays is None
    if ns.hits is not None or ns.count:
        if segments:
            raise SystemExit("--segments takes neither --hits nor --count: it writes visible flags")
        if ns.any:
            raise SystemExit("--any goes with neither --hits nor --count: give one")
        if ns.hits is not None and ns.count:
            raise SystemExit("--hits and --count: give one")
        if ns.hits is not None and not 1 <= ns.hits <= abi.MULTI_MAX_HITS:
            raise SystemExit(f"--hits {ns.hits}: expected 1 .. {abi.MULTI_MAX_HITS}")
    rays = np.load(ns.segments if segments else ns.rays)
    tmax = ns.tmax
    if segments:
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise SystemExit(f"--segments {ns.segments}: expected shape (n, 6), got {rays.shape}")
        if tmax is not None or ns.any:
            raise SystemExit("--segments takes neither --tmax nor --any: a segment is its own bound, the output is visible flags")
    elif rays.ndim != 2 or rays.shape[1] not in (6, 7):
        raise SystemExit(f"--rays {ns.rays}: expected shape (n, 6) or (n, 7), got {rays.shape}")
    elif rays.shape[1] == 7:
        if tmax is not None:
            raise SystemExit("--tmax and a bound column in --rays: give one")
        tmax = np.ascontiguousarray(rays[:, 6], np.float32)
    rays = np.ascontiguousarray(rays[:, :6], np.float32)
    scene = load_scene(ns.scene, ns.noparallel, missing=ns.missing)
    camera = find_camera(scene, ns.camera)
    lib = abi.load_library()
    scene_abi = abi.SceneABI(scene)
    bvh = make_scene_bvh(scene_abi, ns.highqualitybvh, lib)
    lights = make_trace_lights(scene_abi, lib)
    # a context that traces nothing: one sample of a small image
    params = Params(scene=ns.scene, resolution=64, samples=1, bvhstacksize=ns.bvhstacksize, device=ns.device,
                    traversal=ns.traversal)
    state = make_trace_state(scene_abi, bvh, lights, abi.make_params(params, camera), lib)
    t0 = time.perf_counter()
    counts = None
    if segments:
        result = state.visible(rays)
    elif ns.hits is not None:
        result, counts = state.intersect_multi(rays, ns.hits, tmax=tmax)
    elif ns.count:
        result = state.count_hits(rays, tmax=tmax)
    else:
        result = state.occluded(rays, tmax=tmax) if ns.any else state.intersect(rays, tmax=tmax)
    ms = (time.perf_counter() - t0) * 1e3
    traversal = state.traversal
    state.close()
    # through a file object: np.save then keeps the name as given (no ".npy" appended)
    with open(ns.output, "wb") as f:
        if counts is not None:
            np.savez(f, hits=result, counts=counts)
        else:
            np.save(f, result)
    if counts is not None or ns.count:
        total = int((result if counts is None else counts).sum())
        what = f"the {ns.hits} nearest hits" if counts is not None else "hit counts"
        out(f"{len(rays)} rays, {total} hits, {ms:.3f} ms ({what}{'' if tmax is None else ', bounded'}, traversal {traversal})")
        return {"rays": len(rays), "hits": total, "ms": ms}
    if segments:
        visible = int(result.sum())
        out(f"{len(rays)} segments, {visible} visible, {ms:.3f} ms (traversal {traversal})")
        return {"rays": len(rays), "visible": visible, "ms": ms}
    hits = int(result.sum()) if ns.any else int((result["hit"] != 0).sum())
    out(f"{len(rays)} rays, {hits} hits, {ms:.3f} ms ({'any hit' if ns.any else 'closest hit'}{'' if tmax is None else ', bounded'}, "
        f"traversal {traversal})")
    return {"rays": len(rays), "hits": hits, "ms": ms}


def main(args=None):
    return run(_parser().parse_args(sys.argv[1:] if args is None else list(args)))


if __name__ == "__main__":
    main()
