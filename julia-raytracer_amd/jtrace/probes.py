"""Spherical-harmonic radiance probes from the command line (jt_probe_sh): at a file of positions or
on a regular grid over the scene, the incoming radiance over the whole sphere projected onto the
nine real spherical harmonics of bands 0..2.

    python -m jtrace.probes --scene scene.json --grid 8x4x8 --samples 256 --output probes.npz
    python -m jtrace.probes --scene scene.json --points pts.npy --samples 256 --output probes.npz

--points is a .npy of shape (n, 3). --grid NXxNYxNZ places a probe at the centre of every cell of
--bounds x0,y0,z0,x1,y1,z1 (default: the bounding box of the instances' transformed positions), x
fastest, then y, then z (a box whose first number is negative is written --bounds=-1,0,...). The .npz holds `position` (n, 3), `sh` (n, 9, 4) as the call returns it
(include/jtrace.h, jt_probe_sh: the mean of target * Y_k, alpha the coverage flag's projection),
`radiance_sh` (n, 9, 3) = 4 pi rgb, the radiance field's coefficients (jtrace/sh.py turns them into
irradiance about a normal), and `grid` (the three counts, or empty for --points). Probe i draws from
the random stream of pixel i.

The sampler, seed and traversal flags are those of `python -m jtrace.bake`. One line is printed:
probes, samples, milliseconds of the call.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import abi
from .cli import DEFAULT_TRAVERSAL, SAMPLER_TYPES, Params, _bool
from .scene import find_camera
from .sceneio import load_scene
from .sh import sh_radiance
from .trace import make_scene_bvh, make_trace_lights, make_trace_state


def _grid(s: str):
    try:
        nx, ny, nz = (int(x) for x in s.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected NXxNYxNZ, got {s!r}") from None
    if min(nx, ny, nz) < 1:
        raise argparse.ArgumentTypeError(f"every count must be at least 1, got {s!r}")
    return nx, ny, nz


def _bounds(s: str):
    try:
        b = [float(x) for x in s.split(",")]
    except ValueError:
        b = []
    if len(b) != 6:
        raise argparse.ArgumentTypeError(f"expected x0,y0,z0,x1,y1,z1, got {s!r}")
    return np.array(b, np.float64).reshape(2, 3)


def scene_bounds(scene) -> np.ndarray:
    """The bounding box of every instance's positions in world space: (2, 3) float64, min then max.
    A frame is (x, y, z, o): a point p goes to x p.x + y p.y + z p.z + o."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for ins in scene.instances:
        p = np.asarray(scene.shapes[ins.shape].positions, np.float64)
        if len(p) == 0:
            continue
        f = np.asarray(ins.frame, np.float64).reshape(4, 3)
        q = p @ f[:3] + f[3]
        lo, hi = np.minimum(lo, q.min(0)), np.maximum(hi, q.max(0))
    if not np.isfinite(lo).all():
        raise ValueError("the scene has no positions to bound")
    return np.stack([lo, hi])


def grid_points(counts, bounds) -> np.ndarray:
    """The centres of the cells of a counts = (nx, ny, nz) grid over bounds (2, 3): (nx ny nz, 3)
    float32, x fastest, then y, then z. Computed in float64, rounded once."""
    bounds = np.asarray(bounds, np.float64)
    axes = [bounds[0, a] + (np.arange(n) + 0.5) / n * (bounds[1, a] - bounds[0, a]) for a, n in enumerate(counts)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="jtrace.probes", description="spherical-harmonic radiance probes at points or on a grid (jt_probe_sh)")
    p.add_argument("--scene", type=str, required=True, help="scene filename")
    # not an argparse group: the message of the pair given together is ours
    p.add_argument("--points", type=str, help=".npy file of positions, (n, 3) float32")
    p.add_argument("--grid", type=_grid, metavar="NXxNYxNZ", help="probes at the cell centres of a grid, x fastest")
    p.add_argument("--bounds", type=_bounds, metavar="x0,y0,z0,x1,y1,z1", help="the grid's box (default: the scene's bounding box)")
    p.add_argument("--samples", type=int, default=64, help="number of samples per probe")
    p.add_argument("--output", type=str, required=True, help=".npz: position, sh, radiance_sh, grid")
    p.add_argument("--bounces", type=int, default=8, help="number of bounces")
    p.add_argument("--sampler", type=str, default="path", help="sampler type")
    p.add_argument("--clamp", type=int, default=10, help="clamp radiance")
    p.add_argument("--envhidden", type=_bool, default=False, help="hide environment")
    p.add_argument("--nocaustics", type=_bool, default=False, help="disable caustics")
    p.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED, help="RNG seed")
    p.add_argument("--highqualitybvh", type=_bool, default=False, help="enable high quality bvh")
    p.add_argument("--noparallel", type=_bool, default=False, help="disable threading")
    p.add_argument("--bvhstacksize", type=int, default=128, help="max depth of bvh exploration")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--missing", choices=["error", "drop"], default="error", help="missing scene assets: error or drop")
    p.add_argument("--traversal", choices=["reference", "near", "wide", "auto"], default=DEFAULT_TRAVERSAL,
                   help="BVH traversal, as python -m jtrace --traversal")
    return p


def run(ns, out=print) -> dict:
    if ns.samples < 1:
        raise SystemExit("--samples must be at least 1")
    if (ns.points is None) == (ns.grid is None):
        raise SystemExit("give either --points or --grid, not both" if ns.points is not None else "give --points or --grid")
    if ns.bounds is not None and ns.grid is None:
        raise SystemExit("--bounds needs --grid")
    if os.path.splitext(ns.output)[1].lower() != ".npz":
        raise SystemExit(f"--output {ns.output}: expected .npz")
    scene = load_scene(ns.scene, ns.noparallel, missing=ns.missing)
    if ns.grid is None:
        points = np.load(ns.points)
        if points.ndim != 2 or points.shape[1] != 3:
            raise SystemExit(f"--points {ns.points}: expected shape (n, 3), got {points.shape}")
        points = np.ascontiguousarray(points, np.float32)
        grid = np.zeros(0, np.int32)
    else:
        try:
            bounds = ns.bounds if ns.bounds is not None else scene_bounds(scene)
        except ValueError as e:
            raise SystemExit(f"--grid: {e}") from None
        points = grid_points(ns.grid, bounds)
        grid = np.array(ns.grid, np.int32)
    lib = abi.load_library()
    scene_abi = abi.SceneABI(scene)
    bvh = make_scene_bvh(scene_abi, ns.highqualitybvh, lib)
    lights = make_trace_lights(scene_abi, lib)
    # a context that traces nothing itself: a small image, the integrator's parameters
    sampler = SAMPLER_TYPES.index(ns.sampler) + 1 if ns.sampler in SAMPLER_TYPES else 1
    params = Params(scene=ns.scene, resolution=64, samples=ns.samples, bounces=ns.bounces, sampler=sampler, clamp=ns.clamp,
                    envhidden=ns.envhidden, nocaustics=ns.nocaustics, seed=ns.seed, bvhstacksize=ns.bvhstacksize,
                    device=ns.device, traversal=ns.traversal)
    state = make_trace_state(scene_abi, bvh, lights, abi.make_params(params, find_camera(scene, "")), lib)
    t0 = time.perf_counter()
    sh = state.probe_sh(points, 0, ns.samples) if len(points) else np.zeros((0, 9, 4), np.float32)
    ms = (time.perf_counter() - t0) * 1e3
    traversal = state.traversal
    state.close()
    # through a file object: np.savez then keeps the name as given
    with open(ns.output, "wb") as f:
        np.savez(f, position=points, sh=sh, radiance_sh=sh_radiance(sh), grid=grid)
    out(f"{len(points)} probes, {ns.samples} samples, {ms:.3f} ms (traversal {traversal})")
    return {"probes": len(points), "samples": ns.samples, "ms": ms}


def main(args=None):
    return run(_parser().parse_args(sys.argv[1:] if args is None else list(args)))


if __name__ == "__main__":
    main()
