"""Cosine-weighted gathers at the caller's points from the command line (jt_irradiance): the mean
over the hemisphere at a file of points, or a lightmap of one instance, a texel per point.

    python -m jtrace.bake --scene scene.json --points pts.npy --samples 64 --output means.npy
    python -m jtrace.bake --scene scene.json --instance 3 --size 256x256 --samples 64 --output lightmap.npz
    python -m jtrace.bake --scene scene.json --instance 3 --size 256x256 --samples 64 --modulate true --output lightmap.png

--points is a .npy file of shape (n, 6), float32: position and normal per point; the output is a
.npy file of shape (n, 4), float32: the mean of samples [0, --samples) per point. pi * rgb is the
irradiance there, alpha the share of gather rays that met a surface or a visible environment
(include/jtrace.h, jt_irradiance). Point i draws from the random stream of pixel i.

--instance K --size WxH bakes a lightmap of instance K: texel_hits rasterises the texcoords of its
shape on the host, in numpy as scene loading is, jt_eval_hits gives the position and the normal
at every covered texel, and the texels' points go to jt_irradiance in row-major order. The normal
is the shading normal on the side the element normal points to (--side front) or on the other
(--side back). The output is a .npz file with `mean` (h, w, 4), `covered` (h, w) bool, and
`position` and `normal` (h, w, 3), zero at texels no element covers; or a .png whose rgb is the
mean, times the surface's colour with --modulate true (what a matte surface there sends out), and
whose alpha is the coverage. Chart borders are not dilated.

--ao-radius R (a float, or inf) bakes ambient occlusion instead (jt_ambient_occlusion): per point
the share of the --samples hemisphere draws that meet nothing within R, 1 fully open. --points then
writes an (n,) float32 array; the lightmap's .npz holds `visibility` (h, w) in the place of `mean`,
zero at texels no element covers, and the .png is that value as grey, alpha the coverage.

    python -m jtrace.bake --scene scene.json --instance 3 --size 256x256 --samples 64 --ao-radius 0.5 --output ao.png

The sampler, seed and traversal flags are those of `python -m jtrace.radiance`. One line is
printed: points, samples, milliseconds of the call.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import abi
from .cli import DEFAULT_TRAVERSAL, SAMPLER_TYPES, Params, _bool
from .radiance import _size
from .scene import find_camera
from .sceneio import load_scene, save_image
from .trace import make_scene_bvh, make_trace_lights, make_trace_state


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def texel_hits(shape, w: int, h: int):
    """The texels of a w x h lightmap that `shape`'s texcoords cover: (element, u, v) as (h, w)
    arrays, int32 and float32; element is -1 where nothing covers the texel. Texel (i, j) is row j,
    top first, the pixel eval_texture reads for that uv, and its centre is ((i + 0.5) / w,
    (j + 0.5) / h) in the shape's texcoords as loaded, not wrapped. A texel is covered when its
    centre lies in an element's uv triangle, edges included, by float64 edge functions; of several
    elements the lowest index wins. A quad is its two triangles (p1, p2, p4) and (p3, p4, p2), as
    interpolate_quad reads it (src/geometry.jl:278-283): the second triangle's barycentrics
    (u', v') give the element's uv = (1 - u', 1 - v'), and the first triangle wins on the diagonal.
    A triangle of zero uv area covers nothing. (u, v) are the element's own parameters, what a
    jt_hit record carries."""
    tc = np.asarray(shape.texcoords, np.float64)
    if len(tc) == 0:
        raise ValueError("the shape has no texcoords: nothing maps it to a lightmap")
    if len(shape.lines) or len(shape.points):
        raise ValueError("the shape has lines or points: only triangles and quads have a surface to bake")
    tri = len(shape.triangles) != 0
    idx = np.asarray(shape.triangles if tri else shape.quads, np.int64)
    if len(idx) == 0:
        raise ValueError("the shape has no triangles or quads")
    # the halves of an element: the corners (a, b, c) whose weights are (1 - u - v, u, v), and
    # whether the element's uv is (1 - u, 1 - v) of the half's. A half's key orders the claims on a
    # texel: the lowest element first, its first half on the diagonal
    halves = (((0, 1, 2), False),) if tri else (((0, 1, 3), False), ((2, 3, 1), True))
    nh = len(halves)
    A, B, Cc = (np.concatenate([tc[idx[:, cor[k]]] for cor, _ in halves]) for k in range(3))
    key = np.concatenate([np.arange(len(idx), dtype=np.int64) * nh + k for k in range(nh)])
    flip = np.concatenate([np.full(len(idx), f) for _, f in halves])
    area = _cross(B - A, Cc - A)
    lo, hi = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(area) & (area != 0) & np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
    A, B, Cc, key, flip, area, lo, hi = (x[ok] for x in (A, B, Cc, key, flip, area, lo, hi))
    # the texels whose centres can lie in a half's bounding box, one more on every side
    size = np.array([w, h])
    t0 = np.clip(np.floor(np.clip(lo * size, -2.0, size + 2.0) - 0.5).astype(np.int64) - 1, 0, size - 1)
    t1 = np.clip(np.ceil(np.clip(hi * size, -2.0, size + 2.0) - 0.5).astype(np.int64) + 1, 0, size - 1)
    out = (hi[:, 0] * w < 0) | (lo[:, 0] > 1) | (hi[:, 1] * h < 0) | (lo[:, 1] > 1)  # wholly outside the map
    ext = np.where(out[:, None], 0, t1 - t0 + 1)

    claims = []  # (texel, key, u, v) of every (half, texel centre inside it)

    def claim(k, i, j):
        """halves k (indices into the arrays above) against the texels (i, j), elementwise"""
        a, b, c = A[k], B[k], Cc[k]
        p = np.stack([(i + 0.5) / w, (j + 0.5) / h], -1)
        s = np.sign(area[k])
        ea, eb, ec = _cross(c - b, p - b), _cross(a - c, p - c), _cross(b - a, p - a)
        m = (s * ea >= 0) & (s * eb >= 0) & (s * ec >= 0)
        u, v = eb[m] / area[k][m], ec[m] / area[k][m]
        f = flip[k][m]
        claims.append((j[m] * w + i[m], key[k][m], np.where(f, 1 - u, u), np.where(f, 1 - v, v)))

    SMALL = 6  # boxes of up to SMALL x SMALL texels: all halves at once, one offset at a time
    small = (ext <= SMALL).all(1) & (ext > 0).all(1)
    ks = np.flatnonzero(small)
    for dj in range(int(ext[ks, 1].max()) if len(ks) else 0):
        for di in range(int(ext[ks, 0].max()) if len(ks) else 0):
            k = ks[(di < ext[ks, 0]) & (dj < ext[ks, 1])]
            if len(k):
                claim(k, t0[k, 0] + di, t0[k, 1] + dj)
    for k in np.flatnonzero(~small & (ext > 0).all(1)):  # a large half: all its texels at once
        jj, ii = np.mgrid[t0[k, 1]:t1[k, 1] + 1, t0[k, 0]:t1[k, 0] + 1]
        claim(np.full(ii.size, k), ii.reshape(-1), jj.reshape(-1))

    elem = np.full(h * w, -1, np.int32)
    uv = np.zeros((h * w, 2), np.float32)
    if claims:
        texel, ckey, u, v = (np.concatenate(x) for x in zip(*claims))
        best = np.full(h * w, np.iinfo(np.int64).max)
        np.minimum.at(best, texel, ckey)
        win = ckey == best[texel]
        elem[texel[win]] = ckey[win] // nh
        uv[texel[win], 0], uv[texel[win], 1] = u[win], v[win]
    return elem.reshape(h, w), uv[:, 0].reshape(h, w), uv[:, 1].reshape(h, w)


def instance_points(state, instance: int, texels, side: str = "front"):
    """The points of a lightmap of `instance` from texel_hits' (element, u, v) of its shape: (covered
    (h, w) bool, surfaces of the covered texels in row-major order, abi.SURFACE_DTYPE). The shading
    normal faces the side the element normal points to (front) or the other (back): jt_eval_hits
    once for gnormal, once more seen from there."""
    elem, u, v = texels
    covered = elem >= 0
    n = int(covered.sum())
    if n == 0:
        return covered, np.zeros(0, abi.SURFACE_DTYPE)
    hits = np.zeros(n, abi.HIT_DTYPE)
    hits["instance"], hits["element"], hits["u"], hits["v"], hits["hit"] = instance, elem[covered], u[covered], v[covered], 1
    rays = np.zeros((n, 6), np.float32)
    rays[:, 5] = 1.0  # gnormal does not depend on the direction
    gn = state.surfaces(rays, hits)["gnormal"]
    rays[:, 3:] = -gn if side == "front" else gn  # normal faces -d
    return covered, state.surfaces(rays, hits)


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="jtrace.bake", description="cosine-weighted gathers at points or lightmap texels (jt_irradiance)")
    p.add_argument("--scene", type=str, required=True, help="scene filename")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--points", type=str, help=".npy file of points, (n, 6) float32: position, normal")
    src.add_argument("--instance", type=int, help="bake a lightmap of this instance (needs --size)")
    p.add_argument("--size", type=_size, metavar="WxH", help="the lightmap's size")
    p.add_argument("--side", choices=["front", "back"], default="front", help="the side of the surface that gathers")
    p.add_argument("--modulate", type=_bool, default=False, help="multiply the .png's rgb by the surface colour")
    p.add_argument("--samples", type=int, default=16, help="number of samples per point")
    p.add_argument("--ao-radius", type=float, default=None, metavar="R",
                   help="bake ambient occlusion within this distance (a float or inf) instead of irradiance")
    p.add_argument("--output", type=str, required=True, help="--points: .npy of the means; --instance: .npz or .png")
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
    ao = ns.ao_radius is not None
    if ao and not ns.ao_radius > 0:
        raise SystemExit("--ao-radius must be greater than 0 (inf: unbounded)")
    ext = os.path.splitext(ns.output)[1].lower()
    lightmap = ns.points is None
    if lightmap and ns.size is None:
        raise SystemExit("--instance needs --size WxH")
    if ext not in ((".npz", ".png") if lightmap else (".npy",)):
        raise SystemExit(f"--output {ns.output}: expected " + (".npz or .png" if lightmap else ".npy"))
    scene = load_scene(ns.scene, ns.noparallel, missing=ns.missing)
    if lightmap:
        w, h = ns.size
        try:  # what needs no device, before a context is made
            if not 0 <= ns.instance < len(scene.instances):
                raise ValueError(f"the scene has instances 0 .. {len(scene.instances) - 1}")
            texels = texel_hits(scene.shapes[scene.instances[ns.instance].shape], w, h)
        except ValueError as e:
            raise SystemExit(f"--instance {ns.instance}: {e}") from None
    else:
        points = np.load(ns.points)
        if points.ndim != 2 or points.shape[1] != 6:
            raise SystemExit(f"--points {ns.points}: expected shape (n, 6), got {points.shape}")
        points = np.ascontiguousarray(points, np.float32)
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
    if lightmap:
        covered, surf = instance_points(state, ns.instance, texels, ns.side)
        points = np.concatenate([surf["position"], surf["normal"]], 1).astype(np.float32)
    t0 = time.perf_counter()
    if ao:
        rgba = state.ambient_occlusion(points, ns.ao_radius, 0, ns.samples) if len(points) else np.zeros(0, np.float32)
    else:
        rgba = state.irradiance(points, 0, ns.samples) if len(points) else np.zeros((0, 4), np.float32)
    ms = (time.perf_counter() - t0) * 1e3
    traversal = state.traversal
    state.close()
    if not lightmap:
        # through a file object: np.save then keeps the name as given (no ".npy" appended)
        with open(ns.output, "wb") as f:
            np.save(f, rgba)
    else:
        mean = np.zeros((h, w) if ao else (h, w, 4), np.float32)
        mean[covered] = rgba
        if ext == ".npz":
            position, normal = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
            position[covered], normal[covered] = surf["position"], surf["normal"]
            with open(ns.output, "wb") as f:
                np.savez(f, covered=covered, position=position, normal=normal, **{"visibility" if ao else "mean": mean})
        else:
            img = np.repeat(mean[..., None], 4, axis=2) if ao else mean.copy()
            if ns.modulate:
                img[covered, :3] *= surf["color"]
            img[..., 3] = covered
            save_image(ns.output, img, w, h)
    out(f"{len(points)} points, {ns.samples} samples, {ms:.3f} ms (traversal {traversal})")
    return {"points": len(points), "samples": ns.samples, "ms": ms}


def main(args=None):
    return run(_parser().parse_args(sys.argv[1:] if args is None else list(args)))


if __name__ == "__main__":
    main()
