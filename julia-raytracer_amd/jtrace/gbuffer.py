"""A scene's G-buffer from the command line: per pixel the camera ray, its closest hit and the
surface there (jt_gbuffer).

    python -m jtrace.gbuffer --scene assets/scenes/cornellbox/cornellbox.json --output gb.npz --normal-output n.png

The .npz holds `rays` (H, W, 6) float32, `hits` (H, W) with jt_hit's fields (abi.HIT_DTYPE) and
`surfaces` (H, W) with jt_surface's (abi.SURFACE_DTYPE). --sample -1 (the default) sends the rays
through the pixel centres: a deterministic, noise-free buffer; --sample s >= 0 gives the rays the
integrator traces for sample s. The optional PNGs: the shading normal as 0.5 n + 0.5, the albedo
(surfaces.color) through the sRGB writer of `python -m jtrace`, and the depth t scaled to the hit
pixels' [min, max] (nearest white); miss pixels are black and transparent. The scene, camera, BVH
and traversal flags are those of `python -m jtrace.query`; nothing is traced. One line is printed:
pixels, hits, milliseconds of the call.
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
    p = argparse.ArgumentParser(prog="jtrace.gbuffer", description="the surface under every pixel (jt_gbuffer)")
    p.add_argument("--scene", type=str, required=True, help="scene filename")
    p.add_argument("--output", type=str, required=True, help=".npz file of rays, hits and surfaces")
    p.add_argument("--sample", type=int, default=-1, help="-1: pixel centres; s >= 0: the integrator's rays of sample s")
    p.add_argument("--resolution", type=int, default=1280, help="image resolution")
    p.add_argument("--normal-output", type=str, default="", help="PNG of the shading normals, 0.5 n + 0.5")
    p.add_argument("--albedo-output", type=str, default="", help="PNG of the albedo (sRGB)")
    p.add_argument("--depth-output", type=str, default="", help="PNG of the depth, scaled to the hit pixels' range")
    p.add_argument("--camera", type=str, default="", help="camera name")
    p.add_argument("--highqualitybvh", type=_bool, default=False, help="enable high quality bvh")
    p.add_argument("--noparallel", type=_bool, default=False, help="disable threading")
    p.add_argument("--bvhstacksize", type=int, default=128, help="max depth of bvh exploration")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--missing", choices=["error", "drop"], default="error", help="missing scene assets: error or drop")
    p.add_argument("--traversal", choices=["reference", "near", "wide", "auto"], default=DEFAULT_TRAVERSAL,
                   help="BVH traversal of the queries, as python -m jtrace --traversal")
    return p


def guide_images(hits, surfaces) -> dict:
    """The (H, W, 4) float32 images behind the PNGs, linear, alpha 1 on hit pixels and 0 elsewhere:
    `normal` 0.5 n + 0.5 (already display values), `albedo`, `depth`."""
    hit = surfaces["hit"] != 0
    alpha = hit.astype(np.float32)[..., None]
    normal = np.concatenate([(np.float32(0.5) * surfaces["normal"] + np.float32(0.5)) * alpha, alpha], -1)
    albedo = np.concatenate([surfaces["color"] * alpha, alpha], -1)
    t = np.where(hit, hits["t"], 0).astype(np.float32)
    lo, hi = (float(t[hit].min()), float(t[hit].max())) if hit.any() else (0.0, 1.0)
    g = np.where(hit, 1 - (t - lo) / max(hi - lo, 1e-30), 0).astype(np.float32)[..., None]
    depth = np.concatenate([g, g, g, alpha], -1)
    return {"normal": normal, "albedo": albedo, "depth": depth}


def _save_linear(filename, pixels):
    """Display values as they are (no sRGB curve): the normal and depth maps."""
    import os
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    px = np.where(np.isnan(pixels), 0, np.clip(pixels, 0, 1))
    Image.fromarray(np.round(px * 255).astype(np.uint8), "RGBA").save(filename)


def run(ns, out=print) -> dict:
    from .sceneio import save_image
    scene = load_scene(ns.scene, ns.noparallel, missing=ns.missing)
    camera = find_camera(scene, ns.camera)
    lib = abi.load_library()
    scene_abi = abi.SceneABI(scene)
    bvh = make_scene_bvh(scene_abi, ns.highqualitybvh, lib)
    lights = make_trace_lights(scene_abi, lib)
    params = Params(scene=ns.scene, resolution=ns.resolution, samples=1, bvhstacksize=ns.bvhstacksize, device=ns.device,
                    traversal=ns.traversal)
    state = make_trace_state(scene_abi, bvh, lights, abi.make_params(params, camera), lib)
    w, h = state.width, state.height
    t0 = time.perf_counter()
    rays, hits, surfaces = state.gbuffer(ns.sample)
    ms = (time.perf_counter() - t0) * 1e3
    traversal = state.traversal
    state.close()
    rays, hits, surfaces = rays.reshape(h, w, 6), hits.reshape(h, w), surfaces.reshape(h, w)
    with open(ns.output, "wb") as f:
        np.savez(f, rays=rays, hits=hits, surfaces=surfaces)
    img = guide_images(hits, surfaces)
    if ns.normal_output:
        _save_linear(ns.normal_output, img["normal"])
    if ns.albedo_output:
        save_image(ns.albedo_output, img["albedo"], w, h)
    if ns.depth_output:
        _save_linear(ns.depth_output, img["depth"])
    nhits = int((surfaces["hit"] != 0).sum())
    out(f"{w * h} pixels, {nhits} hits, {ms:.3f} ms ({w}x{h}, sample {ns.sample}, traversal {traversal})")
    return {"pixels": w * h, "hits": nhits, "ms": ms}


def main(args=None):
    return run(_parser().parse_args(sys.argv[1:] if args is None else list(args)))


if __name__ == "__main__":
    main()
