"""Radiance along the caller's own rays from the command line (jt_radiance): the path integrator
on a file of rays, or on a lat-long panorama around the camera, which the scene's pinhole or
orthographic camera cannot make.

    python -m jtrace.radiance --scene assets/scenes/cornellbox/cornellbox.json --rays rays.npy --samples 16 --output out.npy
    python -m jtrace.radiance --scene assets/scenes/cornellbox/cornellbox.json --panorama 512x256 --samples 64 --output pano.png

--rays is a .npy file of shape (n, 6), float32: origin and unit direction per ray; the output is a
.npy file of shape (n, 4), float32: the mean of samples [0, --samples) per ray, rgb and alpha (the
fraction of samples that hit a surface or a visible environment). --panorama WxH traces
panorama_rays of the chosen camera instead and writes an (H, W, 4) .npy, or a .png through the
writer of `python -m jtrace`. Ray i draws from the random stream of pixel i. The sampler flags are
those of `python -m jtrace` (cli.py). One line is printed: rays, samples, milliseconds of the call.
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
from .sceneio import load_scene, save_image
from .trace import make_scene_bvh, make_trace_lights, make_trace_state


def panorama_rays(camera, w: int, h: int) -> np.ndarray:
    """The (h*w, 6) float32 rays of a lat-long panorama seen from `camera` (its frame: 12 floats, the
    columns x, y, z, o), row-major texels. Every origin is the frame's origin. Texel (i, j) looks
    along the lat-long direction of its centre in the camera's frame: azimuth 2 pi ((i + 0.5) / w -
    0.5) about the frame's y from its -z towards its x, polar angle pi (j + 0.5) / h from its +y,
    so the centre of the image looks along the camera's -z, the top row up. Directions are
    computed in float64, normalised, and rounded to float32: unit length to float32 rounding."""
    frame = np.asarray(getattr(camera, "frame", camera), np.float64).reshape(4, 3)
    phi = 2 * np.pi * ((np.arange(w) + 0.5) / w - 0.5)
    theta = np.pi * (np.arange(h) + 0.5) / h
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    local = np.stack([st * np.sin(phi)[None, :], np.broadcast_to(ct, (h, w)), -st * np.cos(phi)[None, :]], -1)
    d = local @ frame[:3]  # x * dx + y * dy + z * dz
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.empty((h, w, 6), np.float32)
    rays[..., :3] = frame[3].astype(np.float32)
    rays[..., 3:] = d.astype(np.float32)
    return rays.reshape(h * w, 6)


def _size(text: str):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected WIDTHxHEIGHT, got {text!r}") from None
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"expected a positive size, got {text!r}")
    return w, h


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="jtrace.radiance", description="radiance along the caller's rays (jt_radiance)")
    p.add_argument("--scene", type=str, required=True, help="scene filename")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--rays", type=str, help=".npy file of rays, (n, 6) float32: origin, unit direction")
    src.add_argument("--panorama", type=_size, metavar="WxH", help="a lat-long panorama of that size around the camera")
    p.add_argument("--samples", type=int, default=16, help="number of samples per ray")
    p.add_argument("--output", type=str, required=True, help=".npy file of the means; with --panorama also .png")
    p.add_argument("--bounces", type=int, default=8, help="number of bounces")
    p.add_argument("--sampler", type=str, default="path", help="sampler type")
    p.add_argument("--clamp", type=int, default=10, help="clamp radiance")
    p.add_argument("--envhidden", type=_bool, default=False, help="hide environment")
    p.add_argument("--nocaustics", type=_bool, default=False, help="disable caustics")
    p.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED, help="RNG seed")
    p.add_argument("--camera", type=str, default="", help="camera name")
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
    ext = os.path.splitext(ns.output)[1].lower()
    if ext != ".npy" and (ns.rays or ext != ".png"):
        raise SystemExit(f"--output {ns.output}: expected .npy" + ("" if ns.rays else " or .png"))
    scene = load_scene(ns.scene, ns.noparallel, missing=ns.missing)
    camera = find_camera(scene, ns.camera)
    if ns.rays:
        rays = np.load(ns.rays)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise SystemExit(f"--rays {ns.rays}: expected shape (n, 6), got {rays.shape}")
        rays = np.ascontiguousarray(rays, np.float32)
    else:
        rays = panorama_rays(scene.cameras[camera], *ns.panorama)
    lib = abi.load_library()
    scene_abi = abi.SceneABI(scene)
    bvh = make_scene_bvh(scene_abi, ns.highqualitybvh, lib)
    lights = make_trace_lights(scene_abi, lib)
    # a context that traces nothing itself: a small image, the integrator's parameters
    sampler = SAMPLER_TYPES.index(ns.sampler) + 1 if ns.sampler in SAMPLER_TYPES else 1
    params = Params(scene=ns.scene, resolution=64, samples=ns.samples, bounces=ns.bounces, sampler=sampler, clamp=ns.clamp,
                    envhidden=ns.envhidden, nocaustics=ns.nocaustics, seed=ns.seed, bvhstacksize=ns.bvhstacksize,
                    device=ns.device, traversal=ns.traversal)
    state = make_trace_state(scene_abi, bvh, lights, abi.make_params(params, camera), lib)
    t0 = time.perf_counter()
    rgba = state.radiance(rays, 0, ns.samples)
    ms = (time.perf_counter() - t0) * 1e3
    traversal = state.traversal
    state.close()
    if ns.panorama:
        w, h = ns.panorama
        rgba = rgba.reshape(h, w, 4)
    if ext == ".png":
        save_image(ns.output, rgba, *ns.panorama)
    else:
        # through a file object: np.save then keeps the name as given (no ".npy" appended)
        with open(ns.output, "wb") as f:
            np.save(f, rgba)
    out(f"{len(rays)} rays, {ns.samples} samples, {ms:.3f} ms (traversal {traversal})")
    return {"rays": len(rays), "samples": ns.samples, "ms": ms}


def main(args=None):
    return run(_parser().parse_args(sys.argv[1:] if args is None else list(args)))


if __name__ == "__main__":
    main()
