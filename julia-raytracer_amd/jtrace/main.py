"""Jtrace.main mirror (src/jtrace.jl:31-118): same stage banners, timers and progress lines.

    python -m jtrace --scene assets/scenes/cornellbox/cornellbox.json --samples 256 --output out.png

Scene load, BVH build, lights and PNG write are host work (as in the reference); the
per-sample loop is the HIP library behind jt_trace_samples.
"""
from __future__ import annotations

import math
import sys
import time

import numpy as np

from . import abi
from .cli import Params, parse_cli_args
from .scene import find_camera
from .sceneio import load_scene, save_image
from .trace import make_scene_bvh, make_trace_lights, make_trace_state


def format_seconds(seconds: float) -> str:
    """format_seconds (src/utils.jl:10-32)."""
    hours = math.floor(seconds / 3600)
    minutes = math.floor((seconds - hours * 3600) / 60)
    seconds = seconds - hours * 3600 - minutes * 60
    i_seconds = math.floor(seconds)
    ms = round((seconds - i_seconds) * 1000)
    if hours == 0:
        if minutes == 0:
            return f"{i_seconds:02d}.{ms:03d}"
        return f"{minutes:02d}:{i_seconds:02d}.{ms:03d}"
    return f"{hours:02d}:{minutes:02d}:{i_seconds:02d}.{ms:03d}"


def run(params: Params, out=print) -> dict:
    if params.addsky:
        out("addsky is not yet supported")
        params.addsky = False
    if params.envname != "":
        out("envname is not yet supported")
        params.envname = ""
    render_start = time.perf_counter()
    out(f"loading scene {params.scene}...")
    t0 = time.perf_counter()
    scene = load_scene(params.scene, params.noparallel, missing=params.missing)
    out(f"loaded scene in {format_seconds(time.perf_counter() - t0)}")
    out("finding camera...")
    camera = find_camera(scene, params.camera if isinstance(params.camera, str) else "")
    lib = abi.load_library()
    scene_abi = abi.SceneABI(scene)
    out("building bvh...")
    t0 = time.perf_counter()
    bvh = make_scene_bvh(scene_abi, params.highqualitybvh, lib)
    out(f"built bvh in {format_seconds(time.perf_counter() - t0)}")
    out("making lights...")
    lights = make_trace_lights(scene_abi, lib)
    out("making state...")
    jp = abi.make_params(params, camera)
    devices = int(getattr(params, "devices", 1) or 1)
    state = make_trace_state(scene_abi, bvh, lights, jp, lib, devices=list(range(devices)) if devices > 1 else None)
    out("tracing samples...")
    sampling_start = time.perf_counter()
    # --noise-target: the estimated relative RMS error of the image (jt_get_noise) is checked once
    # max(2, interval) samples are done and every `interval` samples from then on
    noise_target = float(getattr(params, "noise_target", 0.0) or 0.0)
    noise_interval = int(getattr(params, "noise_interval", 16))
    error_output = getattr(params, "error_output", "") or ""
    # --adaptive: a noise check that does not stop the render freezes the tiles that already meet
    # the target (jt_adapt), from --adaptive-start samples on and where every stream holds the same
    # number of samples; the stop stays the image's noise
    adaptive = bool(getattr(params, "adaptive", False))
    adaptive_start = int(getattr(params, "adaptive_start", 64))
    samples_output = getattr(params, "samples_output", "") or ""
    active_tiles = None
    checked = 0
    for _ in range(0, params.samples, params.batch):
        batch_start = time.perf_counter()
        state.trace_samples()
        now = time.perf_counter()
        done = state.samples
        etc = (now - sampling_start) / max(done, 1) * (params.samples - done)
        out(f"sample {done:3d}/{params.samples:3d} in {format_seconds(now - batch_start)} "
            f"ETC: {format_seconds(etc)}")
        if noise_target > 0 and done >= max(2, noise_interval) and done - checked >= noise_interval:
            checked = done
            noise = state.noise()
            out(f"noise {noise:.4f} at {done} samples")
            if noise <= noise_target:
                out(f"noise target reached at {done}/{params.samples} samples")
                break
            if adaptive and done >= adaptive_start and done % state.streams == 0:
                active_tiles = state.adapt(noise_target)
                out(f"adaptive: {active_tiles}/{state.adaptive[1]} tiles active at {done} samples")
                if active_tiles == 0:
                    break
    render_s = time.perf_counter() - sampling_start
    out(f"rendered in {format_seconds(render_s)} ({render_s:.3f}s)")
    samples_traced = state.samples
    # the a-trous filter over the albedo and normal means: jt_denoise, or with --denoise-mode
    # variance jt_denoise_guided, whose colour tolerance is the per-pixel variance
    denoise_mode = getattr(params, "denoise_mode", "plain") or "plain"
    if params.denoise:
        out("denoising...")
        t0 = time.perf_counter()
        image = state.denoise_guided() if denoise_mode == "variance" else state.denoise()
        out(f"denoised in {format_seconds(time.perf_counter() - t0)}")
    out("saving image...")
    if not params.denoise:
        image = state.get_image()
    save_image(params.output, image, state.width, state.height)
    out(f"saved image to {params.output}")
    if error_output:  # the per-pixel standard error of the image: sqrt of the variance of the mean
        error = np.sqrt(state.variance())
        error[..., 3] = 1.0
        save_image(error_output, error, state.width, state.height)
        out(f"saved error image to {error_output}")
    if samples_output:  # the samples behind every pixel: grey = count / max count
        counts = state.sample_counts().astype(np.float32)
        grey = counts / max(float(counts.max()), 1.0)
        save_image(samples_output, np.stack([grey, grey, grey, np.ones_like(grey)], axis=-1), state.width, state.height)
        out(f"saved sample-count image to {samples_output}")
    out(f"total time: {format_seconds(time.perf_counter() - render_start)}")
    counters = state.counters()
    result = {"render_s": render_s, "width": state.width, "height": state.height, "counters": counters,
              "samples_traced": samples_traced, "paths": counters["paths"]}
    if adaptive:  # the traced tiles still active at the last jt_adapt (None: it never ran)
        result["active_tiles"] = active_tiles
    if noise_target > 0 or error_output:
        result["noise"] = state.noise()  # of the image saved (the last check's value when it stopped the loop)
    state.close()
    if params.denoise:
        result["denoised"] = True
        result["denoise_mode"] = denoise_mode
    return result


def main(args=None):
    """Jtrace.main(args::String) (src/jtrace.jl:116)."""
    if args is None:
        args = sys.argv[1:]
    elif isinstance(args, str):
        args = args.split()
    return run(parse_cli_args(args))


if __name__ == "__main__":
    main()
