"""jt_radiance against the megakernel on the same work (EXPERIMENTS.md).

    python scripts/radiance_bench.py [--scenes cornellbox features2] [--width 1280 --height 720] [--samples 16]
                                     [--repeats 3] [--traversal auto] [--json out.json]

Per scene: the camera rays of sample 0 as a device tensor, then jt_radiance_device of samples
[0, samples) on them, timed with a pair of events recorded on the context's own stream around the
call (its counter reset and its kernel), after one warm-up call. The comparison is the megakernel
in its matching configuration, the general kernel on the HBM scene with its light queries through
the traversal loop (options features=all, lds_scene=0, light_inline=0), batch = samples: a fresh
context traces [0, samples) and reports jt_counters.kernel_ms and paths. Both run the same device
functions from the same memory on the same paths (samples x pixels); what remains is the cost of
jt_radiance's simpler scheduling. The two are timed alternately, `repeats` times each; the medians
are reported as Mpaths/s with their ratio. One library per process: choose another build with
JTRACE_LIB. A run without a GPU fails.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))

MATCHING = {"features": "all", "lds_scene": "0", "light_inline": "0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornellbox", "features2"])
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--traversal", default="auto")
    ap.add_argument("--json", default="")
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("radiance_bench: no GPU: a rate is measured on the device or not at all")
    from jtrace import abi, sceneio, trace
    from jtrace.cli import Params
    lib = abi.load_library()
    rows = []
    for name in ns.scenes:
        scene = sceneio.load_scene(str(ROOT / "assets" / "scenes" / name / f"{name}.json"), missing="drop")  # as bench.py
        sa = abi.SceneABI(scene)
        bvh, lights = trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib)
        params = abi.make_params(Params(scene="", width=ns.width, height=ns.height, samples=ns.samples, batch=ns.samples,
                                        traversal=ns.traversal), 0)

        def matching_context():
            try:
                for k, v in MATCHING.items():
                    abi.set_option(lib, k, v)
                return trace.make_trace_state(sa, bvh, lights, params, lib)
            finally:
                abi.set_option(lib, None, None)

        st = trace.make_trace_state(sa, bvh, lights, params, lib)
        n = st.width * st.height
        paths = n * ns.samples
        stream = torch.cuda.ExternalStream(st.device_buffers().stream)
        rays = st.camera_rays(0, device=True)
        out = st.radiance(rays, 0, ns.samples)  # the warm-up call
        alpha = float(out[:, 3].mean())
        mega = matching_context()  # the megakernel's warm-up
        mega.trace_range(0, ns.samples)
        mega.synchronize()
        describe = mega.describe()
        mega.close()
        rad_ms, mega_ms, mega_paths = [], [], 0
        for _ in range(ns.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            st.radiance(rays, 0, ns.samples)
            e1.record(stream)
            e1.synchronize()
            rad_ms.append(e0.elapsed_time(e1))
            mega = matching_context()
            mega.trace_range(0, ns.samples)
            cnt = mega.counters()
            mega.close()
            mega_ms.append(cnt["kernel_ms"])
            mega_paths = cnt["paths"]
        traversal = st.traversal
        st.close()
        assert mega_paths == paths, (mega_paths, paths)
        r, m = float(np.median(rad_ms)), float(np.median(mega_ms))
        row = {"scene": name, "traversal": traversal, "width": ns.width, "height": ns.height, "samples": ns.samples, "paths": paths,
               "radiance_ms": sorted(rad_ms), "megakernel_ms": sorted(mega_ms), "radiance_mpaths": paths / r / 1e3,
               "megakernel_mpaths": paths / m / 1e3, "ratio": m / r, "mean_alpha": alpha, "megakernel": describe,
               "library": lib.jt_version().decode()}
        rows.append(row)
        print(f"{name:11s} {traversal:5s} {ns.width}x{ns.height}x{ns.samples}: jt_radiance {row['radiance_mpaths']:8.1f} Mpaths/s "
              f"({r:.3f} ms), megakernel (features=all lds_scene=0 light_inline=0) {row['megakernel_mpaths']:8.1f} Mpaths/s "
              f"({m:.3f} ms), ratio {row['ratio']:.3f}", flush=True)
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
