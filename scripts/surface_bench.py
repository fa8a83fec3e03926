"""Device time of the surface calls on the GPU (jt_camera_rays_device, jt_intersect_device,
jt_eval_hits_device, jt_gbuffer_device: the zero-copy path).

    python scripts/surface_bench.py [--scenes cornellbox features1 bathroom1] [--sizes 1280x720 1920x1080]
                                    [--sample 0] [--warmup 5] [--repeats 50] [--traversal auto] [--json out.json]

Per scene and image size, with device tensors: camera_rays, intersect of those rays, surfaces of
those hits, and gbuffer (the three in one call). Each call is timed with a pair of events recorded
on the context's own stream around it, after warm-up calls; reported: the median of the repeats,
the fastest and the slowest, in milliseconds, and for `surfaces` the rate in bytes (48 read + 96
written per record). Beside it, timed the same way in the same session on the same
stream: a device-to-device copy that moves the same 144 n bytes (72 n read, 72 n written), the
floor for a kernel that only streams, and `surfaces` of the same records with every hit flag
cleared (`surfaces_miss`): the kernel's own streaming part, 24 B read and the same 96 B written
per record with no scene gather, which tells loads from stores. A run without a GPU fails.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))


def timed(torch, stream, call, warmup, repeats):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.sort(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornellbox", "features1", "bathroom1"])
    ap.add_argument("--sizes", nargs="+", default=["1280x720", "1920x1080"])
    ap.add_argument("--sample", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--traversal", default="auto")
    ap.add_argument("--json", default="")
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: no GPU: a time is measured on the device or not at all")
    from jtrace import abi, sceneio, trace
    from jtrace.cli import Params
    lib = abi.load_library()
    rows = []
    for name in ns.scenes:
        scene = sceneio.load_scene(str(ROOT / "assets" / "scenes" / name / f"{name}.json"), missing="drop")  # as bench.py
        sa = abi.SceneABI(scene)
        bvh, lights = trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib)
        for size in ns.sizes:
            w, h = (int(x) for x in size.split("x"))
            params = abi.make_params(Params(scene="", width=w, height=h, samples=1, traversal=ns.traversal), 0)
            st = trace.make_trace_state(sa, bvh, lights, params, lib)
            n = st.width * st.height
            stream = torch.cuda.ExternalStream(st.device_buffers().stream)
            rays = st.camera_rays(ns.sample, device=True)
            hits = st.intersect(rays)
            nhits = int((hits[:, 5] != 0).sum())
            misses = hits.clone()
            misses[:, 5] = 0
            src = torch.empty(72 * n, dtype=torch.uint8, device=rays.device)
            dst = torch.empty_like(src)

            def copy():
                with torch.cuda.stream(stream):
                    dst.copy_(src)
            calls = (("camera_rays", lambda: st.camera_rays(ns.sample, device=True)), ("intersect", lambda: st.intersect(rays)),
                     ("surfaces", lambda: st.surfaces(rays, hits)), ("surfaces_miss", lambda: st.surfaces(rays, misses)),
                     ("gbuffer", lambda: st.gbuffer(ns.sample, device=True)), ("copy_144n", copy))
            res = {k: timed(torch, stream, call, ns.warmup, ns.repeats) for k, call in calls}
            for k, r in res.items():
                row = {"scene": name, "size": f"{st.width}x{st.height}", "traversal": st.traversal, "call": k, "pixels": n,
                       "hits": nhits, **r, "library": lib.jt_version().decode()}
                if k in ("surfaces", "copy_144n"):
                    row["gb_per_s"] = 144.0 * n / r["median_ms"] / 1e6
                rows.append(row)
                extra = f", {row['gb_per_s']:7.1f} GB/s of 144 B/record" if "gb_per_s" in row else ""
                print(f"{name:11s} {row['size']:9s} {st.traversal:5s} {k:11s} {r['median_ms']:8.4f} ms median "
                      f"({r['min_ms']:.4f} .. {r['max_ms']:.4f}){extra}", flush=True)
            print(f"{name:11s} {size:9s} hits {nhits / n:.3f}; surfaces / copy = "
                  f"{res['surfaces']['median_ms'] / res['copy_144n']['median_ms']:.2f}", flush=True)
            st.close()
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
