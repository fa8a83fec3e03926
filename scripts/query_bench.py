"""Ray-query throughput on the GPU (jt_intersect_device / jt_occluded_device, the zero-copy path).

    python scripts/query_bench.py [--scenes cornellbox bathroom1] [--log2-rays 22] [--warmup 3] [--repeats 20]
                                  [--traversal auto] [--json out.json]

Per scene and ray class, 2^22 seeded rays as a device tensor:
  generic  origins uniform in 1.5 x the scene's bounds, directions uniform on the sphere
  outside  origins 20 to 1000 scene radii away, aimed into the bounds; every other ray reversed (a miss)
Each call is timed with a pair of events recorded on the context's own stream around it (the
call's counter reset and its kernel; the stream handle is jt_get_device_buffers'), after
warm-up calls, repeated; reported: the median, the fastest and the slowest call in Mrays/s and the
spread (slowest - fastest) / median of the call times. One library per process: choose another
build with JTRACE_LIB (EXPERIMENTS.md, "Ray queries"). A run without a GPU fails.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))


def scene_bounds(scene):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        f = np.asarray(inst.frame, np.float64).reshape(4, 3)
        w = np.asarray(scene.shapes[inst.shape].positions, np.float64) @ f[:3] + f[3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


def sphere(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def make_rays(cls, lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    if cls == "generic":
        o, d = c + rng.uniform(-1, 1, size=(n, 3)) * h * 1.5, sphere(rng, n)
    else:
        r = np.linalg.norm(hi - lo) / 2
        o = c + sphere(rng, n) * r * np.exp(rng.uniform(np.log(20), np.log(1000), size=(n, 1)))
        d = c + rng.uniform(-1, 1, size=(n, 3)) * h - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[1::2] *= -1
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornellbox", "bathroom1"])
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--traversal", default="auto")
    ap.add_argument("--json", default="")
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("query_bench: no GPU: a rate is measured on the device or not at all")
    from jtrace import abi, sceneio, trace
    from jtrace.cli import Params
    lib = abi.load_library()
    n = 1 << ns.log2_rays
    rows = []
    for name in ns.scenes:
        scene = sceneio.load_scene(str(ROOT / "assets" / "scenes" / name / f"{name}.json"), missing="drop")  # as bench.py
        sa = abi.SceneABI(scene)
        params = abi.make_params(Params(scene="", resolution=64, samples=1, traversal=ns.traversal), 0)
        st = trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), params, lib)
        stream = torch.cuda.ExternalStream(st.device_buffers().stream)
        lo, hi = scene_bounds(scene)
        for cls in ("generic", "outside"):
            rays = torch.from_numpy(make_rays(cls, lo, hi, n, seed=22)).to("cuda:0")
            for kind, call in (("intersect", st.intersect), ("occluded", st.occluded)):
                for _ in range(ns.warmup):
                    out = call(rays)
                hits = int((out[:, 5] != 0).sum()) if kind == "intersect" else int(out.sum())
                ms, host_ms = [], []
                for _ in range(ns.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record(stream)
                    call(rays)
                    e1.record(stream)
                    e1.synchronize()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                    ms.append(e0.elapsed_time(e1))
                ms = np.sort(ms)
                med = float(np.median(ms))
                row = {"scene": name, "traversal": st.traversal, "class": cls, "kind": kind, "rays": n, "hits": hits,
                       "median_ms": med, "min_ms": float(ms[0]), "max_ms": float(ms[-1]),
                       "mrays_median": n / med / 1e3, "mrays_best": n / float(ms[0]) / 1e3, "mrays_worst": n / float(ms[-1]) / 1e3,
                       "spread": float((ms[-1] - ms[0]) / med), "host_median_ms": float(np.median(host_ms)),
                       "library": lib.jt_version().decode()}
                rows.append(row)
                print(f"{name:11s} {st.traversal:5s} {cls:8s} {kind:9s} hits {hits / n:6.3f}  "
                      f"{row['mrays_median']:9.1f} Mrays/s median ({row['mrays_worst']:.1f} .. {row['mrays_best']:.1f}), "
                      f"{med:7.3f} ms, spread {100 * row['spread']:.1f} %, host {row['host_median_ms']:.3f} ms", flush=True)
            del rays
        st.close()
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
