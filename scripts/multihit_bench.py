"""Multi-hit query throughput on the GPU (jt_intersect_multi_device, jt_count_hits_device; the zero-copy path).

    python scripts/multihit_bench.py [--scenes cornellbox bathroom1] [--log2-rays 22] [--warmup 2] [--repeats 9]
                                     [--traversal auto] [--json out.json]

Per scene and ray class (scripts/query_bench.py's generic and outside rays, 2^22 as a device tensor)
the forms below, alternated in one process: every repeat runs each form once, in turn. A form is
timed with a pair of events on the context's own stream around it, after warm-up rounds; reported is
the median over the repeats, the fastest and the slowest.

  bounded        jt_intersect_bounded_device with a +inf bound array        (what k = 1 is set against)
  multi k=1      jt_intersect_multi_device, k = 1: the cost of the list, the steps are the same
  multi k=4, 8   jt_intersect_multi_device
  peel k=4, 8    what a caller has today: k rounds of jt_intersect_device, the origins advanced past each
                 hit in torch (o += d t (1 + 1e-4) on the rays that hit; the others stay where they are)
  occluded       jt_occluded_device                                          (what count is set against)
  count          jt_count_hits_device

One library per process: choose another build with JTRACE_LIB. A run without a GPU fails.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))
sys.path.insert(0, str(ROOT / "scripts"))

from query_bench import make_rays, scene_bounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornellbox", "bathroom1"])
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--traversal", default="auto")
    ap.add_argument("--json", default="")
    ns = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multihit_bench: no GPU: a rate is measured on the device or not at all")
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
            inf = torch.full((n,), float("inf"), dtype=torch.float32, device="cuda:0")

            def peel(k):
                # the torch work runs on the context's stream, between the library's launches
                with torch.cuda.stream(stream):
                    cur, found = rays.clone(), 0
                    for _ in range(k):
                        torch.cuda.current_stream().synchronize()
                        h = st.intersect(cur)
                        hit = h[:, 5] != 0
                        t = h[:, 4].view(torch.float32)
                        step = torch.where(hit, t * (1 + 1e-4), torch.zeros_like(t))
                        cur[:, :3] += cur[:, 3:] * step[:, None]
                        found = found + hit.sum()
                    return int(found)

            forms = [("bounded", lambda: int((st.intersect(rays, tmax=inf)[:, 5] != 0).sum())),
                     ("multi k=1", lambda: int(st.intersect_multi(rays, 1)[1].sum())),
                     ("multi k=4", lambda: int(st.intersect_multi(rays, 4)[1].sum())),
                     ("peel k=4", lambda: peel(4)),
                     ("multi k=8", lambda: int(st.intersect_multi(rays, 8)[1].sum())),
                     ("peel k=8", lambda: peel(8)),
                     ("occluded", lambda: int(st.occluded(rays).sum())),
                     ("count", lambda: int(st.count_hits(rays).sum()))]
            ms = {f: [] for f, _ in forms}
            found = {}
            for rep in range(ns.warmup + ns.repeats):
                for form, call in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    found[form] = call()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= ns.warmup:
                        ms[form].append(e0.elapsed_time(e1))
            for form, _ in forms:
                t = np.sort(ms[form])
                med = float(np.median(t))
                row = {"scene": name, "traversal": st.traversal, "class": cls, "form": form, "rays": n, "found": found[form],
                       "median_ms": med, "min_ms": float(t[0]), "max_ms": float(t[-1]), "mrays_median": n / med / 1e3,
                       "library": lib.jt_version().decode()}
                rows.append(row)
                print(f"{name:11s} {st.traversal:5s} {cls:8s} {form:10s} found {found[form] / n:7.3f} per ray  "
                      f"{med:8.3f} ms median ({t[0]:.3f} .. {t[-1]:.3f})  {row['mrays_median']:9.1f} Mrays/s", flush=True)
            del rays, inf
        st.close()
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
