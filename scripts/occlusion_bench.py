"""jt_ambient_occlusion against the composed form it replaces, beside jt_irradiance, and a bounded
any-hit query against the unbounded one (EXPERIMENTS.md).

    python scripts/occlusion_bench.py [--scenes cornellbox features2] [--width 1280 --height 720] [--samples 16]
                                      [--repeats 3] [--traversal auto] [--json out.json]

Per scene: the G-buffer of the pixel centres as device tensors; the points are the position and
normal at the pixels that hit. Per radius (a quarter of the scene's diagonal, and +inf) these forms
are timed on them, alternately, `repeats` times each after one warm-up call each, medians reported:

  fused       jt_ambient_occlusion_device of samples [0, samples): one launch
  composed    what a caller had before: per sample jt_hemisphere_rays_device and
              jt_occluded_bounded_device, the visible count folded in torch and divided once:
              2 x samples launches
  irradiance  jt_irradiance_device of the same points and samples (radius-independent): the only
              route to an occlusion value before, for scale
  bounded     jt_occluded_bounded_device of sample 0's hemisphere rays with the radius as bound
  unbounded   jt_occluded_device of the same rays: a bound can only prune

Every call returns when the context's stream is idle, so a form is timed on the host's clock between
two device synchronisations. The fused and the composed results are compared bit for bit. One
library per process: choose another build with JTRACE_LIB. A run without a GPU fails.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))


def diagonal(scene):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        f = np.asarray(inst.frame, np.float64).reshape(4, 3)
        w = np.asarray(scene.shapes[inst.shape].positions, np.float64) @ f[:3] + f[3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return float(np.linalg.norm(hi - lo))


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
        raise SystemExit("occlusion_bench: no GPU: a rate is measured on the device or not at all")
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
        st = trace.make_trace_state(sa, bvh, lights, params, lib)
        _, _, surf = st.gbuffer(-1, device=True)
        s = trace.split_surfaces(surf)
        hit = s["hit"] != 0
        points = torch.cat([s["position"][hit], s["normal"][hit]], 1).contiguous()
        n = len(points)
        work = n * ns.samples
        rays0 = st.hemisphere_rays(points, 0)
        for radius in (np.float32(0.25 * diagonal(scene)), np.float32(np.inf)):
            bound = torch.full((n,), float(radius), dtype=torch.float32, device=points.device)

            def fused():
                return st.ambient_occlusion(points, radius, 0, ns.samples)

            def composed():
                count = torch.zeros(n, dtype=torch.int32, device=points.device)
                for c in range(ns.samples):
                    count += ~st.occluded(st.hemisphere_rays(points, c), tmax=bound)
                return count.to(torch.float32) / float(ns.samples)  # two exact integers, one float32 division

            forms = {"fused": fused, "composed": composed, "irradiance": lambda: st.irradiance(points, 0, ns.samples),
                     "bounded": lambda: st.occluded(rays0, tmax=bound), "unbounded": lambda: st.occluded(rays0)}
            first = {k: f() for k, f in forms.items()}  # the warm-up calls
            same = bool(torch.equal(first["fused"].view(torch.int32), first["composed"].view(torch.int32)))
            ms = {k: [] for k in forms}
            for _ in range(ns.repeats):
                for k, f in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            row = {"scene": name, "traversal": st.traversal, "width": ns.width, "height": ns.height, "samples": ns.samples, "points": n,
                   "radius": float(radius), "ms": {k: sorted(v) for k, v in ms.items()},
                   "mrays": {k: (n if k in ("bounded", "unbounded") else work) / med[k] / 1e3 for k in forms},
                   "composed_over_fused": med["composed"] / med["fused"], "irradiance_over_fused": med["irradiance"] / med["fused"],
                   "unbounded_over_bounded": med["unbounded"] / med["bounded"], "fused_equals_composed": same,
                   "mean_visibility": float(first["fused"].mean()), "library": lib.jt_version().decode()}
            rows.append(row)
            print(f"{name:11s} {st.traversal:5s} radius {float(radius):8.4f} {n} points x {ns.samples}: jt_ambient_occlusion "
                  f"{row['mrays']['fused']:8.1f} Mrays/s ({med['fused']:.3f} ms), composed {med['composed']:.3f} ms "
                  f"(x{row['composed_over_fused']:.3f}), jt_irradiance {med['irradiance']:.3f} ms (x{row['irradiance_over_fused']:.2f}); "
                  f"occluded of sample 0's rays bounded {med['bounded']:.3f} ms, unbounded {med['unbounded']:.3f} ms; "
                  f"mean visibility {row['mean_visibility']:.4f}; fused == composed: {same}", flush=True)
        st.close()
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
