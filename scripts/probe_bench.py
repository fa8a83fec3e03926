"""jt_probe_sh against the composed form it replaces, and beside jt_irradiance (DESIGN.md section 6j,
EXPERIMENTS.md).

    python scripts/probe_bench.py [--scenes cornellbox features2] [--width 1280 --height 720] [--samples 16]
                                  [--repeats 3] [--traversal auto] [--json out.json]

Per scene: the G-buffer of the pixel centres as device tensors; the probes sit at the positions of
the pixels that hit. Three forms of work are timed on them, alternately, `repeats` times each after
one warm-up call each, and the medians reported:

  fused       jt_probe_sh_device of samples [0, samples): one launch
  composed    what a caller had before: per sample jt_sphere_rays_device, jt_radiance_device of that
              one sample, the nine basis values and the float32 running mean of target * Y_k folded
              in torch: 2 x samples launches of the library's
  irradiance  jt_irradiance_device of samples [0, samples) at the same positions with their normals:
              other paths and a 16-byte result, for scale only

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


def torch_basis(torch, d):
    """jtrace.sh.sh_basis on a device tensor (n, 3): every product and difference a float32 kernel
    of its own, in the header's association."""
    from jtrace import sh
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = (float(c) for c in (sh.C0, sh.C1, sh.C2, sh.C3, sh.C4))
    return torch.stack([torch.full_like(x, c0), y * c1, z * c1, x * c1, (x * y) * c2, (y * z) * c2, ((z * z) * 3.0 - 1.0) * c3,
                        (x * z) * c2, (x * x - y * y) * c4], 1)


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
        raise SystemExit("probe_bench: no GPU: a rate is measured on the device or not at all")
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
        positions = s["position"][hit].contiguous()
        points = torch.cat([s["position"][hit], s["normal"][hit]], 1).contiguous()
        n = len(positions)
        work = n * ns.samples

        def fused():
            return st.probe_sh(positions, 0, ns.samples)

        def composed():
            acc = torch.zeros((n, 9, 4), dtype=torch.float32, device=positions.device)
            for c in range(ns.samples):
                rays = st.sphere_rays(positions, c)
                x = st.radiance(rays, c, c + 1)
                v = x[:, None, :] * torch_basis(torch, rays[:, 3:])[:, :, None]
                w = np.float32(1) / np.float32(c + 1)
                acc = acc * float(np.float32(1) - w) + v * float(w)  # two products and a sum, a kernel each: float32, no FMA
            return acc

        def irradiance():
            return st.irradiance(points, 0, ns.samples)

        forms = {"fused": fused, "composed": composed, "irradiance": irradiance}
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
        traversal = st.traversal
        st.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = {"scene": name, "traversal": traversal, "width": ns.width, "height": ns.height, "samples": ns.samples, "points": n,
               "ms": {k: sorted(v) for k, v in ms.items()}, "mrate": {k: work / med[k] / 1e3 for k in forms},
               "composed_over_fused": med["composed"] / med["fused"], "fused_over_irradiance": med["fused"] / med["irradiance"],
               "fused_equals_composed": same, "mean_coverage": float(first["fused"][:, 0, 3].mean()) / 0.282095,
               "library": lib.jt_version().decode()}
        rows.append(row)
        print(f"{name:11s} {traversal:5s} {n} points x {ns.samples}: jt_probe_sh {row['mrate']['fused']:8.1f} M/s ({med['fused']:.3f} ms), "
              f"composed {row['mrate']['composed']:8.1f} M/s ({med['composed']:.3f} ms, x{row['composed_over_fused']:.3f}), "
              f"jt_irradiance {row['mrate']['irradiance']:8.1f} M/s ({med['irradiance']:.3f} ms, probe_sh takes x{row['fused_over_irradiance']:.3f}); "
              f"fused == composed: {same}", flush=True)
    if ns.json:
        Path(ns.json).parent.mkdir(parents=True, exist_ok=True)
        Path(ns.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
