"""Uniform against adaptive sampling to the same noise target, on one GPU:

    python3 scripts/adapt_benefit.py [--scene S] [--width W --height H] [--batch 64] [--stop-at 512]

The uniform render traces --stop-at samples in batches, jt_get_noise after each; its noise there is
the target T (so the uniform loop stops at --stop-at by construction). The adaptive render then
runs the CLI's loop with that T: jt_adapt after every check that does not stop it. Prints, per
render, the samples at the stop, paths, rays, summed kernel_ms and the final noise, and for the
adaptive one a line per batch: its device time against the share of tiles still active."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))

from jtrace import abi, sceneio, trace  # noqa: E402
from jtrace.cli import Params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default=str(ROOT / "assets" / "scenes" / "cornellbox" / "cornellbox.json"))
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--stop-at", type=int, default=512, help="samples of the uniform render; its noise is the target")
ap.add_argument("--limit", type=int, default=4096, help="samples at which the adaptive render gives up")
ap.add_argument("--start", type=int, default=64, help="--adaptive-start")
args = ap.parse_args()

lib = abi.load_library()
sa = abi.SceneABI(sceneio.load_scene(args.scene, missing="drop"))  # as bench.py: the checkout lacks a few files
bvh, lights = trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib)


def render(limit, target, adaptive):
    params = abi.make_params(Params(scene="", width=args.width, height=args.height, samples=limit, batch=args.batch), 0)
    st = trace.make_trace_state(sa, bvh, lights, params, lib)
    st.set_counters(0)
    rows, prev = [], st.counters()
    while st.samples < limit:
        st.trace_samples()
        n, cnt, noise = st.samples, st.counters(), st.noise()
        stop = target is not None and noise <= target
        active = st.adapt(target) if adaptive and not stop and n >= args.start and n % st.streams == 0 else None
        rows.append((n, noise, cnt["kernel_ms"] - prev["kernel_ms"], cnt["paths"] - prev["paths"], active))
        prev = cnt
        if stop or active == 0:
            break
    tiles = st.adaptive[1] if st.adaptive else None
    streams = st.streams
    st.close()
    return rows, prev, tiles, streams


def summary(name, rows, cnt):
    print(f"{name}: stop at {rows[-1][0]} samples, paths {cnt['paths']}, rays {cnt['rays']}, "
          f"kernel_ms {cnt['kernel_ms']:.2f}, noise {rows[-1][1]:.5f}")


urows, ucnt, _, streams = render(args.stop_at, None, False)
T = urows[-1][1]
print(f"{Path(args.scene).stem} {args.width}x{args.height}, batch {args.batch}, {streams} streams, target T = {T:.6f} "
      f"(the uniform render's noise at {args.stop_at} samples)")
print("uniform noise per check: " + " ".join(f"{n}:{x:.4f}" for n, x, *_ in urows))
summary("uniform ", urows, ucnt)
arows, acnt, tiles, _ = render(args.limit, T, True)
summary("adaptive", arows, acnt)
print(f"adaptive / uniform: paths {acnt['paths'] / ucnt['paths']:.3f}, rays {acnt['rays'] / ucnt['rays']:.3f}, "
      f"kernel_ms {acnt['kernel_ms'] / ucnt['kernel_ms']:.3f}")
full_ms = urows[-1][2]
full_paths = args.width * args.height * args.batch
print(f"adaptive batches (uniform batch: {full_ms:.2f} ms): samples, noise, ms, ms share, path share, active tiles after")
for n, noise, ms, paths, active in arows:
    print(f"  {n:5d} {noise:.5f} {ms:8.2f} {ms / full_ms:6.3f} {paths / full_paths:6.3f} "
          f"{'' if active is None else f'{active}/{tiles}'}")
