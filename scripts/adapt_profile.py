"""A render that adapts, for a kernel trace, in the manner of scripts/error_profile.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o kt -- python3 scripts/adapt_profile.py

Cornellbox at the headline shape (1280x720, batches of 64: 32 sample streams), jt_get_noise and
jt_adapt after every batch: adapt_kernel runs once per batch beside error_kernel and
combine_kernel<false>, so their average times in the trace's kernel_stats.csv compare."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "julia-raytracer_amd"))

from jtrace import abi, sceneio, trace  # noqa: E402
from jtrace.cli import Params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--batches", type=int, default=4)
ap.add_argument("--target", type=float, default=0.1)
args = ap.parse_args()

lib = abi.load_library()
sa = abi.SceneABI(sceneio.load_scene(str(ROOT / "assets" / "scenes" / "cornellbox" / "cornellbox.json")))
params = abi.make_params(Params(scene="", width=args.width, height=args.height, samples=args.batch * args.batches,
                                batch=args.batch), 0)
st = trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), params, lib)
st.set_counters(0)
print(f"{args.width}x{args.height}, {st.streams} streams, target {args.target}")
for _ in range(args.batches):
    st.trace_samples()
    noise = st.noise()
    active = st.adapt(args.target)
    print(f"{st.samples} samples: noise {noise:.4f}, {active}/{st.adaptive[1]} tiles active")
st.close()
