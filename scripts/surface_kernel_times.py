"""Kernel times of one scripts/surface_bench.py run from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o kt -- \\
        python scripts/surface_bench.py --scenes cornellbox --sizes 1280x720 --warmup 5 --repeats 20
    python scripts/surface_kernel_times.py OUT --warmup 5 --repeats 20 [--label "cornellbox 1280x720"]

surface_bench.py's event times include the host's share of a call (the wrapper's stream
synchronise and allocation, the argument checks, the launch, the wait for the stream), which at
30-150 us per call is no small part; the trace has the kernels alone. The run must be of ONE scene
and ONE size: the script tells the calls apart by the order of a kernel's dispatches, which
surface_bench.py fixes: camera_kernel 1 (the rays the run starts from), then warm-up + repeats of
camera_rays, then of gbuffer; query_kernel the same with intersect; surface_kernel warm-up + repeats
of surfaces, of surfaces with every record a miss, of gbuffer. The device-to-device copy is not
read from the trace: the runtime's copy kernel also serves the run's other copies, and its
dispatches cannot be told apart; surface_bench.py enqueues that copy without any host step
between its two events, so its event time is its device time.
Reported per call: the median, fastest and slowest kernel time of the timed repeats in microseconds.
"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np


def column(header, *names):
    low = [h.lower() for h in header]
    for n in names:
        if n in low:
            return low.index(n)
    raise SystemExit(f"kernel trace has none of the columns {names}: {header}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--label", default="")
    ns = ap.parse_args()
    files = sorted(Path(ns.dir).rglob("*kernel_trace.csv"))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {ns.dir}")
    rows = list(csv.reader(open(files[0])))
    header, rows = rows[0], rows[1:]
    kn, t0, t1 = column(header, "kernel_name"), column(header, "start_timestamp"), column(header, "end_timestamp")
    rows.sort(key=lambda r: int(r[t0]))
    per = {}
    for r in rows:
        per.setdefault(r[kn], []).append((int(r[t1]) - int(r[t0])) / 1e3)  # ns -> us

    def of(part):
        hit = [k for k in per if part in k]
        return np.array(per[hit[0]]) if len(hit) == 1 else None

    block = ns.warmup + ns.repeats
    out = []

    def report(call, times, first, what):
        if times is None:
            print(f"{ns.label} {call:14s} no dispatch of {what} in the trace")
            return
        if len(times) < first + block:
            raise SystemExit(f"{what}: {len(times)} dispatches, expected at least {first + block}: another --warmup / --repeats?")
        t = times[first + ns.warmup:first + block]
        out.append((call, float(np.median(t))))
        print(f"{ns.label} {call:14s} {np.median(t):8.2f} us median ({t.min():.2f} .. {t.max():.2f}), {len(t)} dispatches of {what}")

    cam, qry, srf = of("camera_kernel"), of("query_kernel"), of("surface_kernel")
    report("camera_rays", cam, 1, "camera_kernel")
    report("intersect", qry, 1, "query_kernel")
    report("surfaces", srf, 0, "surface_kernel")
    report("surfaces_miss", srf, block, "surface_kernel")
    report("gbuffer.camera", cam, 1 + block, "camera_kernel")
    report("gbuffer.query", qry, 1 + block, "query_kernel")
    report("gbuffer.surface", srf, 2 * block, "surface_kernel")
    d = dict(out)
    if "surfaces" in d and "surfaces_miss" in d:
        print(f"{ns.label} surface_kernel: hits {d['surfaces']:.2f} us, misses {d['surfaces_miss']:.2f} us, "
              f"the gathers' share of the hit kernel {100 * (1 - d['surfaces_miss'] / d['surfaces']):.0f} %")


if __name__ == "__main__":
    sys.exit(main())
