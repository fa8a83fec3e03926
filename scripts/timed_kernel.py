"""Name of the timed trace kernel in a rocprofv3 kernel_stats.csv: the production instance (COUNT,
the 4th template argument, 0; ADAPT, the last, false) with the most total time, in the
six-argument form of jt_describe and the roofline records, as
"trace_kernel_lds<1, 16, false, 0, 0, false>" (roofline.timed_kernel).

usage: python scripts/timed_kernel.py <kt_kernel_stats.csv>
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from roofline import timed_kernel  # noqa: E402

print(timed_kernel(sys.argv[1])[0])
