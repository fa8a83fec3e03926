"""The integer rules of a ray-query launch (csrc/jt_intersect.h), enumerated on the CPU.

tests/query_plan_check.cpp is a stand-alone program (its own main, nothing loaded into Python): the
persistent grid for n rays, the size of its stack overflow area, the refill's claim rule replayed
(every ray handed out exactly once, the counter within its bound) and the growth of the staging
buffers. It is built here with the host compiler under the address and undefined-behaviour
sanitizers and run once, as tests/test_plan.py does for csrc/jt_plan.h.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_query_launch_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "query_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "query_plan_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
