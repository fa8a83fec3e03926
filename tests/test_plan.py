"""The launch plan's integer rules (csrc/jt_plan.h), enumerated on the CPU.

tests/plan_check.cpp is a stand-alone program (its own main, nothing loaded into Python): the
slot -> pixel map of the combine, chain and error kernels as a bijection over odd sizes and tile
shares, the tile and pixel counts, the stream-count rule against its pinned table, the combine
weights, the devices' sample shares and the one-stream chunk size. It is built here with the host
compiler under the address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_launch_plan_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "plan_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
