"""The push plan of the binary node step (csrc/jt_push.h), enumerated on the CPU.

tests/push_check.cpp is a stand-alone program (its own main, nothing loaded into Python): it restates
the branch-and-loop pushes the plan replaces and compares both over every node kind, level, axis,
negmask, leaf count, start and stack size. It is built here with the host compiler under the
address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_push_plan_matches_the_loop_form(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "push_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "push_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
