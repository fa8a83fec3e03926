"""The baked node form of the binary node step (csrc/jt_push.h), enumerated on the CPU.

tests/push_baked_check.cpp is a stand-alone program (its own main, nothing loaded into Python): for
every node kind, level, axis, ray mask, leaf count, start and stack size it compares
push_plan_baked(bake_node(...)) with push_plan(...), the reference definition, field by field, and
checks that start and the count can be read back from the baked words. It is built here with the
host compiler under the address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_baked_plan_matches_push_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "push_baked_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "push_baked_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
