"""The instance-root rows of the baking kernels (csrc/jt_push.h), enumerated on the CPU.

tests/instance_root_check.cpp is a stand-alone program (its own main, nothing loaded into Python):
for blob offsets of both parities, 1..64 nodes and 1..64 instances it checks that every root row
lies inside the inst_trav array at the node index its stack entry carries, that an entry encodes
and decodes its instance within IDX_MASK, and that a TLAS leaf baked over the rows pushes push_plan's
entries with every instance index offset by iroot0. It is built here with the host compiler under
the address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_instance_root_rows_and_entries(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "instance_root_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "instance_root_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
