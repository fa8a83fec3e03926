"""The choice of a scene's kernel configuration (csrc/jt_select.h), enumerated on the CPU.

tests/select_check.cpp is a stand-alone program (its own main, nothing loaded into Python):
select_kernel against the rules as jt_trace.hip and jt_launch.h spelt them before (the mask, the
dispatch ladder, the LDS / HBM decision, the auto traversal, test_lds_ring, the lane gates and
jt_describe's expressions), field by field over the whole input domain; the properties of the
configuration table; and the pinned rows behind the describe strings the GPU tests assert. It is
built here with the host compiler alone (no ROCm include path: jt_select.h is plain C++) under the
address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_kernel_selection_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "select_check"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "select_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
