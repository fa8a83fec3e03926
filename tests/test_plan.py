"""The launch plan's integer rules (csrc/jt_plan.h), enumerated on the CPU.

tests/plan_check.cpp is a stand-alone program (its own main, nothing loaded into Python): the
slot -> pixel map of the combine, chain and error kernels as a bijection over odd sizes and tile
shares, the tile and pixel counts, the stream-count rule against its pinned table, the combine
weights, the devices' sample shares, the one-stream chunk size and the chunk schedule of a
one-stream range (which samples, which stream count, which buffer set). It is built here with the
host compiler under the address and undefined-behaviour sanitizers and run once.
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


def test_trace_chunk_option_is_known_and_checked(abi, lib, cornell_abi, options):
    """The tests-only option test_trace_chunk (include/jtrace.h) is a known option, and jt_create
    rejects a value that is no power of two in [1, 64] before it touches a device."""
    import pytest
    from conftest import make_params
    from jtrace import trace
    assert lib.jt_set_option(b"test_trace_chunk", b"4") == 0 and lib.jt_set_option(b"test_trace_chunk", None) == 0
    assert lib.jt_set_option(b"test_trace_chunks", b"4") == -1  # an unknown name still fails
    assert '"test_trace_chunk" "<n>"  (tests only)' in (ROOT / "include" / "jtrace.h").read_text()
    bvh = trace.make_scene_bvh(cornell_abi, False, lib)
    lights = trace.make_trace_lights(cornell_abi, lib)
    params = make_params(abi, width=44, height=36, samples=4, batch=1)
    for bad in ("0", "3", "6", "128", "-4", "x"):
        options("test_trace_chunk", bad)
        with pytest.raises(abi.JTError) as e:
            trace.make_trace_state(cornell_abi, bvh, lights, params, lib)
        assert e.value.status == -1 and "test_trace_chunk" in str(e.value), (bad, str(e.value))
