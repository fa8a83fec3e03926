"""sincos_unit and the baked matte sample's square roots (csrc/jt_device.h, csrc/jt_bsdf.h) over their
whole input set, on the CPU.

tests/sincos_unit_check.cpp is a stand-alone program (its own main, nothing loaded into Python): for
every rand1f value u = k * 2^-24 it compares, bit for bit, the floats of the fused evaluation
(restated with fma()) with those of jl_sincos's unfused one, sine and cosine; checks the quadrant
identity rint(phi * invpio2) == (k + 2^21) >> 22; that 1 - z * z with z = sqrtf(u) lies in [2^-23, 1];
and that u is 0 or at least 2^-24. It is built here with the host compiler under the address and
undefined-behaviour sanitizers, without floating-point contraction, and run once.
"""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_fused_sincos_and_root_domains_over_every_rand1f_value(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sincos_unit_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "sincos_unit_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    m = re.search(r"(\d+) inputs, (\d+) bad", run.stdout)
    assert m and int(m.group(1)) == 1 << 24 and int(m.group(2)) == 0, run.stdout


def test_constants_are_dsincos_smalls():
    """sincos_unit restates dsincos_small's constants (jl_sincos keeps its own text, byte for byte): the
    same fourteen literals appear in both functions of csrc/jt_device.h and in the host program."""
    dev = (ROOT / "julia-raytracer_amd" / "csrc" / "jt_device.h").read_text()
    a, b = dev.index("void dsincos_small("), dev.index("void sincos_unit(")
    old, new = dev[a:dev.index("\n}\n", a)], dev[b:dev.index("\n}\n", b)]
    lit = r"-?\d\.\d{20}e[-+]\d\d"
    want = set(re.findall(lit, old)) - {"6.36619772367581382433e-01"}  # invpio2: the quadrant comes from k
    assert len(want) == 14, sorted(want)
    assert set(re.findall(lit, new)) == want
    host = (ROOT / "tests" / "sincos_unit_check.cpp").read_text()
    assert set(re.findall(lit, host)) == want | {"6.36619772367581382433e-01"}
