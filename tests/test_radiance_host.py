"""jt_radiance (include/jtrace.h), the part that needs no GPU: the two exports and their ctypes
prototypes, the argument errors that are reported, in the header's order, before the context is
looked at, the panorama's rays (jtrace/radiance.py panorama_rays), and the integer rules of the
launch (csrc/jt_radiance.h) through the stand-alone program tests/radiance_plan_check.cpp, built
with the host compiler under the address and undefined-behaviour sanitizers."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

import surface_ref as R
from conftest import ROOT

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_radiance", "jt_radiance_device")


def test_the_two_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5 and "#define JT_ABI_VERSION 5" in HEADER.read_text()
    # (ctx, n, rays, stream_base, sample_begin, sample_end, rgba), as the header declares them
    assert lib.jt_radiance.argtypes == [C.c_void_p, C.c_int64, abi.f32p, C.c_int64, C.c_int32, C.c_int32, abi.f32p]
    assert lib.jt_radiance_device.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    for name in NAMES:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
        kinds = [re.sub(r"\s+\w+$", "", a.strip()) for a in decl.split(",")]
        assert [k.replace("const ", "") for k in kinds] == [
            "jt_ctx*", "int64_t", "float*" if name == "jt_radiance" else "void*", "int64_t", "int32_t", "int32_t",
            "float*" if name == "jt_radiance" else "void*"], (name, kinds)


def test_argument_errors_in_order_need_no_device(abi, lib):
    """Every JT_ERR_INVALID of the header's list names its argument and is reported before the
    context is looked at: the handle below is no context and is never read. Each call breaks one
    rule and, to show the order, every later rule of the list too. n == 0 with valid arguments is
    JT_OK, and nothing is written."""
    rays = np.zeros((4, 6), np.float32)
    out = np.full((4, 4), 7.0, np.float32)
    rp, op = rays.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)
    fake, dev, odd = C.c_void_p(0x10), C.c_void_p(0x1000), C.c_void_p(0x1004)

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    def host(ctx=fake, n=4, r=rp, base=0, s0=0, s1=1, o=op):
        return err(lib.jt_radiance(ctx, n, r, base, s0, s1, o))

    def device(ctx=fake, n=4, r=dev, base=0, s0=0, s1=1, o=dev):
        return err(lib.jt_radiance_device(ctx, n, r, base, s0, s1, o))

    late = dict(n=-1, base=-1, s0=-1, s1=-1)  # every later rule broken too
    assert "ctx" in host(ctx=None, r=None, o=None, **late) and "ctx" in device(ctx=None, r=None, o=odd, **late)
    assert re.match(r"rays\b", host(r=None, o=None, **late)) and re.match(r"d_rays\b", device(r=None, o=None, **late))
    assert re.match(r"rgba\b", host(o=None, **late)) and re.match(r"d_rgba\b", device(o=None, **late))
    for call, o in ((host, op), (device, odd)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s0=-1, s1=-1, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(n=2**30, base=2**30 + 1, s0=-1, s1=-1, o=o))
        assert re.match(r"sample_begin\b", call(s0=-1, s1=-5, o=o))
        assert re.match(r"sample_end must\b", call(s0=3, s1=3, o=o)) and re.match(r"sample_end must\b", call(s0=3, s1=2, o=o))
        assert "2^24" in call(s0=5, s1=5 + 2**24 + 1, o=o)
    assert re.match(r"d_rgba\b.*aligned", device(o=odd)) and re.match(r"d_rgba\b.*aligned", device(n=0, o=C.c_void_p(0x1008)))
    # the largest arguments that break no rule reach the n == 0 return: JT_OK, no device work
    assert lib.jt_radiance(fake, 0, rp, 2**31, 2**31 - 2, 2**31 - 1, op) == 0
    assert lib.jt_radiance(fake, 0, rp, 0, 0, 2**24, op) == 0
    assert lib.jt_radiance_device(fake, 0, dev, 0, 0, 1, dev) == 0
    assert (out == 7.0).all() and (rays == 0).all()


def test_panorama_rays():
    """Unit directions to float32 rounding; every origin is the camera frame's; the centre texel of
    an odd-sized panorama looks along the camera's -z; the top row looks up the camera's y, the
    columns turn from -z towards +x."""
    from jtrace.radiance import panorama_rays
    sc, _, _ = R.case("cornell")
    cam = sc.cameras[0]
    ax, org = R._frame(cam.frame)
    for w, h in ((33, 17), (32, 16), (1, 1), (5, 2)):
        r = panorama_rays(cam, w, h)
        assert r.shape == (w * h, 6) and r.dtype == np.float32
        assert np.array_equal(r[:, :3], np.tile(org.astype(np.float32), (w * h, 1)))
        norm = np.linalg.norm(r[:, 3:].astype(np.float64), axis=1)
        assert np.abs(norm - 1).max() <= 3 * 2.0 ** -24, (w, h, np.abs(norm - 1).max())
    w, h = 33, 17
    d = panorama_rays(cam, w, h)[:, 3:].astype(np.float64).reshape(h, w, 3)
    z = ax[2] / np.linalg.norm(ax[2])
    assert np.abs(d[h // 2, w // 2] + z).max() <= 2.0 ** -23, d[h // 2, w // 2] + z
    y, x = ax[1] / np.linalg.norm(ax[1]), ax[0] / np.linalg.norm(ax[0])
    assert (d[0] @ y > 0.99).all() and (d[-1] @ y < -0.99).all()
    assert d[h // 2, w // 2 + w // 4] @ x > 0.99 and d[h // 2, w // 2 - w // 4] @ x < -0.99
    # a bare frame works as well as a camera
    assert np.array_equal(panorama_rays(cam.frame, 5, 3), panorama_rays(cam, 5, 3))


def test_radiance_plan_rules(tmp_path):
    """tests/radiance_plan_check.cpp: the step vote, its replay, the LDS slots and the range rules."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "radiance_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "radiance_plan_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
