"""The denoiser's host side, without a GPU: the numpy restatement (tests/denoise_ref.py) is a
sound yardstick on the synthetic inputs the GPU test uses, jt_denoise_defaults and the struct
layout match include/jtrace.h, and jt_denoise_image / jt_denoise report every validation error
before any device work."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from conftest import ROOT

HEADER = ROOT / "include" / "jtrace.h"


# ---- the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_and_float64_restatements_agree(shape):
    rgba, alb, nrm = R.synthetic(*shape)
    worst = 0.0
    for p in R.parameter_sets(*shape):
        r64 = R.denoise(rgba, alb, nrm, **p)
        r32 = R.denoise(rgba, alb, nrm, dtype=np.float32, **p)
        assert r32.dtype == np.float32 and np.isfinite(r64).all()
        assert np.array_equal(r64[..., 3], rgba[..., 3])
        worst = max(worst, R.rel_error(r32, r64).max())
    print(f"{shape}: float32 against float64, worst relative difference {worst:.3g}")
    assert worst <= 1e-5


def test_synthetic_inputs_are_what_the_gpu_test_needs():
    rgba, alb, nrm = R.synthetic(45, 70)
    floor = R.DEFAULTS["albedo_floor"]
    below = (alb < floor).all(-1)
    assert below.any() and (alb[below] == 0).any() and not below.all()
    assert len(np.unique(alb.reshape(-1, 3), axis=0)) == 3
    alpha0 = (rgba[..., 3] == 0).mean()
    assert 0.05 < alpha0 < 0.15 and set(np.unique(rgba[..., 3])) == {0.0, 1.0}
    a, b, c = R.synthetic(45, 70)
    assert np.array_equal(a, rgba) and np.array_equal(b, alb) and np.array_equal(c, nrm)


def test_constant_image_comes_back_unchanged():
    H, W = 19, 37
    rgba = np.broadcast_to(np.array([0.4, 0.25, 0.0625, 1.0], np.float32), (H, W, 4)).copy()
    alb = np.broadcast_to(np.array([0.5, 0.25, 0.125], np.float32), (H, W, 3)).copy()
    nrm = np.broadcast_to(np.array([0.0, 0.6, 0.8], np.float32), (H, W, 3)).copy()
    out = R.denoise(rgba, alb, nrm, **R.defaults(4))
    assert R.rel_error(out, rgba).max() <= 1e-12


def test_late_iterations_carry_weight():
    """With sigma_color = 64 the step-16 taps weigh in on the 45x70 input: iteration 5 moves more
    than a tenth of the pixels by more than 1e-3 relative, so a kernel fault there cannot hide."""
    rgba, alb, nrm = R.synthetic(45, 70)
    p = dict(R.defaults(16), sigma_color=R.WIDE_SIGMA_COLOR)
    r5 = R.denoise(rgba, alb, nrm, **dict(p, iterations=5))
    r4 = R.denoise(rgba, alb, nrm, **dict(p, iterations=4))
    moved = (R.rel_error(r5, r4)[..., :3].max(-1) > 1e-3).mean()
    print(f"pixels moved by iteration 5: {moved:.3f}")
    assert moved >= 0.1


# ---- the ABI ----------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [0, 1, 4, 256])
def test_defaults(abi, lib, samples):
    p = abi.jt_denoise_params()
    assert lib.jt_denoise_defaults(samples, C.byref(p)) == 0
    assert p.iterations == 5
    assert p.sigma_color == np.float32(8) / np.sqrt(np.float32(max(samples, 1)))
    assert p.sigma_normal == np.float32(0.3) and p.sigma_albedo == np.float32(0.1)
    assert p.albedo_floor == np.float32(0.01)
    assert lib.jt_denoise_defaults(samples, None) == -1 and b"out" in lib.jt_last_error()


def test_python_defaults_and_restatement_defaults_agree(lib):
    from jtrace import trace
    for samples in (0, 1, 4, 16, 256):
        got = trace.denoise_defaults(samples, lib).as_dict()
        want = R.defaults(samples)
        assert got["iterations"] == want["iterations"]
        for k in ("sigma_color", "sigma_normal", "sigma_albedo", "albedo_floor"):
            assert got[k] == np.float32(want[k]), k


def test_struct_layout_matches_header(abi, tmp_path):
    s = "jt_denoise_params"
    cls = abi.jt_denoise_params
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l)
    assert int(got[s]) == C.sizeof(cls) == 20
    for f, _ in cls._fields_:
        assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, f


def _call(abi, lib, W=4, H=3, null=None, **fields):
    rgba = np.ones((H if H > 0 else 1, W if W > 0 else 1, 4), np.float32)
    alb = np.ones(rgba.shape[:2] + (3,), np.float32)
    nrm = np.ones_like(alb)
    out = np.zeros_like(rgba)
    p = abi.jt_denoise_params()
    assert lib.jt_denoise_defaults(4, C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    args = dict(rgba=rgba.ctypes.data_as(abi.f32p), albedo=alb.ctypes.data_as(abi.f32p),
                normal=nrm.ctypes.data_as(abi.f32p), params=C.byref(p), out_rgba=out.ctypes.data_as(abi.f32p))
    if null:
        args[null] = None
    st = lib.jt_denoise_image(args["rgba"], args["albedo"], args["normal"], W, H, args["params"], 0, args["out_rgba"])
    return st, lib.jt_last_error().decode()


@pytest.mark.parametrize("null", ["rgba", "albedo", "normal", "params", "out_rgba"])
def test_denoise_image_rejects_null_pointers(abi, lib, null):
    st, msg = _call(abi, lib, null=null)
    assert st == -1 and null in msg, (st, msg)


@pytest.mark.parametrize("field,value", [
    ("iterations", 0), ("iterations", 9), ("iterations", -1),
    ("sigma_color", 0.0), ("sigma_color", -1.0), ("sigma_color", float("nan")), ("sigma_color", float("inf")),
    ("sigma_normal", 0.0), ("sigma_normal", float("nan")), ("sigma_normal", float("inf")),
    ("sigma_albedo", -0.1), ("sigma_albedo", float("nan")), ("sigma_albedo", float("inf")),
    ("albedo_floor", 0.0), ("albedo_floor", float("nan")), ("albedo_floor", float("inf")),
])
def test_denoise_image_rejects_bad_parameters(abi, lib, field, value):
    st, msg = _call(abi, lib, **{field: value})
    assert st == -1 and field in msg, (st, msg)


@pytest.mark.parametrize("W,H,name", [(0, 3, "width"), (-2, 3, "width"), (4, 0, "height"), (4, -1, "height"),
                                      (1 << 14, 1 << 13, "width*height"), (2**31 - 1, 2**31 - 1, "width*height")])
def test_denoise_image_rejects_bad_sizes(abi, lib, W, H, name):
    # the arrays are never touched: the size is refused first
    rgba = np.ones(4, np.float32)
    p = abi.jt_denoise_params()
    assert lib.jt_denoise_defaults(4, C.byref(p)) == 0
    ptr = rgba.ctypes.data_as(abi.f32p)
    st = lib.jt_denoise_image(ptr, ptr, ptr, W, H, C.byref(p), 0, ptr)
    msg = lib.jt_last_error().decode()
    assert st == -1 and name in msg, (st, msg)


def test_denoise_rejects_null_context(abi, lib):
    assert lib.jt_denoise(None, None) == -1 and b"ctx" in lib.jt_last_error()
    out = np.zeros(4, np.float32)
    assert lib.jt_get_denoised(None, out.ctypes.data_as(abi.f32p)) == -1


def test_python_wrapper_checks_shapes_and_names(lib):
    from jtrace import trace
    rgba, alb, nrm = R.synthetic(5, 7)
    with pytest.raises(ValueError):
        trace.denoise_image(rgba, alb[:-1], nrm, lib=lib)
    with pytest.raises(TypeError):
        trace.denoise_image(rgba, alb, nrm, lib=lib, sigma_colour=1.0)
    with pytest.raises(abi_error(lib)) as e:
        trace.denoise_image(rgba, alb, nrm, lib=lib, iterations=9)
    assert e.value.status == -1 and "iterations" in str(e.value)


def abi_error(lib):
    from jtrace import abi
    return abi.JTError
