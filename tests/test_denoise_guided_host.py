"""The variance-guided denoiser's host side, without a GPU: the numpy restatement
(tests/denoise_guided_ref.py) is a sound yardstick on the synthetic inputs the GPU test uses and
removes error from the oracle's cornellbox render, jt_denoise_guided_defaults and the struct
layout match include/jtrace.h, jt_denoise_guided_image / jt_denoise_guided report every validation
error before any device work, and the CLI's --denoise-mode."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R
import error_ref as E
from conftest import ROOT, make_params

HEADER = ROOT / "include" / "jtrace.h"
SHAPE_IDS = [f"{s[0]}x{s[1]}" for s in G.SHAPES]


def _inputs(shape):
    rgba, alb, nrm = G.synthetic(*shape)
    return rgba, G.synthetic_variance(rgba, *shape), alb, nrm


# ---- the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_float32_and_float64_restatements_agree(shape):
    """Measured: at most 1.08e-6 over the shapes and the grid (33x130)."""
    rgba, var, alb, nrm = _inputs(shape)
    worst = 0.0
    for p in G.parameter_sets():
        r64 = G.denoise_guided(rgba, var, alb, nrm, **p)
        r32 = G.denoise_guided(rgba, var, alb, nrm, dtype=np.float32, **p)
        assert r32.dtype == np.float32 and np.isfinite(r64).all()
        assert np.array_equal(r64[..., 3], rgba[..., 3])  # neither filtered nor touched by var.a
        worst = max(worst, G.rel_error(r32, r64).max())
    print(f"{shape}: float32 against float64, worst relative difference {worst:.3g}")
    assert worst <= 1e-5


def test_synthetic_variance_is_what_the_gpu_test_needs():
    rgba, var, _, _ = _inputs((45, 70))
    zero = (var[..., :3] == 0).all(-1)
    assert 0.05 < zero.mean() < 0.15
    assert (var[~zero][:, :3] > 0).any(-1).all() and (var >= 0).all() and np.isfinite(var).all()
    assert (var[..., 3] == 0.25).all()
    assert np.array_equal(var, G.synthetic_variance(rgba, 45, 70))


@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_zero_variance_returns_the_input(shape):
    rgba, _, alb, nrm = _inputs(shape)
    out = G.denoise_guided(rgba, np.zeros_like(rgba), alb, nrm, **G.DEFAULTS)
    worst = G.rel_error(out, rgba).max()
    print(f"{shape}: zero variance, worst relative difference from the input {worst:.3g}")
    assert worst <= 1e-6


def test_late_iterations_carry_weight():
    """On 45x70 iteration 5 (step 16) still moves more than a tenth of the pixels by more than 1e-3
    relative, so a kernel fault there cannot hide. Measured: 0.843 at sigma_variance 2."""
    rgba, var, alb, nrm = _inputs((45, 70))
    r5 = G.denoise_guided(rgba, var, alb, nrm, **dict(G.DEFAULTS, iterations=5))
    r4 = G.denoise_guided(rgba, var, alb, nrm, **dict(G.DEFAULTS, iterations=4))
    moved = (G.rel_error(r5, r4)[..., :3].max(-1) > 1e-3).mean()
    print(f"pixels moved by iteration 5: {moved:.3f}")
    assert moved >= 0.1


@pytest.mark.parametrize("shape", [s for s in G.SHAPES if s != (1, 1)], ids=[i for i in SHAPE_IDS if i != "1x1"])
def test_guided_differs_from_plain(shape):
    rgba, var, alb, nrm = _inputs(shape)
    guided = G.denoise_guided(rgba, var, alb, nrm, **G.DEFAULTS)
    plain = R.denoise(rgba, alb, nrm, **R.defaults(16))
    assert G.rel_error(guided, plain)[..., :3].max() > 1e-3


def test_propagated_variance_shrinks():
    """V_I is the variance of a weighted mean: never above the largest input variance, and well
    below V_0 on average once five iterations have averaged."""
    rgba, var, alb, nrm = _inputs((45, 70))
    m = np.maximum(alb.astype(np.float64), G.DEFAULTS["albedo_floor"])
    V0 = (var[..., :3] / (m * m)).sum(-1)
    _, V5 = G.denoise_guided(rgba, var, alb, nrm, return_variance=True, **G.DEFAULTS)
    assert (V5 >= 0).all() and V5.max() <= V0.max() * (1 + 1e-12)
    assert V5.mean() < 0.5 * V0.mean()


# ---- it denoises: the oracle's cornellbox -----------------------------------------------------
def test_restatement_removes_error_from_the_oracle_render(abi, oracle, cornell_abi):
    """Cornellbox 128x128, 16 spp in k = 16 streams (seed 0x5EED), against the oracle's 1024-spp
    render of seed 7. Measured: guided / plain MSE 0.664, guided / noisy 0.316 (a second seed:
    0.646 and 0.318)."""
    w = h = 128
    k = n = 16
    bvh, lights = oracle.build_bvh(cornell_abi), oracle.make_lights(cornell_abi)
    parts = {}
    img, alb, nrm = oracle.trace(cornell_abi, bvh, lights, make_params(abi, width=w, height=h, samples=n, seed=0x5EED),
                                 w, h, 0, n, streams=k, parts=parts)[:3]
    ref = oracle.trace(cornell_abi, bvh, lights, make_params(abi, width=w, height=h, samples=1024, seed=7), w, h, 0,
                       1024)[0][..., :3].astype(np.float64)
    var = E.variance(parts["img"], n, k, img)
    guided = G.denoise_guided(img, var, alb, nrm, **G.DEFAULTS)
    plain = R.denoise(img, alb, nrm, **R.defaults(n))

    def mse(x):
        return float(np.mean((x[..., :3].astype(np.float64) - ref) ** 2))

    noisy_mse, plain_mse, guided_mse = mse(img), mse(plain), mse(guided)
    print(f"cornellbox 128x128 16 spp: MSE noisy {noisy_mse:.6g}, plain {plain_mse:.6g}, guided {guided_mse:.6g}; "
          f"guided / plain {guided_mse / plain_mse:.3f}, guided / noisy {guided_mse / noisy_mse:.3f}")
    assert guided_mse < 0.8 * plain_mse
    assert guided_mse < 0.4 * noisy_mse


# ---- the ABI ----------------------------------------------------------------------------------
def test_defaults(abi, lib):
    p = abi.jt_denoise_guided_params()
    assert lib.jt_denoise_guided_defaults(C.byref(p)) == 0
    assert p.iterations == G.DEFAULTS["iterations"] == 5
    for f in G.FIELDS[1:]:
        assert getattr(p, f) == np.float32(G.DEFAULTS[f]), f
    assert (p.sigma_variance, p.variance_floor) == (2.0, np.float32(1e-10))
    assert lib.jt_denoise_guided_defaults(None) == -1 and b"out" in lib.jt_last_error()


def test_python_defaults_and_restatement_defaults_agree(abi, lib):
    from jtrace import trace
    got = trace.denoise_guided_defaults(lib).as_dict()
    assert list(got) == list(G.FIELDS)
    assert all(got[f] == np.float32(G.DEFAULTS[f]) for f in G.FIELDS)


def test_struct_layout_matches_header(abi, tmp_path):
    s = "jt_denoise_guided_params"
    cls = abi.jt_denoise_guided_params
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));', 'printf("jt_denoise_params %zu\\n", sizeof(jt_denoise_params));',
             'printf("abi %d\\n", JT_ABI_VERSION);']
    for f, _ in cls._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l)
    assert int(got[s]) == C.sizeof(cls) == 24
    assert [f for f, _ in cls._fields_] == list(G.FIELDS)
    for k, (f, _) in enumerate(cls._fields_):
        assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset == 4 * k, f
    # new functions and one new struct only: the plain struct and the ABI version stay
    assert int(got["jt_denoise_params"]) == C.sizeof(abi.jt_denoise_params) == 20 and int(got["abi"]) == 5


def _call(abi, lib, W=4, H=3, null=None, **fields):
    rgba = np.ones((H if H > 0 else 1, W if W > 0 else 1, 4), np.float32)
    var = np.ones_like(rgba)
    alb = np.ones(rgba.shape[:2] + (3,), np.float32)
    nrm = np.ones_like(alb)
    out = np.zeros_like(rgba)
    p = abi.jt_denoise_guided_params()
    assert lib.jt_denoise_guided_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    args = dict(rgba=rgba.ctypes.data_as(abi.f32p), variance=var.ctypes.data_as(abi.f32p),
                albedo=alb.ctypes.data_as(abi.f32p), normal=nrm.ctypes.data_as(abi.f32p), params=C.byref(p),
                out_rgba=out.ctypes.data_as(abi.f32p))
    if null:
        args[null] = None
    st = lib.jt_denoise_guided_image(args["rgba"], args["variance"], args["albedo"], args["normal"], W, H,
                                     args["params"], 0, args["out_rgba"])
    return st, lib.jt_last_error().decode()


@pytest.mark.parametrize("null", ["rgba", "variance", "albedo", "normal", "params", "out_rgba"])
def test_guided_image_rejects_null_pointers(abi, lib, null):
    st, msg = _call(abi, lib, null=null)
    assert st == -1 and null in msg, (st, msg)


BAD_FIELDS = [("iterations", 0), ("iterations", 9), ("iterations", -1)] + [
    (f, v) for f in G.FIELDS[1:] for v in (0.0, -1.0, float("nan"), float("inf"))]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_guided_image_rejects_bad_parameters(abi, lib, field, value):
    st, msg = _call(abi, lib, **{field: value})
    assert st == -1 and field in msg, (st, msg)


def test_guided_image_rejects_a_tolerance_that_underflows(abi, lib):
    """sigma_variance^2 * variance_floor is the least a tap divides by: it must be a normal float."""
    st, msg = _call(abi, lib, sigma_variance=1e-15, variance_floor=1e-10)
    assert st == -1 and "variance_floor" in msg and "underflow" in msg, (st, msg)


@pytest.mark.parametrize("W,H,name", [(0, 3, "width"), (-2, 3, "width"), (4, 0, "height"), (4, -1, "height"),
                                      (1 << 14, 1 << 13, "width*height"), (2**31 - 1, 2**31 - 1, "width*height")])
def test_guided_image_rejects_bad_sizes(abi, lib, W, H, name):
    # the arrays are never touched: the size is refused first
    rgba = np.ones(4, np.float32)
    p = abi.jt_denoise_guided_params()
    assert lib.jt_denoise_guided_defaults(C.byref(p)) == 0
    ptr = rgba.ctypes.data_as(abi.f32p)
    st = lib.jt_denoise_guided_image(ptr, ptr, ptr, ptr, W, H, C.byref(p), 0, ptr)
    msg = lib.jt_last_error().decode()
    assert st == -1 and name in msg, (st, msg)
    assert lib.jt_denoise_guided_image(ptr, ptr, ptr, ptr, 1, 1, C.byref(p), -1, ptr) == -1
    assert b"device" in lib.jt_last_error()


def test_guided_rejects_null_context_and_bad_params_first(abi, lib):
    assert lib.jt_denoise_guided(None, None) == -1 and b"ctx" in lib.jt_last_error()
    # the params are checked before the context is looked at
    not_a_ctx = C.cast(C.create_string_buffer(8), C.c_void_p)
    for field, value in BAD_FIELDS:
        p = abi.jt_denoise_guided_params()
        assert lib.jt_denoise_guided_defaults(C.byref(p)) == 0
        setattr(p, field, value)
        assert lib.jt_denoise_guided(not_a_ctx, C.byref(p)) == -1, (field, value)
        assert field.encode() in lib.jt_last_error(), (field, value)


def test_python_wrapper_checks_shapes_and_names(abi, lib):
    from jtrace import trace
    rgba, var, alb, nrm = _inputs((5, 7))
    with pytest.raises(ValueError):
        trace.denoise_guided_image(rgba, var, alb[:-1], nrm, lib=lib)
    with pytest.raises(ValueError):
        trace.denoise_guided_image(rgba, var[..., :3], alb, nrm, lib=lib)
    with pytest.raises(TypeError):
        trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib, sigma_color=1.0)
    with pytest.raises(abi.JTError) as e:
        trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib, iterations=9)
    assert e.value.status == -1 and "iterations" in str(e.value)


# ---- the CLI ----------------------------------------------------------------------------------
def test_cli_denoise_mode(capsys):
    from jtrace import cli
    p = cli.parse_cli_args(["--scene", "x.json"])
    assert p.denoise_mode == "plain" and p.denoise is False
    assert p == cli.Params(scene="x.json")  # the defaults are Params' own: nothing else moved
    p = cli.parse_cli_args(["--scene", "x", "--denoise", "true"])
    assert (p.denoise, p.denoise_mode, p.batch) == (True, "plain", 1)  # --denoise true alone: as before
    p = cli.parse_cli_args(["--scene", "x", "--denoise", "true", "--denoise-mode", "variance", "--batch", "2"])
    assert (p.denoise, p.denoise_mode, p.batch) == (True, "variance", 2)
    # read only with --denoise true: without it the mode needs no streams
    p = cli.parse_cli_args(["--scene", "x", "--denoise-mode", "variance"])
    assert (p.denoise, p.denoise_mode) == (False, "variance")
    assert cli.parse_cli_args(["--scene", "x", "--denoise-mode", "variance", "--devices", "2"]).devices == 2

    def rejected(*args):
        with pytest.raises(SystemExit) as e:
            cli.parse_cli_args(["--scene", "x", *args])
        assert e.value.code == 2
        return capsys.readouterr().err

    assert "--denoise-mode" in rejected("--denoise-mode", "svgf")
    msg = rejected("--denoise", "true", "--denoise-mode", "variance")  # the reference's default batch is 1
    assert "--denoise-mode variance" in msg and "--batch 2" in msg
    msg = rejected("--denoise", "true", "--denoise-mode", "variance", "--batch", "8", "--devices", "2")
    assert "--denoise-mode variance" in msg and "--devices 1" in msg
