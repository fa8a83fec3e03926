"""The variance-guided denoiser on the GPU (csrc/jt_denoise.hip behind jt_denoise_guided,
jt_get_denoised and jt_denoise_guided_image): the kernels against the float64 restatement
(tests/denoise_guided_ref.py) on synthetic inputs at the shapes where they can go wrong, the
context path and its state rules, the error it removes from a 16-spp cornellbox render compared
with the plain filter, and the CLI's --denoise-mode.

The bound: every pixel and channel within 1e-4 relative (scale floor 1e-6) of the float64
restatement, as tests/test_gpu_denoise.py and for its reason: the float32 restatement differs
from it by at most 1.1e-6 on these inputs (tests/test_denoise_guided_host.py), the rest is room
for a device exp a few ulp off and the division; every term of the sums is non-negative, so
nothing cancels. Measured on the MI355X: at most 1.24e-6 (45x70, sigma_variance 2)."""
import ctypes as C

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R
from conftest import CORNELL, make_params

pytestmark = pytest.mark.gpu

BOUND = 1e-4


def _inputs(shape):
    rgba, alb, nrm = G.synthetic(*shape)
    return rgba, G.synthetic_variance(rgba, *shape), alb, nrm


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the kernels against the restatement ------------------------------------------------------
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_restatement(gpu, lib, shape):
    from jtrace import trace
    rgba, var, alb, nrm = _inputs(shape)
    for p in G.parameter_sets():
        ref = G.denoise_guided(rgba, var, alb, nrm, **p)
        got = trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib, **p)
        assert got.dtype == np.float32 and got.shape == rgba.shape
        err = G.rel_error(got, ref)
        print(f"{shape} iterations={p['iterations']} sigma_variance={p['sigma_variance']}: "
              f"worst relative error {err.max():.3g}")
        assert np.isfinite(got).all()
        assert err.max() <= BOUND, (p, np.unravel_index(err.argmax(), err.shape))
        assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))
        again = trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib, **p)
        assert np.array_equal(_bits(got), _bits(again))


def test_alpha_bits_and_explicit_params_struct(gpu, lib):
    """Alpha passes through by its bits whatever var.a holds, and a jt_denoise_guided_params given
    whole equals the defaults."""
    from jtrace import trace
    rgba, var, alb, nrm = _inputs((19, 37))
    rgba[3, 5, 3] = -0.0
    rgba[4, 6, 3] = 0.37
    got = trace.denoise_guided_image(rgba, var, alb, nrm, params=trace.denoise_guided_defaults(lib), lib=lib)
    assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))
    assert np.array_equal(_bits(got), _bits(trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib)))
    var[..., 3] = np.nan  # v.a is ignored
    assert np.array_equal(_bits(got), _bits(trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib)))


# ---- 2. zero variance: the identity ----------------------------------------------------------------
def test_zero_variance_returns_the_input(gpu, lib):
    from jtrace import trace
    rgba, _, alb, nrm = _inputs((19, 37))
    got = trace.denoise_guided_image(rgba, np.zeros_like(rgba), alb, nrm, lib=lib)
    worst = G.rel_error(got, rgba).max()
    print(f"zero variance on 19x37: worst relative difference from the input {worst:.3g}")
    assert worst <= 1e-6


# ---- 3. the context path ---------------------------------------------------------------------------
def _state(abi, lib, sa, devices=None, batch=4):
    from jtrace import trace
    p = make_params(abi, resolution=48, samples=10, batch=batch)
    return trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), p, lib,
                                  devices=devices)


def _get_denoised_status(st):
    out = np.empty((st.height, st.width, 4), np.float32)
    return st.lib.jt_get_denoised(st.handle, out.ctypes.data_as(C.POINTER(C.c_float)))


def _snapshot(st):
    img = st.get_image()
    alb, nrm, hits = st.get_aovs()
    return img, alb, nrm, hits, st.variance(), st.counters()


def test_context_path(gpu, abi, lib, cornell_abi):
    from jtrace import trace
    st = _state(abi, lib, cornell_abi)
    # nothing traced: neither a filter nor a result; bad params come first
    assert lib.jt_denoise_guided(st.handle, None) == -6 and b"no sample" in lib.jt_last_error()
    bad = abi.jt_denoise_guided_params(5, 2.0, 0.3, 0.1, 0.01, 0.0)
    assert lib.jt_denoise_guided(st.handle, C.byref(bad)) == -1 and b"variance_floor" in lib.jt_last_error()
    assert _get_denoised_status(st) == -6
    st.trace_samples()
    st.trace_samples()
    assert st.samples == 8 and st.streams >= 2
    assert _get_denoised_status(st) == -6
    before = _snapshot(st)
    den = st.denoise_guided()
    after = _snapshot(st)
    for a, b in zip(before[:5], after[:5]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert before[5] == after[5]
    assert _get_denoised_status(st) == 0

    # the same kernels on the arrays read back, and the restatement
    img, alb, nrm, _, var = before[:5]
    assert np.array_equal(_bits(den), _bits(trace.denoise_guided_image(img, var, alb, nrm, lib=lib)))
    err = G.rel_error(den, G.denoise_guided(img, var, alb, nrm, **G.DEFAULTS))
    print(f"context path against the restatement: worst relative error {err.max():.3g}")
    assert err.max() <= BOUND
    assert np.array_equal(_bits(den[..., 3]), _bits(img[..., 3]))

    # the last of the two filters to run wins
    plain = st.denoise()
    assert np.array_equal(_bits(plain), _bits(trace.denoise_image(img, alb, nrm, samples=8, lib=lib)))
    assert not np.array_equal(plain, den)
    assert np.array_equal(_bits(st.denoise_guided()), _bits(den))
    # overrides reach the kernel
    wide = st.denoise_guided(sigma_variance=8.0)
    assert np.array_equal(_bits(wide), _bits(trace.denoise_guided_image(img, var, alb, nrm, lib=lib, sigma_variance=8.0)))
    assert not np.array_equal(wide, den)
    with pytest.raises(TypeError):
        st.denoise_guided(sigma_color=1.0)

    # two more samples: the result is stale, then current again (buffers reused); the estimate
    # the filter computed serves jt_get_variance
    st.trace_samples()
    assert st.samples == 10
    assert _get_denoised_status(st) == -6
    den10 = st.denoise_guided()
    img10, var10 = st.get_image(), st.variance()
    alb10, nrm10, _ = st.get_aovs()
    assert np.array_equal(_bits(den10), _bits(trace.denoise_guided_image(img10, var10, alb10, nrm10, lib=lib)))
    assert not np.array_equal(var10, var)
    st.reset()
    assert _get_denoised_status(st) == -6
    assert lib.jt_denoise_guided(st.handle, None) == -6
    st.close()


def test_context_path_needs_streams_on_one_device(gpu, abi, lib, cornell_abi):
    one = _state(abi, lib, cornell_abi, batch=1)
    one.trace_samples()
    one.trace_samples()
    assert lib.jt_denoise_guided(one.handle, None) == -6 and b"stream" in lib.jt_last_error()
    assert _get_denoised_status(one) == -6
    one.denoise()  # the plain filter needs none
    one.close()

    multi = _state(abi, lib, cornell_abi, devices=[0])
    multi.trace_samples()
    multi.trace_samples()
    assert lib.jt_denoise_guided(multi.handle, None) == -2 and b"multi-device" in lib.jt_last_error()
    assert _get_denoised_status(multi) == -6
    multi.close()


# ---- 4. it denoises ----------------------------------------------------------------------------------
def test_guided_render_is_closer_to_the_converged_one_than_plain(gpu, abi, lib, cornell_abi):
    """Cornellbox 128x128, 16 spp in 16 streams (seed 0x5EED) against the GPU's own 1024-spp render of
    seed 7: the two inequalities of tests/test_denoise_guided_host.py, whose restatement on the
    oracle's render measures 0.664 and 0.316."""
    from jtrace import trace

    def state(samples, seed, batch):
        p = make_params(abi, resolution=128, samples=samples, batch=batch, seed=seed)
        st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib),
                                    trace.make_trace_lights(cornell_abi, lib), p, lib)
        st.trace_range(0, samples)
        return st

    st = state(16, 0x5EED, 16)
    assert st.streams == 16
    noisy, plain, guided = st.get_image(), st.denoise(), st.denoise_guided()
    st.close()
    st = state(1024, 7, 64)
    ref = st.get_image()[..., :3].astype(np.float64)
    st.close()

    def mse(x):
        return float(np.mean((x[..., :3].astype(np.float64) - ref) ** 2))

    noisy_mse, plain_mse, guided_mse = mse(noisy), mse(plain), mse(guided)
    print(f"cornellbox 128x128 16 spp: MSE noisy {noisy_mse:.6g}, plain {plain_mse:.6g}, guided {guided_mse:.6g}; "
          f"guided / plain {guided_mse / plain_mse:.3f}, guided / noisy {guided_mse / noisy_mse:.3f}")
    assert guided_mse < 0.8 * plain_mse
    assert guided_mse < 0.4 * noisy_mse


# ---- 5. the CLI ----------------------------------------------------------------------------------------
def test_cli_denoise_mode(gpu, tmp_path):
    from PIL import Image
    from jtrace import main

    def run(name, *extra):
        out = tmp_path / f"{name}.png"
        lines = []
        res = main.run(main.parse_cli_args(["--scene", CORNELL, "--resolution", "64", "--samples", "4", "--batch", "2",
                                            "--output", str(out), *extra]), out=lines.append)
        return lines, res, np.asarray(Image.open(out))

    def stages(lines):
        return [s.split(" in ")[0].split(" to ")[0].rstrip(".") for s in lines if not s.startswith("sample ")]

    _, res, png = run("noisy")
    plines, pres, ppng = run("plain", "--denoise", "true")
    vlines, vres, vpng = run("variance", "--denoise", "true", "--denoise-mode", "variance")
    assert stages(vlines)[:-1] == stages(plines)[:-1] and "denoising" in stages(vlines)
    assert "denoise_mode" not in res and pres["denoise_mode"] == "plain"
    assert vres["denoised"] is True and vres["denoise_mode"] == "variance"
    assert vpng.shape == ppng.shape == (64, 64, 4)
    assert not np.array_equal(vpng, ppng) and not np.array_equal(vpng, png) and vpng[..., :3].mean() > 5
    assert vres["counters"]["paths"] == pres["counters"]["paths"] == res["counters"]["paths"] == 64 * 64 * 4
