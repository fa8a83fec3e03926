"""The denoiser on the GPU (csrc/jt_denoise.hip behind jt_denoise, jt_get_denoised and
jt_denoise_image): the kernel against the float64 restatement (tests/denoise_ref.py) on
synthetic inputs at the shapes where it can go wrong, the context path and its state rules, the
error it removes from a low-spp cornellbox render, and the CLI's --denoise.

The bound: every pixel and channel within 1e-4 relative (scale floor 1e-6) of the float64
restatement. The float32 restatement differs from it by at most 1.4e-6 on these inputs
(tests/test_denoise_host.py); the bound leaves room for a device exp a few ulp off at arguments
up to 88, and every term of the sums is non-negative, so nothing cancels."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
from conftest import CORNELL, make_params

pytestmark = pytest.mark.gpu

BOUND = 1e-4


def _fields(p):
    return {k: p[k] for k in ("iterations", "sigma_color", "sigma_normal", "sigma_albedo", "albedo_floor")}


# ---- 1. the kernel against the restatement -----------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_restatement(gpu, lib, shape):
    from jtrace import trace
    rgba, alb, nrm = R.synthetic(*shape)
    for p in R.parameter_sets(*shape):
        ref = R.denoise(rgba, alb, nrm, **p)
        got = trace.denoise_image(rgba, alb, nrm, lib=lib, **_fields(p))
        assert got.dtype == np.float32 and got.shape == rgba.shape
        err = R.rel_error(got, ref)
        print(f"{shape} iterations={p['iterations']} sigma_color={p['sigma_color']}: worst relative error {err.max():.3g}")
        assert np.isfinite(got).all()
        assert err.max() <= BOUND, (p, np.unravel_index(err.argmax(), err.shape))
        assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))
        again = trace.denoise_image(rgba, alb, nrm, lib=lib, **_fields(p))
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_negative_zero_alpha_and_explicit_params_struct(gpu, abi, lib):
    """Alpha passes through by its bits, and a jt_denoise_params given whole equals the overrides."""
    from jtrace import trace
    rgba, alb, nrm = R.synthetic(19, 37)
    rgba[3, 5, 3] = -0.0
    rgba[4, 6, 3] = 0.37
    p = trace.denoise_defaults(16, lib)
    got = trace.denoise_image(rgba, alb, nrm, params=p, lib=lib)
    assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))
    assert np.array_equal(got, trace.denoise_image(rgba, alb, nrm, samples=16, lib=lib))


# ---- 2. the context path -------------------------------------------------------------------------
def _state(abi, lib, sa, devices=None):
    from jtrace import trace
    p = make_params(abi, resolution=48, samples=10, batch=4)
    return trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), p, lib,
                                  devices=devices)


def _get_denoised_status(st):
    out = np.empty((st.height, st.width, 4), np.float32)
    return st.lib.jt_get_denoised(st.handle, out.ctypes.data_as(C.POINTER(C.c_float)))


def _snapshot(st):
    img = st.get_image()
    alb, nrm, hits = st.get_aovs()
    return img, alb, nrm, hits, st.counters()


def test_context_path(gpu, abi, lib, cornell_abi):
    from jtrace import trace
    st = _state(abi, lib, cornell_abi)
    # nothing traced: neither a filter nor a result
    assert lib.jt_denoise(st.handle, None) == -6 and b"no sample" in lib.jt_last_error()
    assert _get_denoised_status(st) == -6
    st.trace_samples()
    st.trace_samples()
    assert st.samples == 8
    assert _get_denoised_status(st) == -6
    before = _snapshot(st)
    den = st.denoise()
    after = _snapshot(st)
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert before[4] == after[4]
    assert _get_denoised_status(st) == 0

    # the same kernel on the arrays read back, and the restatement
    img, alb, nrm = before[:3]
    assert np.array_equal(den.view(np.uint32), trace.denoise_image(img, alb, nrm, samples=8, lib=lib).view(np.uint32))
    err = R.rel_error(den, R.denoise(img, alb, nrm, **R.defaults(8)))
    print(f"context path against the restatement: worst relative error {err.max():.3g}")
    assert err.max() <= BOUND
    assert np.array_equal(den[..., 3], img[..., 3])
    # explicit parameters and overrides reach the filter
    wide = st.denoise(sigma_color=64.0, iterations=2)
    assert np.array_equal(wide, trace.denoise_image(img, alb, nrm, samples=8, lib=lib, sigma_color=64.0, iterations=2))
    assert not np.array_equal(wide, den)
    bad = abi.jt_denoise_params(0, 1.0, 1.0, 1.0, 0.01)
    assert lib.jt_denoise(st.handle, C.byref(bad)) == -1 and b"iterations" in lib.jt_last_error()

    # two more samples: the result is stale, then current again (buffers reused)
    st.trace_samples()
    assert st.samples == 10
    assert _get_denoised_status(st) == -6
    den10 = st.denoise()
    img10 = st.get_image()
    alb10, nrm10, _ = st.get_aovs()
    assert np.array_equal(den10, trace.denoise_image(img10, alb10, nrm10, samples=10, lib=lib))
    st.reset()
    assert _get_denoised_status(st) == -6
    assert lib.jt_denoise(st.handle, None) == -6
    st.close()

    # a multi-device context over [0]: the host-array path, the same bits
    multi = _state(abi, lib, cornell_abi, devices=[0])
    assert _get_denoised_status(multi) == -6
    multi.trace_samples()
    multi.trace_samples()
    mbefore = _snapshot(multi)
    mden = multi.denoise()
    mafter = _snapshot(multi)
    assert np.array_equal(mden.view(np.uint32), den.view(np.uint32))
    for a, b in zip(mbefore[:4], mafter[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert mbefore[4] == mafter[4]
    multi.trace_samples()
    assert _get_denoised_status(multi) == -6
    multi.close()


# ---- 3. it denoises ------------------------------------------------------------------------------
def test_denoised_render_is_closer_to_the_converged_one(gpu, abi, lib, cornell_abi):
    from jtrace import trace

    def render(samples, seed):
        p = make_params(abi, resolution=128, samples=samples, batch=min(samples, 64), seed=seed)
        st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib),
                                    trace.make_trace_lights(cornell_abi, lib), p, lib)
        st.trace_range(0, samples)
        out = (st.get_image(), st.denoise())
        st.close()
        return out

    noisy, den = render(4, 0x5EED)
    ref, _ = render(1024, 7)
    mse_noisy = np.mean((noisy[..., :3].astype(np.float64) - ref[..., :3]) ** 2)
    mse_den = np.mean((den[..., :3].astype(np.float64) - ref[..., :3]) ** 2)
    print(f"cornellbox 128x128 4 spp: MSE noisy {mse_noisy:.6g}, denoised {mse_den:.6g}, ratio {mse_den / mse_noisy:.3f}")
    assert mse_den < 0.6 * mse_noisy


# ---- 4. the CLI ----------------------------------------------------------------------------------
def test_cli_denoise_flag(gpu, tmp_path):
    from PIL import Image
    from jtrace import main

    def run(*extra):
        out = tmp_path / f"cb{len(extra)}.png"
        lines = []
        res = main.run(main.parse_cli_args(["--scene", CORNELL, "--resolution", "64", "--samples", "4", "--batch", "2",
                                            "--output", str(out), *extra]), out=lines.append)
        return lines, res, np.asarray(Image.open(out))

    def stages(lines):
        return [s.split(" in ")[0].split(" to ")[0].rstrip(".") for s in lines if not s.startswith("sample ")]

    plain = ["loading scene " + CORNELL, "loaded scene", "finding camera", "building bvh", "built bvh", "making lights",
             "making state", "tracing samples", "rendered", "saving image", "saved image", "total time"]
    lines, res, png = run()
    got = stages(lines)
    assert got[:-1] == plain[:-1] and got[-1].startswith("total time"), got
    assert "denoised" not in res and png.shape == (64, 64, 4)

    dlines, dres, dpng = run("--denoise", "true")
    assert not any("not yet supported" in s for s in dlines)
    dgot = stages(dlines)
    k = dgot.index("rendered")
    assert dgot[k + 1:k + 4] == ["denoising", "denoised", "saving image"], dgot
    assert dgot[:k + 1] == got[:k + 1] and dgot[k + 3:-1] == got[k + 1:-1]
    assert dres["denoised"] is True and dpng.shape == (64, 64, 4)
    assert dres["counters"]["paths"] == res["counters"]["paths"] == 64 * 64 * 4
    assert not np.array_equal(dpng, png) and dpng[..., :3].mean() > 5
