"""The error estimate on the GPU (csrc/jt_error.hip behind jt_get_variance and jt_get_noise):
the kernel against the restatement (tests/error_ref.py) applied to the oracle's stream means,
its reduction, the context's state rules, that a query changes nothing else, tile shares,
multi-device contexts, the CLI's --noise-target / --error-output, and the 1 / sqrt(n) slope.

Cornellbox, traversal near, seed 0x5EED (conftest.make_params). The per-pixel bar is the
project's bitwise_frac: at least 99.9 % of pixels equal on all four channels bit for bit (a
1-ulp libm difference between oracle and device may flip a rare path)."""
import ctypes as C

import numpy as np
import pytest

import error_ref as R
from conftest import CORNELL, make_params

pytestmark = pytest.mark.gpu

W, H = 44, 36  # partial 8x8 tiles on the right and at the bottom; 30 tiles: more than one workgroup


def _state(abi, lib, sa, devices=None, **kw):
    from jtrace import trace
    p = make_params(abi, **kw)
    return trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), p, lib,
                                  devices=devices)


_means = {}


def _oracle_means(abi, oracle, sa, w, h, k, ns, sampler=1):
    """The oracle's stream means (k, h, w, 4) after n samples for every n of `ns` (ascending),
    computed once per case and shared."""
    key = (w, h, k, tuple(ns), sampler)
    if key not in _means:
        p = make_params(abi, width=w, height=h, samples=ns[-1], sampler=sampler)
        bvh, lights = oracle.build_bvh(sa), oracle.make_lights(sa)
        parts, out, s0 = {}, {}, 0
        for n in ns:
            oracle.trace(sa, bvh, lights, p, w, h, s0, n, streams=k, parts=parts)
            out[n] = parts["img"].copy()
            out[n].setflags(write=False)
            s0 = n
        _means[key] = out
    return _means[key]


def _status(lib, st, which="variance"):
    if which == "variance":
        buf = np.empty((st.height, st.width, 4), np.float32)
        rc = lib.jt_get_variance(st.handle, buf.ctypes.data_as(C.POINTER(C.c_float)))
    else:
        rc = lib.jt_get_noise(st.handle, C.byref(C.c_double()))
    return rc, lib.jt_last_error().decode()


def _check_parity(got, means, n, k, label):
    ref = R.variance(means, n, k)
    eq = np.all(got.view(np.uint32) == ref.view(np.uint32), axis=-1)
    s_got, s_ref = float(got.sum(dtype=np.float64)), float(ref.sum(dtype=np.float64))
    print(f"{label}: bitwise_frac {eq.mean():.5f} ({(~eq).sum()} pixels differ), summed variance {s_got:.6g} "
          f"vs {s_ref:.6g} (rel {abs(s_got - s_ref) / s_ref:.2e})")
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all() and (got >= 0).all()
    assert eq.mean() >= 0.999, label
    assert abs(s_got - s_ref) <= 1e-3 * s_ref, label


# ---- 1. per-pixel parity ------------------------------------------------------------------------
def test_variance_matches_restatement_on_unequal_streams(gpu, abi, lib, oracle, cornell_abi, options):
    """k = 4 at 44x36: n = 6 in two calls whose first holds fewer samples than streams (n_j = 2, 2,
    1, 1), and n = 3, where only ns = 3 of the 4 streams hold a sample."""
    options("streams", "4")
    means = _oracle_means(abi, oracle, cornell_abi, W, H, 4, (3, 6))
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    assert st.streams == 4
    st.trace_range(0, 1)
    st.trace_range(1, 6)
    _check_parity(st.variance(), means[6], 6, 4, "44x36 k=4 n=6")
    st.close()
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    st.trace_range(0, 3)
    _check_parity(st.variance(), means[3], 3, 4, "44x36 k=4 n=3")
    st.close()


@pytest.mark.parametrize("sampler", [1, 2], ids=["path", "naive"])
def test_variance_matches_restatement_at_sixteen_streams(gpu, abi, lib, oracle, cornell_abi, options, sampler):
    """32x32, a batch of 32, k = 16, n = 32: two samples per stream. (The stream rule alone gives a
    batch of 32 at this size 32 streams — the case below — so k is set by the option.)"""
    options("streams", "16")
    means = _oracle_means(abi, oracle, cornell_abi, 32, 32, 16, (32,), sampler)
    st = _state(abi, lib, cornell_abi, resolution=32, samples=32, batch=32, sampler=sampler)
    assert st.streams == 16
    st.trace_samples()
    assert st.samples == 32
    _check_parity(st.variance(), means[32], 32, 16, f"32x32 k=16 n=32 sampler {sampler}")
    st.close()


def test_variance_matches_restatement_at_the_automatic_stream_count(gpu, abi, lib, oracle, cornell_abi):
    """32x32, a batch of 32 with the stream count the library picks itself: k = 32, one sample each."""
    means = _oracle_means(abi, oracle, cornell_abi, 32, 32, 32, (32,))
    st = _state(abi, lib, cornell_abi, resolution=32, samples=32, batch=32)
    assert st.streams == 32
    st.trace_samples()
    _check_parity(st.variance(), means[32], 32, 32, "32x32 k=32 n=32")
    st.close()


# ---- 2. the reduction ---------------------------------------------------------------------------
def test_noise_is_the_reduction_of_the_variance(gpu, abi, lib, cornell_abi, options):
    """noise() against sqrt(3 N V) / M in float64 from the GPU's own variance and image, on the
    44x36 context (the lanes of edge tiles outside the image must add 0). Bound 1e-4: a workgroup
    sums at most 256 non-negative floats, so any order is within 255 * 2^-24 = 1.5e-5."""
    options("streams", "4")
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    st.trace_range(0, 6)
    noise = st.noise()
    var, img = st.variance(), st.get_image()
    want = R.noise(var, img)
    print(f"noise {noise:.8g}, from the variance and the image {want:.8g}, rel {abs(noise - want) / want:.2e}")
    assert want > 0 and abs(noise - want) <= 1e-4 * want
    assert st.noise() == noise  # deterministic, and served from the result already there
    st.close()


# ---- 3. state -----------------------------------------------------------------------------------
def test_state_errors(gpu, abi, lib, cornell_abi, options):
    one = _state(abi, lib, cornell_abi, width=W, height=H, samples=8, batch=1)
    assert one.streams == 1
    for which in ("variance", "noise"):
        rc, msg = _status(lib, one, which)
        assert rc == -6 and "streams" in msg and "batch >= 2" in msg, msg
    one.trace_range(0, 4)
    rc, msg = _status(lib, one)
    assert rc == -6 and "streams" in msg, msg
    one.close()

    options("streams", "4")
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    for which in ("variance", "noise"):
        rc, msg = _status(lib, st, which)
        assert rc == -6 and "no sample" in msg, msg  # before any sample
    st.trace_range(0, 1)
    for which in ("variance", "noise"):
        rc, msg = _status(lib, st, which)
        assert rc == -6 and "streams" in msg, msg  # k = 4, n = 1: one stream holds a sample
    st.trace_range(1, 6)
    var6, noise6 = st.variance(), st.noise()
    st.reset()
    for which in ("variance", "noise"):
        rc, msg = _status(lib, st, which)
        assert rc == -6 and "no sample" in msg, msg  # after jt_reset
    st.trace_range(0, 6)
    assert np.array_equal(st.variance().view(np.uint32), var6.view(np.uint32)) and st.noise() == noise6
    st.close()
    fresh = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    fresh.trace_range(0, 6)
    assert np.array_equal(fresh.variance().view(np.uint32), var6.view(np.uint32)) and fresh.noise() == noise6
    fresh.close()


# ---- 4. purity ----------------------------------------------------------------------------------
def _snapshot(st):
    img = st.get_image()
    alb, nrm, hits = st.get_aovs()
    return img, alb, nrm, hits


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_a_query_changes_nothing_else(gpu, abi, lib, cornell_abi, options):
    options("streams", "4")
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    plain = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    for s in (st, plain):
        s.set_counters(1)
    st.trace_range(0, 4)
    st.variance()  # with the AOV combine of the launch still pending
    plain.trace_range(0, 4)
    before, cnt_before = _snapshot(st), st.counters()
    assert _same(before, _snapshot(plain))
    st.variance()
    st.noise()
    after, cnt_after = _snapshot(st), st.counters()
    assert _same(before, after)
    for name in cnt_before:
        if name != "launches":
            assert cnt_before[name] == cnt_after[name], name
    # the stream means too: the next range continues them to the bits of an unqueried render
    st.trace_range(4, 8)
    plain.close()
    plain = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    plain.set_counters(1)
    plain.trace_range(0, 8)
    assert _same(_snapshot(st), _snapshot(plain))
    a, b = st.counters(), plain.counters()
    for name in ("paths", "rays", "light_queries", "nodes", "instances", "prims", "shades"):
        assert a[name] == b[name], name
    assert np.array_equal(st.variance().view(np.uint32), plain.variance().view(np.uint32))
    st.close()
    plain.close()


# ---- 5. tile share ------------------------------------------------------------------------------
def test_tile_share_estimates_its_own_pixels(gpu, abi, lib, cornell_abi, options):
    options("streams", "4")
    full = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    full.trace_range(0, 6)
    var_full, img_full = full.variance(), full.get_image()
    full.close()
    options("tile_share", "2,1")
    share = _state(abi, lib, cornell_abi, width=W, height=H, samples=8)
    assert share.streams == 4
    share.trace_range(0, 6)
    var, noise = share.variance(), share.noise()
    share.close()
    j, i = np.mgrid[0:H, 0:W]
    own = ((j // 8) * ((W + 7) // 8) + i // 8) % 2 == 1
    assert np.all(var[~own].view(np.uint32) == 0)  # exactly 0, sign included
    assert np.array_equal(var[own].view(np.uint32), var_full[own].view(np.uint32))
    assert var[own][..., :3].sum() > 0
    want = R.noise(var_full, img_full, own)  # N counts the share's pixels only
    assert abs(noise - want) <= 1e-4 * want, (noise, want)


# ---- 6. multi-device ----------------------------------------------------------------------------
def test_multi_device_context_is_unsupported(gpu, abi, lib, cornell_abi):
    multi = _state(abi, lib, cornell_abi, devices=[0], resolution=32, samples=8, batch=4)
    multi.trace_samples()
    for which in ("variance", "noise"):
        rc, msg = _status(lib, multi, which)
        assert rc == -2 and "multi-device" in msg, msg
    multi.close()


# ---- 7. the CLI's stopping rule -----------------------------------------------------------------
def test_cli_stops_at_the_noise_target(gpu, abi, oracle, cornell_abi, tmp_path):
    """32x32, --batch 8 (k = 8), --samples 256, a check every 8 samples. The target is the
    geometric mean of the restatement's noise on the oracle at 40 and 48 samples (0.4556 and
    0.4059: 11 % apart, far more than a flipped pixel moves it), so the run stops at 48."""
    from PIL import Image
    from jtrace import main
    means = _oracle_means(abi, oracle, cornell_abi, 32, 32, 8, (40, 48))
    at = {n: R.noise(R.variance(means[n], n, 8), R.combine(means[n], n, 8)) for n in (40, 48)}
    target = float(np.sqrt(at[40] * at[48]))
    print(f"restated noise at 40 samples {at[40]:.4f}, at 48 {at[48]:.4f}, target {target:.4f}")
    assert at[48] < target < at[40]

    def run(name, *extra):
        lines = []
        res = main.run(main.parse_cli_args(["--scene", CORNELL, "--resolution", "32", "--batch", "8", "--traversal", "near",
                                            "--output", str(tmp_path / name), *extra]), out=lines.append)
        return lines, res

    lines, res = run("stop.png", "--samples", "256", "--noise-interval", "8", "--noise-target", repr(target),
                     "--error-output", str(tmp_path / "err.png"))
    print("\n".join(s for s in lines if s.startswith("noise")))
    assert res["samples_traced"] == 48 and res["counters"]["paths"] == 32 * 32 * 48
    assert "noise target reached at 48/256 samples" in lines
    checks = [s for s in lines if s.startswith("noise ") and " at " in s and "target" not in s]
    assert [int(s.split()[3]) for s in checks] == [8, 16, 24, 32, 40, 48], checks
    assert abs(float(checks[-1].split()[1]) - at[48]) <= 2e-3 * at[48]  # the printed four digits
    assert res["noise"] <= target
    plines, pres = run("plain.png", "--samples", "48")
    assert pres["samples_traced"] == 48 and "noise" not in pres
    assert not any(s.startswith("noise") or "error image" in s for s in plines)
    assert (tmp_path / "stop.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    err = np.asarray(Image.open(tmp_path / "err.png"))
    assert err.shape == np.asarray(Image.open(tmp_path / "stop.png")).shape == (32, 32, 4)
    assert (err[..., 3] == 255).all() and err[..., :3].max() > 0


# ---- 8. the slope -------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [1, 2], ids=["path", "naive"])
def test_noise_falls_as_one_over_sqrt_n(gpu, abi, lib, cornell_abi, sampler):
    """32x32, batch 8, k = 8: four times the samples halve the noise (ideal 0.5; the restatement
    on the oracle gives 0.56 for path and 0.51 for naive)."""
    st = _state(abi, lib, cornell_abi, resolution=32, samples=64, batch=8, sampler=sampler)
    assert st.streams == 8
    st.trace_range(0, 16)
    n16 = st.noise()
    st.trace_range(16, 64)
    n64 = st.noise()
    st.close()
    print(f"sampler {sampler}: noise {n16:.4f} at 16 samples, {n64:.4f} at 64, ratio {n64 / n16:.3f}")
    assert 0.4 <= n64 / n16 <= 0.7
