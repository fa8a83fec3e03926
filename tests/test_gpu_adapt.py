"""Adaptive sampling on the GPU (csrc/jt_adapt.hip behind jt_adapt and jt_get_sample_counts, the
frozen-tile skip of the megakernel's hand-out): the frozen set against the restatement
(tests/adapt_ref.py) fed the GPU's own variance and image, that the call changes nothing else,
that later samples skip exactly the frozen tiles and leave every other pixel to the bits of an
unadapted render, the state rules, tile shares, jt_describe and the CLI's --adaptive.

Cornellbox, traversal near, seed 0x5EED (conftest.make_params). The shapes are the error tests'
own: 44x36 (partial edge tiles, 30 tiles: more than one workgroup) and 32x32; 24x20 for the run
through the other kernels' ADAPT instances (HBM mode, the wide traversal, the stack overflow)."""
import ctypes as C

import numpy as np
import pytest

import adapt_ref as A
from conftest import CORNELL, make_params

pytestmark = pytest.mark.gpu

W, H = 44, 36
NAMES = ("image", "albedo", "normal", "hits", "variance")


def _state(abi, lib, sa, **kw):
    from jtrace import trace
    p = make_params(abi, **kw)
    st = trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), p, lib)
    st.set_counters(1)
    return st


def _snapshot(st):
    img = st.get_image()
    alb, nrm, hits = st.get_aovs()
    return dict(zip(NAMES, (img, alb, nrm, hits, st.variance())))


def _same(a, b):
    return [name for name in NAMES if not np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8))]


_plain = {}


def _plain_renders(abi, lib, sa, key, ns, **kw):
    """Snapshots {n: outputs} of a context that never adapts, after n samples for every n of `ns`;
    rendered once per case (`key` names the options in effect) and shared, read-only."""
    key = (key, tuple(ns))
    if key not in _plain:
        st = _state(abi, lib, sa, **kw)
        out, s0 = {}, 0
        for n in ns:
            st.trace_range(s0, n)
            out[n] = _snapshot(st)
            for a in out[n].values():
                a.setflags(write=False)
            s0 = n
        st.close()
        _plain[key] = out
    return _plain[key]


def _median_target(var, img, traced):
    """A noise target whose threshold lies midway between two adjacent distinct values of V_t / N_t
    near the median of the traced tiles (at least 1e-3 apart, relatively: far above the float32
    roundings of vmax and the compare), derived in double through the library's own formula."""
    V, N = A.tile_stats(var)
    r = np.unique((V.astype(np.float64) / np.maximum(N, 1))[traced])
    mid = len(r) // 2
    for i in sorted(range(len(r) - 1), key=lambda i: abs(i - mid)):
        if r[i + 1] - r[i] > 1e-3 * r[i + 1]:
            break
    else:
        raise AssertionError("no two tiles far enough apart")
    vm = 0.5 * (r[i] + r[i + 1])
    M, Npix = A.image_sums(img, traced)
    T = float(np.sqrt(3.0 * vm) * Npix / M)
    assert r[i] < float(A.vmax(T, M, Npix)) < r[i + 1]
    return T


def _adapt_and_continue(abi, lib, sa, key, n1, n2, T=None, share=(1, 0), **kw):
    """Trace n1, jt_adapt(T) (T None: the median target), trace to n2; every check of case 1 but the
    second call. Returns the context at n2 with what the later checks need."""
    w, h = kw["width"], kw["height"]
    traced = A.share_mask(h, w, *share)
    plain = _plain_renders(abi, lib, sa, key, (n1, n2), **kw)
    st = _state(abi, lib, sa, **kw)
    st.trace_range(0, n1)
    before, cnt_before = _snapshot(st), st.counters()
    assert not _same(before, plain[n1])
    assert "adaptive=" not in st.describe()
    if T is None:
        T = _median_target(before["variance"], before["image"], traced)
    frozen = A.freeze(before["variance"], before["image"], T, traced=traced)
    print(f"{key}: T {T:.6g}, restatement freezes {frozen.sum()} of {traced.sum()} traced tiles at n = {n1}")
    active = st.adapt(T)
    assert active == (traced & ~frozen).sum()
    assert st.adaptive == (active, traced.sum())
    # the call changes nothing else
    after, cnt_after = _snapshot(st), st.counters()
    assert not _same(before, after)
    assert cnt_before == cnt_after
    assert st.samples == n1
    counts = st.sample_counts()
    assert counts.dtype == np.int32 and np.array_equal(counts, np.where(A.pixels_of(traced, h, w), n1, 0))
    # later samples skip the frozen tiles and nothing else
    st.trace_range(n1, n2)
    assert st.samples == n2
    frozen_at = np.where(frozen, n1, 0)
    got = _snapshot(st)
    for name in NAMES:
        want = A.implied(frozen_at, {n1: plain[n1][name], n2: plain[n2][name]}, n2)
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    _, N = A.tile_stats(before["variance"])
    cnt = st.counters()
    assert cnt["paths"] - cnt_before["paths"] == (n2 - n1) * int(N[traced & ~frozen].sum())
    want_counts = np.where(A.pixels_of(frozen, h, w), n1, n2) * A.pixels_of(traced, h, w)
    assert np.array_equal(st.sample_counts(), want_counts)
    return st, T, frozen, traced, got, plain


# ---- 1. the frozen set, purity, the skip --------------------------------------------------------
def test_adapt_freezes_the_restated_tiles_and_skips_them(gpu, abi, lib, cornell_abi, options):
    """44x36, k = 4: adapt at 8 with a target at the median tile, trace to 16, adapt again, trace
    to 24."""
    options("streams", "4")
    st, T, frozen, traced, got, _ = _adapt_and_continue(abi, lib, cornell_abi, "44x36 k=4", 8, 16,
                                                         width=W, height=H, samples=32)
    assert frozen.any() and not frozen.all()
    # a second call with the same target freezes a superset; the earlier tiles still report 8
    frozen2 = A.freeze(got["variance"], got["image"], T, frozen=frozen)
    active = st.adapt(T)
    print(f"second call: {frozen2.sum()} tiles frozen, {active} active")
    assert active == (~frozen2).sum() and active <= (~frozen).sum()
    st.trace_range(16, 24)
    want = np.where(A.pixels_of(frozen, H, W), 8, np.where(A.pixels_of(frozen2, H, W), 16, 24))
    assert np.array_equal(st.sample_counts(), want)
    st.close()


# ---- 2. sixteen streams, both samplers ----------------------------------------------------------
@pytest.mark.parametrize("sampler", [1, 2], ids=["path", "naive"])
def test_adapt_at_sixteen_streams(gpu, abi, lib, cornell_abi, options, sampler):
    """32x32, k = 16: adapt at 32 (two samples per stream), trace to 64."""
    options("streams", "16")
    st, _, frozen, _, _, _ = _adapt_and_continue(abi, lib, cornell_abi, f"32x32 k=16 sampler {sampler}", 32, 64,
                                                 width=32, height=32, samples=64, batch=32, sampler=sampler)
    assert st.streams == 16 and frozen.any() and not frozen.all()
    st.close()


# ---- 2b. other kernels' ADAPT instances ---------------------------------------------------------
# (options, make_params arguments, the tokens jt_describe must show): the HBM-mode kernel of
# configuration 0, that of its wide twin (configuration 8), and the LDS-mode kernel whose stack
# overflows into HBM (configuration 5, OVF)
KERNEL_CASES = {
    "hbm": ({"lds_scene": "0"}, {}, ("mode=hbm", "traversal=near")),
    "hbm-wide": ({"lds_scene": "0"}, {"traversal": "wide"}, ("mode=hbm", "traversal=wide")),
    "lds-overflow": ({"test_lds_ring": "2"}, {}, ("mode=lds", "hbm_overflow=1", "ring_used=2")),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_adapt_in_other_kernels(gpu, abi, lib, cornell_abi, options, case):
    """24x20 (9 tiles, a partial bottom row, three adapt workgroups), k = 4: adapt at 8 with the
    median target, trace to 16; every check of the helper, bit for bit against an unadapted
    context under the same options."""
    opts, params, tokens = KERNEL_CASES[case]
    options("streams", "4")
    for name, value in opts.items():
        options(name, value)
    st, _, frozen, _, _, _ = _adapt_and_continue(abi, lib, cornell_abi, case, 8, 16,
                                                 width=24, height=20, samples=32, **params)
    desc = f" {st.describe()} "
    print(f"{case}: {frozen.sum()} of {frozen.size} tiles frozen; {desc.strip()}")
    for token in tokens:
        assert f" {token} " in desc, (token, desc)
    assert frozen.any() and not frozen.all()
    st.close()


# ---- 3. everything frozen -----------------------------------------------------------------------
def test_a_huge_target_freezes_everything(gpu, abi, lib, cornell_abi, options):
    """T = 1e3: no tile stays active, and the next range traces nothing: paths and every output's
    bits stay (16 is a multiple of k = 4), jt_get_samples advances."""
    options("streams", "4")
    st, _, frozen, _, got, plain = _adapt_and_continue(abi, lib, cornell_abi, "44x36 k=4", 8, 16, T=1e3,
                                                       width=W, height=H, samples=32)
    assert frozen.all() and st.adaptive == (0, 30)
    assert not _same(got, plain[8])
    assert st.counters()["paths"] == 8 * W * H
    assert np.array_equal(st.sample_counts(), np.full((H, W), 8))
    st.close()


# ---- 4. nothing but zero variance frozen --------------------------------------------------------
def test_a_tiny_target_freezes_only_zero_variance(gpu, abi, lib, cornell_abi, options):
    """T = 1e-12: only the tiles the restatement freezes (zero variance) freeze, and the rest of
    the render is bitwise the unadapted one (checked inside the helper)."""
    options("streams", "4")
    st, _, frozen, _, _, _ = _adapt_and_continue(abi, lib, cornell_abi, "44x36 k=4", 8, 16, T=1e-12,
                                                 width=W, height=H, samples=32)
    V, _ = A.tile_stats(st.variance())
    assert np.array_equal(frozen, V == 0) or (V[frozen] <= 1e-20).all()
    st.close()


# ---- 5. state -----------------------------------------------------------------------------------
def _adapt_status(lib, st, T=0.1):
    n = C.c_int32(-7)
    rc = lib.jt_adapt(st.handle, T, C.byref(n))
    return rc, lib.jt_last_error().decode()


def test_state_errors_and_reset(gpu, abi, lib, cornell_abi, options):
    one = _state(abi, lib, cornell_abi, width=W, height=H, samples=8, batch=1)
    assert one.streams == 1
    one.trace_range(0, 4)
    rc, msg = _adapt_status(lib, one)
    assert rc == -6 and "streams" in msg, msg
    assert np.array_equal(one.sample_counts(), np.full((H, W), 4))  # a context that never adapted: all n
    one.close()

    options("streams", "4")
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=32)
    rc, msg = _adapt_status(lib, st)
    assert rc == -6 and "no sample" in msg, msg
    assert np.array_equal(st.sample_counts(), np.zeros((H, W)))
    st.trace_range(0, 6)
    rc, msg = _adapt_status(lib, st)
    assert rc == -6 and "6" in msg and "4" in msg and "multiple" in msg, msg
    assert "adaptive=" not in st.describe()
    st.trace_range(6, 8)
    assert st.adapt(1e3) == 0
    st.reset()
    # all tiles are active again and the sample counts follow n
    assert st.adaptive == (30, 30)
    rc, msg = _adapt_status(lib, st)
    assert rc == -6 and "no sample" in msg, msg
    st.trace_range(0, 8)
    assert st.counters()["paths"] == 8 * W * H
    assert np.array_equal(st.sample_counts(), np.full((H, W), 8))
    st.close()


# ---- 6. tile share ------------------------------------------------------------------------------
def test_tile_share_adapts_over_its_own_tiles(gpu, abi, lib, cornell_abi, options):
    """tile_share 2,1 at 44x36: the odd tiles only; the mask is indexed by image tile, M and N are
    the share's, the sample counts are 0 elsewhere (checked inside the helper)."""
    options("streams", "4")
    options("tile_share", "2,1")
    st, _, frozen, traced, got, _ = _adapt_and_continue(abi, lib, cornell_abi, "44x36 k=4 share 2,1", 8, 16, share=(2, 1),
                                                        width=W, height=H, samples=32)
    assert traced.sum() == 15 and frozen.any() and not (frozen | ~traced).all()
    assert (st.sample_counts()[~A.pixels_of(traced, H, W)] == 0).all()
    assert (got["image"][~A.pixels_of(traced, H, W)] == 0).all()
    st.close()


# ---- 7. jt_describe -----------------------------------------------------------------------------
def test_describe_reports_the_active_tiles(gpu, abi, lib, cornell_abi, options):
    options("streams", "4")
    st = _state(abi, lib, cornell_abi, width=W, height=H, samples=32)
    before = st.describe()
    assert "adaptive=" not in before and st.adaptive is None
    st.trace_range(0, 8)
    assert st.describe() == before
    a = st.adapt(0.5)
    assert st.describe() == f"{before} adaptive={a}/30"
    st.close()


# ---- 8. the CLI ---------------------------------------------------------------------------------
def test_cli_adaptive_traces_fewer_paths(gpu, tmp_path):
    """96x96, --batch 32 (k = 32), T = 0.2, a check every 32 samples, against the same without
    --adaptive. The simulation on the oracle at k = 32 (tests/test_adapt_host.py simulate) gives
    uniform: stop at 160 samples, 23 040 tile.samples; adaptive: stop at 224, 13 824 (0.60)."""
    from PIL import Image
    from jtrace import main

    def run(name, *extra):
        lines = []
        res = main.run(main.parse_cli_args(["--scene", CORNELL, "--width", "96", "--height", "96", "--batch", "32",
                                            "--traversal", "near", "--samples", "512", "--noise-target", "0.2",
                                            "--noise-interval", "32", "--output", str(tmp_path / name), *extra]),
                       out=lines.append)
        return lines, res

    ulines, uniform = run("uniform.png")
    alines, adaptive = run("adaptive.png", "--adaptive", "true", "--adaptive-start", "32",
                           "--samples-output", str(tmp_path / "counts.png"))
    shown = [s for s in alines if s.startswith("adaptive:")]
    print("\n".join(shown))
    print(f"uniform: {uniform['samples_traced']} samples, {uniform['paths']} paths, noise {uniform['noise']:.4f}; "
          f"adaptive: {adaptive['samples_traced']} samples, {adaptive['paths']} paths, noise {adaptive['noise']:.4f}, "
          f"{adaptive['active_tiles']} tiles active")
    assert uniform["noise"] <= 0.2 and adaptive["noise"] <= 0.2
    assert uniform["paths"] == 96 * 96 * uniform["samples_traced"] and "active_tiles" not in uniform
    assert adaptive["paths"] < uniform["paths"]
    assert shown and shown[0].endswith("/144 tiles active at 32 samples")
    assert not any(s.startswith("adaptive:") for s in ulines)
    assert adaptive["active_tiles"] == int(shown[-1].split()[1].split("/")[0])
    counts = np.asarray(Image.open(tmp_path / "counts.png"))
    assert counts.shape == np.asarray(Image.open(tmp_path / "adaptive.png")).shape == (96, 96, 4)
    assert (counts[..., 3] == 255).all() and counts[..., 0].max() == 255 and counts[..., 0].min() < 255
