"""Adaptive sampling without a device: the restatement of the freeze rule (tests/adapt_ref.py) on
hand-made variances, the argument checks of jt_adapt / jt_get_sample_counts, the CLI's flags, and
the simulation of the whole loop on the oracle's stream means."""
import ctypes as C

import numpy as np
import pytest

import adapt_ref as A
import error_ref as R
from conftest import make_params

F = np.float32


# ---- the restatement ----------------------------------------------------------------------------
def _var(h, w, value=0.0):
    v = np.zeros((h, w, 4), F)
    v[..., :3] = value
    return v


def test_restatement_on_a_partial_tile_image():
    """12x10: 2x2 tiles, the right column 4 wide, the bottom row 2 high. Tile (0, 0) noisy, the
    rest quiet; N_t counts only the pixels inside the image."""
    h, w = 10, 12
    var, mu = _var(h, w, 1e-6), np.ones((h, w, 4), F)
    var[:8, :8, :3] = 1e-2
    V, N = A.tile_stats(var)
    assert N.tolist() == [[64, 32], [16, 8]]
    assert V[0, 1] == F(32) * (F(1e-6) + F(1e-6) + F(1e-6))  # 32 equal values: every partial sum is exact
    M, Npix = A.image_sums(mu)
    assert (M, Npix) == (3.0 * h * w, h * w)
    # T = 0.01: vmax = (0.01 * 3)^2 / 3 = 3e-4 per pixel: the quiet tiles (3e-6) freeze, the noisy (3e-2) not
    assert A.vmax(0.01, M, Npix) == F((0.01 * M) * (0.01 * M) / (3.0 * Npix * Npix))
    frozen = A.freeze(var, mu, 0.01)
    assert frozen.tolist() == [[False, True], [True, True]]
    # monotone: an earlier mask stays, whatever the variance says now
    assert A.freeze(var, mu, 1e-6, frozen=frozen).tolist() == frozen.tolist()
    assert A.freeze(var, mu, 1.0).all()
    # a tile share: only its own tiles freeze, and M, N are its own
    share = A.share_mask(h, w, 2, 1)
    assert share.tolist() == [[False, True], [False, True]]
    assert A.image_sums(mu, share) == (3.0 * 40, 40)
    assert A.freeze(var, mu, 0.01, traced=share).tolist() == [[False, True], [False, True]]
    assert A.pixels_of(frozen, h, w).sum() == 32 + 16 + 8


def test_zero_variance_and_black_images_freeze():
    h, w = 16, 16
    var, mu = _var(h, w, 1e-3), np.ones((h, w, 4), F)
    var[8:, 8:] = 0
    assert A.freeze(var, mu, 1e-12).tolist() == [[False, False], [False, True]]  # zero variance: at any T
    # M = 0: vmax = 0, and a black image's variance is 0 too: all freeze
    assert A.vmax(0.5, 0.0, h * w) == 0
    assert A.freeze(_var(h, w), np.zeros((h, w, 4), F), 0.5).all()


def test_the_tree_order_matters():
    """2^24 in lane 0, 1 in lanes 1 and 33: the tree pairs the two ones into 2 (lane 1 += lane
    33) before they meet 2^24, giving 2^24 + 2; left to right each 1 is added to 2^24 alone and
    rounds away (ties to even), giving 2^24."""
    v = np.zeros(64, F)
    v[0], v[1], v[33] = 2.0 ** 24, 1.0, 1.0
    left = F(0)
    for x in v:
        left = F(left + x)
    tree = A.tree_sum(v)
    assert tree == F(2.0 ** 24 + 2) and left == F(2.0 ** 24) and tree != left
    # and the rule sees it: a threshold between the two sums freezes under one order only
    var = np.zeros((8, 8, 4), F)
    var[..., 0] = v.reshape(8, 8)
    V, N = A.tile_stats(var)
    assert V[0, 0] == tree
    vm = F(2.0 ** 18)  # N_t * vmax = 2^24: left-to-right would meet it, the tree sum does not
    assert not A.meets(V, N, vm)[0, 0] and left <= F(64) * vm


def test_all_frozen_in_one_call_means_the_target_is_met():
    """If every tile meets its threshold at one call, noise <= T: summed over the tiles the rule
    is 3 N V <= (T M)^2. Margin 1e-5: two orders above the float32 roundings involved (vmax's
    6e-8, the sums' 3.6e-8)."""
    rng = np.random.default_rng(7)
    h, w = 44, 36
    mu = rng.uniform(0.1, 1.0, (h, w, 4)).astype(F)
    var = (rng.uniform(0.0, 1.0, (h, w, 4)) ** 4 * 1e-3).astype(F)
    V, N = A.tile_stats(var)
    M, Npix = A.image_sums(mu)
    # the smallest T in a bracket at which every tile freezes
    lo, hi = 0.0, 10.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if A.meets(V, N, A.vmax(mid, M, Npix)).all() else (mid, hi)
    assert A.freeze(var, mu, hi).all() and not A.freeze(var, mu, lo * (1 - 1e-6)).all()
    noise = R.noise(var, mu)
    print(f"smallest all-freezing T {hi:.8g}, noise {noise:.8g}")
    assert noise <= hi * (1 + 1e-5)


def test_implied_image():
    renders = {n: np.full((10, 12, 4), n, F) for n in (8, 16, 24)}
    at = np.array([[8, 0], [16, 0]])
    img = A.implied(at, renders, 24)
    assert (img[:8, :8] == 8).all() and (img[8:, :8] == 16).all() and (img[:, 8:] == 24).all()


# ---- the ABI's argument checks ------------------------------------------------------------------
def test_bad_arguments_are_reported_without_a_device(lib):
    """JT_ERR_INVALID naming the argument, before the context is looked at: the non-NULL ctx below
    is never dereferenced."""
    n = C.c_int32()
    buf = (C.c_int32 * 4)()
    not_a_ctx = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert lib.jt_adapt(None, 0.1, C.byref(n)) == -1 and b"ctx" in lib.jt_last_error()
    for bad in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        assert lib.jt_adapt(not_a_ctx, bad, C.byref(n)) == -1 and b"noise_target" in lib.jt_last_error(), bad
        assert lib.jt_adapt(not_a_ctx, bad, None) == -1 and b"noise_target" in lib.jt_last_error(), bad
    assert lib.jt_get_sample_counts(None, buf) == -1 and b"ctx" in lib.jt_last_error()
    assert lib.jt_get_sample_counts(not_a_ctx, None) == -1 and b"counts" in lib.jt_last_error()


def test_symbols_are_declared(abi):
    assert "jt_adapt" in abi.EXPORTED_SYMBOLS and "jt_get_sample_counts" in abi.EXPORTED_SYMBOLS


# ---- the CLI ------------------------------------------------------------------------------------
def test_cli_flags(capsys):
    from jtrace import cli
    p = cli.parse_cli_args(["--scene", "x.json"])
    assert (p.adaptive, p.adaptive_start, p.samples_output) == (False, 64, "")
    assert p == cli.Params(scene="x.json")  # the defaults are Params' own: nothing else moved
    p = cli.parse_cli_args(["--scene", "x", "--batch", "32", "--noise-target", "0.2", "--adaptive", "true",
                            "--adaptive-start", "32", "--samples-output", "n.png"])
    assert (p.adaptive, p.adaptive_start, p.samples_output, p.noise_target) == (True, 32, "n.png", 0.2)
    # the start alone changes nothing and needs no target; --adaptive false neither
    assert cli.parse_cli_args(["--scene", "x", "--adaptive-start", "8"]).adaptive is False
    assert cli.parse_cli_args(["--scene", "x", "--adaptive", "false"]).adaptive is False

    def rejected(*args):
        with pytest.raises(SystemExit) as e:
            cli.parse_cli_args(["--scene", "x", *args])
        assert e.value.code == 2
        return capsys.readouterr().err

    msg = rejected("--adaptive", "true", "--batch", "8")
    assert "--adaptive" in msg and "--noise-target" in msg
    msg = rejected("--adaptive", "true", "--noise-target", "0", "--batch", "8")
    assert "--adaptive" in msg and "--noise-target" in msg
    # with the target, the target's own rules apply
    msg = rejected("--adaptive", "true", "--noise-target", "0.1", "--batch", "1")
    assert "--noise-target" in msg and "--batch 2" in msg
    msg = rejected("--adaptive", "true", "--noise-target", "0.1", "--batch", "8", "--devices", "2")
    assert "--noise-target" in msg and "--devices 1" in msg
    assert "--adaptive-start" in rejected("--adaptive-start", "-1")


# ---- the simulation -----------------------------------------------------------------------------
def simulate(abi, oracle, sa, w, h, k, T, step, limit, sampler=1, seed=0x5EED):
    """Uniform against adaptive sampling on the oracle's stream means, a check every `step`
    samples from `step` (a multiple of k): both stop at the first check with noise <= T, the
    adaptive loop freezing tiles (adapt_ref.freeze) at every check that does not stop it, a
    frozen tile keeping the stream means it had. Returns per loop (samples at stop, noise there,
    tile.samples spent) and the adaptive loop's frozen tile count."""
    assert step % k == 0
    p = make_params(abi, width=w, height=h, samples=limit, sampler=sampler, seed=seed)
    bvh, lights = oracle.build_bvh(sa), oracle.make_lights(sa)
    ty, tx = A.tile_grid(h, w)
    parts, uniform, adaptive = {}, None, None
    held = None                               # the adaptive loop's stream means
    frozen_at = np.zeros((ty, tx), np.int64)  # 0: active
    for n in range(step, limit + 1, step):
        oracle.trace(sa, bvh, lights, p, w, h, n - step, n, streams=k, parts=parts)
        means = parts["img"]
        if uniform is None:
            noise = R.noise(R.variance(means, n, k), R.combine(means, n, k))
            if noise <= T:
                uniform = (n, noise, ty * tx * n)
        if adaptive is None:
            px = A.pixels_of(frozen_at > 0, h, w)
            held = means.copy() if held is None else np.where(px[None, ..., None], held, means)
            mu = R.combine(held, n, k)
            var = R.variance(held, n, k, mu)
            noise = R.noise(var, mu)
            if noise <= T:
                adaptive = (n, noise, int(np.where(frozen_at > 0, frozen_at, n).sum()))
            else:
                frozen_at[A.freeze(var, mu, T, frozen=frozen_at > 0) & (frozen_at == 0)] = n
        if uniform and adaptive:
            break
    return uniform, adaptive, int((frozen_at > 0).sum())


def test_simulation_adaptive_needs_fewer_tile_samples(abi, oracle, cornell_abi):
    """Cornellbox 96x96, k = 16, T = 0.2, a check every 32 samples from 32. Measured with a
    coarser schedule: 14 432 tile.samples against about 23 000; with this schedule see the print."""
    uniform, adaptive, nfrozen = simulate(abi, oracle, cornell_abi, 96, 96, 16, 0.2, 32, 1024)
    print(f"uniform: stop at {uniform[0]} samples, noise {uniform[1]:.4f}, {uniform[2]} tile.samples; "
          f"adaptive: stop at {adaptive[0]}, noise {adaptive[1]:.4f}, {adaptive[2]} tile.samples, "
          f"{nfrozen}/144 tiles frozen")
    assert uniform is not None and adaptive is not None
    assert uniform[1] <= 0.2 and adaptive[1] <= 0.2
    assert adaptive[2] < uniform[2]
