"""The error estimate without a device: the restatement (tests/error_ref.py) against the
oracle's sample streams, its calibration against the spread of independent renders, the
argument checks of jt_get_variance / jt_get_noise and the CLI's flags."""
import ctypes as C

import numpy as np
import pytest

import error_ref as R
from conftest import make_params


def _streams(abi, oracle, sa, w, h, k, n, sampler=1, seed=0x5EED):
    """(stream means (k, h, w, 4), the oracle's combined image) after samples [0, n)."""
    p = make_params(abi, width=w, height=h, samples=n, sampler=sampler, seed=seed)
    parts = {}
    img = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), p, w, h, 0, n, streams=k, parts=parts)[0]
    return parts["img"], img


@pytest.mark.parametrize("w,h,k,n", [(44, 36, 4, 6), (32, 32, 16, 32)])
def test_restated_combine_is_the_oracle_image(abi, oracle, cornell_abi, w, h, k, n):
    """The weights n_j / n and the stream order of the restatement are the library's: the image
    recombined from the oracle's stream means equals the oracle's bit for bit."""
    means, img = _streams(abi, oracle, cornell_abi, w, h, k, n)
    assert np.array_equal(R.combine(means, n, k).view(np.uint32), img.view(np.uint32))
    assert abs(float(R.stream_weights(n, k).astype(np.float64).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("sampler", [1, 2], ids=["path", "naive"])
def test_estimator_is_calibrated(abi, oracle, cornell_abi, sampler):
    """32x32, k = 16, 32 spp, seeds 1000..1023: the estimated variance of the mean, averaged over
    the seeds and summed over pixels and rgb, against the empirical variance of the image over the
    same seeds. Measured 1.000 (path) and 0.998 (naive); one seed spreads about +-0.1, the mean of
    24 about +-0.02, so [0.9, 1.1] is more than 4 sigma wide."""
    k, n = 16, 32
    est, imgs = [], []
    for seed in range(1000, 1024):
        means, img = _streams(abi, oracle, cornell_abi, 32, 32, k, n, sampler=sampler, seed=seed)
        est.append(R.variance(means, n, k, img)[..., :3].astype(np.float64))
        imgs.append(img[..., :3].astype(np.float64))
    estimated = np.mean(est, axis=0).sum()
    empirical = np.var(np.stack(imgs), axis=0, ddof=1).sum()
    ratio = estimated / empirical
    singles = [e.sum() / empirical for e in est]
    print(f"sampler {sampler}: estimated / empirical variance {ratio:.4f}; single seeds {min(singles):.3f} .. {max(singles):.3f}")
    assert 0.9 <= ratio <= 1.1, ratio


def test_restatement_basics():
    """Two equal streams: zero variance; a known spread: the weighted formula; noise of it."""
    m = np.zeros((2, 1, 2, 4), np.float32)
    m[0, 0, 0], m[1, 0, 0] = 1.0, 3.0  # n = 2: mu = 2, var = ((1 * 0.5) + (1 * 0.5)) / 1 = 1
    m[:, 0, 1] = 0.5
    var = R.variance(m, 2, 2)
    assert np.array_equal(var[0, 0], np.ones(4, np.float32)) and np.array_equal(var[0, 1], np.zeros(4, np.float32))
    mu = R.combine(m, 2, 2)
    assert R.noise(var, mu) == pytest.approx(np.sqrt(3 * 2 * 3.0) / 7.5)
    assert R.noise(var, np.zeros_like(mu)) == 0.0
    with pytest.raises(ValueError):
        R.variance(m, 1, 2)
    # n = 6 over k = 4: streams 0 and 1 hold two samples, 2 and 3 one
    assert np.array_equal(R.stream_weights(6, 4), np.array([2 / 6, 2 / 6, 1 / 6, 1 / 6], np.float32))
    assert len(R.stream_weights(3, 4)) == 3


def test_null_arguments_are_reported_without_a_device(lib):
    """JT_ERR_INVALID naming the argument, before the context is looked at: the non-NULL ctx below
    is never dereferenced."""
    buf = (C.c_float * 4)()
    val = C.c_double()
    not_a_ctx = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert lib.jt_get_variance(None, buf) == -1 and b"ctx" in lib.jt_last_error()
    assert lib.jt_get_noise(None, C.byref(val)) == -1 and b"ctx" in lib.jt_last_error()
    assert lib.jt_get_variance(not_a_ctx, None) == -1 and b"var_rgba" in lib.jt_last_error()
    assert lib.jt_get_noise(not_a_ctx, None) == -1 and b"noise" in lib.jt_last_error()


def test_cli_flags(capsys):
    from jtrace import cli
    p = cli.parse_cli_args(["--scene", "x.json"])
    assert (p.noise_target, p.noise_interval, p.error_output) == (0.0, 16, "")
    assert p == cli.Params(scene="x.json")  # the defaults are Params' own: nothing else moved
    p = cli.parse_cli_args(["--scene", "x", "--batch", "8", "--noise-target", "0.25", "--noise-interval", "4",
                            "--error-output", "err.png"])
    assert (p.noise_target, p.noise_interval, p.error_output, p.batch) == (0.25, 4, "err.png", 8)
    # the interval alone changes nothing and needs no streams
    assert cli.parse_cli_args(["--scene", "x", "--noise-interval", "4"]).noise_target == 0.0

    def rejected(*args):
        with pytest.raises(SystemExit) as e:
            cli.parse_cli_args(["--scene", "x", *args])
        assert e.value.code == 2
        return capsys.readouterr().err

    msg = rejected("--noise-target", "0.1", "--batch", "1")
    assert "--noise-target" in msg and "--batch 2" in msg
    msg = rejected("--noise-target", "0.1")  # the reference's default batch is 1
    assert "--noise-target" in msg and "--batch" in msg
    msg = rejected("--noise-target", "0.1", "--batch", "8", "--devices", "2")
    assert "--noise-target" in msg and "--devices 1" in msg
    assert "--noise-target" in rejected("--noise-target", "-0.5", "--batch", "8")
    assert "--noise-interval" in rejected("--noise-interval", "0")
    msg = rejected("--error-output", "e.png", "--batch", "1")
    assert "--error-output" in msg and "--batch 2" in msg
    msg = rejected("--error-output", "e.png", "--batch", "4", "--devices", "2")
    assert "--error-output" in msg and "--devices 1" in msg
