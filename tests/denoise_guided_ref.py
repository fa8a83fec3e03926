"""numpy restatement of the variance-guided denoiser's definition (include/jtrace.h
jt_denoise_guided): the a-trous filter of tests/denoise_ref.py with the colour
tolerance of a tap taken from the two pixels' own variance, which is carried through the
iterations. Written from the definition, not from the kernel; float64 unless another dtype is
asked for. Also the seeded synthetic variance the CPU and GPU tests share; the radiance, the
guides, the shapes and the error measure are those of tests/denoise_ref.py."""
import numpy as np

from denoise_ref import KERNEL, SHAPES, rel_error, synthetic  # noqa: F401  (shared with the tests)

# jt_denoise_guided_defaults
DEFAULTS = dict(iterations=5, sigma_variance=2.0, sigma_normal=0.3, sigma_albedo=0.1, albedo_floor=0.01,
                variance_floor=1e-10)
FIELDS = tuple(DEFAULTS)

ITERATIONS = [1, 5, 8]
SIGMA_VARIANCES = [2.0, 8.0]


def parameter_sets():
    """The grid every shape runs with: the defaults at 1, 5 and 8 iterations, sigma_variance 2 and 8."""
    return [dict(DEFAULTS, iterations=it, sigma_variance=sv) for it in ITERATIONS for sv in SIGMA_VARIANCES]


def denoise_guided(rgba, variance, albedo, normal, iterations, sigma_variance, sigma_normal, sigma_albedo, albedo_floor,
                   variance_floor, dtype=np.float64, return_variance=False):
    """(H, W, 4), (H, W, 4), (H, W, 3), (H, W, 3) -> (H, W, 4) of `dtype` (and V_I, (H, W), of
    demodulated radiance, when asked for)."""
    T = np.dtype(dtype).type
    c = np.asarray(rgba).astype(dtype)
    v = np.asarray(variance).astype(dtype)
    a = np.asarray(albedo).astype(dtype)
    n = np.asarray(normal).astype(dtype)
    H, W = c.shape[:2]
    m = np.maximum(a, T(albedo_floor))
    d = c[..., :3] / m
    u = v[..., :3] / (m * m)
    V = (u[..., 0] + u[..., 1]) + u[..., 2]
    sv2 = T(sigma_variance) * T(sigma_variance)
    sn2 = T(sigma_normal) * T(sigma_normal)
    sa2 = T(sigma_albedo) * T(sigma_albedo)
    for i in range(iterations):
        s = 1 << i
        num = np.zeros((H, W, 3), dtype)
        vnum = np.zeros((H, W), dtype)
        den = np.zeros((H, W), dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # pixels p whose tap q = p + (ox, oy) lies inside the image
                y0, y1 = max(0, -oy), min(H, H - oy)
                x0, x1 = max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                e = (((d[P] - d[Q]) ** 2).sum(-1) / (sv2 * np.maximum(V[P] + V[Q], T(variance_floor)))
                     + ((n[P] - n[Q]) ** 2).sum(-1) / sn2 + ((a[P] - a[Q]) ** 2).sum(-1) / sa2)
                w = T(KERNEL[dy + 2]) * T(KERNEL[dx + 2]) * np.exp(-e)
                num[P] += w[..., None] * d[Q]
                vnum[P] += (w * w) * V[Q]
                den[P] += w
        d = num / den[..., None]
        V = vnum / (den * den)
    out = np.empty((H, W, 4), dtype)
    out[..., :3] = d * m
    out[..., 3] = c[..., 3]
    return (out, V) if return_variance else out


def synthetic_variance(rgba, H, W):
    """Seeded variance of the mean for denoise_ref.synthetic(H, W)'s radiance: a relative standard
    error gamma(2, 0.15) per channel, var.rgb = (rgba.rgb * that)^2, exactly 0 on about a tenth
    of the pixels (the variance floor is exercised), var.a = 0.25 (an alpha leak would show)."""
    rng = np.random.default_rng(2)
    rgba = np.asarray(rgba, np.float32)
    assert rgba.shape == (H, W, 4)
    var = np.empty((H, W, 4), np.float32)
    var[..., :3] = (rgba[..., :3] * rng.gamma(2.0, 0.15, (H, W, 3)).astype(np.float32)) ** 2
    var[rng.uniform(size=(H, W)) < 0.1, :3] = 0.0
    var[..., 3] = 0.25
    return var
