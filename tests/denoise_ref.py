"""numpy restatement of the denoiser's definition (include/jtrace.h): the
edge-avoiding a-trous wavelet filter on albedo-demodulated radiance. Written from the definition,
not from the kernel; float64 unless another dtype is asked for. Also the seeded synthetic inputs
the CPU and GPU tests share."""
import numpy as np

KERNEL = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)

# jt_denoise_defaults
DEFAULTS = dict(iterations=5, sigma_normal=0.3, sigma_albedo=0.1, albedo_floor=0.01)


def defaults(samples):
    d = dict(DEFAULTS)
    d["sigma_color"] = float(np.float32(8) / np.sqrt(np.float32(max(samples, 1))))
    return d


def denoise(rgba, albedo, normal, iterations, sigma_color, sigma_normal, sigma_albedo, albedo_floor, dtype=np.float64):
    """(H, W, 4), (H, W, 3), (H, W, 3) -> (H, W, 4) of `dtype`."""
    T = np.dtype(dtype).type
    c = np.asarray(rgba).astype(dtype)
    a = np.asarray(albedo).astype(dtype)
    n = np.asarray(normal).astype(dtype)
    H, W = c.shape[:2]
    m = np.maximum(a, T(albedo_floor))
    d = c[..., :3] / m
    sn2 = T(sigma_normal) * T(sigma_normal)
    sa2 = T(sigma_albedo) * T(sigma_albedo)
    for i in range(iterations):
        s = 1 << i
        sc = T(sigma_color) / T(s)
        sc2 = sc * sc
        num = np.zeros((H, W, 3), dtype)
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
                e = (((d[P] - d[Q]) ** 2).sum(-1) / sc2 + ((n[P] - n[Q]) ** 2).sum(-1) / sn2
                     + ((a[P] - a[Q]) ** 2).sum(-1) / sa2)
                w = T(KERNEL[dy + 2]) * T(KERNEL[dx + 2]) * np.exp(-e)
                num[P] += w[..., None] * d[Q]
                den[P] += w
        d = num / den[..., None]
    out = np.empty((H, W, 4), dtype)
    out[..., :3] = d * m
    out[..., 3] = c[..., 3]
    return out


def rel_error(got, ref):
    """Per channel |got - ref| / max(|got|, |ref|, 1e-6), as conftest.compare_images scales it."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.maximum(np.abs(got), np.abs(ref)), 1e-6)


# H x W: 1x1, 2x3, 5x7 are smaller than the 5 x 5 window; 19x37 is no multiple of a tile; at 20x20
# every tap of steps 8 and 16 but the centre row and column's falls outside; 45x70 and 33x130 span
# several workgroups and more than one wave per row
SHAPES = [(1, 1), (2, 3), (5, 7), (19, 37), (20, 20), (45, 70), (33, 130)]
ITERATIONS = [1, 5, 8]
# a colour sigma at which the step-16 taps still carry weight on the 45x70 input
# (tests/test_denoise_host.py::test_late_iterations_carry_weight)
WIDE_SIGMA_COLOR = 64.0


def synthetic(H, W):
    """Seeded guides and radiance: albedo and normal piecewise constant over three regions (one
    region's albedo below the floor, a channel exactly 0), normals with +-0.02 jitter, strictly
    positive irradiance 0.5 + gamma(2, 0.5), alpha 0 on a tenth of the pixels."""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:H, 0:W]
    region = np.where(x * 3 < W, 0, np.where((x + y) * 2 < W + H, 1, 2))
    alb = np.array([[0.7, 0.2, 0.1], [0.005, 0.0, 0.008], [0.3, 0.6, 0.9]], np.float32)[region]
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], np.float32)[region]
    nrm = (nrm + rng.uniform(-0.02, 0.02, (H, W, 3))).astype(np.float32)
    irr = (0.5 + rng.gamma(2.0, 0.5, (H, W, 3))).astype(np.float32)
    rgba = np.empty((H, W, 4), np.float32)
    rgba[..., :3] = irr * alb
    rgba[..., 3] = (rng.uniform(size=(H, W)) >= 0.1).astype(np.float32)
    return rgba, np.ascontiguousarray(alb), nrm


def parameter_sets(H, W):
    """The parameter sets a shape runs with: the defaults for 16 samples at 1, 5 and 8 iterations,
    and for 45x70 also the wide colour sigma."""
    sets = [dict(defaults(16), iterations=it) for it in ITERATIONS]
    if (H, W) == (45, 70):
        sets += [dict(defaults(16), iterations=it, sigma_color=WIDE_SIGMA_COLOR) for it in ITERATIONS]
    return sets
