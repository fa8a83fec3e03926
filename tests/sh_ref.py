"""What tests/test_sh_host.py (CPU) and tests/test_gpu_probe_sh.py share: the float64 restatement of
the sphere draw of jt_sphere_rays (include/jtrace.h), and the closed forms of the probe at the origin
of tests/irradiance_ref.py's square scene.

The square is the face y = 1 of the cube [-1, 1]^3 seen from its centre: solid angle 4 pi / 6, and
the integral of cos(theta) = d.y over it is pi * SQUARE_F (the form factor irradiance_ref.py states).
A sample that meets the black square has the target 0, one that escapes has L, so the mean of
target * Y_k is L * (the mean of Y_k over the sphere, 0 for k > 0 and c0 for k = 0, minus the face's
integral of Y_k over 4 pi)."""
import numpy as np

import irradiance_ref as IR

C0, C1, C2, C3, C4 = 0.282095, 0.488603, 1.092548, 0.315392, 0.546274
# the issue's figure: a coefficient's per-sample standard deviation is at most 0.28 L (the basis
# functions have the second moment 1 / 4 pi = 0.2821^2 over the sphere), so over the 65 536 samples
# of the square scene the standard error is 1.1e-3 L
SQUARE_SH_SE = 1.1e-3


def sphere_directions64(pairs):
    """sample_sphere of the float32 pairs (n, 2) restated in float64: (n, 3)."""
    u, v = pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64)
    z = 2.0 * v - 1.0
    r = np.sqrt(np.clip(1.0 - z * z, 0.0, 1.0))
    phi = 2.0 * np.pi * u
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def basis64(d):
    """Y_0 .. Y_8 in float64 with the library's six-digit constants: (n, 9)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * x * y, C2 * y * z, C3 * (3 * z * z - 1), C2 * x * z,
                     C4 * (x * x - y * y)], -1)


def square_face_integrals(n=2000):
    """The integral of Y_k over the solid angle of the face y = 1, |x|, |z| <= 1, by an n x n
    midpoint quadrature over the face: d omega = dx dz / r^3 with r^2 = x^2 + 1 + z^2. (9,)"""
    t = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    x, z = np.meshgrid(t, t, indexing="ij")
    r = np.sqrt(x * x + 1.0 + z * z)
    d = np.stack([x / r, 1.0 / r, z / r], -1)
    w = (2.0 / n) ** 2 / r ** 3
    return (basis64(d) * w[..., None]).sum((0, 1))


def square_expected(face=None):
    """The expected sh_k.rgb / L (9,) at the origin of the square scene with the environment
    visible, and the expected sh_k.a (9,) with it hidden (only the square covers)."""
    face = square_face_integrals() if face is None else face
    sky = np.zeros(9)
    sky[0] = C0
    return sky - face / (4.0 * np.pi), face / (4.0 * np.pi)


def square_hit(d):
    """The float64 ray-square test of irradiance_ref.square_hits on directions (n, 3): bool (n,)."""
    up = d[:, 1] > 0
    y = np.where(up, d[:, 1], 1.0)
    return up & (np.abs(d[:, 0] / y) <= 1) & (np.abs(d[:, 2] / y) <= 1)


def square_prediction(oracle, seed):
    """The means over the 64 x 1024 samples of (1 - hit) * Y_k and of hit * Y_k, from the oracle's
    first pairs, the float64 sphere draw and the float64 ray-square test: two (9,) arrays."""
    streams = np.arange(IR.SQUARE_POINTS)
    seen, covered = np.zeros(9), np.zeros(9)
    for s in range(IR.SQUARE_SAMPLES):
        d = sphere_directions64(IR.first_pairs(oracle, seed, streams, s))
        hit = square_hit(d)
        Y = basis64(d)
        seen += (Y * ~hit[:, None]).sum(0)
        covered += (Y * hit[:, None]).sum(0)
    n = IR.SQUARE_POINTS * IR.SQUARE_SAMPLES
    return seen / n, covered / n
