"""The real spherical harmonics of bands 0..2 that jt_probe_sh projects onto (include/jtrace.h;
csrc/jt_sh.h), and what a caller does with a probe's coefficients. numpy only.

sh_basis restates csrc/jt_sh.h in float32, every operation rounded, in the same association, so its
values have the kernel's bits (tests/sh_check.cpp compares the two). The coefficient order is
Y0 | Y1 (y) Y2 (z) Y3 (x) | Y4 (xy) Y5 (yz) Y6 (3 z z - 1) Y7 (xz) Y8 (x x - y y)."""
import numpy as np

F32 = np.float32
C0, C1, C2, C3, C4 = F32(0.282095), F32(0.488603), F32(1.092548), F32(0.315392), F32(0.546274)
SH_COEFFS = 9
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
# the cosine lobe's zonal factors per band: E(n) = sum_k A[band k] L_k Y_k(n)
COSINE_LOBE = np.array([np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0])


def sh_basis(d) -> np.ndarray:
    """Y_0 .. Y_8 at the unit directions d (..., 3): (..., 9) float32, in csrc/jt_sh.h's bits."""
    d = np.asarray(d, F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty(d.shape[:-1] + (SH_COEFFS,), F32)
    out[..., 0] = C0
    out[..., 1] = C1 * y
    out[..., 2] = C1 * z
    out[..., 3] = C1 * x
    out[..., 4] = C2 * (x * y)
    out[..., 5] = C2 * (y * z)
    out[..., 6] = C3 * (F32(3.0) * (z * z) - F32(1.0))
    out[..., 7] = C2 * (x * z)
    out[..., 8] = C4 * (x * x - y * y)
    return out


def sh_fold(acc, target, basis, count: int) -> np.ndarray:
    """One step of jt_probe_sh's running mean in float32: acc (n, 9, 4) after `count` samples, the
    next sample's rgba target (n, 4) and sh_basis of its direction (n, 9). The first step
    (count = 0, acc = 0) is 0 * 0 + v * 1, which turns a product of -0 into +0."""
    acc, target, basis = np.asarray(acc, F32), np.asarray(target, F32), np.asarray(basis, F32)
    w = F32(1) / F32(count + 1)
    v = target[:, None, :] * basis[:, :, None]
    return acc * (F32(1) - w) + v * w


def sh_radiance(sh) -> np.ndarray:
    """The radiance field's SH coefficients of probes (..., 9, 4) as jt_probe_sh returns them: the
    sample directions have the pdf 1 / (4 pi), so L_k = 4 pi rgb: (..., 9, 3) float32."""
    sh = np.asarray(sh, F32)
    return (F32(4.0 * np.pi) * sh[..., :3]).astype(F32)


def sh_irradiance(sh, normals) -> np.ndarray:
    """The irradiance about the unit normals (n, 3) at probes (n, 9, 4), or at one probe (9, 4) for
    every normal: E(n) = sum_k A_l(k) L_k Y_k(n), A = pi, 2 pi / 3, pi / 4: (n, 3) float64."""
    L = sh_radiance(sh).astype(np.float64)
    Y = sh_basis(normals).astype(np.float64)
    return np.einsum("...k,...kc->...c", Y * COSINE_LOBE[BAND], L)
