"""Numpy restatement of the error estimate (include/jtrace.h: jt_get_variance, jt_get_noise),
written from its definition: float32 operations in the stated order, the noise reduction in
float64. Input: the sample streams' means (k, H, W, 4) after n local samples, as the oracle
keeps them (oracle.trace(..., streams=k, parts=...)["img"]).

Local sample t belongs to stream t mod k, so after n samples stream j holds
n_j = (n - 1 - j) // k + 1 of them and ns = min(n, k) streams hold at least one."""
import numpy as np

F = np.float32


def stream_weights(n: int, k: int) -> np.ndarray:
    """w_j = (float)((double)n_j / n) for the ns = min(n, k) streams that hold a sample."""
    ns = min(n, k)
    return np.array([F(np.float64((n - 1 - j) // k + 1) / np.float64(n)) for j in range(ns)], F)


def combine(means: np.ndarray, n: int, k: int) -> np.ndarray:
    """The image the library combines from the means: m_0 * w_0, then + m_j * w_j in stream order."""
    means = np.asarray(means, F)
    assert means.shape[0] == k
    w = stream_weights(n, k)
    mu = means[0] * w[0]
    for j in range(1, len(w)):
        mu = mu + means[j] * w[j]
    return mu


def variance(means: np.ndarray, n: int, k: int, mu: np.ndarray | None = None) -> np.ndarray:
    """Per channel: acc = 0; for j in order: d = m_j - mu; acc = acc + (d * d) * w_j;
    var = acc / (float)(ns - 1). mu None: the combined image."""
    means = np.asarray(means, F)
    ns = min(n, k)
    if ns < 2:
        raise ValueError("fewer than two streams hold a sample")
    w = stream_weights(n, k)
    mu = combine(means, n, k) if mu is None else np.asarray(mu, F)
    acc = np.zeros_like(mu)
    for j in range(ns):
        d = means[j] - mu
        acc = acc + (d * d) * w[j]
    return acc / F(ns - 1)


def noise(var: np.ndarray, mu: np.ndarray, mask: np.ndarray | None = None) -> float:
    """sqrt(3 N V) / M over the pixels of `mask` (all when None), in float64: V the sum of
    (var.x + var.y) + var.z, M that of (mu.x + mu.y) + mu.z (both per pixel in float32), N the
    number of pixels; 0 when M == 0."""
    var, mu = np.asarray(var, F), np.asarray(mu, F)
    v = (var[..., 0] + var[..., 1]) + var[..., 2]
    m = (mu[..., 0] + mu[..., 1]) + mu[..., 2]
    if mask is not None:
        v, m = v[mask], m[mask]
    V, M, N = float(np.sum(v, dtype=np.float64)), float(np.sum(m, dtype=np.float64)), v.size
    return 0.0 if M == 0 else float(np.sqrt(3.0 * N * V) / M)
