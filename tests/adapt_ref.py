"""Numpy restatement of adaptive sampling's freeze rule (include/jtrace.h: jt_adapt), written from
its definition: the threshold in float64 rounded once, the per-tile sum as the halving tree in
float32, the compare in float32. Inputs are the variance and image as jt_get_variance and
jt_get_image return them, (H, W, 4) float32.

Tiles are 8x8, numbered row-major over the image; lane l = 8 * row + col is pixel (col, row) of
its tile. `traced` is a bool mask over the tiles (ty, tx) a context traces (a tile share): None
means all."""
import numpy as np

F = np.float32


def tile_grid(h: int, w: int):
    return (h + 7) // 8, (w + 7) // 8


def pixel_tiles(h: int, w: int) -> np.ndarray:
    """(H, W) int: the image tile of every pixel."""
    j, i = np.mgrid[0:h, 0:w]
    return (j // 8) * ((w + 7) // 8) + i // 8


def share_mask(h: int, w: int, stride: int = 1, offset: int = 0) -> np.ndarray:
    """(ty, tx) bool: the tiles offset, offset + stride, ... of a tile share."""
    ty, tx = tile_grid(h, w)
    t = np.arange(ty * tx).reshape(ty, tx)
    return (t >= offset) & ((t - offset) % stride == 0)


def vmax(T: float, M: float, N: int) -> np.float32:
    """(float)((T * M) * (T * M) / (3.0 * N * N)) in double, rounded once."""
    T, M, N = np.float64(T), np.float64(M), np.float64(N)
    return F((T * M) * (T * M) / (np.float64(3.0) * N * N))


def tree_sum(v: np.ndarray) -> np.float32:
    """for off = 32, 16, ..., 1: v[l] += v[l + off]; lane 0. v: 64 float32."""
    v = np.asarray(v, F).copy()
    assert v.shape == (64,)
    off = 32
    while off > 0:
        v[:off] = v[:off] + v[off:2 * off]
        off >>= 1
    return v[0]


def tile_stats(var: np.ndarray):
    """(V_t (ty, tx) float32, N_t (ty, tx) int): the tree sum of (var.x + var.y) + var.z over each
    tile's lanes, 0 for a lane outside the image, and the tile's pixels inside the image."""
    var = np.asarray(var, F)
    h, w = var.shape[:2]
    ty, tx = tile_grid(h, w)
    v = np.zeros((ty * 8, tx * 8), F)
    v[:h, :w] = (var[..., 0] + var[..., 1]) + var[..., 2]
    inside = np.zeros((ty * 8, tx * 8), bool)
    inside[:h, :w] = True
    V = np.zeros((ty, tx), F)
    N = np.zeros((ty, tx), np.int64)
    for a in range(ty):
        for b in range(tx):
            V[a, b] = tree_sum(v[a * 8:a * 8 + 8, b * 8:b * 8 + 8].reshape(64))
            N[a, b] = inside[a * 8:a * 8 + 8, b * 8:b * 8 + 8].sum()
    return V, N


def image_sums(mu: np.ndarray, traced: np.ndarray | None = None):
    """(M, N): M the float64 sum of (mu.x + mu.y) + mu.z (per pixel in float32) over the traced
    pixels, N their number."""
    mu = np.asarray(mu, F)
    h, w = mu.shape[:2]
    m = (mu[..., 0] + mu[..., 1]) + mu[..., 2]
    if traced is not None:
        m = m[traced.reshape(-1)[pixel_tiles(h, w)]]
    return float(np.sum(m, dtype=np.float64)), int(m.size)


def meets(V: np.ndarray, N: np.ndarray, vm) -> np.ndarray:
    """V_t <= (float)N_t * vmax, in float32."""
    return np.asarray(V, F) <= N.astype(F) * F(vm)


def freeze(var, mu, T: float, frozen: np.ndarray | None = None, traced: np.ndarray | None = None) -> np.ndarray:
    """One jt_adapt(T): the (ty, tx) bool mask of frozen tiles after the call. frozen: the mask
    before it (monotone: those stay); traced: the context's tiles."""
    V, N = tile_stats(var)
    M, Npix = image_sums(mu, traced)
    out = meets(V, N, vmax(T, M, Npix) if Npix else F(0))
    if traced is not None:
        out &= traced
    if frozen is not None:
        out |= frozen
    return out


def pixels_of(tile_mask: np.ndarray, h: int, w: int) -> np.ndarray:
    """(H, W) bool: the pixels of the tiles of a (ty, tx) mask."""
    return np.asarray(tile_mask).reshape(-1)[pixel_tiles(h, w)]


def implied(frozen_at: np.ndarray, renders: dict, n: int) -> np.ndarray:
    """The array an adapted context holds at n samples, from full renders: pixels are independent,
    so it is where(frozen pixel, render at its freeze count, render at n). frozen_at: (ty, tx)
    int, 0 for an active tile; renders: {count: array (H, W[, C])}."""
    out = np.array(renders[n])
    h, w = out.shape[:2]
    for m in np.unique(frozen_at):
        if m:
            px = pixels_of(frozen_at == m, h, w)
            out[px] = renders[int(m)][px]
    return out
