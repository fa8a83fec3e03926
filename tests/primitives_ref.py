"""Single-primitive tests: the probe libraries' bindings, the seeded input sets and the float64
references (tests/test_primitives_host.py on the CPU, tests/test_gpu_primitives.py on the GPU).

The references are written from the textbook definitions and DESIGN.md §3 (the float contract),
not from the device headers or the oracle: IEEE 754-2019 minimum/maximum, the slab rule with its
double compare, Moller-Trumbore, the dielectric and conductor Fresnel equations, the GGX
distribution and Smith G1, the Henyey-Greenstein phase function, exp(-sigma d).
Every input set has an odd length (a lane count that fills no block), is seeded, and is the same
array for the CPU and the GPU tests.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import itertools
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PROBE_LIB = ROOT / "julia-raytracer_amd" / "build" / "libjt_probe.so"

F32 = np.float32
PIF = F32(np.pi)                      # Float32(pi)
TWO_PIF = F32(2) * PIF                # exact: a power-of-two multiple
MIN_ROUGHNESS = F32(0.03) * F32(0.03)
EPS = 2.0 ** -24                      # float32 unit roundoff
FLT_MAX = np.finfo(F32).max
DENORM = F32(1e-40)
ONE_MINUS = F32(1) - F32(2.0 ** -24)  # the largest rand1f


# ------------------------------------------------------------------------------ the device probe
class Probe:
    """ctypes binding of libjt_probe.so (tests/probe/jt_probe.hip)."""

    def __init__(self, path=None):
        # JT_PROBE_LIB: another build of the probe (the mutation record, DESIGN.md §4 Primitives)
        path = path or os.environ.get("JT_PROBE_LIB") or PROBE_LIB
        if not Path(path).exists():
            raise FileNotFoundError(f"{path} is missing: build it with make -C tests/probe (build() does)")
        self.lib = C.CDLL(str(path))
        f32p = C.POINTER(C.c_float)
        self.lib.jp_run.argtypes = [C.c_int, C.c_int64, f32p, f32p]
        self.lib.jp_op_name.argtypes = [C.c_int]
        self.lib.jp_op_name.restype = C.c_char_p
        self.lib.jp_op_nin.argtypes = [C.c_int]
        self.lib.jp_op_nout.argtypes = [C.c_int]
        self.lib.jp_run_texture.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int64, f32p, C.c_int64,
                                            f32p, f32p, C.c_int64, f32p, f32p]

    def ops(self):
        return [(self.lib.jp_op_name(k).decode(), self.lib.jp_op_nin(k), self.lib.jp_op_nout(k))
                for k in range(self.lib.jp_op_count())]

    def run(self, op, x):
        """Op `op` (by name) over the rows of x (n, nin) float32 on the GPU: (n, nout) float32."""
        ops = self.ops()
        k = [o[0] for o in ops].index(op)
        x = np.ascontiguousarray(x, F32).reshape(-1, ops[k][1])
        out = np.empty((x.shape[0], ops[k][2]), F32)
        f32p = C.POINTER(C.c_float)
        st = self.lib.jp_run(k, x.shape[0], x.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
        if st != 0:
            raise RuntimeError(f"probe {op}: HIP status {st}")
        return out


    def run_texture(self, textures, srgb_lut, q):
        """eval_texture on a scene of `textures` only, a list of (pixels (H, W, 4) uint8 or float32,
        linear); q (n, 4) = (texture, u, v, as_linear). The library lays the texels out by the host
        layout's rule; the LUTs are the caller's (the host's: srgb_to_rgb(b / 255) and b / 255)."""
        desc, tb, tf = [], [], []
        for pix, linear in textures:
            isf = pix.dtype == np.float32
            desc.append([pix.shape[1], pix.shape[0], int(bool(linear)), int(isf)])
            (tf if isf else tb).append(np.ascontiguousarray(pix).reshape(-1, 4))
        desc = np.array(desc, np.int32)
        texb = np.concatenate(tb) if tb else np.zeros((0, 4), np.uint8)
        texf = np.concatenate(tf) if tf else np.zeros((0, 4), F32)
        byte_lut = np.arange(256, dtype=F32) / F32(255)
        srgb_lut = np.ascontiguousarray(srgb_lut, F32)
        q = np.ascontiguousarray(q, F32).reshape(-1, 4)
        out = np.empty((len(q), 4), F32)
        f32p = C.POINTER(C.c_float)
        st = self.lib.jp_run_texture(len(desc), desc.ctypes.data_as(C.POINTER(C.c_int32)),
                                     texb.ctypes.data_as(C.POINTER(C.c_uint8)), len(texb), texf.ctypes.data_as(f32p),
                                     len(texf), srgb_lut.ctypes.data_as(f32p), byte_lut.ctypes.data_as(f32p), len(q),
                                     q.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
        if st != 0:
            raise RuntimeError(f"texture probe: status {st}")
        return out


# ------------------------------------------------------------------------------ comparing floats
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    """Elementwise: the same float32 bits, or both NaN (a NaN's payload carries nothing)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def mismatches(a, b):
    """Row indices where two probe outputs differ."""
    a = np.asarray(a, F32)
    a = a.reshape(a.shape[0], -1)
    bad = ~same(a, np.asarray(b, F32).reshape(a.shape))
    return np.flatnonzero(bad.reshape(bad.shape[0], -1).any(axis=1))


def near_midpoint(r64, ulps=4.0):
    """True where the double r64 lies within `ulps` double-ulps of the midpoint of two adjacent
    floats: there, two evaluations that are both within 1 ulp in double (the float contract's
    "evaluated in double and rounded once") may round to different floats. 4 is twice what two
    such evaluations can differ by."""
    r64 = np.asarray(r64, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = r64.astype(F32)
        other = np.nextafter(f, np.where(r64 > f.astype(np.float64), F32(np.inf), F32(-np.inf)).astype(F32))
        mid = 0.5 * (f.astype(np.float64) + other.astype(np.float64))
        return np.isfinite(r64) & np.isfinite(mid) & (np.abs(r64 - mid) <= ulps * np.spacing(np.abs(r64)))


def check_rounded(got, x64, fn64, fn_mp, cap=1e-6, what=""):
    """The float contract's rule for a transcendental: `got` (float32) equals the correctly rounded
    float of fn(x). Where the float64 value lies within 4 double-ulps of a rounding midpoint the
    correctly rounded float is decided with mpmath at 100 bits, and a result one float to the other
    side of that midpoint is accepted too (rounding a < 1 ulp double once more can land there); the
    count of such inputs is printed and capped at `cap` of the set. Returns (bad indices, ambiguous
    count, ambiguous inputs where `got` is not the correctly rounded float)."""
    import mpmath
    got = np.asarray(got, F32).ravel()
    with np.errstate(all="ignore"):
        r64 = fn64(*x64)
    ref = r64.astype(F32)
    amb = np.flatnonzero(near_midpoint(r64))
    ok = same(got, ref)
    wrong_side = 0
    if len(amb):
        mpmath.mp.prec = 100
        for k in amb:
            exact = fn_mp(*[mpmath.mpf(float(a[k])) for a in x64])
            lo, hi = sorted((float(ref[k]), float(np.nextafter(ref[k], F32(np.inf) if r64[k] > ref[k] else F32(-np.inf)))))
            mid = (mpmath.mpf(lo) + mpmath.mpf(hi)) / 2
            best = F32(hi if exact > mid else lo)
            ok[k] = bits(got[k]).item() in (bits(F32(lo)).item(), bits(F32(hi)).item())
            wrong_side += int(bits(got[k]).item() != bits(best).item())
    print(f"{what}: n={got.size} ambiguous={len(amb)} (cap {cap * got.size:.1f}) "
          f"ambiguous_not_correctly_rounded={wrong_side}")
    assert len(amb) <= cap * got.size, f"{what}: {len(amb)} ambiguous inputs exceed the cap; pick another set"
    return np.flatnonzero(~ok), len(amb), wrong_side


# ------------------------------------------------------------------------------ A/B: input sets
@functools.lru_cache(maxsize=None)
def rand_u():
    """Every value rand1f can return: k * 2^-24, k = 0 .. 2^24 - 1."""
    return (np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24).astype(F32)


@functools.lru_cache(maxsize=None)
def phi_all():
    """phi = (2 * pif) * u in float arithmetic for every rand1f value: the whole domain of the
    azimuth sincos of sample_disk, sample_hemisphere_cos, sample_microfacet, sample_phasefunction."""
    return TWO_PIF * rand_u()


def dsincos_small_np(x):
    """jl_sincos's small-argument algorithm as jt_device.h documents it, in numpy float64 (no
    fused operations): Cody-Waite reduction by pi/2 with a 33-bit leading constant, then fdlibm's
    __kernel_sin / __kernel_cos with a zero tail. Returns the doubles (sin, cos)."""
    invpio2, pio2_1, pio2_1t = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11
    n = np.rint(x * invpio2)
    r = (x - n * pio2_1) - n * pio2_1t
    z = r * r
    S1, S2, S3, S4, S5, S6 = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
                              2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
    C1, C2, C3, C4, C5, C6 = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
                              -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)
    sr = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    ks = r + (z * r) * (S1 + z * sr)
    cr = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    hz = 0.5 * z
    w = 1.0 - hz
    kc = w + (((1.0 - w) - hz) + z * cr)
    q = n.astype(np.int64) & 3
    return np.choose(q, [ks, kc, -ks, -kc]), np.choose(q, [kc, -ks, -kc, ks])


def doubles_of(words):
    """The doubles a probe wrote as (lo, hi) 32-bit words in float slots: (n, 2k) float32 -> (n, k)."""
    return np.ascontiguousarray(words, F32).view(np.uint32).astype(np.uint64).reshape(len(words), -1, 2) \
        .dot(np.array([1, 1 << 32], np.uint64)).view(np.float64)


SINCOS_EDGES = np.array([0.0, -0.0, 524287.97, 524288.0, -524287.97, -524288.0, 1e-30, 6.2831855, 1e9,
                         np.inf, -np.inf, np.nan, 1.5707964], F32)


def atan_args(rough):
    """sample_microfacet's atan argument, rough * sqrt(y / (1 - y)) in float arithmetic, every y."""
    y = rand_u()
    with np.errstate(all="ignore"):
        return F32(rough) * np.sqrt(y / (F32(1) - y))


ROUGHNESSES = (float(MIN_ROUGHNESS), 0.04, 0.25, 1.0)
N_STRAT = (1 << 20) + 1


def _odd(a):
    """a, without its first row when the length is even (the edges sit at the end)."""
    return a if len(a) % 2 else a[1:]


def _strat(lo, hi, seed, n=N_STRAT):
    """n stratified (jittered) points of [lo, hi), seeded."""
    rng = np.random.default_rng(seed)
    return (lo + (hi - lo) * (np.arange(n) + rng.random(n)) / n).astype(F32)


def atan2_set():
    """eval_environment's atan2(wl.z, wl.x) of a unit direction: both in [-1, 1]; plus axis edges."""
    ang = _strat(-np.pi, np.pi, 11).astype(np.float64)
    s = np.sqrt(np.random.default_rng(12).random(N_STRAT))  # |(x, z)| of a unit vector, <= 1
    y, x = (s * np.sin(ang)).astype(F32), (s * np.cos(ang)).astype(F32)
    e = np.array([[0, 1], [0, -1], [-0.0, -1], [1, 0], [-1, 0], [0, 0], [-0.0, 0], [0, -0.0], [1, 1], [-1, -1]], F32)
    return _odd(np.concatenate([np.stack([y, x], 1), e]))


def acos_set():
    return _odd(np.concatenate([_strat(-1, 1, 13), np.array([-1, 1, 0, -0.0, ONE_MINUS, -ONE_MINUS], F32)]))


def log_set():
    """sample_transmittance's log(1 - rd): 1 - k 2^-24; a stratified 2^20 of the k, plus both ends."""
    k = np.unique(np.concatenate([(np.arange(1 << 20, dtype=np.int64) << 4) +
                                  np.random.default_rng(14).integers(0, 16, 1 << 20), [0, (1 << 24) - 1, 1]]))
    x = (F32(1) - (k * 2.0 ** -24).astype(F32))
    return x if len(x) % 2 else np.delete(x, 7)  # both ends stay


def exp_set():
    """eval_transmittance's exp(-density * distance): arguments <= 0; dense near 0, out to underflow."""
    a = -np.exp(_strat(np.log(1e-6), np.log(120.0), 15).astype(np.float64)).astype(F32)
    return _odd(np.concatenate([a, np.array([0, -0.0, -87.3, -103.9, -104.0, -1e30], F32)]))


# ------------------------------------------------------------------------------ C: min/max/rcp
MINMAX_VALUES = np.array([0.0, -0.0, DENORM, -DENORM, 1, -1, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], F32)


def minmax_triples():
    return np.array(list(itertools.product(MINMAX_VALUES, repeat=3)), F32)  # 11^3 = 1331 rows


def _ieee_minimum(a, b):
    """IEEE 754-2019 minimum: NaN if either is NaN, -0 < +0."""
    if np.isnan(a) or np.isnan(b):
        return F32(np.nan)
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def _ieee_maximum(a, b):
    if np.isnan(a) or np.isnan(b):
        return F32(np.nan)
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


def minmax_reference(t):
    """Rows (min(a,b), max(a,b), min(a,b,c), max(a,b,c), maximum((a,b,c)), clamp(a, b, c)): Julia's
    min/max are IEEE 754-2019 minimum/maximum; clamp(x, lo, hi) = x > hi ? hi : (x < lo ? lo : x)."""
    out = np.empty((len(t), 6), F32)
    for r, (a, b, c) in enumerate(t):
        out[r, 0] = _ieee_minimum(a, b)
        out[r, 1] = _ieee_maximum(a, b)
        out[r, 2] = _ieee_minimum(_ieee_minimum(a, b), c)
        out[r, 3] = out[r, 4] = _ieee_maximum(_ieee_maximum(a, b), c)
        out[r, 5] = c if a > c else (b if a < b else a)
    return out


def rcp_set():
    """Every exponent x 2^12 mantissas (one per top-12-bit stratum, seeded low bits, both ends
    exact) x both signs; this covers zeros, denormals, 2^126 and above, inf and NaN."""
    low = np.random.default_rng(16).integers(0, 1 << 11, 1 << 12).astype(np.uint32)
    man = (np.arange(1 << 12, dtype=np.uint32) << 11) | low
    man[0], man[-1] = 0, 0x7FFFFF
    e = np.arange(256, dtype=np.uint32)[:, None] << 23
    pos = (e | man[None, :]).ravel()
    allb = np.concatenate([pos, pos | np.uint32(0x80000000), np.array([1], np.uint32)])  # + the least denormal
    return allb.view(F32)


# ------------------------------------------------------------------------------ D: intersection
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ulp_up(x, k=1):
    x = np.asarray(x, F32)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf))
    return x


def bbox_set(n=8191):
    """Rows o(3) dinv(3) tmin tmax bmin(3) bmax(3). Random rays against random boxes at scales 1e-6,
    1 and 1e6 (about half hit), then the edges: a ray lying in a slab plane with a zero direction
    component (0 * inf = NaN culls the box), t0 one ulp above t1 and equal to it, -0.0 direction
    components, tmax exactly on the entry distance."""
    rng = np.random.default_rng(21)
    rows = []
    for scale in (1.0, 1e-6, 1e6):
        m = n // 3
        c = rng.uniform(-1, 1, (m, 3))
        h = rng.uniform(0.05, 0.6, (m, 3))
        o = rng.uniform(-3, 3, (m, 3))
        target = c + rng.uniform(-1.2, 1.2, (m, 3)) * h
        d = unit(target - o)
        bmin, bmax, o32 = ((c - h) * scale).astype(F32), ((c + h) * scale).astype(F32), (o * scale).astype(F32)
        with np.errstate(divide="ignore"):
            dinv = F32(1) / d.astype(F32)
        tmin = np.full((m, 1), 1e-4 * scale, F32)
        tmax = np.where(rng.random((m, 1)) < 0.3, rng.uniform(0, 6, (m, 1)) * scale, np.inf).astype(F32)
        rows.append(np.concatenate([o32, dinv, tmin, tmax, bmin, bmax], 1))
    inf = np.inf
    e = [
        # in the x = 0 slab plane, d.x = +0 and -0: (0 - 0) * inf = NaN -> miss
        [0, .5, -2, inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [0, .5, -2, -inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [1, .5, -2, inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        # d.x = +-0 strictly inside / outside the slab: +-inf slab values, no NaN
        [.5, .5, -2, inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [.5, .5, -2, -inf, -inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [1.5, .5, -2, inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [1.5, .5, -2, -inf, inf, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        # tmax on the entry distance (t0 == t1 == 2), just below it, tmin on the exit distance
        [.5, .5, -2, inf, inf, 1, 0, 2, 0, 0, 0, 1, 1, 1],
        [.5, .5, -2, inf, inf, 1, 0, float(np.nextafter(F32(2), F32(0))), 0, 0, 0, 1, 1, 1],
        [.5, .5, -2, inf, inf, 1, 3, inf, 0, 0, 0, 1, 1, 1],
        [.5, .5, -2, inf, inf, 1, float(_ulp_up(3)), inf, 0, 0, 0, 1, 1, 1],
        # a NaN origin, a NaN tmax
        [np.nan, .5, -2, 1, 1, 1, 0, inf, 0, 0, 0, 1, 1, 1],
        [.5, .5, -2, inf, inf, 1, 0, np.nan, 0, 0, 0, 1, 1, 1],
    ]
    # t0 = t1 + k ulp through tmin: the 1.00000024 factor (about 2 ulp) passes k = 1, 2 and fails beyond
    for k in range(0, 6):
        e.append([.5, .5, -2, inf, inf, 1, float(_ulp_up(3, k)), inf, 0, 0, 0, 1, 1, 1])
    out = np.concatenate(rows + [np.array(e, F32)])
    return _odd(out)


def bbox_reference(x):
    """The slab rule in float64 on the float inputs: (hit, margin). t_axis = (b - o) * dinv;
    t0 = max(mins, tmin), t1 = min(maxs, tmax); hit = t0 <= t1 * 1.00000024; a NaN slab value culls.
    margin = |t0 - 1.00000024 t1| / max(|t0|, |t1|): each float slab value carries two roundings
    (relative error <= 2 * 2^-24), so a decision with margin <= 4 * 2^-24 is below float rounding."""
    x = np.asarray(x, np.float64)
    o, dinv, tmin, tmax, bmin, bmax = x[:, 0:3], x[:, 3:6], x[:, 6], x[:, 7], x[:, 8:11], x[:, 11:14]
    with np.errstate(all="ignore"):
        a, b = (bmin - o) * dinv, (bmax - o) * dinv
        nan = np.isnan(a).any(1) | np.isnan(b).any(1) | np.isnan(tmin) | np.isnan(tmax)
        t0 = np.maximum(np.minimum(a, b).max(1), tmin)
        t1 = np.minimum(np.maximum(a, b).min(1), tmax) * 1.00000024
        hit = ~nan & (t0 <= t1)
        margin = np.abs(t0 - t1) / np.maximum(np.maximum(np.abs(t0), np.abs(t1)), 1e-300)
        margin = np.where(np.isfinite(margin), margin, np.inf)
    return hit, np.where(nan, np.inf, margin)


def _tri_rows(o, d, tmin, tmax, *pts):
    n = len(o)
    col = lambda v: np.broadcast_to(np.asarray(v, np.float64).reshape(-1, 1) if np.ndim(v) else np.full((n, 1), v), (n, 1))
    return np.concatenate([o, d, col(tmin), col(tmax), *pts], 1).astype(F32)


def triangle_set(n=8190):
    """Rows o(3) d(3) tmin tmax p1 p2 p3. Random rays aimed around random triangles at scales 1e-6,
    1, 1e6, then edges: det == 0 (a ray in the triangle's plane, a zero-area triangle), t == tmax
    and one ulp either side, t == tmin, hits exactly on an edge and a vertex (u = 0, v = 0,
    u + v = 1 with exactly representable coordinates), a NaN vertex."""
    rng = np.random.default_rng(22)
    rows = []
    for scale in (1.0, 1e-6, 1e6):
        m = n // 3
        p = rng.uniform(-1, 1, (m, 3, 3))
        bc = rng.uniform(-0.25, 1.0, (m, 2))  # barycentrics in and around the triangle
        target = p[:, 0] + bc[:, :1] * (p[:, 1] - p[:, 0]) + bc[:, 1:] * (p[:, 2] - p[:, 0])
        o = rng.uniform(-3, 3, (m, 3))
        d = unit(target - o)
        tmax = np.where(rng.random(m) < 0.3, rng.uniform(0, 6, m) * scale, np.inf)
        rows.append(_tri_rows(o * scale, d, 1e-4 * scale, tmax, p[:, 0] * scale, p[:, 1] * scale, p[:, 2] * scale))
    P1, P2, P3 = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    inf = np.inf

    def row(o, d, tmin, tmax, p1=P1, p2=P2, p3=P3):
        return np.array([*o, *d, tmin, tmax, *p1, *p2, *p3], F32)
    e = [
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf),                        # plain hit, t = 2
        row([.25, .25, 2], [0, 0, -1], 1e-4, 2),                          # t == tmax: a hit
        row([.25, .25, 2], [0, 0, -1], 1e-4, float(np.nextafter(F32(2), F32(0)))),
        row([.25, .25, 2], [0, 0, -1], 1e-4, float(_ulp_up(2))),
        row([.25, .25, 2], [0, 0, -1], 2, inf),                           # t == tmin: a hit
        row([.25, .25, 2], [0, 0, -1], float(_ulp_up(2)), inf),
        row([.25, .25, 0], [1, 0, 0], 1e-4, inf),                         # in the plane: det == 0
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf, P1, P2, [2, 0, 0]),     # zero area: det == 0
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf, P1, P1, P1),
        row([0, .5, 2], [0, 0, -1], 1e-4, inf),                           # on the edge u = 0
        row([.5, 0, 2], [0, 0, -1], 1e-4, inf),                           # on the edge v = 0
        row([.5, .5, 2], [0, 0, -1], 1e-4, inf),                          # on the edge u + v = 1
        row([0, 0, 2], [0, 0, -1], 1e-4, inf),                            # on the vertices
        row([1, 0, 2], [0, 0, -1], 1e-4, inf),
        row([0, 1, 2], [0, 0, -1], 1e-4, inf),
        row([.5, .5, 2], [0, 0, -1], 1e-4, inf, [1, 1, 0], P3, P2),       # the shared edge from the other side
        row([.25, .25, 2], [-0.0, -0.0, -1], 1e-4, inf),                  # -0.0 direction components
        row([.25, .25, -2], [0, 0, -1], 1e-4, inf),                       # behind the origin
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf, [np.nan, 0, 0]),        # NaN vertex
        row([.25, .25, 2], [0, 0, 0], 1e-4, inf),                         # zero direction
    ]
    out = np.concatenate(rows + [np.array(e, F32)])
    return _odd(out)


def triangle_reference(x, K=16.0):
    """Moller-Trumbore in float64 on the float inputs: (hit, u, v, t, safe, tol). The float
    evaluation's error in u, v, t is bounded to first order by K * 2^-24 * (sum of the absolute
    terms of the numerator / |det| + |value| * sum of the absolute terms of det / |det|), K = 16
    covering the 15 float operations on the longest path (edges 1, cross 3, dot 5, rcp 1, ...).
    `safe` is true where every comparison (det == 0, u, v, u + v against 0 and 1, t against tmin
    and tmax) is farther from its threshold than that bound: only there is the decision compared."""
    x = np.asarray(x, np.float64)
    o, d, tmin, tmax = x[:, 0:3], x[:, 3:6], x[:, 6], x[:, 7]
    p1, p2, p3 = x[:, 8:11], x[:, 11:14], x[:, 14:17]
    with np.errstate(all="ignore"):
        e1, e2 = p2 - p1, p3 - p1
        ae1, ae2 = np.abs(p2) + np.abs(p1), np.abs(p3) + np.abs(p1)
        acr = lambda a, b: np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
        pvec, apvec = np.cross(d, e2), acr(np.abs(d), ae2)
        det, adet = (e1 * pvec).sum(1), (ae1 * apvec).sum(1)
        tvec, atvec = o - p1, np.abs(o) + np.abs(p1)
        qvec, aqvec = np.cross(tvec, e1), acr(atvec, ae1)
        u, v, t = (tvec * pvec).sum(1) / det, (d * qvec).sum(1) / det, (e2 * qvec).sum(1) / det
        k = K * EPS / np.abs(det)
        eu = k * ((atvec * apvec).sum(1) + np.abs(u) * adet)
        ev = k * ((np.abs(d) * aqvec).sum(1) + np.abs(v) * adet)
        et = k * ((ae2 * aqvec).sum(1) + np.abs(t) * adet)
        hit = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
        # a comparison is decided safely when the value clears the threshold by the bound; a miss needs
        # only one safely failed comparison, a hit needs them all safely passed
        fail = ((u < -eu) | (u > 1 + eu) | (v < -ev) | (u + v > 1 + eu + ev) | (t < tmin - et) | (t > tmax + et))
        clear = ((u > eu) & (u < 1 - eu) & (v > ev) & (u + v < 1 - eu - ev) & (t > tmin + et) & (t < tmax - et))
        nondeg = np.abs(det) > K * EPS * adet
        safe = np.isfinite(np.delete(x, 7, 1)).all(1) & nondeg & np.where(hit, clear, fail)
    return hit, u, v, t, safe, np.stack([eu, ev, et], 1)


def quad_set(n=4095):
    """Rows o(3) d(3) tmin tmax p1..p4. Random planar and slightly folded quads, then edges: a hit
    exactly on the p2-p4 diagonal (both halves hit at the same t: the second half's answer is the
    reference's, `i1.distance < i2.distance` being false), a degenerate quad (p3 == p4, a triangle),
    a miss, t == tmax."""
    rng = np.random.default_rng(23)
    rows = []
    for scale in (1.0, 1e-6, 1e6):
        m = n // 3
        c, ex, ey = rng.uniform(-1, 1, (m, 3)), unit(rng.normal(size=(m, 3))), rng.normal(size=(m, 3))
        ey = unit(ey - (ey * ex).sum(1, keepdims=True) * ex)
        w, h = rng.uniform(0.2, 1, (m, 1)), rng.uniform(0.2, 1, (m, 1))
        fold = np.cross(ex, ey) * rng.uniform(-0.05, 0.05, (m, 1))
        p1, p2, p3, p4 = c, c + ex * w, c + ex * w + ey * h + fold, c + ey * h
        uv = rng.uniform(-0.2, 1.2, (m, 2))
        target = c + ex * w * uv[:, :1] + ey * h * uv[:, 1:]
        o = rng.uniform(-3, 3, (m, 3))
        rows.append(_tri_rows(o * scale, unit(target - o), 1e-4 * scale, np.inf, p1 * scale, p2 * scale, p3 * scale,
                              p4 * scale))
    inf = np.inf
    Q = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]

    def row(o, d, tmin, tmax, q=Q):
        return np.array([*o, *d, tmin, tmax, *q[0], *q[1], *q[2], *q[3]], F32)
    e = [
        row([.5, .5, 2], [0, 0, -1], 1e-4, inf),       # on the p2-p4 diagonal, u + v == 1 in both halves
        row([.25, .75, 2], [0, 0, -1], 1e-4, inf),     # on the diagonal again
        row([.75, .25, 4], [0, 0, -1], 1e-4, inf),
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf),     # first half
        row([.75, .75, 2], [0, 0, -1], 1e-4, inf),     # second half
        row([.75, .75, 2], [0, 0, -1], 1e-4, 2),       # t == tmax
        row([1.5, .5, 2], [0, 0, -1], 1e-4, inf),      # miss
        row([.25, .25, 2], [0, 0, -1], 1e-4, inf, [Q[0], Q[1], Q[3], Q[3]]),  # degenerate: p3 == p4
        row([.75, .75, 2], [0, 0, -1], 1e-4, inf, [Q[0], Q[1], Q[3], Q[3]]),  # outside the one triangle
        row([1, 0, 2], [0, 0, -1], 1e-4, inf),         # the shared vertex p2
        row([0, 1, 2], [0, 0, -1], 1e-4, inf),         # the shared vertex p4
    ]
    out = np.concatenate(rows + [np.array(e, F32)])
    return _odd(out)


# ------------------------------------------------------------------------------ E: lobes
M_MATTE, M_GLOSSY, M_REFLECTIVE, M_TRANSPARENT, M_REFRACTIVE, M_SUBSURFACE, M_VOLUMETRIC, M_GLTFPBR = range(8)
LOBE_ROUGHNESS = (0.0, 0.0009, 0.03, 0.3, 1.0)


def _around(v):
    v = F32(v)
    return [float(np.nextafter(v, F32(-np.inf))), float(v), float(np.nextafter(v, F32(np.inf)))]


# the floats around the |ior - 1| < 1e-3 switch (1.001, 0.999) and common indices
LOBE_IOR = tuple(_around(1.001) + _around(0.999) + _around(F32(1) + F32(0.001)) + _around(F32(1) - F32(0.001)) +
                 [1.0, 1.33, 1.5, 2.4])
ANISOTROPY = (0.0, 0.000999, -0.000999, 0.001, -0.001, 0.5, -0.9)
RN_GRID = (0.0, float(ONE_MINUS), 0.25, 0.5, 0.75, 2.0 ** -24, 0.999)


def _directions(rng, m):
    """(n, o, i) triples, float32: random unit vectors, then the special normals and the special
    n.o values {0, +-2^-24, +-1e-4}, i = reflect(o), -o, o."""
    n = unit(rng.normal(size=(m, 3)))
    o = unit(rng.normal(size=(m, 3)))
    i = unit(rng.normal(size=(m, 3)))
    kind = rng.integers(0, 8, m)
    axes = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0]], np.float64)
    sel = kind == 1
    n[sel] = axes[rng.integers(0, 3, sel.sum())]
    # o at a chosen cosine to n: o = c n + sqrt(1 - c^2) t, t a unit tangent
    sel = (kind == 2) | (kind == 3)
    cosv = np.array([0.0, 2.0 ** -24, -2.0 ** -24, 1e-4, -1e-4, 1.0, -1.0])[rng.integers(0, 7, m)]
    tang = unit(np.cross(n, unit(rng.normal(size=(m, 3))) + 1e-3))
    o[sel] = (cosv[:, None] * n + np.sqrt(1 - cosv[:, None] ** 2) * tang)[sel]
    refl = -o + 2 * (n * o).sum(1, keepdims=True) * n
    i = np.where((kind == 4)[:, None] | (kind == 3)[:, None], refl, i)
    i = np.where((kind == 5)[:, None], -o, i)
    i = np.where((kind == 6)[:, None], o, i)
    # the transmitted side: a random direction below the surface as seen from o
    flip = (kind == 7)[:, None] & (((n * i).sum(1) * (n * o).sum(1)) > 0)[:, None]
    i = np.where(flip, i - 2 * (n * i).sum(1, keepdims=True) * n, i)
    return n.astype(F32), o.astype(F32), i.astype(F32)


def lobe_set(oracle, n=(1 << 14) + 1):
    """Rows type color(3) ior roughness n(3) o(3) i(3) rnl rn(2) for the bsdf and parts ops: every
    material type, roughness in {0, 0.0009, 0.03, 0.3, 1} and random, the ior list above, the
    directions of _directions, rn on a grid with 0 and 1 - 2^-24 and random, rnl 0, random, and the
    floats either side of the row's Fresnel value (fresnel_dielectric(ior or 1/ior, n, o), the
    oracle's: the test compares device and oracle on the same inputs, whatever they are)."""
    rng = np.random.default_rng(31)
    nn, o, i = _directions(rng, n)
    typ = (np.arange(n) % 7).astype(F32)
    color = rng.uniform(0, 1, (n, 3)).astype(F32)
    color[rng.random(n) < 0.1] = [0.0, 1.0, 0.995]
    ior = np.where(rng.random(n) < 0.7, np.array(LOBE_IOR)[rng.integers(0, len(LOBE_IOR), n)], rng.uniform(1, 2.5, n)).astype(F32)
    rough = np.where(rng.random(n) < 0.75, np.array(LOBE_ROUGHNESS)[rng.integers(0, 5, n)], rng.uniform(0, 1, n)).astype(F32)
    grid = np.array(RN_GRID)
    rn = np.where(rng.random((n, 2)) < 0.5, grid[rng.integers(0, len(grid), (n, 2))],
                  rng.integers(0, 1 << 24, (n, 2)) * 2.0 ** -24).astype(F32)
    x = np.concatenate([typ[:, None], color, ior[:, None], rough[:, None], nn, o, i, np.zeros((n, 1), F32), rn], 1).astype(F32)
    # the Fresnel value each row's sampler compares rnl with, entering or leaving
    with np.errstate(all="ignore"):
        x2 = x.copy()
        leaving = (nn * o).sum(1) < 0
        x2[leaving, 4] = F32(1) / x[leaving, 4]
    fres = oracle.probe("parts", x2)[:, 0]
    k = rng.integers(0, 6, n)
    rnl = (rng.integers(0, 1 << 24, n) * 2.0 ** -24).astype(F32)
    rnl = np.where(k == 1, F32(0), rnl)
    rnl = np.where(k == 2, fres, rnl)
    rnl = np.where(k == 3, np.nextafter(fres, F32(-np.inf)), rnl)
    rnl = np.where(k == 4, np.nextafter(fres, F32(np.inf)), rnl)
    x[:, 15] = np.where(np.isfinite(rnl), rnl, 0.5)
    return x


def volume_set(n=(1 << 13) + 1):
    """Rows density(3) scattering(3) anisotropy o(3) i(3) rn(2) distance max_distance rl rd."""
    rng = np.random.default_rng(32)
    dens = rng.uniform(0, 4, (n, 3)) * (rng.random((n, 3)) > 0.15)
    dens[rng.random(n) < 0.05] = 0
    scat = rng.uniform(0, 1, (n, 3))
    an = np.where(rng.random(n) < 0.7, np.array(ANISOTROPY)[rng.integers(0, len(ANISOTROPY), n)], rng.uniform(-0.95, 0.95, n))
    o, i = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
    k = rng.integers(0, 6, n)
    i = np.where((k == 0)[:, None], o, np.where((k == 1)[:, None], -o, i))
    grid = np.array(RN_GRID)
    rn = np.where(rng.random((n, 2)) < 0.5, grid[rng.integers(0, len(grid), (n, 2))],
                  rng.integers(0, 1 << 24, (n, 2)) * 2.0 ** -24)
    dist = rng.uniform(0, 5, n) * (rng.random(n) > 0.05)
    maxd = np.where(rng.random(n) < 0.2, np.inf, rng.uniform(0, 5, n))
    rl = np.where(rng.random(n) < 0.3, grid[rng.integers(0, len(grid), n)], rng.random(n))
    rd = np.where(rng.random(n) < 0.3, grid[rng.integers(0, len(grid), n)], rng.integers(0, 1 << 24, n) * 2.0 ** -24)
    return np.concatenate([dens, scat, an[:, None], o, i, rn, dist[:, None], maxd[:, None], rl[:, None],
                           rd[:, None]], 1).astype(F32)


# ------------------------------------------------------------------------------ float64 lobe terms
def fresnel_dielectric_ref(eta, cosw):
    """Unpolarised Fresnel reflectance of a dielectric, relative index eta, |cos| of incidence:
    Snell gives cos_t, R = (r_s^2 + r_p^2) / 2; total internal reflection is 1."""
    cosw = np.abs(cosw)
    sin2t = (1 - cosw * cosw) / (eta * eta)
    with np.errstate(invalid="ignore"):
        cost = np.sqrt(1 - sin2t)
        rs = (cosw - eta * cost) / (cosw + eta * cost)
        rp = (cost - eta * cosw) / (cost + eta * cosw)
    return np.where(sin2t > 1, 1.0, (rs * rs + rp * rp) / 2)


def fresnel_conductor_ref(eta, k, cosw):
    """Unpolarised Fresnel reflectance of a conductor with complex index eta + i k (exact, through
    complex arithmetic: r_s = (cos - sqrt(m^2 - sin^2)) / (cos + ...), r_p likewise with m^2 cos)."""
    m2 = (eta + 1j * k) ** 2
    s2 = 1 - cosw * cosw
    root = np.sqrt(m2 - s2 + 0j)
    rs = (cosw - root) / (cosw + root)
    rp = (m2 * cosw - root) / (m2 * cosw + root)
    return (np.abs(rs) ** 2 + np.abs(rp) ** 2) / 2


def ggx_d_ref(alpha, cos_h):
    """GGX / Trowbridge-Reitz: D = a^2 / (pi ((n.h)^2 (a^2 - 1) + 1)^2), 0 below the surface."""
    return np.where(cos_h > 0, alpha ** 2 / (np.pi * (cos_h ** 2 * (alpha ** 2 - 1) + 1) ** 2), 0.0)


def smith_g1_ref(alpha, cos_n, cos_h):
    """Smith G1 for GGX: 2 / (1 + sqrt(1 + a^2 tan^2)), 0 when the direction is on opposite sides
    of the macro and the micro surface."""
    tan2 = (1 - cos_n ** 2) / cos_n ** 2
    return np.where(cos_n * cos_h > 0, 2 / (1 + np.sqrt(1 + alpha ** 2 * tan2)), 0.0)


def hg_ref(g, cos_theta):
    """Henyey-Greenstein: (1 - g^2) / (4 pi (1 + g^2 - 2 g cos)^(3/2)), cos between the directions
    of travel (-outgoing . incoming in the renderer's convention)."""
    return (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * cos_theta) ** 1.5)


def tolerance(f, xs, K):
    """K * 2^-24 * (|f| + sum_j |x_j df/dx_j|), the derivatives by central differences in float64:
    the first-order bound of a K-operation float evaluation of f at float inputs xs."""
    xs = [np.asarray(x, np.float64) for x in xs]
    f0 = f(*xs)
    s = np.abs(f0)
    for j, x in enumerate(xs):
        h = np.maximum(np.abs(x), 1e-3) * 1e-6
        hi = f(*[x + h if k == j else xs[k] for k in range(len(xs))])
        lo = f(*[x - h if k == j else xs[k] for k in range(len(xs))])
        s = s + np.abs(x * (hi - lo) / (2 * h))
    return K * EPS * s


# ------------------------------------------------------------------------------ F: bilinear wrap
def bilinear_wrap_ref(img, uv):
    """Bilinear lookup with wrap, float64: img (H, W, 4) of linear values; s = mod1(u) * W, texel
    i = floor(s) clamped to W - 1, its neighbour (i + 1) mod W, weights by the fraction."""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    out = np.empty((len(uv), 4))
    for r, (u, v) in enumerate(np.asarray(uv, np.float64)):
        s, t = (u % 1.0) * W, (v % 1.0) * H
        i, j = min(int(np.floor(s)), W - 1), min(int(np.floor(t)), H - 1)
        ii, jj = (i + 1) % W, (j + 1) % H
        a, b = s - i, t - j
        out[r] = (img[j, i] * (1 - a) * (1 - b) + img[jj, i] * (1 - a) * b + img[j, ii] * a * (1 - b) +
                  img[jj, ii] * a * b)
    return out


def texture_set():
    """[(pixels, linear)]: sizes 1x1, 1x5, 5x1, 2x2, 3x2 (width x height) in the formats byte sRGB,
    byte linear and float; the last texture is a byte one (its last texel's pair load reads the
    padding texel). Seeded texels with 0 and 255 (0.0 and 1.0) among them."""
    rng = np.random.default_rng(41)
    out = []
    for k, (w, h) in enumerate([(1, 1), (1, 5), (5, 1), (2, 2), (3, 2)]):
        for fmt in ("srgb", "linear", "float"):
            if fmt == "float":
                pix = rng.random((h, w, 4)).astype(F32)
                pix.flat[0] = 1.0
            else:
                pix = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
                pix.flat[0], pix.flat[-1] = 255, 0
            out.append((pix, fmt != "srgb"))
    out.append(out.pop(-3))  # 3x2 byte sRGB last
    assert out[-1][0].dtype == np.uint8
    return out


def texture_uvs(w, h):
    """Every pair of the special coordinates, for a w x h texture: 0, 1, -1, 2.5, k / w (k / h)
    exactly as floats, -1e-10, 1 - 2^-24, 1e6, and two ordinary values."""
    def axis(n):
        return [0.0, 1.0, -1.0, 2.5, -1e-10, float(ONE_MINUS), 1e6, 0.3, -0.7] + [float(F32(k) / F32(n)) for k in range(n + 1)]
    return np.array(list(itertools.product(axis(w), axis(h))), F32)


def decode_ref(pix, linear, as_linear):
    """Texel values in float64: byte / 255; sRGB to linear by the standard's piecewise curve on the
    colour channels when asked and the texture is not linear; alpha never."""
    v = pix.astype(np.float64) / (255.0 if pix.dtype == np.uint8 else 1.0)
    if as_linear and not linear:
        c = v[..., :3]
        v[..., :3] = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return v


def texture_tolerance(w, h):
    """Bilinear lookup of texels in [0, 1]: K = 16 covers its 15 float operations (two products
    and a weight per texel, three sums); besides, s = mod1(u) * w is rounded at magnitude up to w,
    so the weights carry an absolute error of 2^-24 w (h): 16 * 2^-24 * (1 + w + h)."""
    return 16 * EPS * (1 + w + h)
