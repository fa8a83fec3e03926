"""Single primitives on the CPU: the oracle's probes (oracle/jt_oracle.c or_probe) against the
float64 references of tests/primitives_ref.py, the claims the GPU file (test_gpu_primitives.py)
rests on, and the probe library's build contract. No GPU.
"""
import re
import sys

import numpy as np
import pytest

import primitives_ref as R
from primitives_ref import F32

ROOT = R.ROOT


@pytest.fixture(scope="module")
def probe_ops():
    return R.Probe().ops()  # a missing probe library is an error, not a skip


# ------------------------------------------------------------------------------ the build contract
def _make_vars(path, names):
    """The := / ?= definitions of `names` in a Makefile, continuation lines joined, as token lists."""
    text = path.read_text().replace("\\\n", " ")
    out = {}
    for n in names:
        m = re.search(rf"^{n}\s*[:?]?=\s*(.*)$", text, re.M)
        assert m, f"{path}: no definition of {n}"
        out[n] = m.group(1).split()
    return out


def test_probe_flags_equal_the_products():
    """The probe compiles the product's headers with the product's flags: the flag variables of
    the two Makefiles are the same token for token (JT_EXACT_MATH=1, -ffp-contract=off, ...)."""
    names = ["ARCH", "JT_EXACT_MATH", "JT_WAVES", "CXXFLAGS", "HIPFLAGS", "KFLAGS"]
    prod = _make_vars(ROOT / "julia-raytracer_amd" / "Makefile", names)
    probe = _make_vars(ROOT / "tests" / "probe" / "Makefile", names)
    assert probe == prod
    flat = " ".join(sum(prod.values(), []))
    for need in ("-ffp-contract=off", "-fno-fast-math", "-DJT_EXACT_MATH=$(JT_EXACT_MATH)", "-fno-slp-vectorize", "-O3"):
        assert need in flat
    # and the probe's compile line uses them all, nothing that changes code generation besides
    rule = re.search(r"^\t\$\(HIPCC\) (.*)$", (ROOT / "tests" / "probe" / "Makefile").read_text(), re.M).group(1)
    assert rule.split() == ["$(HIPFLAGS)", "$(KFLAGS)", "-I$(PKG)/csrc", "-shared", "-o", "$@", "jt_probe.hip"]


def test_probe_is_outside_the_source_hash():
    """The product's source hash (scripts/roofline.py, embedded in jt_version and carried by the
    roofline records) covers the product Makefile, csrc/ and the ABI header only: the probe adds
    nothing to it, so the records measured on the parent's sources stay valid."""
    sys.path.insert(0, str(ROOT / "scripts"))
    from roofline import build_files
    fs = build_files()
    assert not [f for f in fs if f.startswith("tests") or "probe" in f]
    assert not list((ROOT / "julia-raytracer_amd" / "csrc").glob("*probe*"))
    assert "probe" not in (ROOT / "julia-raytracer_amd" / "Makefile").read_text()


def test_op_tables_agree(oracle, probe_ops):
    assert oracle.probe_ops() == probe_ops
    assert len({o[0] for o in probe_ops}) == len(probe_ops)


# ------------------------------------------------------------------------------ A: sin / cos claims
@pytest.fixture(scope="module")
def phi_ref():
    phi = R.phi_all().astype(np.float64)
    return phi, np.sin(phi), np.cos(phi)


def test_sincos_set_has_no_ambiguous_input(phi_ref):
    """No phi = (2 pif) u has sin or cos within 4 double-ulps of a float rounding midpoint, so the
    GPU test's cap on exceptions is zero: every result is the correctly rounded float."""
    _, s, c = phi_ref
    assert int(R.near_midpoint(s).sum()) == 0 and int(R.near_midpoint(c).sum()) == 0


def test_sincos_restatement_and_oracle_equal_numpy(phi_ref, oracle):
    """Over the whole set: the device algorithm restated in numpy, and the oracle (the C library's
    double sin/cos), both round to numpy's float32(sin(float64 phi)): 0 mismatches."""
    phi, s, c = phi_ref
    rs, rc = R.dsincos_small_np(phi)
    assert int((~R.same(rs.astype(F32), s.astype(F32))).sum()) == 0
    assert int((~R.same(rc.astype(F32), c.astype(F32))).sum()) == 0
    o = oracle.probe("sincos", R.phi_all()[:: 16])[:, :2]
    assert len(R.mismatches(o, np.stack([s[::16], c[::16]], 1).astype(F32))) == 0


def test_disk_signs_claim(phi_ref):
    """sample_disk_signs restated: comparing the float phi, in double, with the doubles nearest
    pi/2, pi, 3pi/2, 2pi gives the signs of the rounded cos and sin for every rand1f value."""
    phi, s, c = phi_ref
    cneg = (phi > 1.5707963267948966) & (phi < 4.7123889803846897)
    sneg = (phi > 3.1415926535897931) & (phi < 6.2831853071795862)
    assert int((np.signbit(c.astype(F32)) != cneg).sum()) == 0
    assert int((np.signbit(s.astype(F32)) != sneg).sum()) == 0
    # the claim's premise: no rounded result is zero except sin(+0)
    assert int((c.astype(F32) == 0).sum()) == 0 and np.flatnonzero(s.astype(F32) == 0).tolist() == [0]


def test_sincos_edges(oracle):
    """Edge arguments through the oracle: sin(-0.0) is -0.0 in double arithmetic (the device's
    reduction gives +0.0, see the GPU test), the 2^19 switch, inf and NaN give NaN."""
    e = R.SINCOS_EDGES
    o = oracle.probe("sincos", e)[:, :2]
    with np.errstate(invalid="ignore"):
        ref = np.stack([np.sin(e.astype(np.float64)), np.cos(e.astype(np.float64))], 1).astype(F32)
    assert len(R.mismatches(o, ref)) == 0


# ------------------------------------------------------------------------------ B: ambiguous counts
def _mp(name):
    import mpmath
    return getattr(mpmath, name)


@pytest.mark.parametrize("rough", R.ROUGHNESSES)
def test_atan_sets_meet_the_cap(rough, oracle):
    """The ambiguous-input count of each atan set (and of the sincos of its results) is within
    10^-6 of the set, computed here before any GPU run; the oracle's atan obeys the rule on a
    1/16 subset."""
    x = R.atan_args(rough)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        th = np.arctan(x64)
        th32 = th.astype(F32).astype(np.float64)
        counts = [int(R.near_midpoint(v).sum()) for v in (th, np.sin(th32), np.cos(th32))]
    print(f"atan rough={rough}: ambiguous atan/sin/cos = {counts} of {x.size}")
    assert max(counts) <= 1e-6 * x.size
    sub = slice(0, None, 16)
    got = oracle.probe("atan", x[sub])
    bad, _, _ = R.check_rounded(got[:, 0], [x64[sub]], np.arctan, _mp("atan"), cap=1e-5, what=f"oracle atan {rough}")
    assert len(bad) == 0


@pytest.mark.parametrize("op,make,fn,mp", [
    ("atan2", R.atan2_set, np.arctan2, "atan2"), ("acos", R.acos_set, np.arccos, "acos"),
    ("log", R.log_set, np.log, "log"), ("exp", R.exp_set, np.exp, "exp")])
def test_rare_transcendentals_oracle(op, make, fn, mp, oracle):
    x = make()
    assert len(x) % 2 == 1
    cols = [c.astype(np.float64) for c in (x.T if x.ndim == 2 else [x])]
    got = oracle.probe(op, x)
    bad, amb, _ = R.check_rounded(got[:, 0], cols, fn, _mp(mp), what=f"oracle {op}")
    assert len(bad) == 0, (op, bad[:5], x[bad[:5]], got[bad[:5]])


# ------------------------------------------------------------------------------ C: min / max / rcp
def test_minmax_reference_vs_oracle(oracle):
    t = R.minmax_triples()
    assert len(t) == 1331
    bad = R.mismatches(oracle.probe("minmax", t), R.minmax_reference(t))
    assert len(bad) == 0, t[bad[:5]]


def test_rcp_oracle(oracle):
    x = R.rcp_set()
    assert len(x) % 2 == 1
    with np.errstate(all="ignore"):
        ref = F32(1) / x
    assert len(R.mismatches(oracle.probe("rcp", x), ref)) == 0


# ------------------------------------------------------------------------------ D: intersection
def test_bbox_oracle_vs_slab_rule(oracle):
    x = R.bbox_set()
    hit, margin = R.bbox_reference(x)
    got = oracle.probe("bbox", x)[:, 0] > 0
    ok = margin > 4 * R.EPS
    print(f"bbox: n={len(x)} skipped={1 - ok.mean():.5f} hits={hit.mean():.3f}")
    assert 1 - ok.mean() <= 0.01
    assert not (got != hit)[ok].any()
    assert 0.2 < hit.mean() < 0.9


def test_triangle_oracle_vs_moller_trumbore(oracle):
    x = R.triangle_set()
    hit, u, v, t, safe, tol = R.triangle_reference(x)
    y = oracle.probe("triangle", x)
    print(f"triangle: n={len(x)} skipped={1 - safe.mean():.5f} hits={hit.mean():.3f}")
    assert 1 - safe.mean() <= 0.01
    assert not ((y[:, 3] > 0) != hit)[safe].any()
    h = safe & hit
    err = np.abs(y[h, :3] - np.stack([u, v, t], 1)[h])
    assert (err <= tol[h]).all(), float((err / tol[h]).max())
    m = safe & ~hit
    assert (y[m, :2] == 0).all() and np.isinf(y[m, 2]).all()


def test_quad_oracle_is_the_nearer_of_two_triangles(oracle):
    """intersect_quad from its definition: triangles (p1, p2, p4) and (p3, p4, p2), the second's
    (u, v) mirrored, the first only if strictly nearer or the quad is degenerate."""
    x = R.quad_set()
    assert len(x) % 2 == 1
    q = oracle.probe("quad", x)
    t1 = oracle.probe("triangle", np.concatenate([x[:, :8], x[:, 8:14], x[:, 17:20]], 1))[:, :4]
    t2 = oracle.probe("triangle", np.concatenate([x[:, :8], x[:, 14:20], x[:, 11:14]], 1))[:, :4]
    t2 = np.where((t2[:, 3:] > 0), np.concatenate([1 - t2[:, :2], t2[:, 2:]], 1), t2).astype(F32)
    degenerate = (x[:, 14:17] == x[:, 17:20]).all(1)
    ref = np.where((degenerate | (t1[:, 2] < t2[:, 2]))[:, None], t1, t2)
    assert len(R.mismatches(q, ref)) == 0
    assert 0.2 < (q[:, 3] > 0).mean() < 0.9


# ------------------------------------------------------------------------------ E: lobe terms
def _cols(a):
    return [a[:, k].astype(np.float64) for k in range(a.shape[1])]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _check(got, f, xs, K, what, min_share=0.9):
    """got (float32 from the oracle) against f(*xs) in float64 within tolerance(f, xs, K); inputs
    where the tolerance is not finite (a guard threshold between the difference points) are left out.
    The tolerance is first order; (K 2^-24)^2 is added for the second: where f has a double zero
    (the Fresnel reflectance at eta = 1 is the square of a difference that is 0) the first-order
    bound is 0 and the float result is the square of a rounding error."""
    with np.errstate(all="ignore"):
        ref = f(*xs)
        tol = R.tolerance(f, xs, K) + (K * R.EPS) ** 2
    use = np.isfinite(ref) & np.isfinite(tol) & np.isfinite(got)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: n={len(got)} used={use.mean():.4f} max err/tol={np.max(err[use] / np.maximum(tol[use], 1e-300)):.3f}")
    assert use.mean() >= min_share
    assert (err[use] <= tol[use]).all(), what


@pytest.fixture(scope="module")
def lobes(oracle):
    x = R.lobe_set(oracle)
    return x, oracle.probe("parts", x)


def test_fresnel_dielectric_vs_definition(lobes):
    """K = 24: dot 5, |.| 0, sin2 2, eta2 1, cos2t 2, sqrt 1, t1 t2 2, rs 3, rp 3, squares and sum 3, /2 0, + 2 slack."""
    x, y = lobes
    f = lambda eta, nx, ny, nz, ox, oy, oz: R.fresnel_dielectric_ref(eta, _dot((nx, ny, nz), (ox, oy, oz)))
    xs = _cols(x[:, [4, 6, 7, 8, 9, 10, 11]])
    # away from the guards: no total internal reflection (eta >= 1), no grazing direction (at
    # eta = 1, cos = 0 the function is 0/0: the float result is 1, the limit 0)
    keep = (x[:, 4] >= 1) & (np.abs(_dot(xs[1:4], xs[4:7])) > 1e-3)
    _check(y[keep, 0], f, [c[keep] for c in xs], 24, "fresnel_dielectric")


def test_fresnel_conductor_vs_definition(lobes):
    """The conductor of reflectivity r: eta = (1 + sqrt r) / (1 - sqrt r), k = 0. K = 40: eta 4, dot 5,
    cos2 sin2 2, t0 2, a2plusb2 5, t1 1, a 3, t2 2, rs 3, t3 4, t4 1, rp 4, mean 2, + slack.
    Reflectivities from 0.04 (the least of real materials) to 0.98 (the 0.99 clamp): as r -> 0,
    eta -> 1 and rs = (t1 - t2) / (t1 + t2) subtracts two O(1) numbers whose difference is O(r), so
    the absolute error stays about 2^-24 while the first-order bound shrinks with r (measured at
    r = 0.0035: 3.8e-8 against a bound of 1.7e-8); the bound does not describe that range."""
    x, y = lobes

    def f(r, nx, ny, nz, ox, oy, oz):
        c = _dot((nx, ny, nz), (ox, oy, oz))
        rr = np.clip(r, 0, 0.99)
        eta = (1 + np.sqrt(rr)) / (1 - np.sqrt(rr))
        return np.where(c > 0, R.fresnel_conductor_ref(eta, 0.0, np.clip(c, -1, 1)), 0.0)
    for ch in range(3):
        xs = _cols(x[:, [1 + ch, 6, 7, 8, 9, 10, 11]])
        c = _dot(xs[1:4], xs[4:7])
        keep = (np.abs(c) > 1e-3) & (x[:, 1 + ch] < 0.98) & (x[:, 1 + ch] >= 0.04)  # off the cos <= 0 guard
        _check(y[keep, 1 + ch], f, [v[keep] for v in xs], 40, f"fresnel_conductor[{ch}]", min_share=0.8)


def _ggx_case(lobes):
    x, y = lobes

    def half(v):
        n, o, i = v[0:3], v[3:6], v[6:9]
        h = [i[k] + o[k] for k in range(3)]
        l = np.sqrt(_dot(h, h))
        return n, o, i, [c / l for c in h]

    def fd(a, *v):
        n, o, i, h = half(v)
        return R.ggx_d_ref(a, _dot(n, h))

    def fg(a, *v):
        n, o, i, h = half(v)
        return R.smith_g1_ref(a, _dot(n, o), _dot(h, o)) * R.smith_g1_ref(a, _dot(n, i), _dot(h, i))
    xs = _cols(x[:, [5] + list(range(6, 15))])
    with np.errstate(all="ignore"):
        n, o, i, h = half(xs[1:])
        lh = np.sqrt(sum((i[k] + o[k]) ** 2 for k in range(3)))
        # off the guards: a halfway vector that exists, no cosine at a sign test's zero, a rough lobe
        keep = (lh > 1e-2) & (np.abs(_dot(n, h)) > 1e-3) & (x[:, 5] > 0) & (np.abs(_dot(n, o)) > 1e-3) & \
               (np.abs(_dot(n, i)) > 1e-3) & (np.abs(_dot(h, o)) > 1e-3)
    return x, y, xs, keep, fd, fg


def test_ggx_distribution_and_shadowing_vs_definition(lobes):
    """D: K = 18 (h: add 3, dot 5, sqrt, div 3; n.h 5; r2, c2, 4 more, pi, 2 mul, div).
    G = G1(o) G1(i): K = 40 (two G1 of h 12, two dots 10, 8 ops each, one product).
    Roughness from 0.03; the least roughness is the next test's."""
    x, y, xs, keep, fd, fg = _ggx_case(lobes)
    keep = keep & (x[:, 5] >= 0.03)
    _check(y[keep, 22], fd, [v[keep] for v in xs], 18, "microfacet_distribution", min_share=0.5)
    _check(y[keep, 23], fg, [v[keep] for v in xs], 40, "microfacet_shadowing", min_share=0.5)


@pytest.mark.xfail(strict=True, reason="reference formula replicated: c2*r2 + 1 - c2 cancels at the least roughness")
def test_ggx_distribution_at_least_roughness(lobes):
    """At roughness 0.0009 (scene.jl's min_roughness, what every glossy-smooth material is clamped
    to) and n.h within 1e-8 of 1 (incoming = reflect(outgoing)) the reference's denominator
    `c2 * r2 + 1 - c2` adds r2 = 8.1e-7 to 1, whose float spacing is 1.2e-7, before the
    subtraction: the peak of D comes out as 725730 or 283488 where 1 / (pi r2) = 392975 is its
    largest possible value, outside even this test's bound (23 % of the value there). The oracle
    and jt_bsdf.h replicate the expression."""
    x, y, xs, keep, fd, fg = _ggx_case(lobes)
    keep = keep & (x[:, 5] == F32(0.0009))
    assert keep.sum() > 100
    _check(y[keep, 22], fd, [v[keep] for v in xs], 18, "microfacet_distribution at 0.0009", min_share=0.5)


def test_volume_terms_vs_definition(oracle):
    """eval_transmittance = exp(-sigma d), K = 3 (negate, multiply, exp rounded once); the phase
    function is Henyey-Greenstein of cos = -o.i, K = 22 (dot 5, an^2 twice 2, denom 4, sqrt, 4 pi 2,
    products 2, division 1, + slack)."""
    x = R.volume_set()
    y = oracle.probe("volume", x)
    for ch in range(3):
        _check(y[:, ch], lambda s, d: np.exp(-s * d), _cols(x[:, [ch, 15]]), 3, f"transmittance[{ch}]")
    f = lambda g, *v: R.hg_ref(g, -_dot(v[0:3], v[3:6]))
    dens = (x[:, 0:3] != 0).any(1)
    _check(y[dens, 11], f, _cols(x[dens][:, [6] + list(range(7, 13))]), 22, "henyey-greenstein")
    assert (y[~dens, 5:12] == 0).all()  # no density: no scattering


# ------------------------------------------------------------------------------ F: texture lookup
def test_texture_lookup_oracle_vs_bilinear_wrap(oracle):
    for pix, linear in R.texture_set():
        h, w = pix.shape[:2]
        uv = R.texture_uvs(w, h)
        for as_linear in (0, 1):
            got = oracle.probe_texture(pix, linear, np.concatenate([uv, np.full((len(uv), 1), as_linear, F32)], 1))
            ref = R.bilinear_wrap_ref(R.decode_ref(pix, linear, as_linear), uv)
            assert np.abs(got - ref).max() <= R.texture_tolerance(w, h), (pix.shape, pix.dtype, linear, as_linear)


# ------------------------------------------------------------------------------ sampling against pdf
NTH, NPH, SUB = 16, 32, 12


def _sphere_bins(d):
    ct = np.clip(d[:, 2], -1, 1)
    ph = np.arctan2(d[:, 1], d[:, 0]) % (2 * np.pi)
    return np.minimum(((ct + 1) / 2 * NTH).astype(int), NTH - 1) * NPH + np.minimum((ph / (2 * np.pi) * NPH).astype(int), NPH - 1)


def _quadrature_dirs():
    """SUB x SUB midpoints of every (cos theta, phi) bin; each stands for 4 pi / (NTH NPH SUB^2) sr."""
    ct = -1 + 2 * (np.arange(NTH * SUB) + 0.5) / (NTH * SUB)
    ph = 2 * np.pi * (np.arange(NPH * SUB) + 0.5) / (NPH * SUB)
    CT, PH = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1 - CT * CT)
    d = np.stack([st * np.cos(PH), st * np.sin(PH), CT], -1)
    b = (np.arange(NTH * SUB) // SUB)[:, None] * NPH + (np.arange(NPH * SUB) // SUB)[None, :]
    return d.reshape(-1, 3), b.ravel(), 4 * np.pi / (NTH * NPH * SUB * SUB)


def _chi_check(sampled, pdf_at, what):
    """pbrt's sampling test: bin the sampled unit directions on a 16 x 32 (cos theta, phi) grid and
    compare each bin's count with N times the pdf's integral over the bin (midpoint quadrature),
    within 5 sigma of the binomial; bins expecting fewer than 50 are merged into one. Rejected
    samples (the zero vector) count in N and in no bin."""
    N = len(sampled)
    nz = (sampled != 0).any(1)
    ln = np.sqrt((sampled[nz].astype(np.float64) ** 2).sum(1))
    assert np.abs(ln - 1).max() <= 1e-5, (what, float(np.abs(ln - 1).max()))
    obs = np.bincount(_sphere_bins(sampled[nz].astype(np.float64)), minlength=NTH * NPH).astype(np.float64)
    qd, qb, w = _quadrature_dirs()
    p = np.bincount(qb, weights=pdf_at(qd.astype(F32)).astype(np.float64) * w, minlength=NTH * NPH)
    small = N * p < 50
    obs = np.append(obs[~small], obs[small].sum())
    p = np.append(p[~small], p[small].sum())
    sigma = np.sqrt(np.maximum(N * p * (1 - p), 1e-12))
    z = (obs - N * p) / sigma
    keep = N * p >= 50
    print(f"{what}: N={N} rejected={1 - nz.mean():.4f} pdf mass={p.sum():.4f} bins={int(keep.sum())} max |z|={np.abs(z[keep]).max():.2f}")
    assert keep.sum() >= 8
    assert (np.abs(z[keep]) <= 5).all(), (what, float(np.abs(z[keep]).max()))


def _strat2(seed, n=1 << 10):
    """n x n stratified (rn.x, rn.y) on the rand1f lattice, and a seeded rnl each."""
    rng = np.random.default_rng(seed)
    g = (np.arange(n)[:, None] + rng.random((n, n, 2))[..., 0], np.arange(n)[None, :] + rng.random((n, n)))
    rn = np.stack([g[0].ravel() / n, g[1].ravel() / n], 1)
    rn = np.floor(rn * (1 << 24)) * 2.0 ** -24
    return rn.astype(F32), (rng.integers(0, 1 << 24, n * n) * 2.0 ** -24).astype(F32)


# rough refraction: the reference's pdf lacks the eta^2 of the half-vector Jacobian (SURVEY.md
# Appendix B item 9, src/shading.jl:527-533); oracle and device replicate it. Worst bin: hundreds of sigma.
REFRACTIVE_PDF = pytest.mark.xfail(strict=True, reason="reference flaw replicated: sample_refractive_pdf lacks eta^2")
SURFACE_LOBES = [("matte", R.M_MATTE, 0.5, 1.5), ("reflective", R.M_REFLECTIVE, 0.3, 1.5),
                 ("glossy", R.M_GLOSSY, 0.3, 1.5), ("transparent", R.M_TRANSPARENT, 0.3, 1.5),
                 pytest.param("refractive", R.M_REFRACTIVE, 0.3, 1.5, marks=REFRACTIVE_PDF)]


@pytest.mark.parametrize("name,typ,rough,ior", SURFACE_LOBES,
                         ids=["matte", "reflective", "glossy", "transparent", "refractive"])
def test_lobe_sampling_follows_its_pdf(name, typ, rough, ior, oracle):
    n, o = np.array([0, 0, 1], F32), R.unit(np.array([0.6, 0.2, 0.7])).astype(F32)
    rn, rnl = _strat2(40 + typ)

    def rows(i, rnl_, rn_):
        m = len(i)
        head = np.tile(np.array([typ, 0.7, 0.6, 0.5, ior, rough, *n, *o], F32), (m, 1))
        return np.concatenate([head, i, rnl_[:, None], rn_], 1)
    sampled = oracle.probe("bsdf", rows(np.zeros((len(rn), 3), F32), rnl, rn))[:, 3:6]
    pdf_at = lambda d: oracle.probe("bsdf", rows(d, np.zeros(len(d), F32), np.zeros((len(d), 2), F32)))[:, 6]
    _chi_check(sampled, pdf_at, name)


@pytest.mark.parametrize("g", [0.0, 0.5, -0.7])
def test_phase_sampling_follows_its_pdf(g, oracle):
    o = R.unit(np.array([0.3, -0.5, 0.8])).astype(F32)
    rn, _ = _strat2(50 + int(g * 10))

    def rows(i, rn_):
        m = len(i)
        return np.concatenate([np.tile(np.array([1, 1, 1, .5, .5, .5, g, *o], F32), (m, 1)), i, rn_,
                               np.zeros((m, 4), F32)], 1)
    sampled = oracle.probe("volume", rows(np.zeros((len(rn), 3), F32), rn))[:, 8:11]
    pdf_at = lambda d: oracle.probe("volume", rows(d, np.zeros((len(d), 2), F32)))[:, 11]
    _chi_check(sampled, pdf_at, f"hg g={g}")
