"""Device primitives one by one (tests/probe/jt_probe.hip compiles csrc/jt_device.h and jt_bsdf.h
with the product's flags, one kernel per primitive) against the oracle's probes, bit for bit, and
against the float64 references and input sets of tests/primitives_ref.py. The CPU half
(tests/test_primitives_host.py) checks the oracle against the same references and establishes the
counts this file relies on (no ambiguous sin/cos input, the atan sets' ambiguous counts).
"""
import numpy as np
import pytest

import primitives_ref as R
from primitives_ref import F32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(gpu):
    return R.Probe()  # a missing probe library is an error, not a skip


def _mp(name):
    import mpmath
    return getattr(mpmath, name)


def _rows(x, idx, k=4):
    return [x[j].tolist() for j in idx[:k]]


# ------------------------------------------------------------------------------ A: sin / cos
@pytest.fixture(scope="module")
def phi_ref():
    phi = R.phi_all().astype(np.float64)
    return np.sin(phi).astype(F32), np.cos(phi).astype(F32)


def test_sincos_every_azimuth(probe, phi_ref):
    """jl_sincos(phi), phi = (2 pif) u for all 2^24 rand1f values u, is float32(sin / cos(float64
    phi)) bit for bit: DESIGN §3's "evaluated in double and rounded once". No exception is allowed:
    the set has no input within 4 double-ulps of a rounding midpoint (the CPU half proves it)."""
    out = probe.run("sincos", R.phi_all())
    bad = R.mismatches(out[:, :2], np.stack(phi_ref, 1))
    print(f"sincos: n={len(out)} mismatches={len(bad)}")
    assert len(bad) == 0, (_rows(R.phi_all(), bad), _rows(out, bad))
    # "evaluated in double": the doubles that were rounded are those of the documented algorithm
    # (Cody-Waite by pi/2, fdlibm kernels) evaluated without fused operations, bit for bit. This
    # is what notices an FMA contracted into the reduction; the rounded floats almost never do.
    d = R.doubles_of(out[:, 2:])
    rs, rc = R.dsincos_small_np(R.phi_all().astype(np.float64))
    nbad = int((d[:, 0].view(np.uint64) != rs.view(np.uint64)).sum() + (d[:, 1].view(np.uint64) != rc.view(np.uint64)).sum())
    print(f"sincos doubles: differing={nbad}")
    assert nbad == 0


def test_disk_signs_every_azimuth(probe, phi_ref):
    """sample_disk((u, 1)) is (cos phi, sin phi) rounded, and sample_disk_signs((u, 1)) has exactly
    its signs, for every rand1f value u (jt_device.h's claim for the aperture == 0 camera)."""
    out = probe.run("disk", R.rand_u())
    s, c = phi_ref
    assert len(R.mismatches(out[:, :2], np.stack([c, s], 1))) == 0
    assert (np.abs(out[:, 2:]) == 0).all()
    bad = np.flatnonzero((np.signbit(out[:, 2:]) != np.signbit(out[:, :2])).any(1))
    print(f"disk signs: n={len(out)} violations={len(bad)}")
    assert len(bad) == 0, _rows(R.rand_u(), bad)


def test_sincos_edges(probe):
    """The switch to the large-argument path at 2^19 (524287.97 is the last float below it), a huge
    argument, inf and NaN. sin(-0.0): the reduction x - n * pio2 turns -0.0 into +0.0, where the
    double sine keeps the sign; no caller can pass -0.0 (phi = 2 pif u with u >= +0, theta =
    atan(x >= +0), v pi and u 2 pi of texture coordinates in [0, 1]), so the zero's sign is free."""
    e = R.SINCOS_EDGES
    out = probe.run("sincos", e)
    finite = np.isfinite(e)
    assert np.isnan(out[~finite, :2]).all()
    e64 = e[finite].astype(np.float64)
    for col, fn, mp in ((0, np.sin, "sin"), (1, np.cos, "cos")):
        bad, _, _ = R.check_rounded(out[finite, col], [e64], fn, _mp(mp), cap=1.0, what=f"edges {mp}")
        bad = [b for b in bad if not (e64[b] == 0 and out[finite][b, col] == 0)]  # the free sign of sin(-0.0)
        assert not bad, (e64[bad], out[finite][bad])


# ------------------------------------------------------------------------------ B: atan and the rest
@pytest.mark.parametrize("rough", R.ROUGHNESSES)
def test_atan_every_microfacet_argument(rough, probe):
    """jl_atan over sample_microfacet's whole argument set at one roughness, and jl_sincos of the
    angles it returns: the correctly rounded float, except within 4 double-ulps of a midpoint."""
    x = R.atan_args(rough)
    out = probe.run("atan", x)
    bad, _, _ = R.check_rounded(out[:, 0], [x.astype(np.float64)], np.arctan, _mp("atan"), what=f"atan rough={rough}")
    assert len(bad) == 0, (_rows(x, bad), _rows(out, bad))
    th = out[:, 0].astype(np.float64)
    for col, fn, mp in ((1, np.sin, "sin"), (2, np.cos, "cos")):
        bad, _, _ = R.check_rounded(out[:, col], [th], fn, _mp(mp), what=f"{mp}(atan) rough={rough}")
        assert len(bad) == 0, (th[bad[:4]], _rows(out, bad))
    d = R.doubles_of(out[:, 3:])  # the doubles behind that sincos, as in test_sincos_every_azimuth
    rs, rc = R.dsincos_small_np(th)
    assert int((d[:, 0].view(np.uint64) != rs.view(np.uint64)).sum() + (d[:, 1].view(np.uint64) != rc.view(np.uint64)).sum()) == 0


@pytest.mark.parametrize("op,make,fn", [("atan2", R.atan2_set, np.arctan2), ("acos", R.acos_set, np.arccos),
                                        ("log", R.log_set, np.log), ("exp", R.exp_set, np.exp)])
def test_rare_transcendentals(op, make, fn, probe, oracle):
    """jl_atan2 / acos / log / exp over their callers' domains (2^20 stratified, plus edges): the
    correctly rounded float under the same rule, and the oracle's value off the ambiguous inputs."""
    x = make()
    out = probe.run(op, x)
    cols = [c.astype(np.float64) for c in (x.T if x.ndim == 2 else [x])]
    bad, amb, _ = R.check_rounded(out[:, 0], cols, fn, _mp(op), what=op)
    assert len(bad) == 0, (_rows(x, bad), _rows(out, bad))
    assert len(R.mismatches(out, oracle.probe(op, x))) <= amb


# ------------------------------------------------------------------------------ C: min / max / rcp
def test_minmax_every_triple(probe, oracle):
    """jl_min / jl_max / jl_min3 / jl_max3 / max3(v3) / jl_clamp over every triple of {+-0,
    +-denormal, +-1, +-FLT_MAX, +-inf, NaN}: IEEE 754-2019 minimum / maximum (Julia's rule: NaN
    propagates, -0 < +0; a denormal is not flushed), any NaN standing for NaN."""
    t = R.minmax_triples()
    out = probe.run("minmax", t)
    bad = R.mismatches(out, R.minmax_reference(t))
    assert len(bad) == 0, (_rows(t, bad), _rows(out, bad))
    assert len(R.mismatches(out, oracle.probe("minmax", t))) == 0


def test_rcp_every_exponent(probe):
    """jl_rcp against the IEEE division 1 / x it replaces, every exponent x 2^12 mantissas x both
    signs: zeros, denormals (in and out), 2^126 and above, inf, NaN."""
    x = R.rcp_set()
    out = probe.run("rcp", x)
    with np.errstate(all="ignore"):
        ref = F32(1) / x
    bad = R.mismatches(out, ref)
    assert len(bad) == 0, (x[bad[:4]], out[bad[:4]], ref[bad[:4]])


# ------------------------------------------------------------------------------ D: intersection
def test_bbox(probe, oracle):
    x = R.bbox_set()
    out = probe.run("bbox", x)
    bad = R.mismatches(out, oracle.probe("bbox", x))
    assert len(bad) == 0, _rows(x, bad)
    hit, margin = R.bbox_reference(x)
    ok = margin > 4 * R.EPS
    print(f"bbox: n={len(x)} skipped share={1 - ok.mean():.5f}")
    assert 1 - ok.mean() <= 0.01
    assert not ((out[:, 0] > 0) != hit)[ok].any()


def test_triangle_three_forms(probe, oracle):
    """intersect_triangle, intersect_triangle_e and intersect_triangle_pre + tri_hit_before give the
    oracle's (u, v, t, hit) bit for bit, and Moller-Trumbore's decision in float64 wherever that is
    farther from every threshold than float rounding."""
    x = R.triangle_set()
    out = probe.run("triangle", x)
    bad = R.mismatches(out, oracle.probe("triangle", x))
    assert len(bad) == 0, (_rows(x, bad), _rows(out, bad))
    hit, u, v, t, safe, tol = R.triangle_reference(x)
    print(f"triangle: n={len(x)} skipped share={1 - safe.mean():.5f}")
    assert 1 - safe.mean() <= 0.01
    for k in (0, 4, 8):
        assert not ((out[:, k + 3] > 0) != hit)[safe].any()
        h = safe & hit
        assert (np.abs(out[h, k:k + 3] - np.stack([u, v, t], 1)[h]) <= tol[h]).all()


def test_quad(probe, oracle):
    x = R.quad_set()
    out = probe.run("quad", x)
    bad = R.mismatches(out, oracle.probe("quad", x))
    assert len(bad) == 0, (_rows(x, bad), _rows(out, bad))
    # the decision in float64: the nearer of the two triangles' Moller-Trumbore hits, where both are safe
    a = np.concatenate([x[:, :8], x[:, 8:14], x[:, 17:20]], 1)
    b = np.concatenate([x[:, :8], x[:, 14:20], x[:, 11:14]], 1)
    h1, _, _, _, s1, _ = R.triangle_reference(a)
    h2, _, _, _, s2, _ = R.triangle_reference(b)
    degenerate = (x[:, 14:17] == x[:, 17:20]).all(1)
    safe = s1 & (s2 | degenerate)
    print(f"quad: n={len(x)} skipped share={1 - safe.mean():.5f}")
    assert 1 - safe.mean() <= 0.01
    assert not ((out[:, 3] > 0) != np.where(degenerate, h1, h1 | h2))[safe].any()


# ------------------------------------------------------------------------------ E: lobes
@pytest.fixture(scope="module")
def lobe_rows(oracle):
    return R.lobe_set(oracle)


def test_lobes_through_the_dispatchers(probe, oracle, lobe_rows):
    """eval / sample / pdf of every rough and delta lobe through the <FT_ALL> dispatchers, bit for
    bit with the oracle (NaN equal to NaN); no input is excluded."""
    out = probe.run("bsdf", lobe_rows)
    ref = oracle.probe("bsdf", lobe_rows)
    bad = R.mismatches(out, ref)
    print(f"bsdf: n={len(out)} mismatches={len(bad)} nonzero share={np.mean(ref != 0):.3f}")
    assert len(bad) == 0, (_rows(lobe_rows, bad, 2), _rows(out, bad, 2), _rows(ref, bad, 2))
    for t in range(7):  # every material type exercised its lobes
        assert (ref[lobe_rows[:, 0] == t] != 0).any()


def test_fused_eval_pdf_equals_the_two_calls(probe, lobe_rows):
    """jt_bsdf.h: eval_bsdfcos_pdf's results "are unchanged" against eval_bsdfcos and
    sample_bsdfcos_pdf called separately: bit-equal on the device, every row."""
    out = probe.run("bsdf", lobe_rows)
    bad = R.mismatches(out[:, 14:18], out[:, [0, 1, 2, 6]])
    assert len(bad) == 0, (_rows(lobe_rows, bad, 2), _rows(out, bad, 2))


def test_lobe_parts(probe, oracle, lobe_rows):
    """fresnel_dielectric, fresnel_conductor, basis_fromz, sample_hemisphere_cos, sample_microfacet,
    refract, the GGX distribution and shadowing, called directly: bit for bit with the oracle."""
    out = probe.run("parts", lobe_rows)
    ref = oracle.probe("parts", lobe_rows)
    bad = R.mismatches(out, ref)
    print(f"parts: n={len(out)} mismatches={len(bad)}")
    assert len(bad) == 0, (_rows(lobe_rows, bad, 2), _rows(out, bad, 2), _rows(ref, bad, 2))


def test_volume_functions(probe, oracle):
    """eval_transmittance, sample_transmittance(_pdf), eval / sample_scattering(_pdf): bit for bit
    with the oracle over densities with zeros, the anisotropies around the 0.001 switch, rn on 0 and
    1 - 2^-24."""
    x = R.volume_set()
    out = probe.run("volume", x)
    ref = oracle.probe("volume", x)
    bad = R.mismatches(out, ref)
    print(f"volume: n={len(out)} mismatches={len(bad)}")
    assert len(bad) == 0, (_rows(x, bad, 2), _rows(out, bad, 2), _rows(ref, bad, 2))


# ------------------------------------------------------------------------------ F: texture lookup
def test_texture_lookup_hand_built_scene(probe, oracle):
    """eval_texture on a DScene holding textures only (texel storage, offsets and the one padding
    texel by the host layout's rule, the decode LUTs staged into LDS as the trace kernels stage
    them): every size x format, the last texture a byte one, every pair of the special coordinates
    (0, 1, -1, 2.5, k / W exactly, -1e-10, 1 - 2^-24, 1e6), as_linear on and off. Bit for bit with
    the oracle's eval_texture, and float64 bilinear-with-wrap within the lookup's rounding."""
    tex = R.texture_set()
    qs, refs, f64, tols = [], [], [], []
    for k, (pix, linear) in enumerate(tex):
        h, w = pix.shape[:2]
        uv = R.texture_uvs(w, h)
        for as_linear in (0, 1):
            n = len(uv)
            qs.append(np.concatenate([np.full((n, 1), k, F32), uv, np.full((n, 1), as_linear, F32)], 1))
            refs.append(oracle.probe_texture(pix, linear, qs[-1][:, 1:]))
            f64.append(R.bilinear_wrap_ref(R.decode_ref(pix, linear, as_linear), uv))
            tols.append(np.full(n, R.texture_tolerance(w, h)))
    q = np.concatenate(qs)
    q = q if len(q) % 2 else q[:-1]
    out = probe.run_texture(tex, oracle.srgb_lut(), q)
    bad = R.mismatches(out, np.concatenate(refs)[: len(q)])
    print(f"texture: n={len(q)} mismatches={len(bad)}")
    assert len(bad) == 0, (_rows(q, bad), _rows(out, bad))
    assert (np.abs(out - np.concatenate(f64)[: len(q)]).max(1) <= np.concatenate(tols)[: len(q)]).all()


def test_textured_emitter_render(gpu, abi, lib, oracle):
    """The same lookup through the real jt_create path: an orthographic camera over one quad whose
    texcoords span [-1.5, 2.5] in both directions (four wraps each way), emissive through the
    scene's last byte texture (its last texel's pair load reads the padding texel), 1 spp at
    33 x 17: bit-identical to the oracle in every pixel."""
    from conftest import make_params
    from jtrace import scene as S, trace
    sc = S.SceneData()
    sc.cameras.append(S.CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1], F32), orthographic=True,
                                   lens=F32(1), film=F32(1), aspect=F32(33 / 17), focus=F32(1), aperture=F32(0)))
    for pix, linear in R.texture_set()[-3:]:  # 3x2: byte linear, float, byte sRGB last
        sc.textures.append(S.TextureData(width=pix.shape[1], height=pix.shape[0], linear=linear,
                                         pixelsf=pix if pix.dtype == F32 else None,
                                         pixelsb=pix if pix.dtype == np.uint8 else None))
    sc.materials.append(S.MaterialData(type="matte", emission=np.ones(3, F32), color=np.full(3, 0.5, F32),
                                       emission_tex=len(sc.textures) - 1))
    sc.shapes.append(S.ShapeData(quads=np.array([[0, 1, 2, 3]], np.int32),
                                 positions=np.array([[-.6, -.4, 0], [.6, -.4, 0], [.6, .4, 0], [-.6, .4, 0]], F32),
                                 texcoords=np.array([[-1.5, -1.5], [2.5, -1.5], [2.5, 2.5], [-1.5, 2.5]], F32)))
    sc.instances.append(S.InstanceData(frame=S.identity_frame(), shape=0, material=0))
    sa = abi.SceneABI(sc)
    p = make_params(abi, resolution=33, samples=1)
    st = trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib), p, lib)
    st.trace_range(0, 1)
    img = st.get_image()
    st.close()
    assert img.shape[:2] == (17, 33)
    ref = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), p, 33, 17, 0, 1)[0]
    assert len(np.unique(ref[..., :3].reshape(-1, 3), axis=0)) > 100  # the texture is what is seen
    assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(ref, F32).view(np.uint32)), \
        int((img != ref).any(-1).sum())
