"""jt_irradiance, jt_hemisphere_rays (include/jtrace.h) and the lightmap rasteriser of
`python -m jtrace.bake`, the part that needs no GPU: the four exports and their ctypes prototypes,
the argument errors that are reported, in the header's order, before the context is looked at,
texel_hits on small shapes against float64 brute force, and the seed of the analytic scene of
tests/test_gpu_irradiance.py, whose hit count the oracle's directions predict on the CPU.
csrc/jt_radiance.h gains no integer rule (the calls reuse radiance_range_error, which
tests/radiance_plan_check.cpp covers), so there is no stand-alone program here."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import irradiance_ref as IR
import surface_ref as R
from conftest import ROOT

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_irradiance", "jt_irradiance_device", "jt_hemisphere_rays", "jt_hemisphere_rays_device")


def test_the_four_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5 and "#define JT_ABI_VERSION 5" in HEADER.read_text()
    host, dev = [C.c_void_p, C.c_int64, abi.f32p, C.c_int64], [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    assert lib.jt_irradiance.argtypes == host + [C.c_int32, C.c_int32, abi.f32p]
    assert lib.jt_irradiance_device.argtypes == dev + [C.c_int32, C.c_int32, C.c_void_p]
    assert lib.jt_hemisphere_rays.argtypes == host + [C.c_int32, abi.f32p]
    assert lib.jt_hemisphere_rays_device.argtypes == dev + [C.c_int32, C.c_void_p]
    for name in NAMES:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
        kinds = [re.sub(r"\s+\w+$", "", a.strip()).replace("const ", "") for a in decl.split(",")]
        p = "void*" if name.endswith("_device") else "float*"
        samples = ["int32_t", "int32_t"] if "irradiance" in name else ["int32_t"]
        assert kinds == ["jt_ctx*", "int64_t", p, "int64_t"] + samples + [p], (name, kinds)


def test_argument_errors_in_order_need_no_device(abi, lib):
    """Every JT_ERR_INVALID of the header's list names its argument and is reported before the
    context is looked at: the handle below is no context and is never read. Each call breaks one
    rule and, to show the order, every later rule of the list too. n == 0 with valid arguments is
    JT_OK, and nothing is written."""
    pts = np.zeros((4, 6), np.float32)
    out = np.full((4, 6), 7.0, np.float32)
    pp, op = pts.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)
    fake, dev = C.c_void_p(0x10), C.c_void_p(0x1000)
    odd16, odd8 = C.c_void_p(0x1008), C.c_void_p(0x1004)  # off 16 bytes (though on 8), off 8 bytes

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    def irr(ctx=fake, n=4, p=pp, base=0, s0=0, s1=1, o=op):
        return err(lib.jt_irradiance(ctx, n, p, base, s0, s1, o))

    def irr_dev(ctx=fake, n=4, p=dev, base=0, s0=0, s1=1, o=dev):
        return err(lib.jt_irradiance_device(ctx, n, p, base, s0, s1, o))

    def hemi(ctx=fake, n=4, p=pp, base=0, s=0, o=op):
        return err(lib.jt_hemisphere_rays(ctx, n, p, base, s, o))

    def hemi_dev(ctx=fake, n=4, p=dev, base=0, s=0, o=dev):
        return err(lib.jt_hemisphere_rays_device(ctx, n, p, base, s, o))

    late = dict(n=-1, base=-1, s0=-1, s1=-1)  # every later rule broken too
    late1 = dict(n=-1, base=-1, s=-1)
    assert "ctx" in irr(ctx=None, p=None, o=None, **late) and "ctx" in irr_dev(ctx=None, p=None, o=odd16, **late)
    assert "ctx" in hemi(ctx=None, p=None, o=None, **late1) and "ctx" in hemi_dev(ctx=None, p=None, o=odd8, **late1)
    assert re.match(r"points\b", irr(p=None, o=None, **late)) and re.match(r"d_points\b", irr_dev(p=None, o=None, **late))
    assert re.match(r"points\b", hemi(p=None, o=None, **late1)) and re.match(r"d_points\b", hemi_dev(p=None, o=None, **late1))
    assert re.match(r"rgba\b", irr(o=None, **late)) and re.match(r"d_rgba\b", irr_dev(o=None, **late))
    assert re.match(r"rays\b", hemi(o=None, **late1)) and re.match(r"d_rays\b", hemi_dev(o=None, **late1))
    for call, o in ((irr, op), (irr_dev, odd16)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s0=-1, s1=-1, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(n=2**30, base=2**30 + 1, s0=-1, s1=-1, o=o))
        assert re.match(r"sample_begin\b", call(s0=-1, s1=-5, o=o))
        assert re.match(r"sample_end must\b", call(s0=3, s1=3, o=o)) and re.match(r"sample_end must\b", call(s0=3, s1=2, o=o))
        assert "2^24" in call(s0=5, s1=5 + 2**24 + 1, o=o)
    for call, o in ((hemi, op), (hemi_dev, odd8)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s=-1, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s=-1, o=o))
        assert re.match(r"sample must\b", call(s=-1, o=o)) and re.match(r"sample must\b", call(s=-2**31, o=o))
    assert re.match(r"d_rgba\b.*aligned to 16", irr_dev(o=odd16)) and re.match(r"d_rgba\b.*aligned", irr_dev(n=0, o=odd8))
    assert re.match(r"d_rays\b.*aligned to 8", hemi_dev(o=odd8)) and re.match(r"d_rays\b.*aligned", hemi_dev(n=0, o=odd8))
    # a ray record needs 8 bytes only: what is off 16 but on 8 passes the checks (n == 0: no device work)
    assert lib.jt_hemisphere_rays_device(fake, 0, dev, 0, 0, odd16) == 0
    # the largest arguments that break no rule reach the n == 0 return: JT_OK, no device work
    assert lib.jt_irradiance(fake, 0, pp, 2**31, 2**31 - 2, 2**31 - 1, op) == 0
    assert lib.jt_irradiance(fake, 0, pp, 0, 0, 2**24, op) == 0
    assert lib.jt_irradiance_device(fake, 0, dev, 0, 0, 1, dev) == 0
    assert lib.jt_hemisphere_rays(fake, 0, pp, 2**31, 2**31 - 1, op) == 0
    assert lib.jt_hemisphere_rays_device(fake, 0, dev, 0, 0, dev) == 0
    assert (out == 7.0).all() and (pts == 0).all()


# ------------------------------------------------------------------------------ texel_hits
def _shape(texcoords, triangles=None, quads=None):
    from jtrace.scene import ShapeData
    n = len(texcoords)
    rng = np.random.default_rng(3)
    s = ShapeData(positions=rng.normal(size=(n, 3)).astype(np.float32), texcoords=np.asarray(texcoords, np.float32))
    if triangles is not None:
        s.triangles = np.asarray(triangles, np.int32)
    if quads is not None:
        s.quads = np.asarray(quads, np.int32)
    return s


def _uv_triangles(shape):
    """Every element's uv triangles, in order: [(element, a, b, c)] in float64."""
    tc = np.asarray(shape.texcoords, np.float64)
    if len(shape.triangles):
        return [(e, *tc[t]) for e, t in enumerate(shape.triangles)]
    return [(e, *tc[q[list(k)]]) for e, q in enumerate(shape.quads) for k in ((0, 1, 3), (2, 3, 1))]


def _inside(p, a, b, c):
    """p in the closed uv triangle, by float64 edge functions of either orientation."""
    def edge(s, t):
        return (t[0] - s[0]) * (p[1] - s[1]) - (t[1] - s[1]) * (p[0] - s[0])
    e = np.array([edge(a, b), edge(b, c), edge(c, a)])
    return bool((e >= 0).all() or (e <= 0).all()) and edge(a, b) + edge(b, c) + edge(c, a) != 0


def _check(shape, w, h):
    """texel_hits against brute force: a texel is covered iff its centre is inside some uv triangle,
    the element is the lowest that contains it, and surface_ref.texcoord of the record gives the
    centre back within 1e-6. Returns (element, u, v)."""
    from jtrace.bake import texel_hits
    from jtrace.scene import InstanceData, SceneData, identity_frame
    elem, u, v = texel_hits(shape, w, h)
    assert elem.shape == u.shape == v.shape == (h, w) and elem.dtype == np.int32 and u.dtype == v.dtype == np.float32
    tris = _uv_triangles(shape)
    for j in range(h):
        for i in range(w):
            p = ((i + 0.5) / w, (j + 0.5) / h)
            owners = [e for e, a, b, c in tris if _inside(p, a, b, c)]
            assert elem[j, i] == (min(owners) if owners else -1), (i, j, elem[j, i], owners)
    sc = SceneData(shapes=[shape], instances=[InstanceData(frame=identity_frame(), shape=0, material=0)])
    jj, ii = np.nonzero(elem >= 0)
    if len(jj):
        tc, _ = R.texcoord(sc, np.zeros(len(jj), np.int64), elem[jj, ii].astype(np.int64), u[jj, ii], v[jj, ii])
        centre = np.stack([(ii + 0.5) / w, (jj + 0.5) / h], -1)
        assert np.abs(tc - centre).max() <= 1e-6, np.abs(tc - centre).max()
    return elem, u, v


def test_texel_hits_of_a_quad_covers_the_texels_whose_centres_lie_inside():
    quad = _shape([[0.25, 0.25], [0.75, 0.25], [0.75, 0.75], [0.25, 0.75]], quads=[[0, 1, 2, 3]])
    elem, u, v = _check(quad, 8, 8)
    want = np.zeros((8, 8), bool)
    want[2:6, 2:6] = True  # centres 0.3125 .. 0.6875
    assert np.array_equal(elem >= 0, want) and (elem >= 0).sum() == 16
    # both halves and the diagonal u + v = 1, which the first triangle takes: uv as interpolate_quad reads it
    s = (u + v)[want]
    assert (s < 1).any() and (s > 1).any() and (s == 1).sum() == 4
    assert np.allclose(u[2:6, 2:6], np.tile((np.arange(2, 6) + 0.5) / 4 - 0.5, (4, 1)), atol=1e-6)
    assert np.allclose(v[2:6, 2:6], np.tile((np.arange(2, 6) + 0.5) / 4 - 0.5, (4, 1)).T, atol=1e-6)


def test_texel_hits_of_a_triangle_pair_with_an_overlap_and_odd_sizes():
    # two triangles that share an edge, the second turned the other way round, and a third that
    # overlaps both: the lowest element wins; a zero-area triangle covers nothing
    tc = [[0.1, 0.1], [0.9, 0.15], [0.85, 0.9], [0.05, 0.8], [0.3, 0.3], [0.7, 0.35], [0.5, 0.95], [0.2, 0.2], [0.4, 0.4], [0.6, 0.6]]
    tris = _shape(tc, triangles=[[0, 1, 2], [0, 3, 2], [4, 5, 6], [7, 8, 9]])
    for w, h in ((8, 8), (13, 7), (1, 1), (5, 16)):
        elem, _, _ = _check(tris, w, h)
        assert not (elem == 3).any()
    elem, _, _ = _check(tris, 16, 16)
    assert (elem == 0).any() and (elem == 1).any()
    # element 2 lies inside 0 and 1 except for its tip: where it overlaps them, they win
    a, b, c = (np.asarray(tc[k], np.float32).astype(np.float64) for k in (4, 5, 6))
    under = np.array([[_inside(((i + 0.5) / 16, (j + 0.5) / 16), a, b, c) for i in range(16)] for j in range(16)])
    assert under.sum() > 10 and np.isin(elem[under], (0, 1)).all()
    # a skewed quad whose texcoords reach outside [0, 1]: no wrap, the outside is cut off
    skew = _shape([[-0.2, 0.1], [0.6, -0.1], [1.3, 0.7], [0.2, 1.1]], quads=[[0, 1, 2, 3], [0, 1, 2, 3]])
    elem, u, v = _check(skew, 9, 11)
    assert (elem == 0).sum() > 40 and not (elem == 1).any() and ((u + v)[elem == 0] > 1).any() and ((u + v)[elem == 0] < 1).any()


def test_texel_hits_rejects_what_has_no_surface_to_bake():
    import pytest
    from jtrace.bake import texel_hits
    from jtrace.scene import ShapeData
    with pytest.raises(ValueError, match="no texcoords"):
        texel_hits(ShapeData(positions=np.zeros((3, 3), np.float32), triangles=np.array([[0, 1, 2]], np.int32)), 4, 4)
    lines = _shape([[0, 0], [1, 1]])
    lines.lines = np.array([[0, 1]], np.int32)
    with pytest.raises(ValueError, match="lines"):
        texel_hits(lines, 4, 4)


# ------------------------------------------------------------------------------ the analytic scene's seed
def test_the_square_scenes_seed_lies_inside_both_bounds(oracle):
    """tests/test_gpu_irradiance.py number 5, decided before any GPU runs: the oracle's directions of
    the 64 x 1024 gathers and a float64 ray-square test give the exact number of gathers that meet
    the square; its share is within 5 standard errors of F, which is both of that test's bounds
    (rgb = L (1 - share), alpha = share under envhidden)."""
    assert abs(IR.SQUARE_F - 0.55413) < 1e-5
    hits = IR.square_hits(oracle, IR.SQUARE_SEED)
    share = hits / (IR.SQUARE_POINTS * IR.SQUARE_SAMPLES)
    print("hits", hits, "share", share, "F", IR.SQUARE_F, "deviation in standard errors", (share - IR.SQUARE_F) / IR.SQUARE_SE)
    assert abs(share - IR.SQUARE_F) <= 5 * IR.SQUARE_SE
