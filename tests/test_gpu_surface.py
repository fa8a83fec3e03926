"""The surface at a hit on the GPU (csrc/jt_surface.hip behind jt_eval_hits, jt_camera_rays, jt_gbuffer
and their device-pointer variants): against the oracle bit for bit, against float64, against itself.

Images are 67 x 45 (3015 pixels, an odd count: the last wave of every launch is partial). The scenes
are tests/surface_ref.py's: OPAQUE ones, where nothing lowers an opacity below 1 (checked on the CPU,
tests/test_surface_host.py) and no pixel is excluded; ROUNDED ones, opaque scenes whose interpolated
alpha (colour textures, vertex colours) can round a few ulp below 1 (features1: one pixel of sample 7);
and OPACITY ones. In the last two a pixel is left out of the oracle comparison only when its own
record has opacity < 1 (there the integrator passes through at random; the G-buffer reports the
first geometric hit).

Against the oracle: a one-sample oracle trace has weight 1, so its AOVs are lerp(0, x, 1) =
0 * 0 + x * 1 of the sample's own albedo and normal (src/trace.jl:631-648): x itself, except that a
-0.0 becomes +0.0. The device's bits are compared after the same float32 operation.

Against float64 (tests/surface_ref.py, written from src/scene.jl): |device - ref| <= 16 * 2^-24 * A
componentwise, A the sum of the absolute values of the terms added to form the value. Derivation: at
most eight float32 roundings lie on the way from the inputs to a value (the weight 1 - u - v, three
products and two sums of the interpolation, three products and three sums of the frame transform,
counted along the longest chain), each at most 2^-24 relative to a partial sum that A bounds;
doubled for the rounding of the partial sums' own inputs. A normalised vector gets that bound times
the conditioning factor of its normalisations, computed in float64 and printed: for an element normal
|e1||e2| / |e1 x e2| (a quad: its worse triangle's, times 2 / |n1 + n2|), for an interpolated vertex
normal sum |w_k n_k| / |sum w_k n_k|. Two values get a larger A than the literal sum of their own terms,
because their error is not relative to themselves (tests/surface_ref.py): a component of a unit
normal comes from a cross product's component, a difference of products of the whole edges, so its
A is that of a vector whose every component is as large as its length (the frame's absolute column
sums over the transformed normal's length); and a lens sample's cos and sin move by the rounding of
the angle phi = 2 pi u itself, so their A is r (|cos or sin| + phi). The sign of the flip towards -d
is taken in float32 on the device: where float64 puts dot(normal, -d) within 1e-5 |d| of zero either
sign is accepted, and such records are asserted to be fewer than 1 %. A shading normal from a normal map is compared with the oracle
only (bit for bit, above). Fields that are exact float32 functions of the record's own texcoord
(emission, colour, opacity, metallic, roughness without vertex colours) are restated in float32 with
the oracle's eval_texture and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as R
from conftest import make_params

pytestmark = pytest.mark.gpu

W, H, N = R.W, R.H, R.W * R.H
F32, F64 = np.float32, np.float64
BOUND = 16 * 2.0 ** -24
SEED = 0x5EED


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def lerp1(x):
    """lerp(0, x, 1) in float32: the one-sample running mean of the reference."""
    x = np.asarray(x, F32)
    return F32(0) * F32(0) + x * F32(1)


class Case:
    """A test scene with its contexts (one per traversal order, opened on demand) and the oracle's
    scene, built once for the module."""

    def __init__(self, name, abi, lib, oracle):
        self.name, self.abi, self.lib, self.oracle = name, abi, lib, oracle
        self.scene, self.kw, self.opts = R.case(name)
        self.sa = abi.SceneABI(self.scene)
        self.bvh, self.lights = oracle.build_bvh(self.sa), oracle.make_lights(self.sa)
        self.states, self.aovs, self.gb = {}, {}, {}
        self.aspect = F32(W) / F32(H)

    def params(self, order="near", **kw):
        return make_params(self.abi, width=W, height=H, traversal=order, **{**self.kw, **kw})

    def state(self, order="near"):
        from jtrace import trace
        if order not in self.states:
            try:
                for k, v in self.opts.items():
                    self.abi.set_option(self.lib, k, v)
                self.states[order] = trace.TraceState(self.sa, self.bvh, self.lights, self.params(order), self.lib)
            finally:
                self.abi.set_option(self.lib, None, None)
            assert (self.states[order].width, self.states[order].height) == (W, H)
        return self.states[order]

    def gbuffer(self, order, sample):
        """st.gbuffer(sample), computed once and shared (read-only)."""
        key = (order, sample)
        if key not in self.gb:
            self.gb[key] = self.state(order).gbuffer(sample)
            for a in self.gb[key]:
                a.setflags(write=False)
        return self.gb[key]

    def oracle_aovs(self, order, sample):
        """The oracle's one-sample trace of `sample` with the running mean starting there: weight 1."""
        key = (order, sample)
        if key not in self.aovs:
            o = self.oracle.trace(self.sa, self.bvh, self.lights, self.params(order), W, H, sample, sample + 1, first=sample)
            self.aovs[key] = (o[1].reshape(N, 3), o[2].reshape(N, 3), o[3].reshape(N))
        return self.aovs[key]

    def close(self):
        for st in self.states.values():
            st.close()


class Cases(dict):
    def __init__(self, *a):
        super().__init__()
        self.args = a

    def __missing__(self, name):
        self[name] = Case(name, *self.args)
        return self[name]


@pytest.fixture(scope="module")
def cases(gpu, abi, lib, oracle):
    c = Cases(abi, lib, oracle)
    yield c
    for v in c.values():
        v.close()


def orders(name):
    return ("reference", "near", "wide") if name in R.ALL_ORDERS else ("near",)


# ------------------------------------------------------------------------------ 1: the oracle
@pytest.mark.parametrize("name", R.OPAQUE + R.ROUNDED + R.OPACITY)
def test_gbuffer_equals_the_oracle_bit_for_bit(name, cases):
    """Samples 0 and 7 (the oracle's `first` argument starts the running mean at the sample, so its
    weight is 1): on a hit pixel the bits of colour and normal are the albedo and normal AOVs'; on a
    miss pixel the record is all zero, the normal AOV is the camera ray's -d, and the oracle counts a
    hit exactly when the scene has an environment the camera sees."""
    c = cases[name]
    describe = c.state("near").describe()
    assert ("mode=hbm" in describe) if name == "cornell_hbm" else True, describe
    assert ("mode=lds" in describe) if name == "cornell" else True, describe
    env = len(c.scene.environments) != 0  # envhidden is off
    for order in orders(name):
        for sample in (0, 7):
            rays, hits, surf = c.gbuffer(order, sample)
            alb, nrm, cnt = c.oracle_aovs(order, sample)
            hit = surf["hit"] != 0
            assert np.array_equal(hit, hits["hit"] != 0) and set(np.unique(surf["hit"])) <= {0, 1}
            excluded = hit & (surf["opacity"] < 1)
            label = (name, order, sample)
            print(label, "pixels", N, "hits", int(hit.sum()), "excluded (opacity < 1)", int(excluded.sum()),
                  "-0.0 components", int((bits(surf["normal"][hit]) == 0x80000000).sum()))
            if name in R.OPAQUE:
                assert excluded.sum() == 0, label
            elif name in R.ROUNDED:  # an interpolated alpha a few ulp below 1, nothing else
                assert (surf["opacity"][excluded] >= R.ROUNDED_MIN).all(), label
            else:
                assert 0 < excluded.sum(), label
            m = hit & ~excluded
            assert m.sum() > 100 or name in R.OPACITY, label
            for field, aov in (("color", alb), ("normal", nrm)):
                bad = np.flatnonzero(m & (bits(lerp1(surf[field])) != bits(aov)).any(1))
                assert len(bad) == 0, (label, field, len(bad), bad[:4], surf[field][bad[:4]], aov[bad[:4]])
            assert (cnt[m] == 1).all(), label
            miss = ~hit
            bad = np.flatnonzero(miss & (bits(lerp1(-rays[:, 3:6])) != bits(nrm)).any(1))
            assert len(bad) == 0, (label, "camera ray of a miss", len(bad), bad[:4])
            assert (surf[miss].view(np.uint32).reshape(-1, 24) == 0).all(), (label, "miss record")
            assert (cnt[miss] == (1 if env else 0)).all(), (label, "hits of a miss")
            assert (bits(alb[miss]) == bits(F32(1 if env else 0))).all(), label


# ------------------------------------------------------------------------------ 2: float64
def within(dev, ref, A, cond, label):
    err = np.abs(np.asarray(dev, F64) - ref)
    bound = BOUND * A * cond
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    print(label, "max error / bound", float(ratio.max()) if ratio.size else 0.0, "max conditioning", float(np.max(cond)) if np.size(cond) else 1.0)
    bad = np.flatnonzero((err > bound).reshape(len(err), -1).any(1))
    assert len(bad) == 0, (label, len(bad), bad[:4], np.asarray(dev)[bad[:4]], ref[bad[:4]], bound[bad[:4]])


_draws = {}


def draws_of(oracle, sample):
    """The four draws that start every pixel's sample (or_rng_first), computed once."""
    if sample in _draws:
        return _draws[sample]
    out = _draws[sample] = np.empty((N, 4), F32)
    one = np.empty(4, F32)
    for pixel in range(N):
        oracle.lib.or_rng_first(SEED, pixel, sample, 4, one.ctypes.data_as(C.POINTER(C.c_float)))
        out[pixel] = one
    return out


@pytest.mark.parametrize("name", R.OPAQUE + R.ROUNDED + R.OPACITY)
def test_records_against_float64(name, cases, oracle):
    c = cases[name]
    sc = c.scene
    for sample in (0, -1):
        rays, hits, surf = c.gbuffer("near", sample)
        label = f"{name}/{sample}"
        # ---- the camera rays
        cam = sc.cameras[0]
        if sample < 0:
            uv, lens, lens_A = R.image_uv(W, H), np.zeros((N, 2)), None
        else:
            d4 = draws_of(oracle, sample)
            uv = R.image_uv(W, H, d4, tentfilter=bool(c.kw.get("tentfilter")))
            lens, lens_A = R.sample_disk(d4[:, 2:4].astype(F64))
        o, Ao, d, Ad = R.eval_camera(cam, uv, lens, aspect=c.aspect, lens_A=lens_A)
        within(rays[:, :3], o, Ao, 1.0, label + " o")
        within(rays[:, 3:], d, Ad, 1.0, label + " d")
        if sample < 0 and not cam.orthographic:
            assert (bits(rays[:, :3]) == bits(np.asarray(cam.frame, F32)[9:12])).all(), label
        # ---- the hit records
        m = surf["hit"] != 0
        s, h, r = surf[m], hits[m], rays[m]
        inst, elem, u, v = h["instance"], h["element"], h["u"], h["v"]
        p, A = R.position(sc, inst, elem, u, v)
        within(s["position"], p, A, 1.0, label + " position")
        g, A, cond = R.element_normal(sc, inst, elem)
        within(s["gnormal"], g, A, cond, label + " gnormal")
        tc, A = R.texcoord(sc, inst, elem, u, v)
        within(s["texcoord"], tc, A, 1.0, label + " texcoord")
        # the shading normal
        mats = np.array([sc.instances[k].material for k in inst])
        nmap = np.array([sc.materials[k].normal_tex >= 0 for k in mats])
        refr = np.array([sc.materials[k].type == "refractive" for k in mats])
        vn = R.has_vertex_normals(sc, inst)
        minus_d = -r[:, 3:6].astype(F64)
        flat = ~nmap & ~vn
        if flat.any():  # the element normal, or its exact negation to face -d
            front = (s["gnormal"][flat].astype(F64) * minus_d[flat]).sum(1) >= 0
            # the sign test runs in float32 on the device: where float64 is within rounding of zero either is right
            want = np.where((front | refr[flat])[:, None], s["gnormal"][flat], -s["gnormal"][flat])
            dots = np.abs((s["gnormal"][flat].astype(F64) * minus_d[flat]).sum(1))
            sure = dots > 1e-5 * np.linalg.norm(minus_d[flat], axis=1)
            same = (bits(s["normal"][flat]) == bits(want)).all(1)
            other = (bits(s["normal"][flat]) == bits(-want)).all(1)
            assert (same | (~sure & other)).all(), (label, "flat normal", int((~same).sum()))
            assert (~sure).sum() <= len(sure) // 100, (label, "rays within 1e-5 of grazing", int((~sure).sum()))
            print(label, "flat normals", int(flat.sum()), "flipped", int((~front & ~refr[flat]).sum()), "unsure sign", int((~sure).sum()))
        smooth = ~nmap & vn
        if smooth.any():
            n64, A, cond = R.vertex_normal(sc, inst[smooth], elem[smooth], u[smooth], v[smooth])
            dots = (n64 * minus_d[smooth]).sum(1)
            n64 = np.where(((dots >= 0) | refr[smooth])[:, None], n64, -n64)
            sure = np.abs(dots) > 1e-5 * np.linalg.norm(minus_d[smooth], axis=1)
            assert (~sure).sum() <= len(sure) // 100, (label, "rays within 1e-5 of grazing", int((~sure).sum()))
            print(label, "vertex normals", int(smooth.sum()), "unsure sign", int((~sure).sum()))
            dev = s["normal"][smooth].astype(F64)
            dev = np.where((~sure & ((dev * n64).sum(1) < 0))[:, None], -dev, dev)
            within(dev, n64, A, cond, label + " vertex normal")
        # ---- the material point: float32 from the record's own texcoord
        vc = R.has_vertex_colors(sc, inst)
        ref = R.material_point32(oracle, sc, inst, s["texcoord"])
        for k in ("material", "type"):
            assert np.array_equal(s[k], ref[k]), (label, k)
        for k in ("emission", "metallic", "roughness", "ior"):
            assert (bits(s[k]) == bits(ref[k])).all(), (label, k)
        for k in ("color", "opacity"):
            assert (bits(s[k][~vc]) == bits(ref[k][~vc])).all(), (label, k)
        if vc.any():  # the vertex-colour factor in float64
            col, A = R.vertex_color(sc, inst[vc], elem[vc], u[vc], v[vc])
            base = ref["color"][vc].astype(F64)  # material colour times texture, exact float32
            within(s["color"][vc], base * col[:, :3], base * A[:, :3], 1.0, label + " vertex colour")
            within(s["opacity"][vc], ref["opacity"][vc].astype(F64) * col[:, 3], ref["opacity"][vc].astype(F64) * A[:, 3], 1.0,
                   label + " vertex alpha")


# ------------------------------------------------------------------------------ 3: composition
@pytest.mark.parametrize("name", ["cornell", "features1", "random"])
def test_composition_and_position_independence(name, cases, abi):
    c = cases[name]
    st = c.state("near")
    for sample in (0, -1):
        rays, hits, surf = c.gbuffer("near", sample)
        r2 = st.camera_rays(sample)
        h2 = st.intersect(r2)
        s2 = st.surfaces(r2, h2)
        for a, b in ((rays, r2), (hits, h2), (surf, s2)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, sample)
    reps = 300  # 904500 records: more than one launch's worth of any grid, the last block partial
    tiled = st.surfaces(np.tile(rays, (reps, 1)), np.tile(hits, reps))
    blocks = tiled.view(np.uint8).reshape(reps, N * 96)
    differing = np.flatnonzero((blocks != blocks[0]).any(axis=1))
    assert len(differing) == 0 and np.array_equal(blocks[0], surf.view(np.uint8).reshape(-1)), (name, differing[:4])
    for n in (1, 63, 64, 65, 257):
        head = st.surfaces(rays[:n], hits[:n])
        assert np.array_equal(head.view(np.uint8), surf[:n].view(np.uint8)), (name, n)
    empty = st.surfaces(np.zeros((0, 6), F32), np.zeros(0, abi.HIT_DTYPE))
    assert empty.shape == (0,) and empty.dtype == abi.SURFACE_DTYPE


# ------------------------------------------------------------------------------ 4: hostile records
def test_hostile_records_are_misses(cases, abi):
    """Through the device variant: instance ids of ninst, -7 and 2^30, elements of -1 and one past the
    shape's last, NaN and inf uv each give a miss record; the neighbouring valid records keep their
    bits. The kernel's range check comes before any load the record names."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the zero-copy path needs a tensor on the context's device")
    from jtrace.trace import split_surfaces
    for name in ("cornell", "random"):
        c = cases[name]
        st = c.state("near")
        rays, hits, surf = c.gbuffer("near", 0)
        ok = np.flatnonzero(hits["hit"] != 0)
        assert len(ok) > 200
        bad = hits.copy()
        ninst = len(c.scene.instances)
        nelem = np.array([len(c.scene.shapes[i.shape].triangles) or len(c.scene.shapes[i.shape].quads) for i in c.scene.instances])
        victims = ok[::7][:8 * (len(ok[::7]) // 8)].reshape(-1, 8)
        bad["instance"][victims[:, 0]] = ninst
        bad["instance"][victims[:, 1]] = -7
        bad["instance"][victims[:, 2]] = 2 ** 30
        bad["element"][victims[:, 3]] = -1
        bad["element"][victims[:, 4]] = nelem[hits["instance"][victims[:, 4]]]
        bad["u"][victims[:, 5]] = np.nan
        bad["v"][victims[:, 6]] = np.inf
        bad["u"][victims[:, 7]] = -np.inf
        tr = torch.from_numpy(np.array(rays)).to("cuda:0")
        th = torch.from_numpy(bad.view(np.int32).reshape(-1, 6).copy()).to("cuda:0")
        out = st.surfaces(tr, th)
        assert out.dtype == torch.float32 and tuple(out.shape) == (N, 24) and out.is_cuda
        rec = out.cpu().numpy().reshape(-1).view(abi.SURFACE_DTYPE)
        hostile = np.zeros(N, bool)
        hostile[victims.reshape(-1)] = True
        assert (rec[hostile].view(np.uint32) == 0).all(), name
        assert np.array_equal(rec[~hostile].view(np.uint8), surf[~hostile].view(np.uint8)), name
        # the valid records through the device path are the host path's, and split_surfaces names them
        good = st.surfaces(tr, torch.from_numpy(hits.view(np.int32).reshape(-1, 6).copy()).to("cuda:0"))
        assert np.array_equal(good.cpu().numpy().reshape(-1).view(np.uint8), surf.view(np.uint8).reshape(-1)), name
        f = split_surfaces(good)
        assert np.array_equal(f["hit"].cpu().numpy(), surf["hit"]) and np.array_equal(f["material"].cpu().numpy(), surf["material"])
        assert np.array_equal(bits(f["normal"].cpu().numpy()), bits(surf["normal"]))
        # the device forms of camera_rays and gbuffer give the host forms' bits
        dr, dh, ds = st.gbuffer(0, device=True)
        assert np.array_equal(dr.cpu().numpy(), rays) and np.array_equal(ds.cpu().numpy().reshape(-1).view(np.uint8), surf.view(np.uint8).reshape(-1))
        assert np.array_equal(dh.cpu().numpy().reshape(-1).view(np.uint8), hits.view(np.uint8).reshape(-1))
        assert np.array_equal(st.camera_rays(-1, device=True).cpu().numpy(), c.gbuffer("near", -1)[0])


# ------------------------------------------------------------------------------ 5: the product itself
@pytest.mark.parametrize("name", ["cornell", "features1", "coplanar"])
def test_the_integrators_aovs_are_the_gbuffers(name, cases, lib):
    """A fresh k-stream context's first sample: its albedo, normal and hit AOVs are gbuffer(0)'s colour,
    normal and hit on the opaque pixels, bit for bit."""
    from jtrace import trace
    c = cases[name]
    rays, hits, surf = c.gbuffer("near", 0)
    st = trace.TraceState(c.sa, c.bvh, c.lights, c.params("near", samples=32, batch=16), lib)
    assert st.streams > 1
    st.trace_range(0, 1)
    alb, nrm, cnt = st.get_aovs()
    st.close()
    alb, nrm, cnt = alb.reshape(N, 3), nrm.reshape(N, 3), cnt.reshape(N)
    m = (surf["hit"] != 0) & ~(surf["opacity"] < 1)
    assert m.sum() > 100
    assert (bits(lerp1(surf["color"]))[m] == bits(alb)[m]).all() and (bits(lerp1(surf["normal"]))[m] == bits(nrm)[m]).all()
    assert (cnt[m] == 1).all()
    miss = surf["hit"] == 0
    assert (bits(lerp1(-rays[:, 3:6]))[miss] == bits(nrm)[miss]).all()


# ------------------------------------------------------------------------------ 6: the context is untouched
def _render(c, lib, calls):
    """32 samples in three calls with a read between the first two; with `calls`, gbuffer, surfaces
    and camera_rays run while the second range is queued. Everything a caller can read afterwards."""
    from jtrace import trace
    st = trace.TraceState(c.sa, c.bvh, c.lights, c.params("near", samples=32, batch=16), lib)
    st.set_counters(1)
    st.trace_range(0, 16)
    half = st.get_image()
    st.trace_range(16, 24)  # stays queued
    queued = st.samples
    if calls:
        rays, hits, surf = st.gbuffer(3)
        again = st.surfaces(rays, hits)
        centre = st.camera_rays(-1)
        assert st.samples == queued
        want = c.gbuffer("near", 3)
        for a, b in ((rays, want[0]), (hits, want[1]), (surf, want[2]), (again, want[2]), (centre, c.gbuffer("near", -1)[0])):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    st.trace_range(24, 32)
    img = st.get_image()
    alb, nrm, nhits = st.get_aovs()
    out = {"half": half, "image": img, "albedo": alb, "normal": nrm, "hits": nhits, "variance": st.variance()}
    cnt = st.counters()
    cnt.pop("kernel_ms")
    samples, streams = st.samples, st.streams
    st.close()
    return out, cnt, (queued, samples, streams)


@pytest.mark.parametrize("name", ["cornell", "features1"])
def test_surface_calls_leave_the_context_untouched(name, cases, lib):
    c = cases[name]
    a, ca, sa = _render(c, lib, True)
    b, cb, sb = _render(c, lib, False)
    assert sa == sb and sa[1] == 32 and sa[2] > 1, (sa, sb)
    assert ca == cb, (ca, cb)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k)
    assert a["hits"].sum() > 0 and a["albedo"].mean() > 0 and a["image"][..., :3].mean() > 0


# ------------------------------------------------------------------------------ 7: errors
def test_errors(cases, abi, lib):
    from jtrace import trace
    c = cases["cornell"]
    rays, hits, surf = (np.array(a) for a in c.gbuffer("near", 0))
    p = c.params("near", samples=8, batch=4)
    out = np.zeros(N, abi.SURFACE_DTYPE)
    ro, ho = np.zeros((N, 6), F32), np.zeros(N, abi.HIT_DTYPE)
    rp, hp = rays.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit))
    sp = out.ctypes.data_as(C.POINTER(abi.jt_surface))
    rop, hop = ro.ctypes.data_as(abi.f32p), ho.ctypes.data_as(C.POINTER(abi.jt_hit))

    def err(status, expected=-1):
        assert status == expected, (status, lib.jt_last_error())
        return lib.jt_last_error().decode()

    st = trace.TraceState(c.sa, c.bvh, c.lights, p, lib)
    h = st.handle
    assert "ctx" in err(lib.jt_eval_hits(None, 4, rp, hp, sp)) and "ctx" in err(lib.jt_camera_rays(None, 0, rop))
    assert "ctx" in err(lib.jt_gbuffer(None, 0, rop, hop, sp))
    # the order: ctx, rays, hits, out, then n
    assert "rays" in err(lib.jt_eval_hits(h, -1, None, None, None)) and "hits" in err(lib.jt_eval_hits(h, -1, rp, None, None))
    assert "out" in err(lib.jt_eval_hits(h, -1, rp, hp, None))
    assert "d_rays" in err(lib.jt_eval_hits_device(h, 4, None, None, None))
    assert "d_hits" in err(lib.jt_eval_hits_device(h, 4, 0x1000, None, None))
    assert "d_out" in err(lib.jt_eval_hits_device(h, 4, 0x1000, 0x1000, None))
    assert "aligned" in err(lib.jt_eval_hits_device(h, 4, 0x1000, 0x1004, 0x1000))
    assert "aligned" in err(lib.jt_eval_hits_device(h, 4, 0x1000, 0x1000, 0x1008))
    assert "aligned" in err(lib.jt_camera_rays_device(h, 0, 0x1004))
    # jt_gbuffer_device checks every alignment before its first launch: nothing is written
    import torch
    dr, dh = torch.zeros((N, 6), dtype=torch.float32, device="cuda:0"), torch.zeros((N, 6), dtype=torch.int32, device="cuda:0")
    ds = torch.zeros(N * 24 + 2, dtype=torch.float32, device="cuda:0")
    assert "aligned" in err(lib.jt_gbuffer_device(h, 0, dr.data_ptr(), dh.data_ptr(), ds.data_ptr() + 8))
    assert "aligned" in err(lib.jt_gbuffer_device(h, 0, dr.data_ptr(), dh.data_ptr() + 4, ds.data_ptr()))
    torch.cuda.synchronize()
    assert not dr.any() and not dh.any() and not ds.any()
    for n in (-1, 2**30 + 1):
        assert " n " in " " + err(lib.jt_eval_hits(h, n, rp, hp, sp))
    assert lib.jt_eval_hits(h, 0, rp, hp, sp) == 0
    assert "rays" in err(lib.jt_camera_rays(h, -2, None)) and "sample" in err(lib.jt_camera_rays(h, -2, rop))
    assert "d_rays" in err(lib.jt_camera_rays_device(h, 0, None)) and "sample" in err(lib.jt_camera_rays_device(h, -5, 0x1000))
    assert "surfaces" in err(lib.jt_gbuffer(h, -2, rop, hop, None)) and "sample" in err(lib.jt_gbuffer(h, -2, rop, hop, sp))
    assert "d_surfaces" in err(lib.jt_gbuffer_device(h, 0, None, None, None))
    assert "sample" in err(lib.jt_gbuffer_device(h, -2, None, None, 0x1000))
    # no error wrote a result
    assert (out.view(np.uint8) == 0).all() and (ro == 0).all() and (ho.view(np.uint8) == 0).all()
    # rays and hits of jt_gbuffer may be NULL; sample is not bounded by params.samples
    assert lib.jt_gbuffer(h, 0, None, None, sp) == 0
    assert np.array_equal(out.view(np.uint8), surf.view(np.uint8))
    assert lib.jt_camera_rays(h, 1000, rop) == 0 and not np.array_equal(ro, rays)
    # a multi-device context, even of one device: unsupported
    multi = trace.TraceState(c.sa, c.bvh, c.lights, p, lib, devices=[0])
    mh = multi.handle
    out[:] = 0
    ro[:] = 0
    assert "multi-device" in err(lib.jt_eval_hits(mh, 4, rp, hp, sp), -2)
    assert "multi-device" in err(lib.jt_eval_hits_device(mh, 4, 0x1000, 0x1000, 0x1000), -2)
    assert "multi-device" in err(lib.jt_camera_rays(mh, 0, rop), -2) and "multi-device" in err(lib.jt_camera_rays_device(mh, 0, 0x1000), -2)
    assert "multi-device" in err(lib.jt_gbuffer(mh, 0, rop, hop, sp), -2)
    assert "multi-device" in err(lib.jt_gbuffer_device(mh, 0, None, None, 0x1000), -2)
    assert lib.jt_eval_hits(mh, 0, rp, hp, sp) == 0  # n == 0 comes first
    assert (out.view(np.uint8) == 0).all() and (ro == 0).all()
    multi.close()
    # after the errors the context still renders bit-identically
    st.trace_range(0, 8)
    img = st.get_image()
    st.close()
    clean = trace.TraceState(c.sa, c.bvh, c.lights, p, lib)
    clean.trace_range(0, 8)
    assert np.array_equal(img.view(np.uint8), clean.get_image().view(np.uint8))
    clean.close()
