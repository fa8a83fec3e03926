"""Ray queries on a context's scene (csrc/jt_intersect.hip behind jt_intersect, jt_occluded and their
device-pointer variants) against the oracle's or_query, ray by ray: no tolerance, no ray excluded.

The scenes, the seeded ray classes and the orders are those of tests/queries_ref.py (the rays are
checked on the CPU, tests/test_queries_host.py, to be finite and to separate the orders); the
product context is created with the order's traversal and the oracle answers in the same order.
Compared per ray: hit; instance, in the reference's numbering; element; the bits of u and v; the
bits of t on a hit; on a miss t == +inf, instance == element == -1 and u == v == 0 (the oracle's
record of a miss carries t = 0, so the device's +inf is asserted instead).

Forms: binary and wide by the order; the fixed 16-entry stack and the ring with HBM overflow (the
deep scene's bound is 28; cornell, random and quads9 run again with the option test_lds_ring = 2,
in every order); an LDS-mode context (cornell) and an HBM-mode one (option lds_scene = 0): the
query reads the context's HBM copy of the scene in both.
"""
import ctypes as C

import numpy as np
import pytest

import queries_ref as Q
from conftest import make_params

pytestmark = pytest.mark.gpu

RING2 = ("cornell", "random", "quads9")  # run again with test_lds_ring = 2
INSTANCE_SCENES = ("cornell", "random", "twins", "deep")
INSTANCE_CLASSES = ("generic", "edges")
FIELDS = ("instance", "element", "u", "v", "t", "hit")


class Contexts:
    """Product contexts, one per (scene, order, options) for the whole module."""

    def __init__(self, abi, lib, oracle):
        self.abi, self.lib, self.oracle, self.open = abi, lib, oracle, {}

    def get(self, scene, order, **opts):
        from jtrace import trace
        key = (scene, order, tuple(sorted(opts.items())))
        if key not in self.open:
            ctx = Q.context(scene, self.abi, self.oracle)
            try:
                for k, v in opts.items():
                    self.abi.set_option(self.lib, k, v)
                self.open[key] = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, ctx.params[order], self.lib)
            finally:
                self.abi.set_option(self.lib, None, None)
        return self.open[key]

    def close(self):
        for st in self.open.values():
            st.close()


@pytest.fixture(scope="module")
def contexts(gpu, abi, lib, oracle):
    c = Contexts(abi, lib, oracle)
    yield c
    c.close()


_oracle = {}


def oracle_query(oracle, ctx, cls, order, inst=None):
    """or_query of the class's rays in `order`, computed once and shared (read-only)."""
    key = (ctx.name, cls, order, None if inst is None else inst.tobytes())
    if key not in _oracle:
        ref = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], Q.rays(ctx, cls, oracle), inst=inst)
        for a in ref.values():
            a.setflags(write=False)
        _oracle[key] = ref
    return _oracle[key]


def check_hits(out, ref, label):
    """jt_hit records against or_query's result, every ray."""
    assert out.dtype.names == FIELDS and len(out) == len(ref["hit"])
    hit = ref["hit"] != 0
    for k, r in (("hit", "hit"), ("instance", "inst"), ("element", "elem")):
        bad = np.flatnonzero(out[k] != ref[r])
        assert len(bad) == 0, (label, k, len(bad), bad[:4], out[k][bad[:4]], ref[r][bad[:4]])
    for k in ("u", "v"):
        bad = np.flatnonzero(~Q.same_bits(out[k], ref[k]))
        assert len(bad) == 0, (label, k, len(bad), bad[:4], out[k][bad[:4]], ref[k][bad[:4]])
    bad = np.flatnonzero(hit & ~Q.same_bits(out["t"], ref["t"]))
    assert len(bad) == 0, (label, "t", len(bad), bad[:4], out["t"][bad[:4]], ref["t"][bad[:4]])
    miss = out[~hit]
    assert np.isposinf(miss["t"]).all() and (miss["instance"] == -1).all() and (miss["element"] == -1).all(), (label, "miss")
    assert (miss["u"].view(np.uint32) == 0).all() and (miss["v"].view(np.uint32) == 0).all(), (label, "uv of a miss")
    assert set(np.unique(out["hit"])) <= {0, 1}, label


def variants(scene):
    """The option sets a scene's contexts are created with."""
    v = [{}]
    if scene in RING2:
        v.append({"test_lds_ring": 2})
    if scene == "cornell":
        v.append({"lds_scene": 0})
    return v


def mixed_instance_ids(ctx):
    """Q.instance_ids with -1 (a scene query) in every other block of 64 rays: scene and instance
    queries share waves."""
    inst = Q.instance_ids(ctx).copy()
    inst[(np.arange(len(inst)) // 64) % 2 == 1] = -1
    return inst


def describe_fields(st):
    return dict(tok.split("=", 1) for tok in st.describe().split() if "=" in tok)


def test_contexts_cover_every_form(contexts):
    """From jt_describe: binary and wide; the fixed stack and the overflow; an LDS-mode context and
    an HBM-mode one; the shortened ring."""
    d = describe_fields(contexts.get("cornell", "near"))
    assert d["mode"] == "lds" and d["hbm_overflow"] == "0" and d["traversal"] == "near", d
    d = describe_fields(contexts.get("cornell", "near", lds_scene=0))
    assert d["mode"] == "hbm" and d["hbm_overflow"] == "0", d
    d = describe_fields(contexts.get("cornell", "reference"))
    assert d["traversal"] == "reference", d
    for order in ("near", "wide"):
        d = describe_fields(contexts.get("deep", order))
        assert d["stack_bound"] == "28" and d["hbm_overflow"] == "1" and d["lds_ring"] == "16" and d["traversal"] == order, d
        d = describe_fields(contexts.get("cornell", order, test_lds_ring=2))
        assert d["hbm_overflow"] == "1" and d["ring_used"] == "2" and d["traversal"] == order, d
    d = describe_fields(contexts.get("cornell", "wide"))
    assert d["traversal"] == "wide" and d["hbm_overflow"] == "0" and "true>" in d["kernel"], d


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_closest_hit_equals_the_oracle_ray_by_ray(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in Q.ORDERS:
        ref = oracle_query(oracle, ctx, cls, order)
        for opts in variants(scene):
            out = contexts.get(scene, order, **opts).intersect(r)
            check_hits(out, ref, f"{scene}/{cls}/{order}/{opts}")
        print(f"{scene}/{cls}/{order}: {int((ref['hit'] != 0).sum())} hits of {len(r)}, variants {variants(scene)}")


@pytest.mark.parametrize("scene", INSTANCE_SCENES)
@pytest.mark.parametrize("cls", INSTANCE_CLASSES)
def test_instance_queries_equal_the_oracle(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for inst in (Q.instance_ids(ctx), mixed_instance_ids(ctx)):
        for order in Q.ORDERS:
            ref = oracle_query(oracle, ctx, cls, order, inst)
            for opts in variants(scene):
                out = contexts.get(scene, order, **opts).intersect(r, inst)
                check_hits(out, ref, f"{scene}/{cls}/{order}/{opts}/instance")


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_occluded_equals_the_hit_flag(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in Q.ORDERS:
        ref = oracle_query(oracle, ctx, cls, order)
        for opts in variants(scene):
            st = contexts.get(scene, order, **opts)
            occ = st.occluded(r)
            assert occ.dtype == np.bool_ and occ.shape == (len(r),)
            bad = np.flatnonzero(occ != (ref["hit"] != 0))
            assert len(bad) == 0, (scene, cls, order, opts, "against the oracle", len(bad), bad[:4])
            bad = np.flatnonzero(occ != (st.intersect(r)["hit"] != 0))
            assert len(bad) == 0, (scene, cls, order, opts, "against jt_intersect", len(bad), bad[:4])


@pytest.mark.parametrize("order", ["near", "wide"])
@pytest.mark.parametrize("scene", ["cornell", "deep"])
def test_position_independence_and_refill(scene, order, contexts, abi, oracle):
    """The generic rays tiled 640 times, 2.6 M rays: more than four times the largest persistent
    grid (256 x 8 x 256 lanes), so every lane refills. Every block of the result is block 0, bit for
    bit, block 0 is the oracle's, and so are the heads of 1, 63, 64, 65 and 257 rays."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, "generic", oracle)
    ref = oracle_query(oracle, ctx, "generic", order)
    st = contexts.get(scene, order)
    reps = 640
    assert reps * len(r) > 4 * 256 * 8 * 256
    out = st.intersect(np.tile(r, (reps, 1)))
    blocks = out.view(np.uint8).reshape(reps, len(r) * abi.HIT_DTYPE.itemsize)
    differing = np.flatnonzero((blocks != blocks[0]).any(axis=1))
    assert len(differing) == 0, (scene, order, len(differing), differing[:4])
    check_hits(out[:len(r)], ref, f"{scene}/{order}/tiled")
    occ = st.occluded(np.tile(r, (reps, 1))).reshape(reps, len(r))
    assert (occ == (ref["hit"] != 0)[None, :]).all(), (scene, order, "occluded, tiled")
    for n in (1, 63, 64, 65, 257):
        check_hits(st.intersect(r[:n]), {k: v[:n] for k, v in ref.items()}, f"{scene}/{order}/n={n}")
        assert np.array_equal(st.occluded(r[:n]), ref["hit"][:n] != 0), (scene, order, n)
    empty = st.intersect(np.zeros((0, 6), np.float32))
    assert empty.shape == (0,) and st.occluded(np.zeros((0, 6), np.float32)).shape == (0,)


def _render(abi, lib, oracle, scene, query):
    """32 samples in three calls with a read between the first two; with `query`, ray queries run
    while the second range is queued. Everything a caller can read afterwards.

    The deep scene is a traversal scene without a light (no emissive material, no environment). The
    path sampler draws from the scene's lights at every diffuse bounce (sample_lights,
    src/trace.jl:968: an index into an empty list, in the reference a BoundsError), so the scene is
    rendered with the naive sampler, which never does: its image is black, its albedo, normal, hit
    counts, variance and counters are not."""
    from jtrace import trace
    ctx = Q.context(scene, abi, oracle)
    assert (ctx.lights.struct.nlights == 0) == (scene == "deep")
    p = make_params(abi, samples=32, batch=16, traversal="near", sampler=2 if scene == "deep" else 1)
    st = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib)
    st.set_counters(1)
    st.trace_range(0, 16)
    half = st.get_image()  # traces the first half
    st.trace_range(16, 24)  # stays queued: fewer than 64 samples, the render is not complete
    queued = st.samples
    hits = occ = None
    if query:
        r = Q.rays(ctx, "generic", oracle)
        hits, occ = st.intersect(r), st.occluded(r)
        hits2 = st.intersect(r, mixed_instance_ids(ctx))
        assert st.samples == queued
        check_hits(hits, oracle_query(oracle, ctx, "generic", "near"), f"{scene}/queued")
        check_hits(hits2, oracle_query(oracle, ctx, "generic", "near", mixed_instance_ids(ctx)), f"{scene}/queued/instance")
        assert np.array_equal(occ, hits["hit"] != 0)
    st.trace_range(24, 32)
    img = st.get_image()
    alb, nrm, nhits = st.get_aovs()
    out = {"half": half, "image": img, "albedo": alb, "normal": nrm, "hits": nhits, "variance": st.variance()}
    cnt = st.counters()
    cnt.pop("kernel_ms")
    samples, streams = st.samples, st.streams
    st.close()
    return out, cnt, (queued, samples, streams)


@pytest.mark.parametrize("scene", ["cornell", "deep"])
def test_queries_leave_the_context_untouched(scene, abi, lib, oracle, gpu):
    a, ca, sa = _render(abi, lib, oracle, scene, query=True)
    b, cb, sb = _render(abi, lib, oracle, scene, query=False)
    assert sa == sb and sa[1] == 32 and sa[2] > 1, (sa, sb)
    assert ca == cb, (ca, cb)  # every field but kernel_ms: a query that traced the queue would add a launch
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (scene, k)
    assert a["hits"].sum() > 0 and a["albedo"].mean() > 0 and (scene == "deep" or a["image"][..., :3].mean() > 0)


def test_device_pointer_path_gives_the_host_path_bits(contexts, abi, oracle):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the zero-copy path needs a tensor on the context's device")
    from jtrace.trace import split_hits
    for scene, order in (("cornell", "near"), ("deep", "wide")):
        ctx = Q.context(scene, abi, oracle)
        st = contexts.get(scene, order)
        r = Q.rays(ctx, "generic", oracle)
        inst = mixed_instance_ids(ctx)
        tr = torch.from_numpy(np.array(r)).to("cuda:0")
        for ins in (None, inst):
            host = st.intersect(r, ins)
            dev = st.intersect(tr, None if ins is None else torch.from_numpy(ins).to("cuda:0"))
            assert dev.dtype == torch.int32 and tuple(dev.shape) == (len(r), 6) and dev.is_cuda
            assert np.array_equal(dev.cpu().numpy().reshape(-1).view(np.uint8), host.view(np.uint8)), (scene, order)
            f = split_hits(dev)
            assert np.array_equal(f["t"].cpu().numpy().view(np.uint32), host["t"].view(np.uint32))
            assert np.array_equal(f["instance"].cpu().numpy(), host["instance"])
        occ = st.occluded(tr)
        assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), st.occluded(r))
        # an instance id out of range reports a miss in the device variant
        wild = inst.copy()
        wild[::3], wild[1::3] = ctx.ninst, -7
        dev = st.intersect(tr, torch.from_numpy(wild).to("cuda:0")).cpu().numpy().reshape(-1).view(abi.HIT_DTYPE)
        out_of_range = (wild >= ctx.ninst) | (wild < -1)
        miss = dev[out_of_range]
        assert (miss["hit"] == 0).all() and (miss["instance"] == -1).all() and (miss["element"] == -1).all()
        assert np.isposinf(miss["t"]).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all()
        good = st.intersect(r, np.where(out_of_range, -1, wild).astype(np.int32))
        assert np.array_equal(dev[~out_of_range].view(np.uint8), good[~out_of_range].view(np.uint8))


def test_errors(abi, lib, oracle, gpu):
    from jtrace import trace
    ctx = Q.context("cornell", abi, oracle)
    r = Q.rays(ctx, "generic", oracle)
    p = make_params(abi, samples=8, batch=4, traversal="near")
    hits = np.zeros(len(r), abi.HIT_DTYPE)
    occ = np.zeros(len(r), np.uint8)
    rp, hp, op = r.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit)), occ.ctypes.data_as(abi.u8p)

    def err(status, expected=-1):
        assert status == expected, (status, lib.jt_last_error())
        return lib.jt_last_error().decode()

    st = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib)
    h = st.handle
    assert "ctx" in err(lib.jt_intersect(None, 4, rp, None, hp)) and "ctx" in err(lib.jt_occluded(None, 4, rp, op))
    assert "rays" in err(lib.jt_intersect(h, 4, None, None, hp)) and "hits" in err(lib.jt_intersect(h, 4, rp, None, None))
    assert "rays" in err(lib.jt_occluded(h, 4, None, op)) and "occluded" in err(lib.jt_occluded(h, 4, rp, None))
    assert "d_rays" in err(lib.jt_intersect_device(h, 4, None, None, None))
    assert "d_hits" in err(lib.jt_intersect_device(h, 4, 0x1000, None, None))
    assert "d_occluded" in err(lib.jt_occluded_device(h, 4, 0x1000, None))
    for n in (-1, 2**30 + 1):
        assert " n " in " " + err(lib.jt_intersect(h, n, rp, None, hp)) and " n " in " " + err(lib.jt_occluded(h, n, rp, op))
    assert lib.jt_intersect(h, 0, rp, None, hp) == 0 and lib.jt_occluded(h, 0, rp, op) == 0
    for wrong in (ctx.ninst, -2):
        inst = np.full(len(r), -1, np.int32)
        inst[77] = wrong
        msg = err(lib.jt_intersect(h, len(r), rp, inst.ctypes.data_as(abi.i32p), hp))
        assert "instance[77]" in msg and str(wrong) in msg, msg
    assert (hits.view(np.uint8) == 0).all() and (occ == 0).all()  # no error wrote a result
    # a multi-device context, even of one device: unsupported, as jt_get_variance
    multi = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib, devices=[0])
    assert "multi-device" in err(lib.jt_intersect(multi.handle, 4, rp, None, hp), -2)
    assert "multi-device" in err(lib.jt_occluded(multi.handle, 4, rp, op), -2)
    assert "multi-device" in err(lib.jt_intersect_device(multi.handle, 4, 0x1000, None, 0x1000), -2)
    assert "multi-device" in err(lib.jt_occluded_device(multi.handle, 4, 0x1000, 0x1000), -2)
    assert lib.jt_intersect(multi.handle, 0, rp, None, hp) == 0  # n == 0 comes first
    multi.close()
    # after the errors the context still renders bit-identically
    st.trace_range(0, 8)
    img = st.get_image()
    st.close()
    clean = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib)
    clean.trace_range(0, 8)
    assert np.array_equal(img.view(np.uint8), clean.get_image().view(np.uint8))
    clean.close()
