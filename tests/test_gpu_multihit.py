"""All hits along a ray on the GPU (csrc/jt_multihit.hip behind jt_intersect_multi, jt_count_hits and
their device-pointer variants), ray by ray, no tolerance and no ray excluded.

The reference of the reference and near orders is the restatement of tests/multihit_ref.py, which
tests/test_multihit_host.py holds to the brute force; the wide order, whose quantised boxes are not
restated, is held to the brute force itself with the differing rays capped at 0.1 % of a case's rays
(queries_ref.CAPPED's bar). N = 4099 rays per case, the scenes, classes and contexts of
tests/test_gpu_intersect.py (LDS mode and lds_scene = 0, test_lds_ring = 2, the deep scene through
the overflow).
"""
import ctypes as C

import numpy as np
import pytest

import bounded_ref as B
import multihit_ref as M
import queries_ref as Q
import scenes_ref as SR
from conftest import make_params
from test_gpu_intersect import INSTANCE_CLASSES, INSTANCE_SCENES, contexts, mixed_instance_ids, variants  # noqa: F401

pytestmark = pytest.mark.gpu

ORDERS = ("reference", "near")
# the cases with the most hits per ray (90: evictions in the far-first order) and with exact-t pairs
MANY = (("plates", "stacked"), ("coplanar", "generic"))
WIDE_CASES = [(s, c) for s in ("cornell", "random", "deep") for c in Q.CAPPED] + [("plates", "stacked")]


def check(out, ref, label):
    """(records, counts) of the device against the restatement's, every bit of every ray."""
    (rec, cnt), (rrec, rcnt) = out, ref
    assert rec.dtype == rrec.dtype and rec.shape == rrec.shape and cnt.dtype == np.int32 and cnt.shape == rcnt.shape, label
    bad = M.differing(rec, cnt, rrec, rcnt)
    assert len(bad) == 0, (label, len(bad), bad[:4], cnt[bad[:4]], rcnt[bad[:4]], rec[bad[:2]], rrec[bad[:2]])


# ------------------------------------------------------------------------------ 1., 2. the restatement
@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_multi_and_counts_equal_the_restatement_bit_for_bit(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    ks = (1, 2, 4, 16) if (scene, cls) in MANY else (4,)
    for order in ORDERS:
        for opts in variants(scene):
            st = contexts.get(scene, order, **opts)
            for k in ks:
                check(st.intersect_multi(r, k), M.multi(ctx, oracle, order, r, k), f"{scene}/{cls}/{order}/{opts}/k={k}")
            cnt = st.count_hits(r)
            ref = M.count(ctx, oracle, order, r)
            bad = np.flatnonzero(cnt != ref)
            assert cnt.dtype == np.int32 and len(bad) == 0, (scene, cls, order, opts, "count", len(bad), bad[:4], cnt[bad[:4]], ref[bad[:4]])
    rec, cnt = M.multi(ctx, oracle, "reference", r, 4)
    print(f"{scene}/{cls}: {int(cnt.sum())} records at k = 4, {int(M.count(ctx, oracle, 'reference', r).sum())} hits counted, "
          f"{int(((cnt >= 2) & (rec['t'][:, 0] == rec['t'][:, 1])).sum())} rays with an exact-t pair in front")


@pytest.mark.parametrize("scene", INSTANCE_SCENES)
@pytest.mark.parametrize("cls", INSTANCE_CLASSES)
def test_instance_queries_equal_the_restatement(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for inst in (Q.instance_ids(ctx), mixed_instance_ids(ctx)):
        for order in ORDERS:
            for opts in variants(scene):
                st = contexts.get(scene, order, **opts)
                check(st.intersect_multi(r, 4, inst), M.multi(ctx, oracle, order, r, 4, inst), f"{scene}/{cls}/{order}/{opts}/instance")
                assert np.array_equal(st.count_hits(r, instance=inst), M.count(ctx, oracle, order, r, inst)), (scene, cls, order, opts)


# ------------------------------------------------------------------------------ 3. the wide context
@pytest.mark.parametrize("scene,cls", WIDE_CASES)
def test_wide_order_against_brute_force_capped(scene, cls, contexts, abi, oracle):
    """The wide order's quantised boxes are not restated: its lists are held to the brute force,
    which the restated orders equal on every one of these rays (tests/test_multihit_host.py). The
    differing rays, the slab test's culls at the wide planes, are printed and capped at 0.1 %."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    b = M.brute(ctx, oracle, r)
    st = contexts.get(scene, "wide")
    cap = len(r) // 1000
    for k in (1, 4, 16):
        rec, cnt = st.intersect_multi(r, k)
        bad = M.differing(rec, cnt, *b.multi(abi.HIT_DTYPE, k))
        print(f"{scene}/{cls}/wide k={k}: {len(bad)} of {len(r)} rays differ from the brute force (cap {cap})")
        assert len(bad) <= cap, (scene, cls, k, len(bad), bad[:4], rec[bad[:2]], r[bad[:2]].tolist())
    cnt = st.count_hits(r)
    bad = np.flatnonzero(cnt != b.total)
    print(f"{scene}/{cls}/wide counts: {len(bad)} of {len(r)} rays differ from the brute total (cap {cap})")
    assert len(bad) <= cap, (scene, cls, "count", len(bad), bad[:4], cnt[bad[:4]], b.total[bad[:4]])
    assert b.total.sum() > 50


# ------------------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("scene,cls", [("cornell", "generic"), ("coplanar", "generic"), ("deep", "outside"), ("plates", "stacked")])
def test_bounds_on_the_second_hit(scene, cls, contexts, abi, oracle):
    """bounded_ref's families on the second hit's t (the brute force's; a ray with fewer than two
    hits takes the seeded finite bound of a miss): A its bits, a hit exactly on the bound, B the
    float below, C a seeded multiple. No bound array equals one of +inf."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    second = M.brute(ctx, oracle, r).nth_t(1)
    free = {"hit": np.isfinite(second), "t": np.where(np.isfinite(second), second, np.float32(0))}
    assert free["hit"].sum() > 50
    for family in "ABC":
        bounds = B.family_bounds(ctx, cls, family, free)
        for order in ORDERS:
            for opts in variants(scene):
                st = contexts.get(scene, order, **opts)
                for k in (1, 4):
                    check(st.intersect_multi(r, k, tmax=bounds), M.multi(ctx, oracle, order, r, k, tmax=bounds),
                          f"{scene}/{cls}/{order}/{opts}/{family}/k={k}")
                assert np.array_equal(st.count_hits(r, tmax=bounds), M.count(ctx, oracle, order, r, tmax=bounds)), (scene, cls, order, family)
    for order in ("reference", "near", "wide"):
        st = contexts.get(scene, order)
        inf = np.full(len(r), np.inf, np.float32)
        a, b = st.intersect_multi(r, 4), st.intersect_multi(r, 4, tmax=inf)
        assert len(M.differing(*a, *b)) == 0 and np.array_equal(st.count_hits(r), st.count_hits(r, tmax=inf)), (scene, cls, order)


# ------------------------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize("scene,cls,order", [("cornell", "generic", "near"), ("deep", "generic", "wide"), ("plates", "stacked", "reference")])
def test_sizes_splits_and_refills(scene, cls, order, contexts, abi, oracle):
    """Heads of 1 .. 257 rays, halves and odd slices, and 700 copies across the grid's refills and
    the waves' claims (and, on the host path, three chunks): always the bits of the one call."""
    ctx = Q.context(scene, abi, oracle)
    st = contexts.get(scene, order)
    r = Q.rays(ctx, cls, oracle)
    k = 4
    rec, cnt = st.intersect_multi(r, k)
    tot = st.count_hits(r)
    assert cnt.sum() > 100 and tot.sum() >= cnt.sum()
    for n in (1, 63, 64, 65, 255, 256, 257):
        a, c = st.intersect_multi(r[:n], k)
        assert len(M.differing(a, c, rec[:n], cnt[:n])) == 0 and np.array_equal(st.count_hits(r[:n]), tot[:n]), (scene, order, n)
    for cuts in ((0, len(r) // 2, len(r)), (0, 333, 1000, 1001, 3070, len(r))):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            a, c = st.intersect_multi(r[lo:hi], k)
            assert len(M.differing(a, c, rec[lo:hi], cnt[lo:hi])) == 0 and np.array_equal(st.count_hits(r[lo:hi]), tot[lo:hi]), (scene, order, lo, hi)
    reps = 700
    assert reps * len(r) > 4 * 256 * 8 * 256 and reps * len(r) > 2 * ((1 << 22) // k)
    rr = np.tile(r, (reps, 1))
    big, bigc = st.intersect_multi(rr, k)
    blocks = big.view(np.uint8).reshape(reps, -1)
    differing = np.flatnonzero((blocks != rec.view(np.uint8).reshape(1, -1)).any(axis=1) | (bigc.reshape(reps, -1) != cnt[None, :]).any(axis=1))
    assert len(differing) == 0, (scene, order, len(differing), differing[:4])
    assert (st.count_hits(rr).reshape(reps, -1) == tot[None, :]).all(), (scene, order, "count, tiled")
    e = st.intersect_multi(np.zeros((0, 6), np.float32), k)
    assert e[0].shape == (0, k) and e[1].shape == (0,) and st.count_hits(np.zeros((0, 6), np.float32)).shape == (0,)


def test_the_overflow_path_and_the_chunk_boundary(contexts, abi, oracle):
    """deep with two LDS ring entries in use: nearly every push overflows to HBM. And the host
    variant with test_multi_chunk = 1500: three chunks, the last partial, give the bits of one launch."""
    ctx = Q.context("deep", abi, oracle)
    r = Q.rays(ctx, "generic", oracle)
    inst = mixed_instance_ids(ctx)
    for order in ORDERS:
        st = contexts.get("deep", order, test_lds_ring=2)
        for k in (1, 16):
            check(st.intersect_multi(r, k), M.multi(ctx, oracle, order, r, k), f"deep/{order}/ring 2/k={k}")
        assert np.array_equal(st.count_hits(r), M.count(ctx, oracle, order, r)), order
    for order in ("near", "wide"):
        whole, chunked = contexts.get("deep", order), contexts.get("deep", order, test_multi_chunk=1500)
        n = 2 * 1500 + 700
        bounds = np.where(np.arange(n) % 3 == 0, np.float32(np.inf), np.float32(1.5)).astype(np.float32)
        for k in (3, 16):
            a = whole.intersect_multi(r[:n], k, inst[:n], bounds)
            b = chunked.intersect_multi(r[:n], k, inst[:n], bounds)
            assert len(M.differing(*a, *b)) == 0 and a[1].sum() > 100, (order, k)


# ------------------------------------------------------------------------------ 6. device variants
def test_device_pointer_path_gives_the_host_path_bits(contexts, abi, lib, oracle):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the zero-copy path needs a tensor on the context's device")
    for scene, order in (("cornell", "near"), ("deep", "wide")):
        ctx = Q.context(scene, abi, oracle)
        st = contexts.get(scene, order)
        r = Q.rays(ctx, "generic", oracle)
        inst = mixed_instance_ids(ctx)
        bounds = np.where(np.arange(len(r)) % 2 == 0, np.float32(np.inf), np.float32(2.0)).astype(np.float32)
        tr, tb = torch.from_numpy(np.array(r)).to("cuda:0"), torch.from_numpy(bounds).to("cuda:0")
        for ins in (None, inst):
            ti = None if ins is None else torch.from_numpy(ins).to("cuda:0")
            for tm, ttm in ((None, None), (bounds, tb)):
                for k in ((1, 5) if ins is None else (5,)):
                    host, hc = st.intersect_multi(r, k, ins, tm)
                    dev, dc = st.intersect_multi(tr, k, ti, ttm)
                    assert dev.dtype == torch.int32 and tuple(dev.shape) == (len(r), k, 6) and dev.is_cuda and dc.dtype == torch.int32
                    assert np.array_equal(dev.cpu().numpy().reshape(-1).view(np.uint8), host.reshape(-1).view(np.uint8)), (scene, order, k)
                    assert np.array_equal(dc.cpu().numpy(), hc), (scene, order, k)
                assert np.array_equal(st.count_hits(tr, ttm, ti).cpu().numpy(), st.count_hits(r, tm, ins)), (scene, order)
        # an instance id out of range gives an empty list in the device variant
        wild = inst.copy()
        wild[::3], wild[1::3] = ctx.ninst, -7
        out_of_range = (wild >= ctx.ninst) | (wild < -1)
        dev, dc = st.intersect_multi(tr, 3, torch.from_numpy(wild).to("cuda:0"))
        rec = dev.cpu().numpy().reshape(-1).view(abi.HIT_DTYPE).reshape(len(r), 3)
        assert (dc.cpu().numpy()[out_of_range] == 0).all() and (rec["hit"][out_of_range] == 0).all()
        assert np.isposinf(rec["t"][out_of_range]).all() and (rec["instance"][out_of_range] == -1).all()
        good = st.intersect_multi(r, 3, np.where(out_of_range, -1, wild).astype(np.int32))
        assert np.array_equal(rec[~out_of_range].view(np.uint8), good[0][~out_of_range].view(np.uint8))
        assert (st.count_hits(tr, instance=torch.from_numpy(wild).to("cuda:0")).cpu().numpy()[out_of_range] == 0).all()
        # misaligned outputs are refused before anything runs
        buf = torch.zeros(len(r) * 3 * 6 + 4, dtype=torch.int32, device="cuda:0")
        cnt = torch.zeros(len(r) + 4, dtype=torch.int32, device="cuda:0")
        h = st.handle
        assert lib.jt_intersect_multi_device(h, len(r), tr.data_ptr(), None, None, 3, buf.data_ptr() + 4, cnt.data_ptr()) == -1
        assert "d_hits" in lib.jt_last_error().decode()
        assert lib.jt_intersect_multi_device(h, len(r), tr.data_ptr(), None, None, 3, buf.data_ptr(), cnt.data_ptr() + 2) == -1
        assert "d_counts" in lib.jt_last_error().decode()
        assert lib.jt_count_hits_device(h, len(r), tr.data_ptr(), None, None, cnt.data_ptr() + 1) == -1
        assert "d_counts" in lib.jt_last_error().decode()
        assert int(buf.abs().sum()) == 0 and int(cnt.abs().sum()) == 0
        # 8-byte alignment is enough for the records
        assert lib.jt_intersect_multi_device(h, len(r), tr.data_ptr(), None, None, 3, buf.data_ptr() + 8, cnt.data_ptr() + 4) == 0
        torch.cuda.synchronize()
        assert np.array_equal(buf[2:2 + len(r) * 18].cpu().numpy().view(np.uint8), st.intersect_multi(r, 3)[0].reshape(-1).view(np.uint8))


def test_errors_on_a_context(abi, lib, oracle, gpu):
    from jtrace import trace
    ctx = Q.context("cornell", abi, oracle)
    r = Q.rays(ctx, "generic", oracle)
    p = make_params(abi, samples=8, batch=4, traversal="near")
    hits = np.zeros((len(r), 2), abi.HIT_DTYPE)
    counts = np.zeros(len(r), np.int32)
    rp, hp, cp = r.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit)), counts.ctypes.data_as(abi.i32p)

    def err(status, expected=-1):
        assert status == expected, (status, lib.jt_last_error())
        return lib.jt_last_error().decode()

    st = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib)
    for wrong in (ctx.ninst, -2):
        inst = np.full(len(r), -1, np.int32)
        inst[77] = wrong
        for msg in (err(lib.jt_intersect_multi(st.handle, len(r), rp, None, inst.ctypes.data_as(abi.i32p), 2, hp, cp)),
                    err(lib.jt_count_hits(st.handle, len(r), rp, None, inst.ctypes.data_as(abi.i32p), cp))):
            assert "instance[77]" in msg and str(wrong) in msg, msg
    with pytest.raises(abi.JTError, match="k must"):
        st.intersect_multi(r, 17)
    assert (hits.view(np.uint8) == 0).all() and (counts == 0).all()  # no error wrote a result
    multi = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib, devices=[0])
    assert "multi-device" in err(lib.jt_intersect_multi(multi.handle, 4, rp, None, None, 2, hp, cp), -2)
    assert "multi-device" in err(lib.jt_count_hits(multi.handle, 4, rp, None, None, cp), -2)
    assert "multi-device" in err(lib.jt_intersect_multi_device(multi.handle, 4, 0x1000, None, None, 2, 0x1000, 0x1000), -2)
    assert "multi-device" in err(lib.jt_count_hits_device(multi.handle, 4, 0x1000, None, None, 0x1000), -2)
    assert lib.jt_intersect_multi(multi.handle, 0, rp, None, None, 2, hp, cp) == 0  # n == 0 comes first
    multi.close()
    st.close()


# ------------------------------------------------------------------------------ 7. the context is untouched
def _render(abi, lib, oracle, scene, call):
    """Four traced samples and one queued; with `call`, the new entry points run while it is queued."""
    from jtrace import trace
    ctx = Q.context(scene, abi, oracle)
    p = make_params(abi, samples=8, batch=4, traversal="near", sampler=2 if scene == "deep" else 1)
    st = trace.TraceState(ctx.sa, ctx.bvh, ctx.lights, p, lib)
    st.set_counters(1)
    st.trace_range(0, 4)
    first = st.get_image()  # traces the four samples
    st.trace_range(4, 5)    # stays queued
    queued = st.samples
    if call:
        r = Q.rays(ctx, "generic", oracle)
        st.intersect_multi(r, 4), st.intersect_multi(r, 16, mixed_instance_ids(ctx), tmax=1.5), st.count_hits(r), st.count_hits(r, tmax=0.7)
        st.transmittance(r, k=2)
        assert st.samples == queued
    img = st.get_image()
    alb, nrm, nhits = st.get_aovs()
    out = {"first": first, "image": img, "albedo": alb, "normal": nrm, "hits": nhits, "variance": st.variance()}
    cnt = st.counters()
    cnt.pop("kernel_ms")
    state = (queued, st.samples, st.streams)
    st.close()
    return out, cnt, state


@pytest.mark.parametrize("scene", ["cornell", "deep"])
def test_the_new_calls_leave_the_context_untouched(scene, abi, lib, oracle, gpu):
    a, ca, sa = _render(abi, lib, oracle, scene, True)
    b, cb, sb = _render(abi, lib, oracle, scene, False)
    assert sa == sb and sa[1] == 5, (sa, sb)
    assert ca == cb, (ca, cb)  # every field but kernel_ms
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (scene, k)
    assert a["hits"].sum() > 0 and a["albedo"].mean() > 0


# ------------------------------------------------------------------------------ 8. transmittance
def test_transmittance_through_half_opaque_plates(abi, lib, oracle, gpu):
    """The plates scene with opacity 0.5: T is 0.5^count exactly (powers of two) wherever the list
    is complete, and complete is false exactly where count_hits >= k."""
    from jtrace import trace
    sc = SR.plates_scene()
    sc.materials[0].opacity = np.float32(0.5)
    sa = abi.SceneABI(sc)
    st = trace.make_trace_state(sa, trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib),
                                make_params(abi, traversal="near"), lib)
    ctx = Q.context("plates", abi, oracle)
    r = np.concatenate([Q.rays(ctx, "generic", oracle)[:2000], Q.rays(ctx, "stacked", oracle)[:99]])
    counts = st.count_hits(r)
    for k in (8, 3):
        T, complete = st.transmittance(r, k=k)
        assert T.dtype == np.float32 and complete.dtype == np.bool_ and T.shape == complete.shape == (len(r),)
        assert np.array_equal(complete, counts < k), k
        assert complete.sum() > 100 and (~complete).sum() > 99 and (counts[complete] > 1).sum() > 20
        assert np.array_equal(T[complete], np.ldexp(np.float32(1), -counts[complete]).astype(np.float32)), k
        assert np.array_equal(T[~complete], np.full(int((~complete).sum()), 0.5 ** k, np.float32)), k
    T, complete = st.transmittance(r, tmax=0.3, k=8)
    bounded = st.count_hits(r, tmax=0.3)
    assert np.array_equal(complete, bounded < 8) and np.array_equal(T[complete], np.ldexp(np.float32(1), -bounded[complete]).astype(np.float32))
    print(f"transmittance: {len(r)} rays, {int(counts.sum())} crossings, {int((counts >= 8).sum())} rays with 8 or more")
    st.close()
