"""Bounded ray queries on a context's scene (csrc/jt_intersect.hip behind jt_intersect_bounded,
jt_occluded_bounded, jt_visible and their device-pointer variants), ray by ray, no tolerance.

The reference of the reference and near orders is the restatement of tests/bounded_ref.py (held to
or_query at an infinite bound by tests/test_bounded_host.py); the wide order, whose quantised boxes
are not restated, is held to what follows from the contract alone. N = 4099 rays per case, the
scenes, classes and contexts of tests/test_gpu_intersect.py (LDS mode and lds_scene = 0,
test_lds_ring = 2, the deep scene through the overflow).

Bounds per ray come from the order's own unbounded t_i (a miss: a seeded finite bound of the
scene's size), bounded_ref.family_bounds:
  A  the bits of t_i: a hit exactly on the bound, the tie path runs
  B  nextafter(t_i, 0)
  C  t_i * u, u seeded log-uniform in [0.25, 4]
  D  +inf, FLT_MAX and no bound array at all

Family B in every order: every ray is a miss, exactly. A bounded query's tmax never exceeds the
unbounded query's at the same node and the slab test is monotone in tmax, so it visits a subset of
the unbounded query's leaves, and none of them holds a hit below t_i.
Wide order, hits: with the bound 2 t_i the result is the wide order's own unbounded record, except
where a rounding cull differs (the cause behind queries_ref.ORDER_DIFFS), capped at 0.1 % of a
case's rays; tests/test_bounded_host.py shows the same inputs at 0 in the restated orders.
"""
import numpy as np
import pytest

import bounded_ref as B
import queries_ref as Q
from conftest import make_params
from test_bounded_host import DOUBLED
from test_gpu_intersect import (INSTANCE_CLASSES, INSTANCE_SCENES, check_hits, contexts, mixed_instance_ids,  # noqa: F401
                                oracle_query, variants)

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SEGMENT_TMAX = np.float32(1) - np.float32(0.0001)  # jt_visible's bound: 1 - ray_eps in float32


def same_records(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def miss_record(out):
    return ((out["hit"] == 0) & (out["instance"] == -1) & (out["element"] == -1) & np.isposinf(out["t"]) &
            (out["u"].view(np.uint32) == 0) & (out["v"].view(np.uint32) == 0))


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_bounded_hits_equal_the_restatement_ray_by_ray(scene, cls, contexts, abi, oracle):
    """Families A to C. Reference and near: every field and bit of the restatement's record, no ray
    excluded. Every order: occluded_bounded is intersect_bounded's hit flag, and family B misses."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in Q.ORDERS:
        free = oracle_query(oracle, ctx, cls, order)
        for family in "ABC":
            bounds = B.family_bounds(ctx, cls, family, free)
            ref = B.query(ctx, oracle, order, r, None, bounds) if order != "wide" else None
            for opts in variants(scene):
                label = f"{scene}/{cls}/{order}/{family}/{opts}"
                st = contexts.get(scene, order, **opts)
                out = st.intersect(r, tmax=bounds)
                if ref is not None:
                    check_hits(out, ref, label)
                occ = st.occluded(r, tmax=bounds)
                assert occ.dtype == np.bool_ and occ.shape == (len(r),)
                bad = np.flatnonzero(occ != (out["hit"] != 0))
                assert len(bad) == 0, (label, "occluded against intersect", len(bad), bad[:4])
                if family == "B":
                    bad = np.flatnonzero(~miss_record(out))
                    assert len(bad) == 0, (label, "a hit below the closest hit", len(bad), bad[:4], out[bad[:4]])
            if ref is not None:
                print(f"{scene}/{cls}/{order}/{family}: {int(ref['hit'].sum())} hits of {int((free['hit'] != 0).sum())} unbounded, "
                      f"{int(ref['tie'].sum())} ties on the first run")


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_an_infinite_bound_gives_the_bits_of_intersect(scene, cls, contexts, abi, oracle):
    """Family D, every order: +inf, FLT_MAX (above every t of these scenes) and no bound."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in Q.ORDERS:
        for opts in variants(scene):
            st = contexts.get(scene, order, **opts)
            free, occ = st.intersect(r), st.occluded(r)
            for bound in (np.inf, np.full(len(r), np.inf, np.float32), FLT_MAX, None):
                assert same_records(st.intersect(r, tmax=bound), free), (scene, cls, order, opts, bound)
                assert np.array_equal(st.occluded(r, tmax=bound), occ), (scene, cls, order, opts, bound)


@pytest.mark.parametrize("scene", INSTANCE_SCENES)
@pytest.mark.parametrize("cls", INSTANCE_CLASSES)
def test_bounded_instance_queries_equal_the_restatement(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for inst in (Q.instance_ids(ctx), mixed_instance_ids(ctx)):
        for order in ("reference", "near"):
            free = oracle_query(oracle, ctx, cls, order, inst)
            for family in "ABC":
                bounds = B.family_bounds(ctx, cls, family, free)
                ref = B.query(ctx, oracle, order, r, inst, bounds)
                for opts in variants(scene):
                    out = contexts.get(scene, order, **opts).intersect(r, inst, tmax=bounds)
                    check_hits(out, ref, f"{scene}/{cls}/{order}/{family}/{opts}/instance")


@pytest.mark.parametrize("scene,cls", DOUBLED)
def test_wide_order_with_twice_the_hit_distance_keeps_its_record(scene, cls, contexts, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    st = contexts.get(scene, "wide")
    free = st.intersect(r)
    check_hits(free, oracle_query(oracle, ctx, cls, "wide"), f"{scene}/{cls}/wide/unbounded")
    bounds = B.doubled_bounds(ctx, cls, {"hit": free["hit"], "t": free["t"]})
    out = st.intersect(r, tmax=bounds)
    bad = np.flatnonzero((out.view(np.uint8).reshape(len(r), -1) != free.view(np.uint8).reshape(len(r), -1)).any(axis=1))
    print(f"{scene}/{cls}/wide, bound 2 t: {len(bad)} of {len(r)} rays differ from the unbounded record")
    assert len(bad) <= len(r) // 1000, (scene, cls, len(bad), bad[:4], out[bad[:4]], free[bad[:4]])
    assert (free["hit"] != 0).sum() > 50


def wall_segments(st, seed=11, n=Q.N):
    """Segments between seeded pairs of the surface points under the context's pixels."""
    _, hits, surf = st.gbuffer(-1)
    p = surf["position"][hits["hit"] != 0]
    assert len(p) > 1000
    rng = np.random.default_rng(seed)
    a, b = p[rng.integers(len(p), size=n)], p[rng.integers(len(p), size=n)]
    keep = (a != b).any(axis=1)
    return np.ascontiguousarray(np.concatenate([a, b], 1)[keep], np.float32)


@pytest.mark.parametrize("order", Q.ORDERS)
def test_visible_is_the_bounded_any_hit_query_of_the_segment(order, contexts, abi, oracle):
    st = contexts.get("cornell", order)
    seg = wall_segments(st)
    rays = np.concatenate([seg[:, :3], seg[:, 3:] - seg[:, :3]], 1).astype(np.float32)  # one float32 subtraction per component
    vis = st.visible(seg)
    assert vis.dtype == np.bool_ and vis.shape == (len(seg),)
    assert np.array_equal(vis, ~st.occluded(rays, tmax=SEGMENT_TMAX)), order
    # what the unbounded closest hit decides: nothing at or below the bound, so nothing hides b from a;
    # among these are the pairs whose first hit is the target's own surface at t ~ 1
    first = st.intersect(rays)
    free = (first["hit"] == 0) | (first["t"] > SEGMENT_TMAX)
    own = (first["hit"] != 0) & (np.abs(first["t"] - 1) < 5e-5)
    assert vis[free].all(), (order, int((~vis[free]).sum()))
    assert own.sum() > 500 and vis[own].all() and (~vis).sum() > 100, (order, int(own.sum()), int((~vis).sum()))
    print(f"{order}: {len(seg)} segments, {int(vis.sum())} visible, {int(own.sum())} end on the target's own surface")


@pytest.mark.parametrize("scene,order", [("cornell", "near"), ("deep", "wide")])
def test_order_and_split_independence(scene, order, contexts, abi, oracle):
    """A permuted array gives permuted results; heads of 1, 63, 64, 65 rays; 700 copies across the
    grid's refills, whose blocks 0, 1, 349 and 699 are the small call's."""
    ctx = Q.context(scene, abi, oracle)
    st = contexts.get(scene, order)
    r = Q.rays(ctx, "generic", oracle)
    bounds = B.family_bounds(ctx, "generic", "C", oracle_query(oracle, ctx, "generic", order))
    seg = np.concatenate([r[:, :3], r[:, :3] + r[:, 3:] * bounds[:, None]], 1).astype(np.float32)
    small = st.intersect(r, tmax=bounds), st.occluded(r, tmax=bounds), st.visible(seg)
    assert (small[0]["hit"] != 0).sum() > 20 and (small[0]["hit"] == 0).sum() > 20
    perm = np.random.default_rng(5).permutation(len(r))
    assert same_records(st.intersect(r[perm], tmax=bounds[perm]), small[0][perm])
    assert np.array_equal(st.occluded(r[perm], tmax=bounds[perm]), small[1][perm])
    assert np.array_equal(st.visible(seg[perm]), small[2][perm])
    for n in (1, 63, 64, 65):
        assert same_records(st.intersect(r[:n], tmax=bounds[:n]), small[0][:n]), n
        assert np.array_equal(st.occluded(r[:n], tmax=bounds[:n]), small[1][:n]), n
        assert np.array_equal(st.visible(seg[:n]), small[2][:n]), n
    reps, blocks = 700, (0, 1, 349, 699)
    assert reps * len(r) > 4 * 256 * 8 * 256
    rr, bb = np.tile(r, (reps, 1)), np.tile(bounds, reps)
    big = st.intersect(rr, tmax=bb).reshape(reps, len(r)), st.occluded(rr, tmax=bb).reshape(reps, len(r)), \
        st.visible(np.tile(seg, (reps, 1))).reshape(reps, len(r))
    for k in blocks:
        assert same_records(big[0][k], small[0]), (scene, order, k)
        assert np.array_equal(big[1][k], small[1]) and np.array_equal(big[2][k], small[2]), (scene, order, k)
    assert st.intersect(np.zeros((0, 6), np.float32), tmax=1.0).shape == (0,)
    assert st.occluded(np.zeros((0, 6), np.float32), tmax=1.0).shape == (0,) and st.visible(np.zeros((0, 6), np.float32)).shape == (0,)


def test_device_pointer_path_gives_the_host_path_bits(contexts, abi, oracle):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the zero-copy path needs a tensor on the context's device")
    for scene, order in (("cornell", "near"), ("deep", "wide")):
        ctx = Q.context(scene, abi, oracle)
        st = contexts.get(scene, order)
        r = Q.rays(ctx, "generic", oracle)
        bounds = B.family_bounds(ctx, "generic", "C", oracle_query(oracle, ctx, "generic", order))
        inst = mixed_instance_ids(ctx)
        tr, tb = torch.from_numpy(np.array(r)).to("cuda:0"), torch.from_numpy(bounds).to("cuda:0")
        for ins in (None, inst):
            host = st.intersect(r, ins, tmax=bounds)
            dev = st.intersect(tr, None if ins is None else torch.from_numpy(ins).to("cuda:0"), tmax=tb)
            assert dev.dtype == torch.int32 and tuple(dev.shape) == (len(r), 6) and dev.is_cuda
            assert np.array_equal(dev.cpu().numpy().reshape(-1).view(np.uint8), host.view(np.uint8)), (scene, order)
        occ = st.occluded(tr, tmax=tb)
        assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), st.occluded(r, tmax=bounds))
        # a scalar bound on the device path, and a bound given as a numpy array
        assert np.array_equal(st.occluded(tr, tmax=0.5).cpu().numpy(), st.occluded(r, tmax=0.5))
        assert np.array_equal(st.occluded(tr, tmax=bounds).cpu().numpy(), st.occluded(r, tmax=bounds))
        seg = np.concatenate([r[:, :3], r[:, :3] + r[:, 3:] * bounds[:, None]], 1).astype(np.float32)
        vis = st.visible(torch.from_numpy(seg).to("cuda:0"))
        assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), st.visible(seg))


def _render(abi, lib, oracle, scene, call):
    """Four traced samples and one queued; with `call`, every new entry point runs while it is queued."""
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
        seg = np.concatenate([r[:, :3], r[:, :3] + r[:, 3:]], 1).astype(np.float32)
        st.intersect(r, tmax=1.5), st.intersect(r, mixed_instance_ids(ctx), tmax=1.5), st.occluded(r, tmax=1.5), st.visible(seg)
        st.ambient_occlusion(r, 0.7, 0, 3), st.ambient_occlusion(r, np.inf, 2, 3, stream_base=5)
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
