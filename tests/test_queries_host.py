"""Closest-hit queries on the CPU: the oracle's traversals (oracle/jt_oracle.c or_query: the
reference order, near-first and wide, tie re-run included) against a brute force over every
primitive (or_query_brute, no BVH), ray by ray, over the scenes and ray classes of
tests/queries_ref.py. tests/test_gpu_queries.py compares the device with or_query bit for bit; this
file is what makes or_query worth comparing with. No GPU.

The rule, per ray and order: t_bvh >= t_brute exactly (a traversal tests only primitives the brute
force tests too, with the same arithmetic), and either t_bvh == t_brute with the traversal's
(instance, element) among the brute force's minimisers, or the ray is excused: for every minimiser,
some box on the path from the root to its leaf in jt_scene_bvh rejects the ray under the reference's
own slab test (or_intersect_bbox, tmax = t_brute) — the reference culling its own hit. Excused rays
are counted and printed; on the generic and outside classes their share is capped at 0.1 %, the bar
of the image tests. The degenerate classes (axis-parallel directions from origins on box planes,
where 0 * inf is NaN and the slab test rejects) have no cap: their counts are the record.
"""
import numpy as np
import pytest

import queries_ref as Q

CAP = 64  # minimisers kept per ray (coplanar twins of doubled triangles at a shared vertex: 8 x 2 x 2)

ORDER_DIFFS = Q.ORDER_DIFFS  # the pinned cases where an order differs from the reference order

_cache = {}


def results(abi, oracle, scene, cls):
    """Per case, computed once: the rays, or_query in the three orders (t of a miss: inf), the brute force."""
    key = (scene, cls)
    if key not in _cache:
        ctx = Q.context(scene, abi, oracle)
        r = Q.rays(ctx, cls, oracle)
        q = {o: oracle.query(ctx.sa, ctx.bvh, ctx.params[o], r) for o in Q.ORDERS}
        for o in Q.ORDERS:
            q[o]["tm"] = np.where(q[o]["hit"] != 0, q[o]["t"], np.float32(np.inf)).astype(np.float32)
        _cache[key] = ctx, r, q, oracle.query_brute(ctx.sa, r, cap=CAP)
    return _cache[key]


def rejecting_box(ctx, oracle, ray, inst, elem, tmax):
    """Does a box on the path root -> leaf of (inst, elem) in jt_scene_bvh reject the ray at tmax?"""
    o, d = ray[:3], ray[3:]
    for k in ctx.tlas.path(inst):
        n = ctx.tlas.nodes[k]
        if not oracle.intersect_bbox(o, d, 1e-4, tmax, n["bmin"], n["bmax"]):
            return True
    lo, ld = oracle.instance_ray(ctx.scene.instances[inst].frame, o, d)
    tree = ctx.blas[ctx.scene.instances[inst].shape]
    for k in tree.path(elem):
        n = tree.nodes[k]
        if not oracle.intersect_bbox(lo, ld, 1e-4, tmax, n["bmin"], n["bmax"]):
            return True
    return False


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_traversal_against_brute_force(abi, oracle, scene, cls):
    ctx, r, q, (tb, nmin, mins) = results(abi, oracle, scene, cls)
    assert len(r) % 2 == 1 and np.isfinite(r).all()
    assert (nmin <= CAP).all(), nmin.max()
    line = []
    for order in Q.ORDERS:
        t = q[order]["tm"]
        assert (t >= tb).all(), (order, np.flatnonzero(~(t >= tb))[:4])
        same = t == tb
        hit = same & np.isfinite(tb)
        among = ((mins[:, :, 0] == q[order]["inst"][:, None]) & (mins[:, :, 1] == q[order]["elem"][:, None])).any(1)
        assert among[hit].all(), (order, np.flatnonzero(hit & ~among)[:4])
        farther = np.flatnonzero(~same)
        unexplained = [i for i in farther
                       if not all(rejecting_box(ctx, oracle, r[i], int(m[0]), int(m[1]), float(tb[i])) for m in mins[i, :nmin[i]])]
        line.append(f"{order}={len(farther)}")
        assert not unexplained, (order, unexplained[:4], r[unexplained[:2]].tolist())
        if cls in Q.CAPPED:
            assert len(farther) <= 1e-3 * len(r), (order, len(farther))
    print(f"excused {scene}/{cls}: n={len(r)} hits={int(np.isfinite(tb).sum())} " + " ".join(line))


@pytest.mark.parametrize("order", ["near", "wide"])
@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_orders_agree_with_the_reference_order(abi, oracle, scene, cls, order, request):
    """The near-first and the wide order report the reference order's hit on every ray, ties
    included (a tie is re-run in the reference's order). ORDER_DIFFS pins, strictly, the cases where
    the reference's own slab test makes the orders differ."""
    if (scene, cls, order) in ORDER_DIFFS:
        request.applymarker(pytest.mark.xfail(strict=True, reason="the reference's slab test culls differently per order: SURVEY.md Appendix B"))
    ctx, r, q, _ = results(abi, oracle, scene, cls)
    a, b = q[order], q["reference"]
    ids = (a["inst"] != b["inst"]) | (a["elem"] != b["elem"]) | (a["hit"] != b["hit"])
    bits = ~(Q.same_bits(a["tm"], b["tm"]) & (Q.same_bits(a["u"], b["u"]) & Q.same_bits(a["v"], b["v"]) | (b["hit"] == 0)))
    print(f"order diff {scene}/{cls}/{order}: ids={int(ids.sum())} bits={int(bits.sum())}")
    assert not ids.any() and not bits.any(), (int(ids.sum()), int(bits.sum()), np.flatnonzero(ids | bits)[:4])


def test_order_differences_are_the_references_own_culls(abi, oracle):
    """Every ray on which an order differs from the reference order (the pinned cases above) is
    explained by the reference's boxes: on the path of one of the two reported hits, a box of
    jt_scene_bvh rejects the ray at the nearer of the two distances. The orders ask those boxes at
    different moments (tmax larger or smaller) or, in the wide order, ask quantised ones instead."""
    for scene, cls, order in sorted(ORDER_DIFFS):
        ctx, r, q, _ = results(abi, oracle, scene, cls)
        a, b = q[order], q["reference"]
        diff = np.flatnonzero((a["inst"] != b["inst"]) | (a["elem"] != b["elem"]) | (a["hit"] != b["hit"]) |
                              ~Q.same_bits(a["tm"], b["tm"]))
        ties = int((a["tm"][diff] == b["tm"][diff]).sum())
        for i in diff:
            t = float(min(a["tm"][i], b["tm"][i]))
            assert any(w["hit"][i] and rejecting_box(ctx, oracle, r[i], int(w["inst"][i]), int(w["elem"][i]), t)
                       for w in (a, b)), (scene, cls, order, int(i), r[i].tolist())
        print(f"order diff {scene}/{cls}/{order}: {len(diff)} rays ({ties} ties, {len(diff) - ties} other t), all culled by a reference box")


def test_instance_queries_against_brute_force(abi, oracle):
    """intersect_instance_bvh in the three orders against the brute force over that instance alone,
    generic and edges rays, every scene."""
    for scene in Q.SCENES:
        ctx = Q.context(scene, abi, oracle)
        for cls in ("generic", "edges"):
            r, inst = Q.rays(ctx, cls, oracle), Q.instance_ids(ctx)
            tb, nmin, mins = oracle.query_brute(ctx.sa, r, inst=inst, cap=CAP)
            for order in Q.ORDERS:
                q = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], r, inst=inst)
                t = np.where(q["hit"] != 0, q["t"], np.float32(np.inf))
                assert (t >= tb).all(), (scene, cls, order)
                assert ((q["inst"] == inst) | (q["hit"] == 0)).all()
                farther = np.flatnonzero(t != tb)
                bad = [i for i in farther
                       if not all(rejecting_box(ctx, oracle, r[i], int(m[0]), int(m[1]), float(tb[i])) for m in mins[i, :nmin[i]])]
                assert not bad, (scene, cls, order, bad[:4])
                if cls in Q.CAPPED:
                    assert len(farther) <= 1e-3 * len(r), (scene, order, len(farther))


def test_deep_scene_bound_and_plates_hit_count(abi, oracle):
    """What the GPU tests rest on: the deep scene's laid-out stack bound is above 16 (the overflow
    forms spill with the whole 16-entry ring in use), and some stacked ray accepts more than 63 hits
    in the reference order (the device's count saturates there)."""
    probe = Q.QueryProbe()
    deep = Q.context("deep", abi, oracle)
    for order in Q.ORDERS:
        info = probe.layout_info(deep, order)
        assert info["need"] > 16, info
    assert len(deep.elems) <= 4096  # "a few thousand triangles"
    plates = Q.context("plates", abi, oracle)
    q = oracle.query(plates.sa, plates.bvh, plates.params["reference"], Q.rays(plates, "stacked"))
    assert q["nh"].max() > 63 and (q["hit"] != 0).all(), q["nh"].max()
    print("plates stacked: accepted hits max", int(q["nh"].max()), "rays above 63:", int((q["nh"] > 63).sum()))


def test_query_probe_is_outside_the_product():
    """libjt_query.so is test infrastructure: the product Makefile does not know it, the source hash
    does not cover it, and its compile line starts with the product's flag variables."""
    import re
    import sys
    sys.path.insert(0, str(Q.ROOT / "scripts"))
    from roofline import build_files
    assert not [f for f in build_files() if "query" in f or f.startswith("tests")]
    assert "query" not in (Q.ROOT / "julia-raytracer_amd" / "Makefile").read_text()
    from test_primitives_host import _make_vars
    probe_mk = Q.ROOT / "tests" / "probe" / "Makefile"
    rules = re.findall(r"^\t\$\(HIPCC\) (.*)$", probe_mk.read_text(), re.M)
    assert len(rules) == 5 and rules[3].split()[:4] == ["$(HIPFLAGS)", "$(KFLAGS)", "-I$(PKG)/csrc", "-c"], rules
    assert rules[3].split()[-1] == "jt_query.hip" and "$(HIPFLAGS)" not in rules[4]  # the last one only links
    # the two host units take the product's HOSTFLAGS (its jt_layout.o rule), defined the same way
    assert all(r.split()[:2] == ["$(HOSTFLAGS)", "-c"] for r in rules[1:3]), rules
    names = ["HOSTFLAGS", "ROCM_INC"]
    assert _make_vars(probe_mk, names) == _make_vars(Q.ROOT / "julia-raytracer_amd" / "Makefile", names)


@pytest.mark.parametrize("lib", [Q.QUERY_LIB, Q.ROOT / "julia-raytracer_amd" / "build" / "libjt_probe.so"])
def test_probe_kernels_are_built_for_gfx950(lib):
    """The device image of a probe library targets gfx950 and nothing else. (hipcc drops
    --offload-arch from a command line that carries -x c++, and the kernels then come out for the
    compiler's default GPU: a library without an image for the device fails at its first launch.)"""
    import re
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", lib.read_bytes()))
    assert targets == {b"gfx950"}, targets
