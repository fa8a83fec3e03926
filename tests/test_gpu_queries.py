"""The product's BVH traversal, ray by ray: tests/probe/jt_query.hip lays a scene out with the
product's host code, uploads it and runs csrc/jt_traverse.h's own functions (query_start, prim_step,
node_step_any, rerun_tie; COUNT = 1) over the rays of tests/queries_ref.py, one lane per ray, in
every traversal form the product builds. Each ray's result is compared with the oracle's or_query
in the same order, bit for bit, no ray excluded and no tolerance; tests/test_queries_host.py (CPU)
compares or_query with a brute force.

Compared per ray: hit, instance (mapped back to the reference's numbering), element, the bits of u
and v; the bits of t on a hit (a miss leaves t = +inf on the device, the query's tmax, and 0 in the
oracle's record: the device's inf is asserted); nh & 63 against min(the oracle's accepted hits, 63);
the node, instance and primitive counts; the largest sp against the laid-out bound; the guard
entries behind every stack.

Counters in the wide order: compared too. The oracle's wide traversal (w_scene / w_shape) counts one
node per record visit, one instance per instance visit and one primitive per test, tie re-run
included, which is wide_visit's and prim_step's convention (established from the two sources).

Forms (jt_query.hip FORMS; the feature masks the traversal can tell apart differ in FT_XFORM and
FT_QUAD only). Each runs with FT_ALL and with the smallest of FT_NONE, FT_MESH, FT_MESH_ENV_QUAD
that covers the scene, where the product builds that combination (CONFIGS, csrc/jt_select.h):
  binary, order_flip 0 and 7:  hbm_fixed (child pre-test, 16 entries) all / none
                               hbm_ovf at S.ring 16 and 2           all / mesh / mesh_env_quad
                               lds_plan (push_plan)                 all
                               lds_baked (bake_nodes, PB)           none
                               lds_ovf at S.ring 16 and 2           all
  wide:                        wide_hbm_fixed all / none, wide_hbm_ovf at rings 16 and 2 all / mesh /
                               mesh_env_quad, wide_lds all / none
Skipped, with the reason:
  - fixed-stack forms with FT_MESH / FT_MESH_ENV_QUAD, overflow forms with FT_NONE, LDS forms with
    FT_MESH / FT_MESH_ENV_QUAD, lds_ovf other than FT_ALL: the product never builds them (no such
    row in CONFIGS, or the row has no LDS-mode kernel);
  - lds_plan with FT_NONE: the product's LDS FT_NONE binary fixed-stack kernels are the baking ones
    (node_baked), which is lds_baked;
  - per scene, as jq_form_skip answers and the test prints: a mask that does not cover the scene or
    is not its smallest cover; hbm_fixed and every LDS fixed form on the deep scene (bound 28 > 16:
    the product runs such a scene with overflow); every LDS form on the deep scene (its blob is
    above the 48 KiB LDS budget); lds_baked on scenes that are not identity-frame matte triangles.
"""
import numpy as np
import pytest

import queries_ref as Q

pytestmark = pytest.mark.gpu

BINARY = ("hbm_fixed/all", "hbm_fixed/none", "hbm_ovf/all", "hbm_ovf/mesh", "hbm_ovf/mesh_env_quad", "lds_plan/all",
          "lds_baked/none", "lds_ovf/all")
WIDE = ("wide_hbm_fixed/all", "wide_hbm_fixed/none", "wide_hbm_ovf/all", "wide_hbm_ovf/mesh", "wide_hbm_ovf/mesh_env_quad",
        "wide_lds/all", "wide_lds/none")
HIT_KEYS = ("hit", "inst", "elem")
COUNT_KEYS = ("nodes", "instances", "prims")


@pytest.fixture(scope="module")
def qprobe(gpu):
    p = Q.QueryProbe()  # a missing probe library is an error, not a skip
    assert tuple(p.forms) == BINARY + WIDE
    return p


@pytest.fixture(scope="module")
def device(qprobe, abi, oracle):
    """The scene laid out for an order and uploaded: once per (scene, order) for the whole module."""
    opened = {}

    def get(scene, order):
        if (scene, order) not in opened:
            opened[scene, order] = qprobe.open(Q.context(scene, abi, oracle), order)
        return opened[scene, order]
    yield get
    for d in opened.values():
        d.close()


def rings(form):
    return (16, 2) if "ovf" in form else (16,)


def check_against_oracle(out, ref, need, label):
    """One form's output against or_query's, every ray."""
    assert (out["flags"] == 0).all(), (label, "guard / step cap / bound", np.unique(out["flags"]))
    for k in HIT_KEYS:
        bad = np.flatnonzero(out[k] != ref[k])
        assert len(bad) == 0, (label, k, len(bad), bad[:4], out[k][bad[:4]], ref[k][bad[:4]])
    hit = ref["hit"] != 0
    for k in ("u", "v"):
        bad = np.flatnonzero(~Q.same_bits(out[k], ref[k]))
        assert len(bad) == 0, (label, k, len(bad), bad[:4])
    bad = np.flatnonzero(hit & ~Q.same_bits(out["t"], ref["t"]))
    assert len(bad) == 0, (label, "t", len(bad), bad[:4], out["t"][bad[:4]], ref["t"][bad[:4]])
    assert np.isposinf(out["t"][~hit]).all(), (label, "t of a miss")
    bad = np.flatnonzero(out["nh63"] != np.minimum(ref["nh"], 63))
    assert len(bad) == 0, (label, "nh & 63", len(bad), bad[:4], out["nh63"][bad[:4]], ref["nh"][bad[:4]])
    for k in COUNT_KEYS:
        bad = np.flatnonzero(out[k] != ref[k])
        assert len(bad) == 0, (label, k, len(bad), bad[:4], out[k][bad[:4]], ref[k][bad[:4]])
    assert out["maxsp"].max() <= need, (label, "largest sp", int(out["maxsp"].max()), need)


def differing(a, b):
    """Ray indices where two results (device or oracle) differ in hit, ids or the bits of u, v, t."""
    hit = (a["hit"] != 0) | (b["hit"] != 0)
    d = np.zeros(len(a["hit"]), bool)
    for k in HIT_KEYS:
        d |= a[k] != b[k]
    for k in ("u", "v", "t"):
        d |= hit & ~Q.same_bits(a[k], b[k])
    return np.flatnonzero(d)


def run_forms(dev, forms, r, inst, ref, label):
    """Every form of `forms` the scene allows, at every ring: each equals the oracle, and all of
    them (FT_ALL and the specialised mask, rings 16 and 2, HBM and LDS) equal each other."""
    ran, skipped = [], []
    for form in forms:
        reason = dev.skip_reason(form)
        if reason:
            skipped.append(f"{form}: {reason}")
            continue
        for ring in rings(form):
            out = dev.run(form, r, inst=inst, ring=ring)
            check_against_oracle(out, ref, dev.need, f"{label}/{form}/ring{ring}")
            ran.append((f"{form}/ring{ring}", out))
    assert ran, label
    base = ran[0][1]
    for name, out in ran[1:]:
        for k in HIT_KEYS + COUNT_KEYS + ("nh63",):
            assert np.array_equal(out[k], base[k]), (label, name, k)
        for k in ("u", "v", "t"):
            assert Q.same_bits(out[k], base[k]).all(), (label, name, k)
    return ran, skipped


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_every_form_equals_the_oracle_ray_by_ray(scene, cls, device, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r, inst = Q.rays(ctx, cls, oracle), Q.instance_ids(ctx)
    first, oref = {}, {}
    for order in Q.ORDERS:
        dev = device(scene, order)
        assert dev.order_flip == (0 if order == "reference" else 7) and dev.wide == (order == "wide")
        for kind, ins in (("scene", None), ("instance", inst)):
            ref = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], r, inst=ins)
            ran, skipped = run_forms(dev, WIDE if order == "wide" else BINARY, r, ins, ref, f"{scene}/{cls}/{order}/{kind}")
            first[order, kind], oref[order, kind] = ran[0][1], ref
            if (scene, cls, kind) == ("deep", "edges", "scene") and order != "wide":
                # the whole 16-entry ring in use and still some entries spill to HBM
                assert max(int(o["maxsp"].max()) for _, o in ran) > 16
            if kind == "scene":
                print(f"{scene}/{cls}/{order}: need={dev.need} feat={dev.feat} ran {[n for n, _ in ran]} "
                      f"largest sp {max(int(o['maxsp'].max()) for _, o in ran)} hits {int((ref['hit'] != 0).sum())} "
                      f"max accepted {int(ref['nh'].max())}; skipped {skipped}")
    # the near and the wide order report the reference order's hit on every ray, ties included;
    # where the reference's own slab test makes the oracle's orders differ (Q.ORDER_DIFFS, pinned
    # and explained on the CPU), the device differs on exactly those rays
    for order in ("near", "wide"):
        for kind in ("scene", "instance"):
            d = differing(first[order, kind], first["reference", kind])
            o = differing(oref[order, kind], oref["reference", kind])
            assert np.array_equal(d, o), (scene, cls, order, kind, d[:4], o[:4])
            if kind == "scene" and (scene, cls, order) not in Q.ORDER_DIFFS:
                assert len(d) == 0, (scene, cls, order, d[:4])


def test_saturated_hit_count(device, abi, oracle):
    """Rays through all 90 plates accept a hit on every plate in the reference order: the oracle
    counts more than 63, the device's nh & 63 stays at 63, and in the HBM form with the child
    pre-test (whose snapshots are that count) the hit is still the oracle's."""
    ctx = Q.context("plates", abi, oracle)
    r = Q.rays(ctx, "stacked")
    ref = oracle.query(ctx.sa, ctx.bvh, ctx.params["reference"], r)
    many = ref["nh"] > 63
    assert many.sum() > 1000
    out = device("plates", "reference").run("hbm_fixed/all", r)
    assert (out["nh63"][many] == 63).all() and (out["nh63"][~many] == ref["nh"][~many]).all()
    assert len(differing(out, dict(ref, t=np.where(ref["hit"] != 0, ref["t"], np.float32(np.inf)).astype(np.float32)))) == 0


@pytest.mark.parametrize("scene", ["cornell", "random", "quads9", "coplanar"])
def test_inst_leaf_query_leaves_the_state_of_start_and_step(scene, device, abi, oracle):
    """inst_leaf_query on the one-leaf light shapes: every field of the query and the counters end
    as query_start + node_step leave them (its comment's promise), in the LDS fixed-stack binary
    kernels that call it: <FT_ALL> on push_plan and, for matte identity-frame scenes, the baking
    <FT_NONE | FT_LINL>."""
    ctx = Q.context(scene, abi, oracle)
    for order in ("reference", "near"):
        dev = device(scene, order)
        assert len(dev.leaf_roots) > 0, scene
        for cls in ("generic", "axis", "edges"):
            r = Q.rays(ctx, cls, oracle)
            inst = dev.leaf_roots[np.arange(len(r)) % len(dev.leaf_roots)].astype(np.int32)
            for baked in ((0, 1) if dev.feat == 0 else (0,)):
                a, b = dev.run_leaf(baked, r, inst)
                bad = np.flatnonzero((a != b).any(1))
                assert len(bad) == 0, (scene, order, cls, baked, len(bad), bad[:4], a[bad[:2]].tolist(), b[bad[:2]].tolist())
                assert (a[:, 19] == 0).all()  # sp
