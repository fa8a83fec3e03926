"""The instance-root rows of the baking kernels (csrc/jt_push.h instance_root_base; bake_nodes,
node_step, query_start, inst_leaf_query) against the kernels that read the same scene with plain
instance entries, and against the oracle.

In the fixed-stack LDS kernels of matte scenes an instance's stack entry is the node index of a baked
copy of its BLAS root, written over the LDS copy of inst_trav; HBM mode (lds_scene=0) and the LDS
ring-overflow kernel (test_lds_ring) keep the instance number and read inst_blas. Each scene runs
through all three at 32x32 x 4 spp, batch 4, in the reference and the near-first order, with the
bars of tests/test_gpu_node_bake.py: the three images and hit counts bit-identical; nodes, instances,
prims, rays and light queries equal to each other and to the oracle's; the image against the oracle
at bitwise_frac >= 0.999, frac_pix_rel_le_1e-3 >= 0.999, image_mean_rel <= 1e-4.

Scenes (all matte, identity frames, triangles):
  nine     nine instances: the TLAS has internal nodes and leaves of differing sizes, so runs of
           1..4 root rows are pushed from several starts; one instance is an emissive quad, whose
           one-leaf root the inline light chain reads from its row (inst_leaf_query)
  shared   two instances of one box shape in the same place: two rows copy the same root, and in the
           near-first order the second box's hits land exactly on tmax, so the query runs again in
           the reference's order (rerun_tie) through the rows with the re-run's push mask
  even/odd two scenes that differ only in one shape's triangle count (1 or 3: one primitive record
           more), so that o_inst_trav - o_nodes is even in one and odd in the other: iroot0 with
           and without the half-node round-up
  steps    the light-hit-steps kernel's scene (mask 0): the light is a box whose BVH has more than
           one leaf, and every triangle of it is listed twice, so a light's instance query — started
           by query_start with the instance's row entry — ties inside the instance in the near-first
           order and rerun_tie starts the instance-tagged query again
"""
import ctypes as C

import numpy as np
import pytest

from conftest import compare_images, make_params
from jtrace.scene import CameraData, InstanceData, MaterialData, SceneData, ShapeData

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 4
NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("start", "<i4"), ("num", "<i2"), ("axis", "i1"),
                 ("internal", "i1")])
MODES = {"lds": None, "hbm": ("lds_scene", "0"), "ring": ("test_lds_ring", "2")}
COUNTERS = ("nodes", "instances", "prims", "rays", "light_queries")

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
BOX_TRIS = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
UNIT = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _box(rng, size, centre):
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    return ((corners * size) @ _rotation(rng).T + np.asarray(centre, np.float64)).astype(np.float32)


def _quad(size, centre):
    return (UNIT * size + np.asarray(centre, np.float64)).astype(np.float32)


def _base():
    sc = SceneData()
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], np.float32), aspect=np.float32(1.0)))
    sc.materials += [MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)),
                     MaterialData(emission=np.array([8, 7, 6], np.float32), color=np.zeros(3, np.float32)),
                     MaterialData(color=np.array([0.3, 0.6, 0.4], np.float32))]
    return sc


def _add(sc, positions, triangles, material):
    sc.shapes.append(ShapeData(positions=positions, triangles=triangles))
    sc.instances.append(InstanceData(frame=IDENTITY, shape=len(sc.shapes) - 1, material=material))


def nine_scene():
    rng = np.random.default_rng(23)
    sc = _base()
    _add(sc, _quad(1.2, [0, 0, 3.5]), QUAD_TRIS, 1)   # the light
    _add(sc, _quad(3.5, [0, 0, -2.5]), QUAD_TRIS, 0)  # the floor
    _add(sc, _box(rng, 0.7, [2.0, -1.8, -1.2]), BOX_TRIS, 2)
    # small shapes keep the blob within LDS mode's budget: three quads and three single triangles
    for k, centre in enumerate([[-2.2, -2.0, -1.2], [-2.0, 1.9, -0.8], [0.3, 0.4, -0.2]]):
        _add(sc, _quad(0.7, centre), QUAD_TRIS, 2 * (k & 1))
    for k, centre in enumerate([[-0.4, -2.1, -1.0], [2.1, 2.0, -1.1], [-2.6, 0.0, -0.5]]):
        tri = rng.normal(size=(3, 3)) * 0.8 + np.asarray(centre)
        _add(sc, tri.astype(np.float32), np.array([[0, 1, 2]], np.int32), 2 * (k & 1))
    return sc


def shared_scene():
    sc = _base()
    _add(sc, _quad(1.2, [0, 0, 3.5]), QUAD_TRIS, 1)
    _add(sc, _quad(3.0, [0, 0, -2.5]), QUAD_TRIS, 0)
    _add(sc, _box(np.random.default_rng(5), 1.1, [0.4, -0.2, -0.8]), BOX_TRIS, 0)
    sc.instances.append(InstanceData(frame=IDENTITY, shape=2, material=2))  # the box once more, coincident
    return sc


def parity_scene(ntri):
    sc = _base()
    _add(sc, _quad(1.2, [0, 0, 3.5]), QUAD_TRIS, 1)
    _add(sc, _quad(3.0, [0, 0, -2.5]), QUAD_TRIS, 0)
    fan = np.array([[-0.5, -0.5, -0.6], [2.0, -1.5, -0.5], [2.2, 0.8, -0.2], [0.5, 2.2, -0.4], [-1.8, 1.6, -0.8]], np.float32)
    _add(sc, fan, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], np.int32)[:ntri], 2)
    return sc


def steps_scene():
    sc = _base()
    _add(sc, _box(np.random.default_rng(7), 1.4, [-0.6, 0.3, 0.5]), np.concatenate([BOX_TRIS, BOX_TRIS]), 1)
    _add(sc, _quad(3.0, [0, 0, -2.5]), QUAD_TRIS, 0)
    _add(sc, _box(np.random.default_rng(9), 0.7, [2.0, -1.6, -1.2]), BOX_TRIS, 2)
    return sc


_oracle = {}


def oracle_run(abi, oracle, name, order, streams):
    """The oracle's (image, ..., hits, counters) of a scene in one order, computed once."""
    if (name, order, streams) not in _oracle:
        sa = scene_abi(abi, name)
        params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=1, traversal=order)
        _oracle[name, order, streams] = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, W, H, 0, SPP,
                                                     streams=streams)
    return _oracle[name, order, streams]


def assert_reruns(abi, oracle, out, name):
    """A near-first run whose ties were run again in the reference's order. A re-run is the same
    query (rays and light queries as in the reference order) with its node, instance and primitive
    work counted once more; without re-runs the near-first order visits no more nodes than the
    reference order on these scenes (`nine`, which has no ties: fewer of all three). _check has
    already tied the kernels' counters to the oracle's near-first ones."""
    near = out["lds"][2]
    ref = oracle_run(abi, oracle, name, "reference", out["lds"][4])[4]
    print(name, "near", {k: near[k] for k in COUNTERS}, "reference order", {k: ref[k] for k in COUNTERS})
    for key in ("rays", "light_queries"):
        assert near[key] == ref[key], (name, key, near[key], ref[key])
    for key in ("nodes", "instances", "prims"):
        assert near[key] > ref[key], (name, key, near[key], ref[key], "no tie re-run took place")


BUILD = {"nine": nine_scene, "shared": shared_scene, "even": lambda: parity_scene(1), "odd": lambda: parity_scene(3),
         "steps": steps_scene}
_scenes = {}


def scene_abi(abi, name):
    if name not in _scenes:
        _scenes[name] = abi.SceneABI(BUILD[name]())
    return _scenes[name]


def _leaf_sizes(tree):
    nodes = np.ctypeslib.as_array(C.cast(tree.nodes, C.POINTER(C.c_uint8)), shape=(tree.nnodes * 32,)).view(NODE)
    return sorted(int(n["num"]) for n in nodes if not n["internal"])


def tlas_leaf_sizes(bvh):
    return _leaf_sizes(bvh.struct.tlas)


def blas_leaf_sizes(bvh, shape):
    return _leaf_sizes(bvh.struct.blas[shape])


def layout_offsets(abi, lib, sa, bvh, lights, params):
    """(o_nodes, o_inst_trav) from the scalars line of jt_debug_layout_digest (no device is touched)."""
    buf = C.create_string_buffer(1 << 14)
    abi.check(lib, lib.jt_debug_layout_digest(sa.ref, bvh.ref, lights.ref, C.byref(params), buf, len(buf)))
    line = next(l for l in buf.value.decode().splitlines() if l.startswith("scalars"))
    assert " o_nodes=" in line and " o_inst_trav=" in line, line
    sc = dict(t.split("=") for t in line.split()[1:])
    return int(sc["o_nodes"]), int(sc["o_inst_trav"])


def _run(abi, lib, oracle, options, name, order):
    """The scene through the three kernels, and the oracle once: {mode: (image, hits, counters, describe)}, oracle."""
    from jtrace import trace
    sa = scene_abi(abi, name)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=1, traversal=order)
    bvh = trace.make_scene_bvh(sa, False, lib)
    lights = trace.make_trace_lights(sa, lib)
    out, k = {}, None
    for mode, opt in MODES.items():
        options("lds_scene", None)
        options("test_lds_ring", None)
        if opt:
            options(*opt)
        st = trace.make_trace_state(sa, bvh, lights, params, lib)
        st.trace_range(0, SPP)
        out[mode] = (st.get_image(), st.get_aovs()[2], st.counters(), st.describe(), st.streams)
        k = st.streams
        st.close()
    options("lds_scene", None)
    options("test_lds_ring", None)
    o = oracle_run(abi, oracle, name, order, k)
    return out, o, bvh, layout_offsets(abi, lib, sa, bvh, lights, params)


def _check(out, o, label, lds_mask):
    lds, hbm, ring = out["lds"], out["hbm"], out["ring"]
    # the baking kernel, the HBM-mode kernel and the LDS ring-overflow kernel (both with plain instance entries)
    assert f"kernel=trace_kernel_lds<1,16,false,1,{lds_mask},false> mode=lds " in lds[3], lds[3]
    assert "kernel=trace_kernel<1,16,false,1," in hbm[3] and " mode=hbm " in hbm[3], hbm[3]
    assert "kernel=trace_kernel_lds<1,16,true,1,255,false> mode=lds " in ring[3] and "ring_used=2" in ring[3], ring[3]
    for mode, g in out.items():
        print(label, mode, {key: g[2][key] for key in COUNTERS}, "oracle", {key: o[4][key] for key in COUNTERS})
    assert lds[0][..., :3].mean() > 0 and lds[1].sum() > 0, (label, "the scene must be hit and lit")
    assert o[4]["instances"] > 0 and o[4]["light_queries"] > 0, (label, "the oracle must visit instances and query lights")
    for mode in ("hbm", "ring"):
        assert np.array_equal(lds[0], out[mode][0]), (label, mode, compare_images(lds[0], out[mode][0]))
        assert np.array_equal(lds[1], out[mode][1]), (label, mode)
    for mode, g in out.items():
        for key in COUNTERS:
            assert g[2][key] == o[4][key], (label, mode, key, g[2][key], o[4][key])
    stats = compare_images(lds[0], o[0])
    print(label, stats)
    assert stats["frac_pix_rel_le_1e-3"] >= 0.999 and stats["bitwise_frac"] >= 0.999, (label, stats)
    assert stats["image_mean_rel"] <= 1e-4, (label, stats)
    assert np.array_equal(lds[1], o[3]), label  # hit counts


ORDERS = ["reference", "near"]


@pytest.mark.parametrize("order", ORDERS)
def test_nine_instances_in_leaves_of_differing_sizes(gpu, abi, lib, oracle, options, order):
    out, o, bvh, _ = _run(abi, lib, oracle, options, "nine", order)
    sizes = tlas_leaf_sizes(bvh)
    assert len(sizes) >= 2 and len(set(sizes)) >= 2 and sum(sizes) == 9, sizes
    assert blas_leaf_sizes(bvh, 0) == [2], "the light must be one leaf: its chain runs inline"
    assert "light_inline=1" in out["lds"][3], out["lds"][3]
    _check(out, o, f"nine/{order}", 8192)


@pytest.mark.parametrize("order", ORDERS)
def test_two_instances_share_one_root(gpu, abi, lib, oracle, options, order):
    out, o, bvh, _ = _run(abi, lib, oracle, options, "shared", order)
    assert len(blas_leaf_sizes(bvh, 2)) > 1, "the shared box must have internal nodes"
    _check(out, o, f"shared/{order}", 8192)
    if order == "near":  # the coincident boxes tie: scene queries run again through rerun_tie
        assert_reruns(abi, oracle, out, "shared")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["even", "odd"])
def test_both_alignments_of_the_row_base(gpu, abi, lib, oracle, options, name, order):
    out, o, bvh, (o_nodes, o_inst_trav) = _run(abi, lib, oracle, options, name, order)
    assert (o_inst_trav - o_nodes) % 2 == (0 if name == "even" else 1), (name, o_nodes, o_inst_trav)
    _check(out, o, f"{name}/{order}", 8192)


@pytest.mark.parametrize("order", ORDERS)
def test_light_hit_steps_instance_queries(gpu, abi, lib, oracle, options, order):
    out, o, bvh, _ = _run(abi, lib, oracle, options, "steps", order)
    assert len(blas_leaf_sizes(bvh, 0)) > 1, "the light's BVH must have more than one leaf"
    assert "light_inline=0" in out["lds"][3], out["lds"][3]
    _check(out, o, f"steps/{order}", 0)
    if order == "near":  # every hit on the doubled light ties inside its instance
        assert_reruns(abi, oracle, out, "steps")
