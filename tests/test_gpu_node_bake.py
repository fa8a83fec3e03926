"""The baked node step (csrc/jt_push.h bake_node / push_plan_baked; the bake pass of
trace_kernel_lds) against the kernels that read the same scene unbaked, and against the oracle.

The fixed-stack LDS kernels of matte scenes (the FT_NONE kernels, with inline light chains or
with light-hit steps) rewrite the nodes of their LDS copy once per launch and step on the baked
words; HBM mode (lds_scene=0) and the LDS ring-overflow kernel (test_lds_ring) keep
push_plan on the host's words. Each scene runs through all three at 32x32 x 4 spp, batch 4, in the
reference and the near-first order: the three images must be bit-identical and nodes, instances,
prims, rays and light queries equal, and equal to the oracle's (the image against the oracle at
tests/test_gpu_edge.py's bar: the oracle's libm may round a pixel differently).

Scenes:
  one     one instance of an emissive 12-triangle box: the TLAS root is itself a leaf of one
          instance (npush 1), the BLAS has internal nodes and leaves, and the light's BVH of more
          than one leaf makes it the light-hit-steps kernel's scene (mask 0)
  four    four instances in one TLAS leaf (npush 4): an emissive quad (the inline light chain reads
          its one-leaf BLAS root from the baked copy: inst_leaf_query), a one-triangle shape (a
          BLAS that is one leaf of one primitive), a quad and a box
  tie     `four` with a second instance of the quad's shape in the same place: in the near-first
          order the second hit lands exactly on tmax, so the query runs again in the reference's
          order, through the baked step with the re-run's push mask
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


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _box(rng, size, centre):
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    return ((corners * size) @ _rotation(rng).T + centre).astype(np.float32)


def _base():
    sc = SceneData()
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], np.float32), aspect=np.float32(1.0)))
    return sc


def one_scene():
    sc = _base()
    sc.materials.append(MaterialData(emission=np.array([2.0, 1.5, 1.0], np.float32), color=np.array([0.6, 0.5, 0.4], np.float32)))
    sc.shapes.append(ShapeData(positions=_box(np.random.default_rng(7), 2.0, np.zeros(3)), triangles=BOX_TRIS))
    sc.instances.append(InstanceData(frame=IDENTITY, shape=0, material=0))
    return sc


def four_scene(tie):
    rng = np.random.default_rng(11)
    sc = _base()
    sc.materials += [MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)),
                     MaterialData(emission=np.array([8, 7, 6], np.float32), color=np.zeros(3, np.float32)),
                     MaterialData(color=np.array([0.3, 0.6, 0.4], np.float32))]
    unit = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)
    light = (unit * 1.2 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
    floor = (unit * 3.0 + np.array([0.0, 0.0, -2.5])).astype(np.float32)
    tri = np.array([[-3, -3, -1], [0.5, -2.5, -0.5], [-2, 1, 0]], np.float32)
    sc.shapes += [ShapeData(positions=light, triangles=QUAD_TRIS),
                  ShapeData(positions=tri, triangles=np.array([[0, 1, 2]], np.int32)),
                  ShapeData(positions=floor, triangles=QUAD_TRIS),
                  ShapeData(positions=_box(rng, 0.9, np.array([1.5, 0.5, -1.0])), triangles=BOX_TRIS)]
    for shape, material in ((0, 1), (1, 0), (2, 0), (3, 2)):
        sc.instances.append(InstanceData(frame=IDENTITY, shape=shape, material=material))
    if tie:  # the floor once more, coincident, with another material
        sc.instances.append(InstanceData(frame=IDENTITY, shape=2, material=2))
    return sc


BUILD = {"one": one_scene, "four": lambda: four_scene(False), "tie": lambda: four_scene(True)}
_scenes = {}


def scene_abi(abi, name):
    if name not in _scenes:
        _scenes[name] = abi.SceneABI(BUILD[name]())
    return _scenes[name]


def tlas_leaf_sizes(bvh):
    t = bvh.struct.tlas
    nodes = np.ctypeslib.as_array(C.cast(t.nodes, C.POINTER(C.c_uint8)), shape=(t.nnodes * 32,)).view(NODE)
    return sorted(int(n["num"]) for n in nodes if not n["internal"])


def blas_leaf_sizes(bvh, shape):
    t = bvh.struct.blas[shape]
    nodes = np.ctypeslib.as_array(C.cast(t.nodes, C.POINTER(C.c_uint8)), shape=(t.nnodes * 32,)).view(NODE)
    return sorted(int(n["num"]) for n in nodes if not n["internal"])


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
        out[mode] = (st.get_image(), st.get_aovs()[2], st.counters(), st.describe())
        k = st.streams
        st.close()
    o = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, W, H, 0, SPP, streams=k)
    return out, o, bvh


def _check(out, o, label, lds_mask):
    lds, hbm, ring = out["lds"], out["hbm"], out["ring"]
    # the baking kernel, the HBM-mode kernel and the LDS ring-overflow kernel (both unbaked)
    assert f"kernel=trace_kernel_lds<1,16,false,1,{lds_mask},false> mode=lds " in lds[3], lds[3]
    assert "kernel=trace_kernel<1,16,false,1," in hbm[3] and " mode=hbm " in hbm[3], hbm[3]
    assert "kernel=trace_kernel_lds<1,16,true,1,255,false> mode=lds " in ring[3] and "ring_used=2" in ring[3], ring[3]
    for mode, g in out.items():
        print(label, mode, {key: g[2][key] for key in COUNTERS}, "oracle", {key: o[4][key] for key in COUNTERS})
    assert lds[0][..., :3].mean() > 0 and lds[1].sum() > 0, (label, "the scene must be hit and lit")
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


@pytest.mark.parametrize("order", ["reference", "near"])
def test_one_instance_root_leaf(gpu, abi, lib, oracle, options, order):
    out, o, bvh = _run(abi, lib, oracle, options, "one", order)
    assert tlas_leaf_sizes(bvh) == [1], "the TLAS root must be a leaf of one instance"
    assert len(blas_leaf_sizes(bvh, 0)) > 1
    assert "light_inline=0" in out["lds"][3], out["lds"][3]
    _check(out, o, f"one/{order}", 0)


@pytest.mark.parametrize("order", ["reference", "near"])
def test_four_instance_leaf_and_one_triangle_blas(gpu, abi, lib, oracle, options, order):
    out, o, bvh = _run(abi, lib, oracle, options, "four", order)
    assert tlas_leaf_sizes(bvh) == [4], "the TLAS root must be a leaf of four instances"
    assert blas_leaf_sizes(bvh, 1) == [1], "shape 1 must be one leaf of one triangle"
    assert "light_inline=1" in out["lds"][3], out["lds"][3]
    _check(out, o, f"four/{order}", 8192)


def test_tie_rerun_through_the_baked_step(gpu, abi, lib, oracle, options):
    """Two coincident quads in the near-first order: the re-run in the reference's order must give
    what the reference order gives, so its counted work exceeds a plain near-first query's."""
    out, o, bvh = _run(abi, lib, oracle, options, "tie", "near")
    assert 4 in tlas_leaf_sizes(bvh)
    _check(out, o, "tie/near", 8192)
