"""The baked shading of the LDS-mode matte kernels (csrc/jt_kernels.h bake_shading; csrc/jt_bsdf.h
basis_baked, sample_matte_baked, eval_matte_pdf_baked) against the kernels that compute the same
values per bounce, and against the oracle.

The fixed-stack LDS kernels of matte scenes (configurations 0 and 7) read the hemisphere basis of a hit
element's normal and the material's color / pi from their workgroup's LDS copy, where a bake pass wrote
them once; HBM mode (lds_scene=0), the LDS ring-overflow kernel (test_lds_ring) and the general kernel
(features=all) call basis_fromz and divide by pi on every bounce. Each scene runs through all of them
at 32x32 x 4 spp, batch 4, with both samplers; the baking kernel also without counters (the other
COUNT level, the one a render without counters launches). The images, the albedo and normal means, the
hit counts and every counter must be bit-identical, the traversal and light counters equal to the
oracle's, and the image against the oracle within the bars of tests/test_gpu_node_bake.py:
bitwise_frac >= 0.999, frac_pix_rel_le_1e-3 >= 0.999, image_mean_rel <= 1e-4.

Scenes (all matte, identity frames, triangles; three materials of different colours and an emissive one):
  box     a closed axis-aligned box seen from inside, its triangles wound outwards: every hit is on a
          back face, so the baked basis is taken flipped. Its faces have the normals (+-1, 0, 0),
          (0, 0, +-1) — z == 0 exactly, and (0, 0, -1) where sign + z = -2 — and (0, +-1, 0), where
          Y.y of the basis cancels to +0 in both orientations (tests/shade_bake_check.cpp). A quad
          light inside: one leaf, so the chains run inline (configuration 0).
  plane   a floor seen from behind, a triangle whose stored normal n is not a fixed point of
          normalize (the stored Z differs from n in the last bit; picked below on the CPU, and
          asserted), instanced twice with two materials, and a zero-area triangle (its normal is the
          zero vector: baked like any other, never hit).
  steps   the box with a box-shaped light of more than one leaf: the light-hit-steps kernel
          (configuration 7, mask 0), which bakes too.
"""
import numpy as np
import pytest

from conftest import compare_images, make_params
from jtrace.scene import CameraData, InstanceData, MaterialData, SceneData, ShapeData

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 4
F32 = np.float32
MODES = {"lds": None, "hbm": ("lds_scene", "0"), "ring": ("test_lds_ring", "2"), "all": ("features", "all")}
TRAVERSAL = ("nodes", "instances", "prims", "rays", "light_queries")
COUNTERS = ("paths", "shades") + TRAVERSAL

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
# corners (x, y, z) in {-1, 1}^3, index 4 x + 2 y + z; every triangle's normal points out of the box
BOX_TRIS = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
CORNERS = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
UNIT = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)


def _dot(a, b):  # the device's left fold, in float32
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _normalize(a):
    length = np.sqrt(_dot(a, a))
    return (a / length).astype(F32) if length != 0 else a


def element_normal(p):
    """enrm_id of a triangle as the layout computes it (csrc/jt_layout.cpp): normalize(cross(p2 - p1,
    p3 - p1)), then transform_normal by the identity frame, which normalizes once more."""
    a, b = (p[1] - p[0]).astype(F32), (p[2] - p[0]).astype(F32)
    c = np.array([F32(a[1] * b[2]) - F32(a[2] * b[1]), F32(a[2] * b[0]) - F32(a[0] * b[2]),
                  F32(a[0] * b[1]) - F32(a[1] * b[0])], F32)
    n = _normalize(c)
    one, zero = F32(1), F32(0)
    t = np.array([F32(F32(one * n[0] + zero * n[1]) + zero * n[2]), F32(F32(zero * n[0] + one * n[1]) + zero * n[2]),
                  F32(F32(zero * n[0] + zero * n[1]) + one * n[2])], F32)
    return _normalize(t)


def unstable_triangle():
    """A rotated triangle whose stored normal changes in its last bit when normalized again."""
    rng = np.random.default_rng(41)
    for _ in range(1000):
        p = (rng.normal(size=(3, 3)) * 0.9 + np.array([1.3, 0.6, -1.0])).astype(F32)
        n = element_normal(p)
        if not np.array_equal(_normalize(n).view(np.uint32), n.view(np.uint32)):
            return p
    raise AssertionError("no triangle whose normal is not a fixed point of normalize")


def _base(cam_z):
    sc = SceneData()
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, cam_z], F32), aspect=F32(1.0)))
    sc.materials += [MaterialData(color=np.array([0.7, 0.6, 0.5], F32)),
                     MaterialData(emission=np.array([8, 7, 6], F32), color=np.array([0.2, 0.1, 0.3], F32)),
                     MaterialData(color=np.array([0.3, 0.6, 0.4], F32)),
                     MaterialData(color=np.array([0.15, 0.25, 0.8], F32))]
    return sc


def _add(sc, positions, triangles, material):
    sc.shapes.append(ShapeData(positions=np.asarray(positions, F32), triangles=triangles))
    sc.instances.append(InstanceData(frame=IDENTITY, shape=len(sc.shapes) - 1, material=material))


def box_scene(box_light=False):
    sc = _base(2.8)  # the camera is inside the box
    _add(sc, CORNERS * 3.0, BOX_TRIS, 0)
    if box_light:  # more than one leaf: light-hit steps
        _add(sc, CORNERS * 0.5 + np.array([0.4, 0.9, -1.5]), BOX_TRIS, 1)
    else:
        _add(sc, UNIT * 0.9 + np.array([0.3, 1.2, -2.5]), QUAD_TRIS, 1)
    _add(sc, CORNERS * 0.6 + np.array([-1.2, -2.25, -1.0]), BOX_TRIS, 2)  # seen from outside: front faces
    _add(sc, UNIT * 0.7 + np.array([1.5, -1.0, -2.0]), QUAD_TRIS, 3)
    return sc


def plane_scene():
    sc = _base(12.0)
    _add(sc, UNIT * 1.2 + np.array([0, 0, 3.5]), QUAD_TRIS, 1)  # the light, facing the floor
    _add(sc, (UNIT * 3.5 + np.array([0, 0, -2.5]))[::-1], QUAD_TRIS, 0)  # the floor, wound away from the camera
    _add(sc, unstable_triangle(), np.array([[0, 1, 2]], np.int32), 2)
    sc.instances.append(InstanceData(frame=IDENTITY, shape=2, material=3))  # the same shape once more
    _add(sc, np.array([[-1, -1, 0], [0, 0, 0], [1, 1, 0]], F32) + np.array([-1.0, 1.0, -1.0], F32),
         np.array([[0, 1, 2]], np.int32), 3)  # zero area
    return sc


BUILD = {"box": box_scene, "plane": plane_scene, "steps": lambda: box_scene(box_light=True)}
_scenes, _oracle = {}, {}


def scene_abi(abi, name):
    if name not in _scenes:
        _scenes[name] = abi.SceneABI(BUILD[name]())
    return _scenes[name]


def oracle_run(abi, oracle, name, sampler, streams):
    """The oracle's (image, albedo, normal, hits, counters) of a scene, computed once."""
    if (name, sampler, streams) not in _oracle:
        sa = scene_abi(abi, name)
        params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=sampler)
        _oracle[name, sampler, streams] = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, W, H, 0, SPP,
                                                       streams=streams)
    return _oracle[name, sampler, streams]


def _render(abi, lib, sa, bvh, lights, params, counters=True):
    from jtrace import trace
    st = trace.make_trace_state(sa, bvh, lights, params, lib)
    if not counters:
        st.set_counters(0)
    st.trace_range(0, SPP)
    out = (st.get_image(),) + st.get_aovs() + (st.counters(), st.describe(), st.streams)
    st.close()
    return out  # image, albedo, normal, hits, counters, describe, streams


def _run(abi, lib, options, name, sampler):
    from jtrace import trace
    sa = scene_abi(abi, name)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=sampler)
    bvh = trace.make_scene_bvh(sa, False, lib)
    lights = trace.make_trace_lights(sa, lib)
    out = {}
    for mode, opt in MODES.items():
        for key in ("lds_scene", "test_lds_ring", "features"):
            options(key, None)
        if opt:
            options(*opt)
        out[mode] = _render(abi, lib, sa, bvh, lights, params)
        if mode == "lds":
            out["lds0"] = _render(abi, lib, sa, bvh, lights, params, counters=False)
    for key in ("lds_scene", "test_lds_ring", "features"):
        options(key, None)
    return out


def _check(abi, oracle, out, name, sampler, mask):
    lds = out["lds"]
    s = sampler
    # the baking kernel at both counter levels, and the three kernels that compute per bounce
    assert f"kernel=trace_kernel_lds<{s},16,false,1,{mask},false> mode=lds " in lds[5], lds[5]
    assert f"kernel=trace_kernel_lds<{s},16,false,0,{mask},false> mode=lds " in out["lds0"][5], out["lds0"][5]
    assert f"kernel=trace_kernel<{s},16,false,1," in out["hbm"][5] and " mode=hbm " in out["hbm"][5], out["hbm"][5]
    assert f"kernel=trace_kernel_lds<{s},16,true,1,255,false> mode=lds " in out["ring"][5], out["ring"][5]
    assert f"kernel=trace_kernel_lds<{s},16,false,1,255,false> mode=lds " in out["all"][5], out["all"][5]
    o = oracle_run(abi, oracle, name, sampler, lds[6])
    label = f"{name}/sampler{sampler}"
    for mode, g in out.items():
        print(label, mode, {key: g[4][key] for key in COUNTERS}, "oracle", {key: o[4][key] for key in TRAVERSAL})
    assert lds[0][..., :3].mean() > 0 and lds[3].sum() > 0, (label, "the scene must be hit and lit")
    assert lds[4]["shades"] > lds[3].sum() > 0, (label, "paths must go on from their first hit and hit again")
    for mode in ("lds0", "hbm", "ring", "all"):
        g = out[mode]
        assert np.array_equal(lds[0], g[0]), (label, mode, compare_images(lds[0], g[0]))
        for k, what in ((1, "albedo"), (2, "normal"), (3, "hits")):
            assert np.array_equal(lds[k], g[k]), (label, mode, what)
        if mode != "lds0":
            for key in COUNTERS:
                assert g[4][key] == lds[4][key], (label, mode, key, g[4][key], lds[4][key])
    for key in TRAVERSAL:
        assert lds[4][key] == o[4][key], (label, key, lds[4][key], o[4][key])
    stats = compare_images(lds[0], o[0])
    print(label, stats)
    assert stats["frac_pix_rel_le_1e-3"] >= 0.999 and stats["bitwise_frac"] >= 0.999, (label, stats)
    assert stats["image_mean_rel"] <= 1e-4, (label, stats)
    assert np.array_equal(lds[3], o[3]), label  # hit counts
    return lds, o


SAMPLERS = [1, 2]


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_closed_box_from_inside_axis_normals_flipped(gpu, abi, lib, oracle, options, sampler):
    out = _run(abi, lib, options, "box", sampler)
    assert "light_inline=1" in out["lds"][5], out["lds"][5]
    lds, _ = _check(abi, oracle, out, "box", sampler, 8192)
    # the camera is inside: its rays end on a wall or on something in front of one
    assert lds[3].mean() > 0.99 * SPP, "the camera rays must hit the box from inside"


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_back_faced_plane_unstable_normal_shared_shape_zero_area(gpu, abi, lib, oracle, options, sampler):
    p = unstable_triangle()
    n = element_normal(p)
    assert not np.array_equal(_normalize(n).view(np.uint32), n.view(np.uint32)), (p, n)
    out = _run(abi, lib, options, "plane", sampler)
    _check(abi, oracle, out, "plane", sampler, 8192)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_light_hit_steps_kernel_bakes_too(gpu, abi, lib, oracle, options, sampler):
    out = _run(abi, lib, options, "steps", sampler)
    assert "light_inline=0" in out["lds"][5], out["lds"][5]
    _check(abi, oracle, out, "steps", sampler, 0)
