"""The inline light chain (jtk::light_chain, csrc/jt_integrator.h) against the oracle.

A bounce's light chains run inside the shading phase: per instance light a loop of
intersect_instance_bvh queries that a lane leaves at its first miss, the chain's end
(light_chain_end) once for the wave after that loop, and the next scene query started from the
1/d the chain left in the query state (query_restart) when every lane of the wave comes from a
chain. These scenes are the smallest that take each way through that code:

  two_lights  two emissive quads among matte ones: light_advance starts a second chain (the loop
              over lights); the FT_NONE|FT_LINL kernel, the flagship's
  double_hit  one emissive shape of two parallel quads a short distance apart (one BLAS leaf): a
              direction towards it crosses both, so lanes leave the query loop at different
              iterations
  mixed       two_lights with a reflective (delta) and a glossy quad: some lanes of a wave come
              from a chain and others do not (the FT_ALL kernel)
  xform       two_lights with each light under a rotated frame of its own (FT_XFORM): the last
              chain query before a scene query leaves instance-space 1/d and mask in the query
              state, which must not reach that scene query
  strip       test_gpu_node_push.py's strip under a constant environment: no instance light, no
              chain, so no restart
  box_light   a 12-triangle emissive box: its BLAS is not one leaf, so the chains run through
              light_hit in the traversal loop

The path sampler in the reference, the near-first and the wide order, LDS mode (the fixed-stack
kernels: inst_leaf_query chains in the binary orders) and lds_scene=0 (the chains through
query_start + node_step; in the wide order both modes go through node_step_wide, whose instance
entry a transformed light drives in xform), at 48x48 x 4 spp with batch 4. The bar is tests/test_gpu_node_push.py's: >= 99.9 % of pixels bit-identical
and within 1e-3, image mean within 1e-4, hit counts equal; nodes, instances, prims, rays and
light_queries equal the oracle's exactly, in the wide order too: the commit before the wide cases
were added met them exactly (xform: rays 16474, light_queries 27441, nodes 137329 in both modes),
so they hold the exact bar and not test_order_parity's 1e-3 * oracle + 8.
"""
import numpy as np
import pytest

from conftest import compare_images, make_params
from jtrace.scene import CameraData, EnvironmentData, InstanceData, MaterialData, SceneData, ShapeData, TextureData

ORDERS = ("reference", "near", "wide")
W = H = 48
SPP = 4
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
# scene -> (kernel feature mask, light_inline as describe() prints it). strip has no instance
# light, so "every instance light's BLAS is one leaf" holds vacuously and the library reports 1;
# that no chain runs there shows in its light_queries, 0 on the oracle and on the GPU.
EXPECT = {"two_lights": (8192, 1), "double_hit": (8192, 1), "mixed": (255, 1), "xform": (255, 1),
          "strip": (255, 1), "box_light": (0, 0)}


def _identity():
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _camera(sc):
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], np.float32),
                                 aspect=np.float32(1.0)))


def _quad(centre, ex, ey):
    c, ex, ey = (np.asarray(v, np.float64) for v in (centre, ex, ey))
    return np.array([c - ex - ey, c + ex - ey, c + ex + ey, c - ex + ey])


def _add(sc, positions, triangles, material, frame=None):
    sc.shapes.append(ShapeData(positions=np.asarray(positions, np.float32), triangles=np.asarray(triangles, np.int32)))
    sc.instances.append(InstanceData(frame=_identity() if frame is None else frame, shape=len(sc.shapes) - 1,
                                     material=material))


def _box(centre, half, rot):
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    tris = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return (corners * half) @ rot.T + np.asarray(centre, np.float64), tris


def light_scene(kind):
    """A floor, a back wall and three tilted quads under the scene's light(s). Materials: 0 matte,
    1 and 2 emissive, 3 and 4 two of the quads' (matte; in `mixed` reflective, the floor too, and
    glossy)."""
    rng = np.random.default_rng(77)
    sc = SceneData()
    _camera(sc)
    mixed = kind == "mixed"
    sc.materials += [
        MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)),
        MaterialData(emission=np.array([8, 7, 6], np.float32), color=np.zeros(3, np.float32)),
        MaterialData(emission=np.array([3, 5, 9], np.float32), color=np.zeros(3, np.float32)),
        MaterialData(type="reflective", color=np.array([0.9, 0.9, 0.9], np.float32)) if mixed
        else MaterialData(color=np.array([0.3, 0.6, 0.4], np.float32)),
        MaterialData(type="glossy", color=np.array([0.4, 0.5, 0.8], np.float32), roughness=np.float32(0.3)) if mixed
        else MaterialData(color=np.array([0.5, 0.4, 0.7], np.float32)),
    ]
    # the lights first: light k is instance k
    if kind == "double_hit":
        low, high = _quad([0, 2.6, -1], [1.6, 0, 0], [0, 0, 1.6]), _quad([0, 2.9, -1], [1.6, 0, 0], [0, 0, 1.6])
        _add(sc, np.concatenate([low, high]), np.concatenate([QUAD_TRIS, QUAD_TRIS + 4]), 1)
    elif kind == "box_light":
        _add(sc, *_box([0, 2.6, -1], 0.8, _rotation(rng)), 1)
    else:
        lights = ((_quad([-1.6, 2.6, -0.5], [1.0, 0.2, 0], [0, 0, 1.0]), 1),
                  (_quad([1.8, 2.2, -1.5], [0.8, 0, 0], [0, 0.3, 0.8]), 2))
        for world, material in lights:
            if kind == "xform":
                # the same world quad, stored in the space of a rotated and moved frame of its own.
                # Both lights, so that the last query of a bounce's chains, whichever light it asks,
                # leaves instance-space values in the query state
                rot, origin = _rotation(rng), world.mean(axis=0)
                frame = np.concatenate([rot.T.reshape(-1), origin]).astype(np.float32)  # the axes are rot's columns
                _add(sc, (world - origin) @ rot, QUAD_TRIS, material, frame)
            else:
                _add(sc, world, QUAD_TRIS, material)
    _add(sc, _quad([0, -3, -1], [4.5, 0, 0], [0, 0, 4.5]), QUAD_TRIS, 3 if mixed else 0)  # floor (a mirror in `mixed`)
    _add(sc, _quad([0, 0, -4.5], [4.5, 0, 0], [0, 4.0, 0]), QUAD_TRIS, 0)  # back wall
    _add(sc, _quad([-2.2, -1.2, 0.3], [1.2, 0.5, 0], [0, 0.4, 1.2]), QUAD_TRIS, 3)
    _add(sc, _quad([2.0, -1.5, 0.0], [1.1, -0.4, 0.2], [0.1, 0.5, 1.1]), QUAD_TRIS, 4)
    _add(sc, _quad([0.2, -0.4, -2.0], [1.3, 0, 0.3], [0, 1.0, 0]), QUAD_TRIS, 0)
    return sc


def strip_scene():
    """tests/test_gpu_node_push.py's strip: one instance of a folded 64-triangle strip under a
    constant environment, the scene's only light."""
    sc = SceneData()
    _camera(sc)
    sc.materials.append(MaterialData(color=np.array([0.6, 0.6, 0.6], np.float32)))
    sc.textures.append(TextureData(width=2, height=2, linear=True, pixelsf=np.ones((2, 2, 4), np.float32)))
    sc.environments.append(EnvironmentData(frame=_identity(), emission=np.array([1.0, 0.9, 0.8], np.float32),
                                           emission_tex=0))
    x = np.linspace(-4, 4, 33)
    pos = np.array([[xi, y, 1.2 * abs(xi) - 3] for xi in x for y in (-1.5, 1.5)], np.float32)
    tris = np.array([t for i in range(32) for t in ([2 * i, 2 * i + 2, 2 * i + 3], [2 * i, 2 * i + 3, 2 * i + 1])], np.int32)
    sc.shapes.append(ShapeData(positions=pos, triangles=tris))
    sc.instances.append(InstanceData(frame=_identity(), shape=0, material=0))
    return sc


_scenes, _oracle = {}, {}


def scene_abi(abi, name):
    if name not in _scenes:
        _scenes[name] = abi.SceneABI(strip_scene() if name == "strip" else light_scene(name))
    return _scenes[name]


def oracle_trace(oracle, sa, name, params, order, k):
    """The oracle's render of a scene, computed once per (scene, order, streams) and shared by the
    scene modes."""
    key = (name, order, k)
    if key not in _oracle:
        _oracle[key] = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, W, H, 0, SPP, streams=k)
    return _oracle[key]


def _both(abi, lib, oracle, name, order, options, lds):
    from jtrace import trace
    sa = scene_abi(abi, name)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=1, traversal=order)
    if lds is not None:
        options("lds_scene", lds)
    bvh = trace.make_scene_bvh(sa, False, lib)
    lights = trace.make_trace_lights(sa, lib)
    st = trace.make_trace_state(sa, bvh, lights, params, lib)
    st.trace_range(0, SPP)
    g = (st.get_image(), *st.get_aovs(), st.counters())
    k, desc = st.streams, st.describe()
    st.close()
    return g, oracle_trace(oracle, sa, name, params, order, k), k, desc


def _check(g, o, label):
    stats = compare_images(g[0], o[0])
    print(label, stats, "gpu", g[4], "oracle", o[4])
    assert g[0].shape[:2] == (H, W)
    assert g[3].sum() > 0 and g[0][..., :3].mean() > 0, (label, "the scene must be hit and lit")
    assert stats["frac_pix_rel_le_1e-3"] >= 0.999, (label, stats)
    assert stats["bitwise_frac"] >= 0.999, (label, stats)
    assert stats["image_mean_rel"] <= 1e-4, (label, stats)
    assert np.array_equal(g[3], o[3]), label  # hit counts
    for key in ("nodes", "instances", "prims", "rays", "light_queries"):
        assert g[4][key] == o[4][key], (label, key, g[4][key], o[4][key])
    for key in ("paths", "shades"):
        assert abs(g[4][key] - o[4][key]) <= 1e-3 * o[4][key] + 8, (label, key, g[4][key], o[4][key])
    for a, b in ((g[1], o[1]), (g[2], o[2])):
        assert compare_images(a, b)["frac_pix_rel_le_1e-3"] >= 0.999, label


def _cpu_counters(abi, oracle, name, order="near"):
    sa = scene_abi(abi, name)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=1, traversal=order)
    return oracle_trace(oracle, sa, name, params, order, 1)[4]


def test_scene_preconditions_on_the_oracle(abi, oracle):
    """What each scene is for, stated on the oracle's counters (CPU only). A scene that does not
    meet its line gets another geometry, not another threshold."""
    c = {name: _cpu_counters(abi, oracle, name) for name in EXPECT}
    print(c)
    # two lights: every non-delta shade asks each light at least once
    assert c["two_lights"]["light_queries"] >= 2 * c["two_lights"]["shades"] * 0.99
    # the double quad: chains of two and more hits are common
    assert c["double_hit"]["light_queries"] >= 1.5 * c["double_hit"]["shades"]
    # delta lanes: the mixed scene asks fewer queries per shade than its all-matte twin's two
    assert 0 < c["mixed"]["light_queries"] < 2 * c["mixed"]["shades"] * 0.99
    assert c["xform"]["light_queries"] >= 2 * c["xform"]["shades"] * 0.99
    assert c["strip"]["light_queries"] == 0 and c["strip"]["shades"] > 0
    assert c["box_light"]["light_queries"] >= c["box_light"]["shades"] * 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["lds", "hbm"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(EXPECT))
def test_light_chains_match_the_oracle(gpu, abi, lib, oracle, options, name, order, mode):
    g, o, k, desc = _both(abi, lib, oracle, name, order, options, "0" if mode == "hbm" else None)
    mask, inline = EXPECT[name]
    kernel = "trace_kernel_lds" if mode == "lds" else "trace_kernel"
    wide = "true" if order == "wide" else "false"
    assert f"kernel={kernel}<1,16,false,1,{mask},{wide}> mode={mode} " in desc, desc
    assert f"traversal={order}" in desc, desc
    assert f"light_inline={inline}" in desc, desc
    _check(g, o, f"{name}/{mode}/{order}/k{k}")
    if name == "double_hit":
        assert o[4]["light_queries"] >= 1.5 * o[4]["shades"], o[4]
    if name == "strip":
        assert g[4]["light_queries"] == 0, g[4]
