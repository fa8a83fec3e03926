"""Synthetic scenes shared by several test files: the builders of tests/test_gpu_edge.py,
tests/test_gpu_node_push.py and tests/test_gpu_variants.py, moved here unchanged so that the ray-query
tests (tests/queries_ref.py) build the same scenes, and the three scenes those tests add.
"""
import copy

import numpy as np

from jtrace.scene import CameraData, EnvironmentData, InstanceData, MaterialData, SceneData, ShapeData, TextureData

# seeds of quad_scene's instance positions, searched on the CPU with the oracle's BVH build so that
# TLAS leaves of 1, 2, 3 and 4 instances all occur across the set (tests/test_gpu_node_push.py asserts it)
SEEDS = {1: 1, 2: 1, 3: 1, 5: 4, 7: 1, 9: 4}


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _identity():
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def _camera(sc):
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], np.float32),
                                 aspect=np.float32(1.0)))


def random_instanced_scene(seed=7):
    """Random geometry in front of the camera: three shapes (triangles, quads with degenerate
    ones, a sliver-heavy triangle soup), six instances with rotated and non-uniformly scaled
    frames, two of them emissive (the lights), matte and glossy materials."""
    rng = np.random.default_rng(seed)
    sc = SceneData()
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], np.float32)
    sc.cameras.append(CameraData(frame=cam, aspect=np.float32(1.0)))
    sc.materials += [
        MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)),
        MaterialData(type="glossy", color=np.array([0.4, 0.5, 0.8], np.float32), roughness=np.float32(0.3)),
        MaterialData(emission=np.array([6, 5, 4], np.float32), color=np.zeros(3, np.float32)),
    ]
    # shape 0: a triangle soup around the origin. The scene is small enough for the LDS blob
    # (jt_create takes LDS mode only if it keeps 4 workgroups per CU: about 6 KiB of scene here)
    n = 10
    c = rng.normal(size=(n, 1, 3)) * 1.5
    pos = (c + rng.normal(size=(n, 3, 3)) * 0.4).reshape(-1, 3).astype(np.float32)
    sc.shapes.append(ShapeData(positions=pos, triangles=np.arange(3 * n, dtype=np.int32).reshape(n, 3)))
    # shape 1: quads, every third a triangle stored as a degenerate quad (p3 == p4)
    n = 5
    c = rng.normal(size=(n, 1, 3))
    pos = (c + rng.normal(size=(n, 4, 3)) * 0.5).reshape(-1, 3).astype(np.float32)
    idx = np.arange(4 * n, dtype=np.int32).reshape(n, 4)
    idx[::3, 3] = idx[::3, 2]
    sc.shapes.append(ShapeData(positions=pos, quads=idx))
    # shape 2: a small two-triangle emitter (one BVH leaf: light chains inline)
    pos = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float32)
    sc.shapes.append(ShapeData(positions=pos, triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
    for i in range(6):
        shape = 2 if i in (2, 5) else i % 2
        m = _rotation(rng) * rng.uniform(1.0, 3.0, size=3)  # rotated, non-uniformly scaled axes
        o = rng.uniform(-4, 4, size=3)
        o[2] = rng.uniform(-6, 2)
        frame = np.concatenate([m.reshape(-1), o]).astype(np.float32)
        sc.instances.append(InstanceData(frame=frame, shape=shape, material=2 if shape == 2 else i % 2))
    return sc


def quad_scene(n, glossy, seed):
    """n two-triangle quads and one 12-triangle box in front of the camera, each its own shape in
    world coordinates under an identity frame; quad 0 is the light."""
    rng = np.random.default_rng(1000 * n + seed)
    sc = SceneData()
    _camera(sc)
    sc.materials += [
        MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)),
        MaterialData(emission=np.array([8, 7, 6], np.float32), color=np.zeros(3, np.float32)),
        MaterialData(type="glossy", color=np.array([0.4, 0.5, 0.8], np.float32), roughness=np.float32(0.3))
        if glossy else MaterialData(color=np.array([0.3, 0.6, 0.4], np.float32)),
    ]
    unit = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)
    for k in range(n):
        centre = np.array([0.0, 0.0, 2.5]) if k == 0 else rng.uniform([-3.5, -3.5, -4], [3.5, 3.5, 1])
        pos = (unit * rng.uniform(0.8, 1.6)) @ _rotation(rng).T + centre
        sc.shapes.append(ShapeData(positions=pos.astype(np.float32), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
        sc.instances.append(InstanceData(frame=_identity(), shape=k, material=1 if k == 0 else 0))
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    tris = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    pos = (corners * 0.9) @ _rotation(rng).T + rng.uniform([-2, -2, -2], [2, 2, 0])
    sc.shapes.append(ShapeData(positions=pos.astype(np.float32), triangles=tris))
    sc.instances.append(InstanceData(frame=_identity(), shape=n, material=2))
    return sc


def strip_scene():
    """One instance of a 64-triangle strip along x, folded at x = 0 so its wings see each other,
    under a constant environment (the scene's only light: an emissive strip's light records would
    push the scene out of LDS mode)."""
    sc = SceneData()
    _camera(sc)
    sc.materials.append(MaterialData(color=np.array([0.6, 0.6, 0.6], np.float32)))
    sc.textures.append(TextureData(width=2, height=2, linear=True, pixelsf=np.ones((2, 2, 4), np.float32)))
    sc.environments.append(EnvironmentData(frame=_identity(), emission=np.array([1.0, 0.9, 0.8], np.float32),
                                           emission_tex=0))
    x = np.linspace(-4, 4, 33)
    pos = np.array([[xi, y, 1.2 * abs(xi) - 3] for xi in x for y in (-1.5, 1.5)], np.float32)
    tris = np.array([t for i in range(32) for t in ([2 * i, 2 * i + 2, 2 * i + 3], [2 * i, 2 * i + 3, 2 * i + 1])], np.int32)
    assert len(tris) == 64
    sc.shapes.append(ShapeData(positions=pos, triangles=tris))
    sc.instances.append(InstanceData(frame=_identity(), shape=0, material=0))
    return sc


def coplanar_tie_scene(cornell):
    """Every cornellbox instance gets a coplanar twin (the same shape and frame) with a differently
    coloured material of opacity 0.6, and every shape repeats its own triangles, so almost every
    hit is a tie — between two instances (TLAS leaves) and between two triangles of one BLAS leaf."""
    sc = copy.deepcopy(cornell)
    rng = np.random.default_rng(11)
    for s in sc.shapes:
        s.triangles = np.concatenate([s.triangles, s.triangles[::-1]]).astype(np.int32)
    base_m = len(sc.materials)
    for m in list(sc.materials):
        sc.materials.append(MaterialData(type=m.type, emission=m.emission.copy(),
                                         color=rng.uniform(0.1, 0.9, 3).astype(np.float32), opacity=np.float32(0.6)))
    twins = [InstanceData(frame=i.frame.copy(), shape=i.shape, material=base_m + i.material, name=i.name + "_twin")
             for i in sc.instances]
    sc.instances = [x for pair in zip(sc.instances, twins) for x in pair]
    return sc


# ------------------------------------------------------------------------------ the ray-query tests' own
def twin_scene(seed=3):
    """The same shapes twice under the same frame (a rotated, non-uniformly scaled one and an
    identity one): every hit of a scene query is an exact tie between two instances, which the
    reference resolves by its TLAS order."""
    rng = np.random.default_rng(seed)
    sc = SceneData()
    _camera(sc)
    sc.materials.append(MaterialData(color=np.array([0.7, 0.6, 0.5], np.float32)))
    n = 24
    c = rng.normal(size=(n, 1, 3)) * 1.2
    pos = (c + rng.normal(size=(n, 3, 3)) * 0.5).reshape(-1, 3).astype(np.float32)
    sc.shapes.append(ShapeData(positions=pos, triangles=np.arange(3 * n, dtype=np.int32).reshape(n, 3)))
    n = 7
    c = rng.normal(size=(n, 1, 3))
    pos = (c + rng.normal(size=(n, 4, 3)) * 0.6).reshape(-1, 3).astype(np.float32)
    sc.shapes.append(ShapeData(positions=pos, quads=np.arange(4 * n, dtype=np.int32).reshape(n, 4)))
    m = _rotation(rng) * rng.uniform(0.7, 2.0, size=3)
    frames = [np.concatenate([m.reshape(-1), [0.5, -0.3, -1.0]]).astype(np.float32), _identity()]
    for shape, frame in ((0, frames[0]), (1, frames[1]), (0, frames[0]), (1, frames[1])):
        sc.instances.append(InstanceData(frame=frame.copy(), shape=shape, material=0))
    return sc


def deep_scene(seed=1, n=2000):
    """One shape of n small triangles whose centres follow a power law along a line, so the
    middle-split BVH is deep: the laid-out stack bound is above 16 (tests/test_queries_host.py
    asserts it), and the overflow forms spill without a shortened ring. Two instances, one rotated."""
    rng = np.random.default_rng(seed)
    sc = SceneData()
    _camera(sc)
    sc.materials.append(MaterialData(color=np.array([0.6, 0.6, 0.6], np.float32)))
    t = rng.uniform(0, 1, size=(n, 1)) ** 6  # dense near the origin: every split halves little
    c = t * np.array([[4.0, 3.0, 2.0]]) + rng.normal(size=(n, 3)) * 0.02 * (t + 0.01)
    pos = (c[:, None, :] + rng.normal(size=(n, 3, 3)) * 0.3 * (t[:, None, :] + 0.03)).reshape(-1, 3).astype(np.float32)
    sc.shapes.append(ShapeData(positions=pos, triangles=np.arange(3 * n, dtype=np.int32).reshape(n, 3)))
    sc.instances.append(InstanceData(frame=_identity(), shape=0, material=0))
    m = _rotation(rng) * 0.8
    sc.instances.append(InstanceData(frame=np.concatenate([m.reshape(-1), [-2.0, 1.0, -1.0]]).astype(np.float32),
                                     shape=0, material=0))
    return sc


PLATES = 90


def plates_scene():
    """PLATES parallel two-triangle plates [-1, 1]^2 along z, 0.05 apart, in one shape under an
    identity frame: a ray along the axis crosses them all, and in the reference's far-first order
    it accepts a hit on every one (more than the 63 the device's hit count holds)."""
    sc = SceneData()
    _camera(sc)
    sc.materials.append(MaterialData(color=np.array([0.5, 0.6, 0.7], np.float32)))
    pos, tris = [], []
    for k in range(PLATES):
        z = -2.0 + 0.05 * k
        b = 4 * k
        pos += [[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]]
        tris += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    sc.shapes.append(ShapeData(positions=np.array(pos, np.float32), triangles=np.array(tris, np.int32)))
    sc.instances.append(InstanceData(frame=_identity(), shape=0, material=0))
    return sc
