"""What tests/test_irradiance_host.py (CPU) and tests/test_gpu_irradiance.py share: the oracle's
direction of a hemisphere sample, and the scene whose cosine-weighted gather is known in closed form.

A gather's direction (include/jtrace.h, jt_irradiance) is sample_hemisphere_cos(normal, ruv) with ruv
the first two draws of the stream (seed, stream_base + i, sample). The oracle has both halves:
or_rng_first gives the draws, and slots 13..15 of a row of its "parts" probe are
sample_hemisphere_cos of the normal in x[6:9] and the pair in x[16:18], the bar tests/
test_gpu_primitives.py already holds the device function to.

The square scene: a constant environment of radiance L (a constant float texture, so the
environment is a sampled light as in any scene), one black matte square of half-width 1 at height 1
above the origin, facing down, nothing else. From the point (origin, +y) a gather ray either meets
the square, where a path ends with radiance 0, or escapes to L. The share of the cosine-weighted
hemisphere the square fills is the form factor of a differential area to a parallel square above its
centre, four corner rectangles of a = b = 1 at h = 1: F = 4 / (pi sqrt 2) atan(1 / sqrt 2)."""
import ctypes as C

import numpy as np

F32 = np.float32

SQUARE_L = np.array([2.0, 1.0, 0.5], F32)
SQUARE_F = 4.0 / (np.pi * np.sqrt(2.0)) * np.arctan(1.0 / np.sqrt(2.0))
SQUARE_POINTS, SQUARE_SAMPLES = 64, 1024
# the standard error of the hit share over all 65536 samples, each 0 or 1
SQUARE_SE = float(np.sqrt(SQUARE_F * (1.0 - SQUARE_F) / (SQUARE_POINTS * SQUARE_SAMPLES)))
SQUARE_SEED = 0x5EED  # inside both bounds: test_irradiance_host.py counts its hits on the CPU


def first_pairs(oracle, seed, streams, sample):
    """The first two draws of (seed, stream, sample) for every stream: (n, 2) float32."""
    out = np.empty((len(streams), 2), F32)
    one = np.empty(2, F32)
    p = one.ctypes.data_as(C.POINTER(C.c_float))
    for k, stream in enumerate(streams):
        oracle.lib.or_rng_first(seed, int(stream), int(sample), 2, p)
        out[k] = one
    return out


def oracle_directions(oracle, seed, normals, sample, stream_base=0):
    """sample_hemisphere_cos(normals[i], the first pair of stream stream_base + i) by the oracle: (n, 3) float32."""
    normals = np.asarray(normals, F32)
    n = len(normals)
    x = np.zeros((n, 18), F32)
    x[:, 1:4], x[:, 4], x[:, 5] = 0.5, 1.5, 0.5  # a material the other slots of the probe can digest
    x[:, 6:9] = normals
    x[:, 9:12] = x[:, 12:15] = normals
    x[:, 16:18] = first_pairs(oracle, seed, np.arange(n) + stream_base, sample)
    return oracle.probe("parts", x)[:, 13:16]


def square_scene():
    from jtrace.scene import CameraData, EnvironmentData, InstanceData, MaterialData, SceneData, ShapeData, TextureData, identity_frame
    sc = SceneData()
    sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 12], F32), aspect=F32(1.0)))
    sc.materials.append(MaterialData(color=np.zeros(3, F32)))  # matte, black, no emission
    sc.textures.append(TextureData(width=4, height=2, linear=True, pixelsf=np.ones((2, 4, 4), F32)))
    sc.environments.append(EnvironmentData(frame=identity_frame(), emission=SQUARE_L.copy(), emission_tex=0))
    # (p1, p2, p4) turns so that the element normal is -y: the square faces down
    pos = np.array([[-1, 1, -1], [1, 1, -1], [1, 1, 1], [-1, 1, 1]], F32)
    sc.shapes.append(ShapeData(positions=pos, quads=np.array([[0, 1, 2, 3]], np.int32)))
    sc.instances.append(InstanceData(frame=identity_frame(), shape=0, material=0))
    return sc


def square_points():
    """64 copies of (origin, +y): 64 streams."""
    return np.tile(np.array([0, 0, 0, 0, 1, 0], F32), (SQUARE_POINTS, 1))


def square_hits(oracle, seed):
    """How many of the 64 x 1024 gather directions meet the square, by a float64 ray-square test on
    the oracle's directions: the ray from the origin crosses y = 1 at d / d.y."""
    hits = 0
    normals = square_points()[:, 3:]
    for s in range(SQUARE_SAMPLES):
        d = oracle_directions(oracle, seed, normals, s).astype(np.float64)
        up = d[:, 1] > 0
        y = np.where(up, d[:, 1], 1.0)
        hits += int((up & (np.abs(d[:, 0] / y) <= 1) & (np.abs(d[:, 2] / y) <= 1)).sum())
    return hits
