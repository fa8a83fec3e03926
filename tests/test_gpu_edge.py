"""Edge cases of the HIP path against the oracle on the same seeded inputs (round 6).

- Ragged and tiny framings (`--width/--height` not multiples of the 8x8 tiles, down to one
  pixel), at one sample stream (the reference's `--batch 1`) and at k > 1 streams: the partial
  edge tiles, the stream-slot arithmetic and the persistent grid with fewer units than waves.
- A random instanced scene no shipped scene resembles: rotated and scaled instance frames (the
  instance-space ray transform of `intersect_instance_bvh`, src/bvh.jl:493-520), quads, degenerate
  triangles, glossy and matte materials and emissive instances as lights, in both scene modes (LDS
  and HBM) and every traversal order, both samplers.

The bar is §8(c)'s (tests/test_gpu_parity.py): >= 99.9 % of pixels bit-identical and within 1e-3,
image mean within 1e-4, hits equal, traversal counters within 0.1 %.
"""
import numpy as np
import pytest

from conftest import compare_images, make_params
from scenes_ref import random_instanced_scene  # moved there unchanged: the ray-query tests build it too

pytestmark = pytest.mark.gpu

ORDERS = {"reference": 0, "near": 1, "wide": 2}


def _both(abi, lib, oracle, sa, params, s0, s1, options=None, lds=None):
    from jtrace import trace
    if options is not None and lds is not None:
        options("lds_scene", lds)
    bvh = trace.make_scene_bvh(sa, False, lib)
    lights = trace.make_trace_lights(sa, lib)
    st = trace.make_trace_state(sa, bvh, lights, params, lib)
    st.trace_range(s0, s1)
    g = (st.get_image(), *st.get_aovs(), st.counters())
    k, desc = st.streams, st.describe()
    st.close()
    o = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, g[0].shape[1], g[0].shape[0],
                     s0, s1, streams=k)
    return g, o, k, desc


def _check(g, o, label):
    stats = compare_images(g[0], o[0])
    print(label, stats, "gpu", g[4], "oracle", o[4])
    assert stats["frac_pix_rel_le_1e-3"] >= 0.999, (label, stats)
    assert stats["bitwise_frac"] >= 0.999, (label, stats)
    assert stats["image_mean_rel"] <= 1e-4, (label, stats)
    assert np.array_equal(g[3], o[3]), label  # hit counts
    for key in ("rays", "light_queries", "nodes", "instances", "prims", "shades"):
        assert abs(g[4][key] - o[4][key]) <= 1e-3 * o[4][key] + 8, (label, key, g[4][key], o[4][key])
    for a, b in ((g[1], o[1]), (g[2], o[2])):
        assert compare_images(a, b)["frac_pix_rel_le_1e-3"] >= 0.999, label


@pytest.mark.parametrize("batch", [1, 7])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 13), (13, 1), (9, 7), (17, 33), (65, 3)])
def test_ragged_framings_match_the_oracle(gpu, abi, lib, oracle, cornell_abi, w, h, batch):
    """Framings smaller than a tile or one pixel past a tile boundary: every pixel is traced once
    (paths = W*H*spp), edge tiles skip their outside pixels, and the bits equal the oracle's."""
    params = make_params(abi, width=w, height=h, samples=7, batch=batch)
    g, o, k, desc = _both(abi, lib, oracle, cornell_abi, params, 0, 7)
    assert g[0].shape[:2] == (h, w), g[0].shape
    assert k == (1 if batch == 1 else 4), desc  # k <= the batch (stream_log2)
    assert g[4]["paths"] == o[4]["paths"] == w * h * 7
    _check(g, o, f"{w}x{h}/batch{batch}/k{k}")
    # the bits do not depend on how the range is split into calls
    from jtrace import trace
    st = trace.make_trace_state(cornell_abi, trace.make_scene_bvh(cornell_abi, False, lib),
                                trace.make_trace_lights(cornell_abi, lib), params, lib)
    for a, b in ((0, 2), (2, 3), (3, 7)):
        st.trace_range(a, b)
    assert np.array_equal(st.get_image(), g[0])
    st.close()


@pytest.mark.parametrize("share", [None, "4,3"])
def test_one_stream_chunk_on_partial_edge_tiles(gpu, abi, lib, cornell_abi, options, share):
    """chain_kernel (csrc/jt_accum.hip) on partial edge tiles under a tile share: 44x36 (6x5 tiles,
    the last column and row 4 pixels wide), one stream, 5 samples of the path sampler. A context
    that reads the image after every sample flushes each time (one launch per sample, no chain);
    one that queues all 5 and reads once runs them as one chunk folded by chain_kernel. Image,
    albedo, normal and hits are equal bit for bit, and under the share "4,3" every pixel outside
    tiles 3, 7, ..., 27 is zero."""
    from jtrace import trace
    options("tile_share", share)
    params = make_params(abi, width=44, height=36, samples=5, batch=1, sampler=1)
    bvh = trace.make_scene_bvh(cornell_abi, False, lib)
    lights = trace.make_trace_lights(cornell_abi, lib)
    outs = []
    for per_sample in (True, False):
        st = trace.make_trace_state(cornell_abi, bvh, lights, params, lib)
        assert st.streams == 1, st.describe()
        for _ in range(5):
            st.trace_samples()
            if per_sample:
                st.get_image()
        assert st.samples == 5
        outs.append((st.get_image(), *st.get_aovs(), st.counters()["launches"]))
        st.close()
    exp, got = outs
    assert exp[4] == 5 and got[4] == 1, (exp[4], got[4])  # per-sample launches against one chunk
    for a, b, name in zip(exp[:4], got[:4], ("image", "albedo", "normal", "hits")):
        assert np.array_equal(a, b), name
    assert got[3].sum() > 0 and got[0][..., :3].max() > 0, "the share's tiles must be hit and lit"
    if share:
        ty, tx = np.divmod(np.arange(30), 6)
        mask = np.zeros((36, 44), bool)
        for t in range(3, 30, 4):
            mask[ty[t] * 8:ty[t] * 8 + 8, tx[t] * 8:tx[t] * 8 + 8] = True
        for a, name in zip(got[:4], ("image", "albedo", "normal", "hits")):
            assert np.all(a[~mask] == 0), name
        assert np.any(got[0][mask] != 0)


@pytest.fixture(scope="module")
def random_abi(abi):
    return abi.SceneABI(random_instanced_scene())


@pytest.mark.parametrize("sampler", [1, 2])
@pytest.mark.parametrize("order", ["near", "wide", "reference"])
@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_random_instanced_scene_matches_the_oracle(gpu, abi, lib, oracle, options, random_abi, mode, order, sampler):
    params = make_params(abi, resolution=80, samples=6, batch=6, sampler=sampler, traversal=order)
    g, o, k, desc = _both(abi, lib, oracle, random_abi, params, 0, 6, options=options,
                          lds="0" if mode == "hbm" else None)
    assert (f"mode={mode}" in desc) and (f"traversal={order}" in desc), desc
    assert g[3].sum() > 0 and g[0][..., :3].mean() > 0, "the scene must be hit and lit"
    _check(g, o, f"random/{mode}/{order}/{sampler}/k{k}")
