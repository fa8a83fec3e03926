"""The trace kernels' per-lane work item holds its pixel's image coordinates ((j << 16) | i,
csrc/jt_plan.h): the sample start takes the pixel from it, the item's store its launch slot. Rendered
against the oracle at sizes with partial edge tiles in x and in y (13x9, 70x9) and with whole tiles
only (64x64), path and naive samplers, 8 samples, through each way an item's means are started and
stored:

  one      one call: every item starts from zero and stores its stream's record (item_slot)
  two      two calls of 4: the second call's items reload their stream's record (the earlier-launch path)
  batch1   batch=1, one stream (lk = 0): the items read and write the image buffers by pixel index
  share    a tile share (option tile_share) with stride 2: item_slot's quotient by the stride

The bars are test_cornellbox_parity's (tests/test_gpu_parity.py): hits equal, bitwise_frac >= 0.999 on
image, albedo and normal (at these sizes: every pixel), counters within 1e-3 relative + 8. A tile share
traces its own tiles only while the oracle traces every pixel, so there the share's pixels are
compared, the others must be untouched, and of the counters only the paths (exact).
"""
import numpy as np
import pytest

from conftest import compare_images, make_params

pytestmark = pytest.mark.gpu

SIZES = [(13, 9), (70, 9), (64, 64)]
SPP = 8
_oracle_cache = {}


def _oracle(oracle, scene_abi, params, w, h, sampler, k):
    """The oracle's render of samples [0, SPP) with k streams: computed once per (size, sampler, k),
    shared by the modes, never modified."""
    key = (w, h, sampler, k)
    if key not in _oracle_cache:
        ob, ol = oracle.build_bvh(scene_abi), oracle.make_lights(scene_abi)
        out = oracle.trace(scene_abi, ob, ol, params, w, h, 0, SPP, streams=k)
        for a in out[:4]:
            a.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


@pytest.mark.parametrize("mode", ["one", "two", "batch1", "share"])
@pytest.mark.parametrize("sampler", [1, 2])
@pytest.mark.parametrize("w,h", SIZES)
def test_item_coordinates_render(gpu, abi, lib, oracle, cornell_abi, options, w, h, sampler, mode):
    from jtrace import trace
    if mode == "share":
        options("tile_share", "2,1")
    params = make_params(abi, width=w, height=h, samples=SPP, sampler=sampler, batch=1 if mode == "batch1" else SPP)
    bvh = trace.make_scene_bvh(cornell_abi, False, lib)
    lights = trace.make_trace_lights(cornell_abi, lib)
    outs = []
    for level in (1, 0):  # the counting twin (every traversal counter), then the production kernel
        st = trace.make_trace_state(cornell_abi, bvh, lights, params, lib)
        k = st.streams
        assert (k == 1) == (mode == "batch1"), st.describe()
        st.set_counters(level)
        if mode == "two":
            st.trace_range(0, SPP // 2)
            st.trace_range(SPP // 2, SPP)
        else:
            st.trace_range(0, SPP)
        outs.append((st.get_image(), *st.get_aovs(), st.counters()))
        st.close()
    gimg, galb, gnrm, ghits, gcnt = outs[0]
    for a, b in zip(outs[0][:4], outs[1][:4]):  # the production kernel: the counting twin's bits
        assert np.array_equal(a, b)
    for c in ("paths", "rays", "light_queries"):
        assert outs[0][4][c] == outs[1][4][c], c
    assert gimg.shape[:2] == (h, w)
    oimg, oalb, onrm, ohits, ocnt = _oracle(oracle, cornell_abi, params, w, h, sampler, k)

    mask = np.ones((h, w), bool)
    if mode == "share":  # tiles 1, 3, ... of the image's tiles, row-major
        tiles_x = (w + 7) // 8
        jj, ii = np.mgrid[0:h, 0:w]
        mask = ((jj // 8) * tiles_x + ii // 8) % 2 == 1
        assert mask.any() and not mask.all()
        assert not gimg[~mask].any() and not galb[~mask].any() and not gnrm[~mask].any() and not ghits[~mask].any(), \
            "a pixel outside the share was written"
    n = int(mask.sum())
    for name, g, o in (("image", gimg, oimg), ("albedo", galb, oalb), ("normal", gnrm, onrm)):
        stats = compare_images(g[mask].reshape(n, 1, -1), o[mask].reshape(n, 1, -1))
        print(w, h, "sampler", sampler, mode, "streams", k, name, stats)
        assert stats["bitwise_frac"] >= 0.999, (name, stats)
    assert np.array_equal(ghits[mask], ohits[mask])
    print("gpu counters", gcnt, "oracle counters", ocnt)
    assert gcnt["paths"] == n * SPP
    if mode != "share":
        assert ocnt["paths"] == n * SPP
        for c in ("rays", "light_queries", "nodes", "instances", "prims", "shades"):
            assert abs(gcnt[c] - ocnt[c]) <= 1e-3 * ocnt[c] + 8, (c, gcnt[c], ocnt[c])
