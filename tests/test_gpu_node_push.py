"""The binary node step's straight-line pushes (csrc/jt_push.h, jtk::node_step) against the oracle.

The fixed-stack LDS kernels write an internal node's two children and a TLAS leaf's one to four
instances as four unconditional stack writes. These scenes put TLAS leaves of every size in front
of them: N in {1, 2, 3, 5, 7, 9} identity-frame instances of two-triangle quads plus one
12-triangle box, one quad emissive so the inline light chain runs (the FT_NONE|FT_LINL kernel),
the same set with a glossy box (the FT_ALL LDS kernel), and one instance of a folded 64-triangle
strip under a constant environment (a deep BLAS: pushes near the top of the fixed stack).
Both samplers, the reference and the near-first order, LDS mode and lds_scene=0, at 48x48 x 4 spp
with batch 4.

The bar is tests/test_gpu_edge.py's (>= 99.9 % of pixels bit-identical and within 1e-3, image mean
within 1e-4, hits equal). The scenes have no decision that depends on a libm rounding (the oracle
gives the same counters at 1 and 16 threads), so nodes, instances, prims, rays and light_queries
must equal the oracle's exactly.
"""
import numpy as np
import pytest

from conftest import compare_images, make_params
from scenes_ref import SEEDS, quad_scene, strip_scene  # moved there unchanged: the ray-query tests build them too

pytestmark = pytest.mark.gpu

ORDERS = {"reference": 0, "near": 1}
QUADS = (1, 2, 3, 5, 7, 9)
W = H = 48
SPP = 4
NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("start", "<i4"), ("num", "<i2"), ("axis", "i1"),
                 ("internal", "i1")])


def tlas_leaf_sizes(bvh):
    """The instance counts of the TLAS leaves of a built scene BVH (the library's or the oracle's)."""
    import ctypes as C
    t = bvh.struct.tlas
    nodes = np.ctypeslib.as_array(C.cast(t.nodes, C.POINTER(C.c_uint8)), shape=(t.nnodes * 32,)).view(NODE)
    return sorted(int(n["num"]) for n in nodes if not n["internal"])


_scenes, _oracle = {}, {}


def scene_abi(abi, name):
    if name not in _scenes:
        kind, n = name
        _scenes[name] = abi.SceneABI(strip_scene() if kind == "strip" else quad_scene(n, kind == "glossy", SEEDS[n]))
    return _scenes[name]


def oracle_trace(oracle, sa, name, params, sampler, order, k):
    """The oracle's render of a scene, computed once per (scene, sampler, order, streams) and
    shared by the scene modes."""
    key = (name, sampler, order, k)
    if key not in _oracle:
        _oracle[key] = oracle.trace(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, W, H, 0, SPP, streams=k)
    return _oracle[key]


def _both(abi, lib, oracle, name, sampler, order, options, lds):
    from jtrace import trace
    sa = scene_abi(abi, name)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=sampler, traversal=order)
    if lds is not None:
        options("lds_scene", lds)
    bvh = trace.make_scene_bvh(sa, False, lib)
    lights = trace.make_trace_lights(sa, lib)
    st = trace.make_trace_state(sa, bvh, lights, params, lib)
    st.trace_range(0, SPP)
    g = (st.get_image(), *st.get_aovs(), st.counters())
    k, desc = st.streams, st.describe()
    st.close()
    return g, oracle_trace(oracle, sa, name, params, sampler, order, k), k, desc


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


def _expect_kernel(desc, mode, sampler, mask):
    kernel = "trace_kernel_lds" if mode == "lds" else "trace_kernel"
    assert f"kernel={kernel}<{sampler},16,false,1,{mask},false> mode={mode} " in desc, desc


def test_tlas_leaves_of_every_size_occur(abi, lib, oracle):
    """Across the set the built TLAS has leaves of 1, 2, 3 and 4 instances: every count the push
    plan absorbs in its four writes. The library's build and the oracle's agree."""
    from jtrace import trace
    seen = set()
    for n in QUADS:
        sa = scene_abi(abi, ("matte", n))
        sizes = tlas_leaf_sizes(trace.make_scene_bvh(sa, False, lib))
        assert sizes == tlas_leaf_sizes(oracle.build_bvh(sa)), n
        assert sum(sizes) == n + 1 and max(sizes) <= 4, (n, sizes)
        seen |= set(sizes)
    assert seen == {1, 2, 3, 4}, seen


@pytest.mark.parametrize("mode", ["lds", "hbm"])
@pytest.mark.parametrize("order", ["reference", "near"])
@pytest.mark.parametrize("sampler", [1, 2])
@pytest.mark.parametrize("kind", ["matte", "glossy"])
def test_tlas_leaf_pushes_match_the_oracle(gpu, abi, lib, oracle, options, kind, sampler, order, mode):
    """Every scene of the set: the matte ones run the FT_NONE|FT_LINL kernel (the flagship's), the
    glossy ones the FT_ALL kernel; images, hit counts and traversal counters equal the oracle's."""
    for n in QUADS:
        g, o, k, desc = _both(abi, lib, oracle, (kind, n), sampler, order, options, "0" if mode == "hbm" else None)
        assert "light_inline=1" in desc and f"traversal={order}" in desc, desc
        _expect_kernel(desc, mode, sampler, 8192 if kind == "matte" else 255)
        _check(g, o, f"{kind}{n}/{mode}/{order}/{sampler}/k{k}")


@pytest.mark.parametrize("mode", ["lds", "hbm"])
@pytest.mark.parametrize("order", ["reference", "near"])
@pytest.mark.parametrize("sampler", [1, 2])
def test_deep_blas_pushes_match_the_oracle(gpu, abi, lib, oracle, options, sampler, order, mode):
    """One instance of a 64-triangle strip: the deepest BLAS of the set, whose pushes reach the top
    of the fixed stack (stack_bound entries). The environment makes it the FT_ALL LDS kernel's."""
    g, o, k, desc = _both(abi, lib, oracle, ("strip", 0), sampler, order, options, "0" if mode == "hbm" else None)
    assert f"traversal={order}" in desc and "stack_bound=10 " in desc, desc
    _expect_kernel(desc, mode, sampler, 255)
    _check(g, o, f"strip/{mode}/{order}/{sampler}/k{k}")
