"""The host layout of a scene (csrc/jt_layout.cpp), checked on the CPU through the library's debug
hooks jt_debug_layout_digest / jt_debug_layout_array (csrc/jt_trace.hip; no device is touched).

1. Digests: every array jt_create uploads (length and FNV-1a 64 of its bytes), the LDS blob and the
   derived scalars equal tests/golden/layout_digests.json. The goldens were recorded from the
   jt_create of the commit before the layout became its own unit (uploads redirected into the same
   digest), so they pin the refactor to the bytes the kernels read before it. A digest that differs
   means the layout is wrong, not the golden.
2. Structure: invariants the kernels rely on, evaluated on the raw arrays with numpy. They hold
   whatever the goldens say, so they catch a wrong golden as well as a wrong layout.
"""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT, make_params

GOLDEN = Path(__file__).resolve().parent / "golden" / "layout_digests.json"

# (scene, traversal, high-quality BVH, options)
CASES = [
    ("cornellbox", "near", False, {}), ("cornellbox", "wide", False, {}), ("cornellbox", "reference", False, {}),
    ("cornellbox", "auto", False, {}), ("cornellbox", "near", False, {"lds_scene": "0"}),
    ("cornellbox", "near", False, {"features": "all"}),
    ("features1", "near", False, {}), ("features1", "wide", False, {}), ("features1", "auto", False, {}),
    ("features2", "near", False, {}), ("features2", "wide", False, {}), ("features2", "auto", False, {}),
    ("features2", "near", False, {"env_alias": "1"}),
    ("shapes1", "near", False, {}), ("shapes1", "auto", False, {}), ("shapes1", "near", True, {}),
    ("bathroom1", "near", False, {}), ("bathroom1", "auto", False, {}),
    ("ecosys", "auto", False, {}),
]


def case_id(case):
    scene, traversal, hq, opts = case
    return "-".join([scene, traversal] + (["hq"] if hq else []) + [f"{k}={v}" for k, v in sorted(opts.items())])


_loaded = {}


def load(abi, lib, scene, hq):
    """(SceneABI, SceneBvh, TraceLights) of a scene, built once per module run."""
    if (scene, hq) not in _loaded:
        from jtrace import sceneio, trace
        sa = abi.SceneABI(sceneio.load_scene(str(ROOT / "assets" / "scenes" / scene / f"{scene}.json"), missing="drop"))
        _loaded[scene, hq] = (sa, trace.make_scene_bvh(sa, hq, lib), trace.make_trace_lights(sa, lib))
    return _loaded[scene, hq]


def layout_digest(abi, lib, sa, bvh, lights, params):
    """{"arrays": {name: [length, fnv1a64 hex]}, "scalars": {name: int}} of jt_debug_layout_digest."""
    buf = C.create_string_buffer(1 << 14)
    abi.check(lib, lib.jt_debug_layout_digest(sa.ref, bvh.ref, lights.ref, C.byref(params), buf, len(buf)))
    out = {"arrays": {}, "scalars": {}}
    for line in buf.value.decode().splitlines():
        tok = line.split()
        if tok[0] == "scalars":
            out["scalars"] = {k: int(v) for k, v in (t.split("=") for t in tok[1:])}
        else:
            out["arrays"][tok[0]] = [int(tok[1]), tok[2]]
    return out


def layout_array(abi, lib, sa, bvh, lights, params, name, dtype):
    n = C.c_int64()
    args = (sa.ref, bvh.ref, lights.ref, C.byref(params), name.encode())
    abi.check(lib, lib.jt_debug_layout_array(*args, None, C.c_int64(0), C.byref(n)))
    raw = np.zeros(max(1, n.value), np.uint8)
    abi.check(lib, lib.jt_debug_layout_array(*args, raw.ctypes.data_as(C.c_void_p), C.c_int64(raw.size), C.byref(n)))
    return raw[:n.value].view(dtype)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_layout_digest_matches_golden(abi, lib, options, case):
    scene, traversal, hq, opts = case
    for k, v in opts.items():
        options(k, v)
    sa, bvh, lights = load(abi, lib, scene, hq)
    got = layout_digest(abi, lib, sa, bvh, lights, make_params(abi, traversal=traversal, highqualitybvh=hq))
    want = json.loads(GOLDEN.read_text())[case_id(case)]
    assert got["scalars"] == want["scalars"]
    assert got["arrays"] == want["arrays"]


# ------------------------------------------------------------------------------------ structure
DNODE = np.dtype([("a", "<f4", 4), ("bz", "<f4", 2), ("start", "<i4"), ("meta", "<u4")])
DWIDE = np.dtype([("origin", "<f4", 3), ("meta", "<u4"), ("r1", "<u4", 4), ("r2", "<u4", 4), ("word", "<u4", 4)])
DSHAPE = np.dtype([("kind", "<i4"), ("blas_root", "<i4"), ("prim_base", "<i4"), ("idx_base", "<i4"), ("bases", "<i4", 4)])
W_EMPTY, W_LEAF, W_INST, W_START = 0xFFFFFFFF, 0x80000000, 0x40000000, 0x0FFFFFFF


def wide_slots(nodes, n):
    """The binary nodes a wide record of binary node n holds in its four slots (-1: empty)."""
    slot = [-1] * 4
    if not nodes[n]["internal"]:
        slot[0] = n
        return slot
    for half, ch in enumerate((int(nodes[n]["start"]), int(nodes[n]["start"]) + 1)):
        if nodes[ch]["internal"]:
            slot[2 * half], slot[2 * half + 1] = int(nodes[ch]["start"]), int(nodes[ch]["start"]) + 1
        else:
            slot[2 * half] = ch
    return slot


def check_wide_tree(wnodes, root, nodes, check_leaf):
    """Walks the records from `root` beside the binary tree they stand for: every occupied slot's
    dequantised box contains the child's box (float32, the device's o + q * scale), empty slots
    hold W_EMPTY, and every leaf word passes check_leaf(start, num)."""
    if len(nodes) == 0 or (not nodes[0]["internal"] and nodes[0]["num"] <= 0):
        assert all(int(w) == W_EMPTY for w in wnodes[root]["word"])  # the empty tree's record
        return 0
    leaves, stack = 0, [(root, 0)]
    while stack:
        rec, n = stack.pop()
        W = wnodes[rec]
        meta = int(W["meta"])
        lo_hi = [(W["r1"][0], W["r1"][1]), (W["r1"][2], W["r1"][3]), (W["r2"][0], W["r2"][1])]
        for c, b in enumerate(wide_slots(nodes, n)):
            word = int(W["word"][c])
            if b < 0:
                assert word == W_EMPTY
                continue
            assert word != W_EMPTY
            for ax in range(3):
                scale = np.array([((meta >> (8 * ax)) & 255) << 23], np.uint32).view(np.float32)[0]
                lo = np.float32((int(lo_hi[ax][0]) >> (8 * c)) & 255)
                hi = np.float32((int(lo_hi[ax][1]) >> (8 * c)) & 255)
                assert np.float32(W["origin"][ax] + np.float32(lo * scale)) <= nodes[b]["bmin"][ax]
                assert np.float32(W["origin"][ax] + np.float32(hi * scale)) >= nodes[b]["bmax"][ax]
            if nodes[b]["internal"]:
                assert not word & W_LEAF and word < len(wnodes)
                stack.append((word, b))
            else:
                assert word & W_LEAF
                num = ((word >> 28) & 3) + 1
                assert num == nodes[b]["num"]
                check_leaf(word, word & W_START, num)
                leaves += 1
    return leaves


@pytest.mark.parametrize("traversal", ["near", "wide"])
@pytest.mark.parametrize("scene", ["cornellbox", "features2"])
def test_layout_structure(abi, lib, scene, traversal):
    sa, bvh, lights = load(abi, lib, scene, False)
    params = make_params(abi, traversal=traversal)
    sc = layout_digest(abi, lib, sa, bvh, lights, params)["scalars"]
    arr = lambda name, dtype: layout_array(abi, lib, sa, bvh, lights, params, name, dtype)
    prims = arr("prims", np.float32).reshape(-1, 4)
    shapes, inst_blas = arr("shapes", DSHAPE), arr("inst_blas", np.int32).reshape(-1, 4)
    ninst, nshapes = len(inst_blas), len(shapes)
    stride = [5 if s["kind"] == 0 else 4 for s in shapes]
    trees = [bvh.tree(s)[0] for s in range(nshapes)]
    tlas = bvh.tree(-1)[0]

    # prims ends with the four zero float4s prim_step reads past the last leaf
    assert len(prims) >= 4 and not prims[-4:].any()
    # each shape's prim_base * stride lands on a record boundary: where the shape before it ends,
    # after fewer than `stride` zero float4s of padding; the last shape ends at the four zeros
    end = 0
    for s in range(nshapes):
        leaves = trees[s][trees[s]["internal"] == 0]["num"].astype(np.int64)
        nrec = int(((leaves + 1) // 2).sum() if stride[s] == 5 else leaves.sum())
        off = int(shapes[s]["prim_base"]) * stride[s]
        assert 0 <= off - end < stride[s] and not prims[end:off].any(), s
        end = off + nrec * stride[s]
    assert end + 4 == len(prims)

    seen = np.zeros(ninst, np.int64)  # TLAS leaf ranges covering each instance id

    def tlas_leaf(start, num):
        assert 0 <= start and start + num <= ninst
        seen[start:start + num] += 1

    def blas_leaf(s, start, num):
        nrec = (num + 1) // 2 if stride[s] == 5 else num
        assert shapes[s]["prim_base"] <= start and (start + nrec) * stride[s] <= len(prims) - 4

    if traversal == "wide":
        wnodes = arr("wnodes", DWIDE)
        assert len(arr("nodes", DNODE)) == 0  # the binary nodes are not uploaded
        def tleaf(word, start, num):
            assert word & W_INST
            tlas_leaf(start, num)
        check_wide_tree(wnodes, 0, tlas, tleaf)
        assert sc["tlas_wnodes"] >= 1
        for k in range(ninst):
            s = int(inst_blas[k][3]) & 0x3FFFFFFF
            root = int(inst_blas[k][0])
            assert sc["tlas_wnodes"] <= root < len(wnodes)
            def bleaf(word, start, num, s=s):
                assert not word & W_INST
                blas_leaf(s, start, num)
            nleaf = check_wide_tree(wnodes, root, trees[s], bleaf)
            assert nleaf == int((trees[s]["internal"] == 0).sum()) or len(trees[s]) <= 1
    else:
        nodes = arr("nodes", DNODE)
        assert len(arr("wnodes", DWIDE)) == 0 and sc["tlas_wnodes"] == 0
        assert sc["tlas_nnodes"] == len(tlas)
        internal, num = (nodes["meta"] >> 24) & 1, (nodes["meta"] & 0xFFFF).astype(np.int64)
        for k in range(sc["tlas_nnodes"]):
            if not internal[k]:
                tlas_leaf(int(nodes["start"][k]), int(num[k]))
        for s in range(nshapes):
            r = int(shapes[s]["blas_root"])
            assert r >= sc["tlas_nnodes"] and r + len(trees[s]) <= len(nodes)
            for k in range(r, r + len(trees[s])):
                if internal[k]:
                    assert r <= nodes["start"][k] and nodes["start"][k] + 1 < r + len(trees[s])
                else:
                    blas_leaf(s, int(nodes["start"][k]), int(num[k]))
    # every TLAS instance id appears in exactly one leaf range
    assert (seen == 1).all()
