"""All hits along a ray (include/jtrace.h: jt_intersect_multi, jt_count_hits and their device variants),
the part that needs no GPU:

1. the restatement (tests/multihit_ref.py), in the reference and the near order, against the brute
   force over every element, for every (scene, class) of queries_ref.CASES at k = 1, 4 and 16: on the
   classes STRICT no ray may differ in any bit; on axis, planar and edges the count is printed and
   each differing ray's cause is proved, a box on the path to a missing primitive that the reference's
   own slab test rejects although the primitive's t lies within the tmax it is asked with;
2. the two orders agree at k = 4 and 16 on every ray; at k = 1 they differ in strip/edges only, and
   k = 1's flag and t are or_query's in each order;
3. jt_count_hits restated: the same count in both orders on every ray, the brute force's total on
   the STRICT classes, and min(16, count) is the length of the k = 16 list there;
4. bounds: with the bits of the second hit's t as the bound the list is the unbounded list cut at
   t <= B; a bound below ray_eps, zero or negative gives an empty list;
5. the stand-alone program of the list's rules (tests/multihit_check.cpp) under the address and
   undefined-behaviour sanitizers;
6. the four exports, their header prototypes and ctypes mirrors, and every argument error in the
   header's order on a handle that is never read;
7. the command line's rejections.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import multihit_ref as M
import queries_ref as Q
from conftest import ROOT
from test_queries_host import rejecting_box

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_intersect_multi", "jt_count_hits")
KS = (1, 4, 16)
ORDERS = ("reference", "near")
# the classes on which the restatement must equal the brute force on every ray
STRICT = ("generic", "tiny", "surface", "outside", "stacked")
K1_ORDER_DIFFS = {("strip", "edges")}  # queries_ref.ORDER_DIFFS' own near-order entry


def case(abi, oracle, scene, cls):
    ctx = Q.context(scene, abi, oracle)
    return ctx, Q.rays(ctx, cls, oracle)


# ------------------------------------------------------------------------------ 1. against brute force
def culled(ctx, oracle, ray, rec, cnt, brec, bcnt, k, bound=np.inf):
    """A brute-force entry the restatement's list lacks, on whose path a reference box rejects the
    ray at the query's final tmax (its smallest: a box that rejected at any tmax the query held
    rejects at this one, the slab test being monotone in tmax), which is no less than the entry's t."""
    have = {(int(rec["instance"][j]), int(rec["element"][j])) for j in range(cnt)}
    final = float(rec["t"][k - 1]) if cnt == k else float(bound)
    for j in range(bcnt):
        ie = (int(brec["instance"][j]), int(brec["element"][j]))
        if ie not in have:
            assert brec["t"][j] <= final, (ie, brec["t"][j], final)
            return rejecting_box(ctx, oracle, ray, ie[0], ie[1], final)
    return False


@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_the_restatement_against_brute_force(scene, cls, abi, oracle):
    ctx, r = case(abi, oracle, scene, cls)
    b = M.brute(ctx, oracle, r)
    line = []
    for k in KS:
        brec, bcnt = b.multi(abi.HIT_DTYPE, k)
        for order in ORDERS:
            rec, cnt = M.multi(ctx, oracle, order, r, k)
            bad = M.differing(rec, cnt, brec, bcnt)
            line.append(f"k={k}/{order}={len(bad)}")
            if cls in STRICT:
                assert len(bad) == 0, (scene, cls, k, order, len(bad), bad[:4], rec[bad[:2]], brec[bad[:2]])
            for i in bad:
                assert culled(ctx, oracle, r[i], rec[i], int(cnt[i]), brec[i], int(bcnt[i]), k), (scene, cls, k, order, int(i), r[i].tolist())
    print(f"multi against brute {scene}/{cls}: n={len(r)} most hits on a ray {int(b.total.max())}; differing rays " + " ".join(line))


# ------------------------------------------------------------------------------ 2. order and k = 1
@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_the_orders_agree_and_k1_is_the_closest_hit(scene, cls, abi, oracle):
    ctx, r = case(abi, oracle, scene, cls)
    for k in (4, 16):
        bad = M.differing(*M.multi(ctx, oracle, "reference", r, k), *M.multi(ctx, oracle, "near", r, k))
        assert len(bad) == 0, (scene, cls, k, len(bad), bad[:4])
    one = {o: M.multi(ctx, oracle, o, r, 1) for o in ORDERS}
    bad = M.differing(*one["reference"], *one["near"])
    print(f"k = 1, reference against near, {scene}/{cls}: {len(bad)} rays differ")
    assert (len(bad) > 0) == ((scene, cls) in K1_ORDER_DIFFS), (scene, cls, len(bad), bad[:4])
    for order in ORDERS:
        rec, cnt = one[order]
        ref = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], r)
        hit = ref["hit"] != 0
        assert np.array_equal(cnt, ref["hit"]) and np.array_equal(rec["hit"][:, 0], ref["hit"]), (scene, cls, order)
        bad = np.flatnonzero(hit & ~Q.same_bits(rec["t"][:, 0], ref["t"]))
        assert len(bad) == 0, (scene, cls, order, "t", len(bad), bad[:4])
        ids = np.flatnonzero(hit & ((rec["instance"][:, 0] != ref["inst"]) | (rec["element"][:, 0] != ref["elem"])))
        # an exact-t tie: the smallest id here, the last one tested there
        smaller = M.key_less(rec["t"][ids, 0], rec["instance"][ids, 0], rec["element"][ids, 0], ref["t"][ids], ref["inst"][ids], ref["elem"][ids])
        assert smaller.all(), (scene, cls, order, ids[:4])
        print(f"k = 1 against or_query, {scene}/{cls}/{order}: {len(ids)} exact-t ties resolved to the smaller id")


# ------------------------------------------------------------------------------ 3. counts
@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_counts(scene, cls, abi, oracle):
    ctx, r = case(abi, oracle, scene, cls)
    c = {o: M.count(ctx, oracle, o, r) for o in ORDERS}
    bad = np.flatnonzero(c["reference"] != c["near"])
    assert len(bad) == 0, (scene, cls, len(bad), bad[:4])
    b = M.brute(ctx, oracle, r)
    short = np.flatnonzero(c["reference"] != b.total)
    print(f"counts {scene}/{cls}: {int(c['reference'].sum())} hits, most {int(c['reference'].max())}, {len(short)} rays differ from the brute total")
    assert (c["reference"] <= b.total).all()
    if cls in STRICT:
        assert len(short) == 0, (scene, cls, short[:4])
        for o in ORDERS:
            assert np.array_equal(M.multi(ctx, oracle, o, r, 16)[1], np.minimum(16, c[o])), (scene, cls, o)
    inst = Q.instance_ids(ctx)
    ci = {o: M.count(ctx, oracle, o, r, inst) for o in ORDERS}
    assert np.array_equal(ci["reference"], ci["near"]), (scene, cls, "instance")
    if cls in STRICT:
        assert np.array_equal(ci["reference"], M.brute(ctx, oracle, r, inst).total), (scene, cls, "instance")


# ------------------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("scene,cls", [c for c in Q.CASES if c[1] in STRICT])
def test_a_bound_on_the_second_hit_cuts_the_list_there(scene, cls, abi, oracle):
    ctx, r = case(abi, oracle, scene, cls)
    b = M.brute(ctx, oracle, r)
    bound = b.nth_t(1)  # the bits of the second hit's t; +inf where a ray has fewer
    for k in (1, 4):
        want = b.multi(abi.HIT_DTYPE, k, bound)
        for order in ORDERS:
            bad = M.differing(*M.multi(ctx, oracle, order, r, k, tmax=bound), *want)
            assert len(bad) == 0, (scene, cls, k, order, len(bad), bad[:4])
    on = np.isfinite(bound)
    assert (b.count(bound)[on] >= 2).all()  # the hit on the bound counts
    assert on.sum() > 20 or scene in ("random", "strip"), (scene, cls, int(on.sum()))
    print(f"bound on the second hit {scene}/{cls}: {int(on.sum())} rays have one")
    for order in ORDERS:
        assert np.array_equal(M.count(ctx, oracle, order, r, tmax=bound), b.count(bound)), (scene, cls, order)


def test_a_bound_below_ray_eps_gives_an_empty_list(abi, oracle):
    ctx, r = case(abi, oracle, "cornell", "generic")
    for bound in (np.nextafter(np.float32(0.0001), np.float32(0)), 0.0, -0.0, -1.0, -np.inf):
        for order in ORDERS:
            rec, cnt = M.multi(ctx, oracle, order, r, 4, tmax=bound)
            assert (cnt == 0).all() and (rec["hit"] == 0).all() and np.isposinf(rec["t"]).all(), (bound, order)
            assert (M.count(ctx, oracle, order, r, tmax=bound) == 0).all(), (bound, order)


# ------------------------------------------------------------------------------ 5. the rules program
def test_multihit_list_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "multihit_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "multihit_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout


# ------------------------------------------------------------------------------ 6. exports, prototypes, errors
def test_the_four_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for base in NAMES:
        for name in (base, base + "_device"):
            assert re.search(rf"\bint {name}\s*\(", text), name
            assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5 and "#define JT_ABI_VERSION 5" in HEADER.read_text()
    assert re.search(r"#define JT_MULTI_MAX_HITS 16\b", HEADER.read_text()) and abi.MULTI_MAX_HITS == 16
    v, f, i, hit = C.c_void_p, abi.f32p, abi.i32p, C.POINTER(abi.jt_hit)
    assert lib.jt_intersect_multi.argtypes == [v, C.c_int64, f, f, i, C.c_int32, hit, i]
    assert lib.jt_count_hits.argtypes == [v, C.c_int64, f, f, i, i]
    assert lib.jt_intersect_multi_device.argtypes == [v, C.c_int64, v, v, v, C.c_int32, v, v]
    assert lib.jt_count_hits_device.argtypes == [v, C.c_int64, v, v, v, v]
    want = {
        "jt_intersect_multi": ["jt_ctx*", "int64_t", "float*", "float*", "int32_t*", "int32_t", "jt_hit*", "int32_t*"],
        "jt_count_hits": ["jt_ctx*", "int64_t", "float*", "float*", "int32_t*", "int32_t*"],
    }
    for base, kinds in want.items():
        for name in (base, base + "_device"):
            decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
            got = [re.sub(r"\s+\w+$", "", a.strip()).replace("const ", "") for a in decl.split(",")]
            if name.endswith("_device"):
                kinds = [k if not k.endswith("*") or k == "jt_ctx*" else "void*" for k in kinds]
            assert got == kinds, (name, got)


def test_argument_errors_in_order_need_no_device(abi, lib):
    """Every JT_ERR_INVALID names its argument and is reported before the context is looked at: the
    handle below is no context and is never read. Each call breaks one rule and every later rule
    too. n == 0 with valid arguments is JT_OK, and nothing is written."""
    rays = np.zeros((4, 6), np.float32)
    bound = np.ones(4, np.float32)
    hits = np.zeros((4, 16), abi.HIT_DTYPE)
    counts = np.full(4, 7, np.int32)
    rp, bp = rays.ctypes.data_as(abi.f32p), bound.ctypes.data_as(abi.f32p)
    hp, cp = hits.ctypes.data_as(C.POINTER(abi.jt_hit)), counts.ctypes.data_as(abi.i32p)
    fake, dev, odd4, odd2 = C.c_void_p(0x10), C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x1002)

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    for tm in (bp, None):
        assert "ctx" in err(lib.jt_intersect_multi(None, -1, None, tm, None, 0, None, None))
        assert re.match(r"rays\b", err(lib.jt_intersect_multi(fake, -1, None, tm, None, 0, None, None)))
        assert re.match(r"hits\b", err(lib.jt_intersect_multi(fake, -1, rp, tm, None, 0, None, None)))
        assert re.match(r"counts\b", err(lib.jt_intersect_multi(fake, -1, rp, tm, None, 0, hp, None)))
        assert "ctx" in err(lib.jt_count_hits(None, -1, None, tm, None, None))
        assert re.match(r"rays\b", err(lib.jt_count_hits(fake, -1, None, tm, None, None)))
        assert re.match(r"counts\b", err(lib.jt_count_hits(fake, -1, rp, tm, None, None)))
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", err(lib.jt_intersect_multi(fake, n, rp, tm, None, 0, hp, cp))), n
            assert re.match(r"n must\b", err(lib.jt_count_hits(fake, n, rp, tm, None, cp))), n
        for n, k in ((4, 0), (4, -1), (4, 17), (0, 0), (0, 17), (2**30, 2), (2**26 + 1, 16), (4, 2**31 - 1), (4, -2**31)):
            assert re.match(r"k\b", err(lib.jt_intersect_multi(fake, n, rp, tm, None, k, hp, cp))), (n, k)
        for k in (1, 16):
            assert lib.jt_intersect_multi(fake, 0, rp, tm, None, k, hp, cp) == 0
        assert lib.jt_count_hits(fake, 0, rp, tm, None, cp) == 0
    for tm in (dev, None):
        assert "ctx" in err(lib.jt_intersect_multi_device(None, -1, None, tm, None, 0, None, None))
        assert re.match(r"d_rays\b", err(lib.jt_intersect_multi_device(fake, -1, None, tm, None, 0, None, None)))
        assert re.match(r"d_hits\b", err(lib.jt_intersect_multi_device(fake, -1, dev, tm, None, 0, None, None)))
        assert re.match(r"d_counts\b", err(lib.jt_intersect_multi_device(fake, -1, dev, tm, None, 0, odd4, None)))
        assert re.match(r"n must\b", err(lib.jt_intersect_multi_device(fake, -1, dev, tm, None, 0, odd4, odd2)))
        assert re.match(r"k\b", err(lib.jt_intersect_multi_device(fake, 4, dev, tm, None, 0, odd4, odd2)))
        assert re.match(r"k\b", err(lib.jt_intersect_multi_device(fake, 2**30, dev, tm, None, 2, odd4, odd2)))
        assert re.match(r"d_hits\b.*aligned to 8", err(lib.jt_intersect_multi_device(fake, 4, dev, tm, None, 4, odd4, odd2)))
        assert re.match(r"d_hits\b.*aligned to 8", err(lib.jt_intersect_multi_device(fake, 0, dev, tm, None, 4, odd4, dev)))  # before n == 0
        assert re.match(r"d_counts\b.*aligned to 4", err(lib.jt_intersect_multi_device(fake, 4, dev, tm, None, 4, dev, odd2)))
        assert re.match(r"d_counts\b.*aligned to 4", err(lib.jt_intersect_multi_device(fake, 0, dev, tm, None, 4, dev, odd2)))
        assert lib.jt_intersect_multi_device(fake, 0, dev, tm, None, 16, dev, odd4) == 0
        assert "ctx" in err(lib.jt_count_hits_device(None, -1, None, tm, None, None))
        assert re.match(r"d_rays\b", err(lib.jt_count_hits_device(fake, -1, None, tm, None, None)))
        assert re.match(r"d_counts\b", err(lib.jt_count_hits_device(fake, -1, dev, tm, None, None)))
        assert re.match(r"n must\b", err(lib.jt_count_hits_device(fake, 2**30 + 1, dev, tm, None, odd2)))
        assert re.match(r"d_counts\b.*aligned to 4", err(lib.jt_count_hits_device(fake, 0, dev, tm, None, odd2)))
        assert lib.jt_count_hits_device(fake, 0, dev, tm, None, odd4) == 0
    assert (counts == 7).all() and (hits.view(np.uint8) == 0).all() and (rays == 0).all()
    assert lib.jt_set_option(b"test_multi_chunk", b"1000") == 0 and lib.jt_set_option(b"test_multi_chunk", None) == 0


# ------------------------------------------------------------------------------ 7. the command line
def test_cli_rejections(tmp_path):
    """--hits and --count exclude each other, --any and --segments; k is 1 .. 16. Refused before the
    scene is loaded: the scene file named here does not exist."""
    from jtrace import query
    rays = tmp_path / "rays.npy"
    np.save(rays, np.zeros((3, 6), np.float32))
    base = ["--scene", str(tmp_path / "none.json"), "--output", str(tmp_path / "out.npz")]
    for extra, word in ((["--rays", str(rays), "--hits", "4", "--count", "true"], "--hits"),
                        (["--rays", str(rays), "--hits", "4", "--any", "true"], "--any"),
                        (["--rays", str(rays), "--count", "true", "--any", "true"], "--any"),
                        (["--segments", str(rays), "--hits", "4"], "--segments"),
                        (["--segments", str(rays), "--count", "true"], "--segments"),
                        (["--rays", str(rays), "--hits", "0"], "--hits"),
                        (["--rays", str(rays), "--hits", "17"], "--hits")):
        with pytest.raises(SystemExit) as e:
            query.main(base + extra)
        assert word in str(e.value), (extra, e.value)
    assert not (tmp_path / "out.npz").exists()
