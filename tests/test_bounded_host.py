"""Bounded ray queries and ambient occlusion (include/jtrace.h: jt_intersect_bounded,
jt_occluded_bounded, jt_visible, jt_ambient_occlusion and their device variants), the part that
needs no GPU:

1. the restatement of the bounded query (tests/bounded_ref.py) equals or_query in every bit at
   tmax = +inf, for every (scene, class) of queries_ref.CASES, in the reference and the near order,
   scene queries and instance queries: until this holds the restatement judges nothing;
2. the eight exports, their header prototypes and their ctypes mirrors;
3. every argument error, in the header's order, on a handle that is never read;
4. the stand-alone program of the new argument rules (tests/bounded_rules_check.cpp) under the
   address and undefined-behaviour sanitizers;
5. the inputs of the capped wide-order check of tests/test_gpu_bounded.py: with the bound 2 t_i the
   restatement returns exactly the unbounded record, for every ray, in both orders.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounded_ref as B
import queries_ref as Q
from conftest import ROOT

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_intersect_bounded", "jt_occluded_bounded", "jt_visible", "jt_ambient_occlusion")
FIELDS = ("inst", "elem", "hit", "u", "v", "t")
# the capped GPU case: the classes of queries_ref.CAPPED on the scenes with the most geometry
DOUBLED = [(s, c) for s in ("cornell", "random", "deep") for c in Q.CAPPED]


def differing(a, b):
    """Rays whose records differ in any field or bit."""
    bad = np.zeros(len(a["hit"]), bool)
    for k in ("inst", "elem", "hit"):
        bad |= a[k] != b[k]
    for k in ("u", "v", "t"):
        bad |= ~Q.same_bits(a[k], b[k])
    return np.flatnonzero(bad)


# ------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("scene,cls", Q.CASES)
def test_the_restatement_equals_or_query_at_an_infinite_bound(scene, cls, abi, oracle):
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in ("reference", "near"):
        for inst in (None, Q.instance_ids(ctx)):
            ref = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], r, inst=inst)
            got = B.query(ctx, oracle, order, r, inst)
            bad = differing(got, ref)
            assert len(bad) == 0, (scene, cls, order, inst is not None, len(bad), bad[:4], {k: (got[k][bad[:4]], ref[k][bad[:4]]) for k in FIELDS})
            # an explicit +inf array is the same query
            if order == "near" and inst is None:
                again = B.query(ctx, oracle, order, r, inst, np.full(len(r), np.inf, np.float32))
                assert len(differing(again, ref)) == 0
        print(f"{scene}/{cls}: {int(ref['hit'].sum())} hits, ties seen by the near order {int(got['tie'].sum())}")


# ------------------------------------------------------------------------------ 2. exports and prototypes
def test_the_eight_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for base in NAMES:
        for name in (base, base + "_device"):
            assert re.search(rf"\bint {name}\s*\(", text), name
            assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5 and "#define JT_ABI_VERSION 5" in HEADER.read_text()
    v, f, i, u, hit = C.c_void_p, abi.f32p, abi.i32p, abi.u8p, C.POINTER(abi.jt_hit)
    assert lib.jt_intersect_bounded.argtypes == [v, C.c_int64, f, f, i, hit]
    assert lib.jt_occluded_bounded.argtypes == [v, C.c_int64, f, f, u]
    assert lib.jt_visible.argtypes == [v, C.c_int64, f, u]
    assert lib.jt_ambient_occlusion.argtypes == [v, C.c_int64, f, C.c_int64, C.c_int32, C.c_int32, C.c_float, f]
    assert lib.jt_intersect_bounded_device.argtypes == [v, C.c_int64, v, v, v, v]
    assert lib.jt_occluded_bounded_device.argtypes == [v, C.c_int64, v, v, v]
    assert lib.jt_visible_device.argtypes == [v, C.c_int64, v, v]
    assert lib.jt_ambient_occlusion_device.argtypes == [v, C.c_int64, v, C.c_int64, C.c_int32, C.c_int32, C.c_float, v]
    want = {
        "jt_intersect_bounded": ["jt_ctx*", "int64_t", "float*", "float*", "int32_t*", "jt_hit*"],
        "jt_occluded_bounded": ["jt_ctx*", "int64_t", "float*", "float*", "uint8_t*"],
        "jt_visible": ["jt_ctx*", "int64_t", "float*", "uint8_t*"],
        "jt_ambient_occlusion": ["jt_ctx*", "int64_t", "float*", "int64_t", "int32_t", "int32_t", "float", "float*"],
    }
    for base, kinds in want.items():
        for name in (base, base + "_device"):
            decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
            got = [re.sub(r"\s+\w+$", "", a.strip()).replace("const ", "") for a in decl.split(",")]
            if name.endswith("_device"):
                kinds_d = [k if not k.endswith("*") or k == "jt_ctx*" else "void*" for k in kinds]
                assert got == kinds_d, (name, got)
            else:
                assert got == kinds, (name, got)


# ------------------------------------------------------------------------------ 3. argument errors
def test_argument_errors_in_order_need_no_device(abi, lib):
    """Every JT_ERR_INVALID names its argument and is reported before the context is looked at: the
    handle below is no context and is never read. Each call breaks one rule and, to show the order,
    every later rule too. n == 0 with valid arguments is JT_OK, and nothing is written."""
    rays = np.zeros((4, 6), np.float32)
    bound = np.ones(4, np.float32)
    hits = np.zeros(4, abi.HIT_DTYPE)
    flags = np.full(4, 7, np.uint8)
    vis = np.full(4, 7.0, np.float32)
    rp, bp, hp = rays.ctypes.data_as(abi.f32p), bound.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit))
    fp, vp = flags.ctypes.data_as(abi.u8p), vis.ctypes.data_as(abi.f32p)
    fake, dev, odd4 = C.c_void_p(0x10), C.c_void_p(0x1000), C.c_void_p(0x1002)

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    # ---- the bounded queries: jt_intersect's ladder, with and without a bound array
    for tm in (bp, None):
        assert "ctx" in err(lib.jt_intersect_bounded(None, -1, None, tm, None, None))
        assert re.match(r"rays\b", err(lib.jt_intersect_bounded(fake, -1, None, tm, None, None)))
        assert re.match(r"hits\b", err(lib.jt_intersect_bounded(fake, -1, rp, tm, None, None)))
        assert "ctx" in err(lib.jt_occluded_bounded(None, -1, None, tm, None))
        assert re.match(r"rays\b", err(lib.jt_occluded_bounded(fake, -1, None, tm, None)))
        assert re.match(r"occluded\b", err(lib.jt_occluded_bounded(fake, -1, rp, tm, None)))
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", err(lib.jt_intersect_bounded(fake, n, rp, tm, None, hp))), n
            assert re.match(r"n must\b", err(lib.jt_occluded_bounded(fake, n, rp, tm, fp))), n
        assert lib.jt_intersect_bounded(fake, 0, rp, tm, None, hp) == 0 and lib.jt_occluded_bounded(fake, 0, rp, tm, fp) == 0
    for tm in (dev, None):
        assert "ctx" in err(lib.jt_intersect_bounded_device(None, -1, None, tm, None, None))
        assert re.match(r"d_rays\b", err(lib.jt_intersect_bounded_device(fake, -1, None, tm, None, None)))
        assert re.match(r"d_hits\b", err(lib.jt_intersect_bounded_device(fake, -1, dev, tm, None, None)))
        assert re.match(r"d_rays\b", err(lib.jt_occluded_bounded_device(fake, -1, None, tm, None)))
        assert re.match(r"d_occluded\b", err(lib.jt_occluded_bounded_device(fake, -1, dev, tm, None)))
        assert re.match(r"n must\b", err(lib.jt_intersect_bounded_device(fake, 2**30 + 1, dev, tm, None, dev)))
        assert re.match(r"n must\b", err(lib.jt_occluded_bounded_device(fake, -1, dev, tm, dev)))
        assert lib.jt_intersect_bounded_device(fake, 0, dev, tm, None, dev) == 0
        assert lib.jt_occluded_bounded_device(fake, 0, dev, tm, dev) == 0
    assert "ctx" in err(lib.jt_visible(None, -1, None, None)) and "ctx" in err(lib.jt_visible_device(None, -1, None, None))
    assert re.match(r"segments\b", err(lib.jt_visible(fake, -1, None, None)))
    assert re.match(r"visible\b", err(lib.jt_visible(fake, -1, rp, None)))
    assert re.match(r"d_segments\b", err(lib.jt_visible_device(fake, -1, None, None)))
    assert re.match(r"d_visible\b", err(lib.jt_visible_device(fake, -1, dev, None)))
    for n in (-1, 2**30 + 1):
        assert re.match(r"n must\b", err(lib.jt_visible(fake, n, rp, fp))) and re.match(r"n must\b", err(lib.jt_visible_device(fake, n, dev, dev)))
    assert lib.jt_visible(fake, 0, rp, fp) == 0 and lib.jt_visible_device(fake, 0, dev, dev) == 0

    # ---- jt_ambient_occlusion: jt_radiance's ladder, the radius after the sample range, then alignment
    def ao(ctx=fake, n=4, p=rp, base=0, s0=0, s1=1, radius=1.0, o=vp):
        return err(lib.jt_ambient_occlusion(ctx, n, p, base, s0, s1, radius, o))

    def ao_dev(ctx=fake, n=4, p=dev, base=0, s0=0, s1=1, radius=1.0, o=dev):
        return err(lib.jt_ambient_occlusion_device(ctx, n, p, base, s0, s1, radius, o))

    nan = float("nan")
    late = dict(n=-1, base=-1, s0=-1, s1=-1, radius=nan)
    assert "ctx" in ao(ctx=None, p=None, o=None, **late) and "ctx" in ao_dev(ctx=None, p=None, o=odd4, **late)
    assert re.match(r"points\b", ao(p=None, o=None, **late)) and re.match(r"d_points\b", ao_dev(p=None, o=None, **late))
    assert re.match(r"visibility\b", ao(o=None, **late)) and re.match(r"d_visibility\b", ao_dev(o=None, **late))
    for call, o in ((ao, vp), (ao_dev, odd4)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s0=-1, s1=-1, radius=nan, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s0=-1, s1=-1, radius=nan, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s0=-1, s1=-1, radius=nan, o=o))
        assert re.match(r"sample_begin\b", call(s0=-1, s1=-5, radius=nan, o=o))
        assert re.match(r"sample_end must\b", call(s0=3, s1=3, radius=nan, o=o))
        assert "2^24" in call(s0=5, s1=5 + 2**24 + 1, radius=nan, o=o)
        for radius in (nan, 0.0, -0.0, -1.0, float("-inf")):
            assert re.match(r"radius\b", call(radius=radius, o=o)), radius
            assert re.match(r"radius\b", call(n=0, radius=radius, o=o)), radius  # before the n == 0 return
    assert re.match(r"d_visibility\b.*aligned to 4", ao_dev(o=odd4)) and re.match(r"d_visibility\b.*aligned", ao_dev(n=0, o=odd4))
    # the largest arguments that break no rule reach the n == 0 return: JT_OK, no device work
    for radius in (1e-30, 0.25, float("inf")):
        assert lib.jt_ambient_occlusion(fake, 0, rp, 2**31, 2**31 - 2, 2**31 - 1, radius, vp) == 0
        assert lib.jt_ambient_occlusion(fake, 0, rp, 0, 0, 2**24, radius, vp) == 0
        assert lib.jt_ambient_occlusion_device(fake, 0, dev, 0, 0, 1, radius, dev) == 0
    assert (vis == 7.0).all() and (flags == 7).all() and (hits.view(np.uint8) == 0).all() and (rays == 0).all()


# ------------------------------------------------------------------------------ 4. the rules program
def test_bounded_argument_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "bounded_rules_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "bounded_rules_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout


# ------------------------------------------------------------------------------ 5. the capped case's inputs
@pytest.mark.parametrize("scene,cls", DOUBLED)
def test_a_bound_of_twice_the_hit_distance_changes_no_record(scene, cls, abi, oracle):
    """The bound 2 t_i of a ray's own unbounded hit (a miss: a finite bound of the scene's size) in
    the reference and the near order: the restatement returns the unbounded record for every ray.
    The wide order's GPU check of the same rays may differ through a rounding cull only, capped."""
    ctx = Q.context(scene, abi, oracle)
    r = Q.rays(ctx, cls, oracle)
    for order in ("reference", "near"):
        free = oracle.query(ctx.sa, ctx.bvh, ctx.params[order], r)
        got = B.query(ctx, oracle, order, r, None, B.doubled_bounds(ctx, cls, free))
        bad = differing(got, free)
        print(f"{scene}/{cls}/{order}: {len(bad)} of {len(r)} rays differ")
        assert len(bad) == 0, (scene, cls, order, len(bad), bad[:4])
