"""TEST INFRASTRUCTURE ONLY — ctypes binding of the CPU oracle (oracle/jt_oracle.c).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module,
and only as the checker / the timed CPU baseline — never on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB = HERE / "build" / "libjt_oracle.so"


def build():
    subprocess.run(["make", "-C", str(HERE)], check=True, capture_output=True)


def _load(abi):
    if not LIB.exists():
        build()
    lib = C.CDLL(str(LIB))
    lib.or_build_scene_bvh.argtypes = [C.POINTER(abi.jt_scene), C.c_int32, C.POINTER(abi.jt_scene_bvh)]
    lib.or_free_scene_bvh.argtypes = [C.POINTER(abi.jt_scene_bvh)]
    lib.or_free_scene_bvh.restype = None
    lib.or_make_lights.argtypes = [C.POINTER(abi.jt_scene), C.POINTER(abi.jt_lights)]
    lib.or_free_lights.argtypes = [C.POINTER(abi.jt_lights)]
    lib.or_free_lights.restype = None
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    lib.or_trace_rows.argtypes = [C.POINTER(abi.jt_scene), C.POINTER(abi.jt_scene_bvh), C.POINTER(abi.jt_lights),
                                  C.POINTER(abi.jt_params), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, i64p, C.c_int32,
                                  f32p, f32p, f32p, i64p, C.c_int32, C.POINTER(Counters)]
    lib.or_order_diff.argtypes = [C.POINTER(abi.jt_scene), C.POINTER(abi.jt_scene_bvh), C.POINTER(abi.jt_lights),
                                  C.POINTER(abi.jt_params), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.POINTER(C.c_uint64)]
    lib.or_intersect_triangle.argtypes = [f32p, f32p, C.c_float, C.c_float, f32p, f32p, f32p, f32p]
    lib.or_intersect_bbox.argtypes = [f32p, f32p, C.c_float, C.c_float, f32p, f32p]
    lib.or_fresnel_dielectric.argtypes = [C.c_float, f32p, f32p]
    lib.or_fresnel_dielectric.restype = C.c_float
    lib.or_rng_first.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, f32p]
    lib.or_rng_first.restype = None
    lib.or_inverse_frame.argtypes = [f32p, C.c_int32, f32p]
    lib.or_inverse_frame.restype = None
    lib.or_srgb_to_rgb.argtypes = [C.POINTER(C.c_uint8), C.c_int32, f32p]
    lib.or_srgb_to_rgb.restype = None
    lib.or_set_env_alias.argtypes = [C.c_int32]
    lib.or_set_env_alias.restype = None
    lib.or_alias_table.argtypes = [f32p, C.c_int32, f32p, C.POINTER(C.c_int32)]
    lib.or_wide_check.argtypes = [C.POINTER(abi.jt_bvh_tree), C.POINTER(abi.jt_bvh_tree), C.c_int32,
                                  C.POINTER(C.c_int64)]
    lib.or_probe.argtypes = [C.c_int, C.c_int64, f32p, f32p]
    lib.or_probe_name.argtypes = [C.c_int]
    lib.or_probe_name.restype = C.c_char_p
    lib.or_probe_nin.argtypes = [C.c_int]
    lib.or_probe_nout.argtypes = [C.c_int]
    lib.or_probe_texture.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), f32p, C.c_int64, f32p, f32p]
    lib.or_srgb_to_rgb.argtypes = [C.POINTER(C.c_uint8), C.c_int32, f32p]
    i32p = C.POINTER(C.c_int32)
    lib.or_query.argtypes = [C.POINTER(abi.jt_scene), C.POINTER(abi.jt_scene_bvh), C.POINTER(abi.jt_params), C.c_int64,
                             f32p, i32p, i32p, f32p, i64p]
    lib.or_query_brute.argtypes = [C.POINTER(abi.jt_scene), C.c_int64, f32p, i32p, f32p, i32p, i32p, C.c_int32]
    lib.or_instance_ray.argtypes = [f32p, f32p, f32p, f32p]
    lib.or_instance_ray.restype = None
    return lib


class Counters(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("light_queries", C.c_uint64),
                ("nodes", C.c_uint64), ("instances", C.c_uint64), ("prims", C.c_uint64),
                ("shades", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Oracle:
    def __init__(self, abi):
        self.abi = abi
        self.lib = _load(abi)

    def build_bvh(self, scene_abi, high_quality=False):
        out = self.abi.jt_scene_bvh()
        st = self.lib.or_build_scene_bvh(scene_abi.ref, int(high_quality), C.byref(out))
        if st != 0:
            raise RuntimeError(f"oracle bvh build failed: {st}")
        return _Owned(out, self.lib.or_free_scene_bvh)

    def make_lights(self, scene_abi):
        out = self.abi.jt_lights()
        st = self.lib.or_make_lights(scene_abi.ref, C.byref(out))
        if st != 0:
            raise RuntimeError(f"oracle lights failed: {st}")
        return _Owned(out, self.lib.or_free_lights)

    def alias_table(self, cdf):
        """The env_alias option's Vose table of one light CDF: (keep (n,) float32, other (n,) int32)."""
        cdf = np.ascontiguousarray(cdf, np.float32)
        keep = np.empty(len(cdf), np.float32)
        other = np.empty(len(cdf), np.int32)
        st = self.lib.or_alias_table(cdf.ctypes.data_as(C.POINTER(C.c_float)), len(cdf),
                                     keep.ctypes.data_as(C.POINTER(C.c_float)), other.ctypes.data_as(C.POINTER(C.c_int32)))
        if st != 0:
            raise RuntimeError(f"oracle alias table failed: {st}")
        return keep, other

    def probe_ops(self):
        """The single-primitive probes' table: [(name, nin, nout)], the index is the op id."""
        return [(self.lib.or_probe_name(k).decode(), self.lib.or_probe_nin(k), self.lib.or_probe_nout(k))
                for k in range(self.lib.or_probe_count())]

    def probe(self, op, x):
        """Op `op` (a name of probe_ops) over the rows of x (n, nin) float32: (n, nout) float32."""
        ops = self.probe_ops()
        k = [o[0] for o in ops].index(op)
        x = np.ascontiguousarray(x, np.float32).reshape(-1, ops[k][1])
        out = np.empty((x.shape[0], ops[k][2]), np.float32)
        f32p = C.POINTER(C.c_float)
        st = self.lib.or_probe(k, x.shape[0], x.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
        if st != 0:
            raise RuntimeError(f"oracle probe {op} failed: {st}")
        return out

    def probe_texture(self, pixels, linear, q):
        """eval_texture of one texture, pixels (H, W, 4) uint8 or float32, at the rows of
        q (n, 3) = (u, v, as_linear): (n, 4) float32."""
        pixels = np.ascontiguousarray(pixels)
        H, W = pixels.shape[:2]
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        out = np.empty((len(q), 4), np.float32)
        f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        pb = pixels.ctypes.data_as(u8p) if pixels.dtype == np.uint8 else None
        pf = pixels.ctypes.data_as(f32p) if pixels.dtype == np.float32 else None
        assert (pb is None) != (pf is None), pixels.dtype
        st = self.lib.or_probe_texture(W, H, int(bool(linear)), pb, pf, len(q), q.ctypes.data_as(f32p),
                                       out.ctypes.data_as(f32p))
        if st != 0:
            raise RuntimeError(f"oracle texture probe failed: {st}")
        return out

    def query(self, scene_abi, bvh, params, rays, inst=None):
        """The rows of rays (n, 6) = (o, d) through the traversal params.traversal selects (or_query):
        scene queries, or the instance query of inst[i] >= 0. Returns a dict of inst, elem, hit
        (int32), u, v, t (float32), nh (hits accepted by the reporting run, unsaturated), nodes,
        instances, prims (int64), each of length n."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        ids = np.empty((n, 3), np.int32)
        uvt = np.empty((n, 3), np.float32)
        cnt = np.empty((n, 4), np.int64)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        ip = None
        if inst is not None:
            inst = np.ascontiguousarray(inst, np.int32)
            assert inst.shape == (n,)
            ip = inst.ctypes.data_as(i32p)
        st = self.lib.or_query(scene_abi.ref, C.byref(bvh.struct), C.byref(params), n, rays.ctypes.data_as(f32p), ip,
                               ids.ctypes.data_as(i32p), uvt.ctypes.data_as(f32p), cnt.ctypes.data_as(C.POINTER(C.c_int64)))
        if st != 0:
            raise RuntimeError(f"oracle query failed: {st}")
        return {"inst": ids[:, 0].copy(), "elem": ids[:, 1].copy(), "hit": ids[:, 2].copy(), "u": uvt[:, 0].copy(),
                "v": uvt[:, 1].copy(), "t": uvt[:, 2].copy(), "nh": cnt[:, 0].copy(), "nodes": cnt[:, 1].copy(),
                "instances": cnt[:, 2].copy(), "prims": cnt[:, 3].copy()}

    def query_brute(self, scene_abi, rays, inst=None, cap=8):
        """The closest hit without a BVH (or_query_brute): t (n,) float32 (inf: a miss), nmin (n,)
        the number of (instance, element) pairs that reach it, mins (n, cap, 2) the first of them."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        t = np.empty(n, np.float32)
        nmin = np.zeros(n, np.int32)
        mins = np.full((n, cap, 2), -1, np.int32)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        ip = None
        if inst is not None:
            inst = np.ascontiguousarray(inst, np.int32)
            ip = inst.ctypes.data_as(i32p)
        st = self.lib.or_query_brute(scene_abi.ref, n, rays.ctypes.data_as(f32p), ip, t.ctypes.data_as(f32p),
                                     nmin.ctypes.data_as(i32p), mins.ctypes.data_as(i32p), cap)
        if st != 0:
            raise RuntimeError(f"oracle brute-force query failed: {st}")
        return t, nmin, mins

    def instance_ray(self, frame, o, d):
        """The ray an instance visit traces (or_instance_ray): (o, d) in the instance's space."""
        f32p = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32) for x in (frame, o, d)]
        out = np.empty(6, np.float32)
        self.lib.or_instance_ray(a[0].ctypes.data_as(f32p), a[1].ctypes.data_as(f32p), a[2].ctypes.data_as(f32p),
                                 out.ctypes.data_as(f32p))
        return out[:3], out[3:]

    def intersect_bbox(self, o, d, tmin, tmax, bmin, bmax):
        """The reference's slab test (or_intersect_bbox), 1/d computed as the traversal computes it."""
        f32p = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32) for x in (o, d, bmin, bmax)]
        return bool(self.lib.or_intersect_bbox(a[0].ctypes.data_as(f32p), a[1].ctypes.data_as(f32p), float(tmin), float(tmax),
                                               a[2].ctypes.data_as(f32p), a[3].ctypes.data_as(f32p)))

    def srgb_lut(self):
        """srgb_to_rgb(byte / 255) of every byte (src/color.jl:12-23), float32."""
        b = np.arange(256, dtype=np.uint8)
        out = np.empty(256, np.float32)
        self.lib.or_srgb_to_rgb(b.ctypes.data_as(C.POINTER(C.c_uint8)), 256, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def wide_check(self, bvh):
        """The wide records of every tree of `bvh` (JT_TRAVERSAL_WIDE): dict of records,
        non-conservative children (must be 0), leaves, mean dequantised/exact box volume ratio."""
        out = (C.c_int64 * 4)()
        b = bvh.struct
        st = self.lib.or_wide_check(C.byref(b.tlas), b.blas, b.nshapes, out)
        if st != 0:
            raise RuntimeError(f"oracle wide check failed: {st}")
        return {"records": out[0], "violations": out[1], "leaves": out[2], "volume_ratio": out[3] / 1000.0}

    def trace(self, scene_abi, bvh, lights, params, width, height, s0, s1, first=0, rows=None,
              nthreads=None, state=None, streams=1, parts=None, env_alias=False):
        """Returns (image (H,W,4), albedo (H,W,3), normal (H,W,3), hits (H,W), counters).

        streams: the sample streams per pixel k (a power of two, the library's jt_get_streams;
        include/jtrace.h jt_trace_range states the contract). For k > 1 the streams' running
        means are kept in `parts` (a dict of arrays, created when None and filled in place), which
        a caller passes again to continue the same render with a later range.

        env_alias: restate the library's env_alias option (environment texels drawn through
        alias tables, oracle/jt_oracle.c) for this call."""
        if params.traversal not in (0, 1, 2):
            raise ValueError(f"the oracle restates an explicit BVH order (0 reference, 1 near, 2 wide), got "
                             f"{params.traversal}: resolve auto (3) to the order the library ran first")
        k = int(streams)
        if k < 1 or k > 64 or k & (k - 1):
            raise ValueError(f"streams must be a power of two in [1, 64], got {streams}")
        lk = k.bit_length() - 1
        if nthreads is None:
            nthreads = min(16, os.cpu_count() or 1)
        if state is None:
            image = np.zeros((height, width, 4), np.float32)
            albedo = np.zeros((height, width, 3), np.float32)
            normal = np.zeros((height, width, 3), np.float32)
            hits = np.zeros((height, width), np.int64)
        else:
            image, albedo, normal, hits = state
        f32p = C.POINTER(C.c_float)
        i64p = C.POINTER(C.c_int64)
        if lk > 0:
            if parts is None:
                parts = {}
            if not parts:
                parts.update(img=np.zeros((k, height, width, 4), np.float32),
                             alb=np.zeros((k, height, width, 3), np.float32),
                             nrm=np.zeros((k, height, width, 3), np.float32),
                             hits=np.zeros((k, height, width), np.int64))
            pp = (parts["img"].ctypes.data_as(f32p), parts["alb"].ctypes.data_as(f32p),
                  parts["nrm"].ctypes.data_as(f32p), parts["hits"].ctypes.data_as(i64p))
        else:
            pp = (None, None, None, None)
        r0, r1 = rows if rows is not None else (0, height)
        cnt = Counters()
        self.lib.or_set_env_alias(int(bool(env_alias)))
        try:
            st = self._trace_rows(scene_abi, bvh, lights, params, width, height, r0, r1, first, s0, s1, image, albedo,
                                  normal, hits, lk, pp, nthreads, cnt)
        finally:
            self.lib.or_set_env_alias(0)
        if st != 0:
            raise RuntimeError(f"oracle trace failed: {st}")
        return image, albedo, normal, hits, cnt.as_dict()

    def _trace_rows(self, scene_abi, bvh, lights, params, width, height, r0, r1, first, s0, s1, image, albedo,
                    normal, hits, lk, pp, nthreads, cnt):
        f32p = C.POINTER(C.c_float)
        i64p = C.POINTER(C.c_int64)
        return self.lib.or_trace_rows(scene_abi.ref, C.byref(bvh.struct), C.byref(lights.struct), C.byref(params),
                                    width, height, r0, r1, first, s0, s1, image.ctypes.data_as(f32p),
                                    albedo.ctypes.data_as(f32p), normal.ctypes.data_as(f32p),
                                    hits.ctypes.data_as(i64p), lk, *pp, nthreads, C.byref(cnt))


    def order_diff(self, scene_abi, bvh, lights, params, alt_traversal, width, height, s0, s1, nthreads=None):
        """Diagnostic: trace [s0, s1) in params.traversal and compare every closest-hit scene query
        with the same query in alt_traversal (oracle/jt_oracle.c or_order_diff)."""
        if nthreads is None:
            nthreads = min(16, os.cpu_count() or 1)
        d = (C.c_uint64 * 10)()
        st = self.lib.or_order_diff(scene_abi.ref, C.byref(bvh.struct), C.byref(lights.struct), C.byref(params),
                                    alt_traversal, width, height, s0, s1, nthreads, d)
        if st != 0:
            raise RuntimeError(f"oracle order_diff failed: {st}")
        keys = ("queries", "same", "tie", "alt_only_hit", "ref_only_hit", "alt_closer", "alt_farther", "paths_differing")
        return {k: int(d[i]) for i, k in enumerate(keys)}


class _Owned:
    def __init__(self, struct, free):
        self.struct = struct
        self._free = free

    @property
    def ref(self):
        return C.byref(self.struct)

    def __del__(self):
        try:
            self._free(C.byref(self.struct))
        except Exception:
            pass
