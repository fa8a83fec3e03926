"""Ray queries: the scenes, the seeded ray classes and the binding of the device query probe
(tests/probe/jt_query.hip), shared by tests/test_queries_host.py (CPU: the oracle's or_query against
the brute force or_query_brute) and tests/test_gpu_queries.py (the product's traversal functions
against or_query, bit for bit).

Every ray class comes from rays(ctx, cls): seeded, N rays (odd: the last wave of a launch is
partial), float32, no NaN and no infinite component. The same array serves the CPU and the GPU
tests.
"""
from __future__ import annotations

import ctypes as C
import functools
import zlib
from pathlib import Path

import numpy as np

import scenes_ref as SR

ROOT = Path(__file__).resolve().parent.parent
QUERY_LIB = ROOT / "julia-raytracer_amd" / "build" / "libjt_query.so"
CORNELL = str(ROOT / "assets" / "scenes" / "cornellbox" / "cornellbox.json")
F32 = np.float32
N = 4099
ORDERS = ("reference", "near", "wide")

NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("start", "<i4"), ("num", "<i2"), ("axis", "i1"),
                 ("internal", "i1")])

SCENES = ("cornell", "random", "quads9", "strip", "coplanar", "twins", "deep", "plates")
# every class runs on every scene, except stacked: the plates scene only
CLASSES = ("generic", "axis", "planar", "tiny", "edges", "surface", "outside")
CASES = [(s, c) for s in SCENES for c in CLASSES] + [("plates", "stacked")]
# the classes whose excused share (tests/test_queries_host.py) is capped at the image tests' 0.1 %
CAPPED = ("generic", "outside")


# The (scene, class, order) cases where an order's hits differ from the reference order's on the CPU
# (oracle against oracle; tests/test_queries_host.py prints the counts and proves each ray's cause).
# The causes are the reference's own: its slab test rejects a box that holds the hit (0 * inf = NaN
# for an axis-parallel ray from an origin on a box plane; rounding at a box edge), and which boxes it
# asks depends on the order (tmax has shrunk or not) and on the planes (the wide records' quantised
# boxes are larger and their planes differ). SURVEY.md Appendix B lists them. The device reproduces
# each order's own result bit for bit (tests/test_gpu_queries.py), so these are pinned, not fixed.
ORDER_DIFFS = {
    ("cornell", "axis", "wide"), ("cornell", "planar", "wide"), ("random", "edges", "wide"), ("strip", "axis", "wide"),
    ("strip", "planar", "wide"), ("strip", "edges", "near"), ("coplanar", "axis", "wide"), ("coplanar", "planar", "wide"),
    ("coplanar", "edges", "wide"), ("twins", "edges", "wide"), ("plates", "edges", "wide"),
}


def build_scene(name):
    from jtrace import sceneio
    if name == "cornell":
        return sceneio.load_scene(CORNELL)
    if name == "coplanar":
        return SR.coplanar_tie_scene(sceneio.load_scene(CORNELL))
    return {"random": SR.random_instanced_scene, "quads9": lambda: SR.quad_scene(9, False, SR.SEEDS[9]),
            "strip": SR.strip_scene, "twins": SR.twin_scene, "deep": SR.deep_scene, "plates": SR.plates_scene}[name]()


def tree_nodes(tree):
    return np.ctypeslib.as_array(C.cast(tree.nodes, C.POINTER(C.c_uint8)), shape=(tree.nnodes * 32,)).view(NODE).copy()


def tree_prims(tree):
    return np.ctypeslib.as_array(tree.primitives, shape=(tree.nprimitives,)).copy() if tree.nprimitives else np.zeros(0, np.int32)


class Tree:
    """One tree of a jt_scene_bvh as arrays: its nodes, each node's parent, each primitive's leaf."""

    def __init__(self, tree):
        self.nodes, self.prims = tree_nodes(tree), tree_prims(tree)
        self.parent = np.full(len(self.nodes), -1)
        self.leaf_of = {}
        for k, n in enumerate(self.nodes):
            if n["internal"]:
                self.parent[n["start"]] = self.parent[n["start"] + 1] = k
            else:
                for p in self.prims[n["start"]:n["start"] + n["num"]]:
                    self.leaf_of[int(p)] = k

    def path(self, prim):
        """The nodes from the root to the leaf that lists primitive `prim`."""
        k, out = self.leaf_of[prim], []
        while k >= 0:
            out.append(k)
            k = self.parent[k]
        return out[::-1]


class Context:
    """A scene with what the tests and the ray classes need of it (built once per scene)."""

    def __init__(self, name, abi, oracle):
        from conftest import make_params
        self.name, self.abi = name, abi
        self.scene = build_scene(name)
        self.sa = abi.SceneABI(self.scene)
        self.bvh = oracle.build_bvh(self.sa)
        self.lights = oracle.make_lights(self.sa)
        self.params = {o: make_params(abi, traversal=o) for o in ORDERS}
        self.ninst = len(self.scene.instances)
        self.tlas = Tree(self.bvh.struct.tlas)
        self.blas = [Tree(self.bvh.struct.blas[k]) for k in range(self.bvh.struct.nshapes)]
        # world-space float32 vertices per instance, and the elements as vertex tuples
        self.verts, self.elems = [], []
        for inst in self.scene.instances:
            f = np.asarray(inst.frame, np.float64).reshape(4, 3)
            sh = self.scene.shapes[inst.shape]
            w = (np.asarray(sh.positions, np.float64) @ f[:3] + f[3]).astype(F32)
            self.verts.append(w)
            idx = sh.triangles if len(sh.triangles) else sh.quads
            self.elems += [w[list(e)] for e in idx]
        allv = np.concatenate(self.verts)
        self.lo, self.hi = allv.min(0).astype(np.float64), allv.max(0).astype(np.float64)
        # coordinates a ray origin can sit on exactly: per axis, every TLAS / BLAS node plane and vertex
        planes = [self.tlas.nodes] + [b.nodes for b in self.blas]
        self.coords = [np.unique(np.concatenate([allv[:, a]] + [p["bmin"][:, a] for p in planes] + [p["bmax"][:, a] for p in planes]))
                       for a in range(3)]
        self.coords = [c[np.isfinite(c)] for c in self.coords]

    def rng(self, cls):
        return np.random.default_rng(zlib.crc32(f"{self.name}/{cls}".encode()))


@functools.lru_cache(maxsize=None)
def _context(name, abi, oracle):
    return Context(name, abi, oracle)


def context(name, abi, oracle):
    return _context(name, abi, oracle)


# ------------------------------------------------------------------------------ the ray classes
def _sphere(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _box_origins(ctx, rng, n, scale=1.5):
    c, h = (ctx.lo + ctx.hi) / 2, np.maximum((ctx.hi - ctx.lo) / 2, 1e-3)
    return c + rng.uniform(-1, 1, size=(n, 3)) * h * scale


def _snapped_origins(ctx, rng, n):
    """Origins in 1.5 x the bounds; every other one has one coordinate taken verbatim from a BVH
    node's bmin / bmax or from a vertex."""
    o = _box_origins(ctx, rng, n).astype(F32)
    for i in range(0, n, 2):
        a = int(rng.integers(3))
        o[i, a] = rng.choice(ctx.coords[a])
    return o


def _finish(o, d):
    r = np.concatenate([np.asarray(o, F32), np.asarray(d, F32)], 1)
    assert r.shape == (N, 6) and np.isfinite(r).all()
    return np.ascontiguousarray(r)


def _generic(ctx, rng):
    return _finish(_box_origins(ctx, rng, N), _sphere(rng, N))


def _axis(ctx, rng):
    """Directions exactly +-e_x, +-e_y, +-e_z; each zero component is +0.0 or -0.0 (all four sign
    pairs occur for every axis)."""
    d = np.zeros((N, 3), F32)
    k = np.arange(N)
    a = k % 3
    d[k, a] = np.where((k // 3) % 2, F32(-1), F32(1))
    z1 = np.where((k // 6) % 2, F32(-0.0), F32(0.0))
    z2 = np.where((k // 12) % 2, F32(-0.0), F32(0.0))
    d[k, (a + 1) % 3] = z1
    d[k, (a + 2) % 3] = z2
    return _finish(_snapped_origins(ctx, rng, N), d)


def _planar(ctx, rng):
    d = _sphere(rng, N).astype(F32)
    k = np.arange(N)
    d[k, k % 3] = np.where((k // 3) % 2, F32(-0.0), F32(0.0))
    return _finish(_snapped_origins(ctx, rng, N), d)


def _tiny(ctx, rng):
    """One direction component is +-2^e, e from -100 down through the denormals (-149): 1 / d is huge
    (up to 2^126 and, for the denormals below 2^-128, infinite)."""
    d = _sphere(rng, N).astype(F32)
    k = np.arange(N)
    e = -100 - (k // 3) % 50
    d[k, k % 3] = (np.ldexp(1.0, e) * np.where((k // 150) % 2, -1, 1)).astype(F32)
    assert (d[k, k % 3] != 0).all()
    return _finish(_box_origins(ctx, rng, N), d)


def _edges(ctx, rng):
    """From random origins towards float32 vertices, edge midpoints and the shared diagonal of every
    quad and two-triangle pair (consecutive triangles that share two vertices)."""
    targets = []
    for e in ctx.elems:
        m = len(e)
        targets += [e[j] for j in range(m)] + [(e[j].astype(np.float64) + e[(j + 1) % m]) / 2 for j in range(m)]
        if m == 4:  # the diagonal p2-p4 the reference splits a quad along (src/geometry.jl:238-258)
            targets += [(e[1].astype(np.float64) + e[3]) / 2, e[1] * 0.25 + e[3].astype(np.float64) * 0.75]
    for a, b in zip(ctx.elems[:-1], ctx.elems[1:]):
        if len(a) == 3 and len(b) == 3:
            shared = [p for p in a if any((p == q).all() for q in b)]
            if len(shared) == 2:
                targets += [(shared[0].astype(np.float64) + shared[1]) / 2, shared[0] * 0.3 + shared[1].astype(np.float64) * 0.7]
    targets = np.asarray(targets, np.float64)
    t = targets[rng.integers(len(targets), size=N)]
    o = _box_origins(ctx, rng, N).astype(F32)
    d = t - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    bad = ~np.isfinite(d).all(1) | (np.abs(d).sum(1) == 0)
    d[bad] = [0, 0, 1]
    return _finish(o, d)


def _surface(ctx, rng, oracle):
    """Origins are the float32 hit points o + t d of generic rays, as a bounce ray starts: a third of
    the directions random, a third into the surface (the incoming direction goes on through it), a
    third within 1e-3 of the tangent plane."""
    g = _generic(ctx, ctx.rng("surface/seed"))
    q = oracle.query(ctx.sa, ctx.bvh, ctx.params["reference"], g)
    hit = np.flatnonzero(q["hit"] != 0)
    assert len(hit) > 50, (ctx.name, len(hit))
    pick = hit[rng.integers(len(hit), size=N)]
    o = (g[pick, :3] + q["t"][pick, None] * g[pick, 3:]).astype(F32)
    # the geometric normal of the hit element
    off = np.cumsum([0] + [len(s.triangles) if len(s.triangles) else len(s.quads)
                           for s in (ctx.scene.shapes[i.shape] for i in ctx.scene.instances)])
    e = [ctx.elems[off[i] + k].astype(np.float64) for i, k in zip(q["inst"][pick], q["elem"][pick])]
    nrm = np.array([np.cross(v[1] - v[0], v[-1] - v[0]) for v in e])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    d = _sphere(rng, N)
    k = np.arange(N) % 3
    d[k == 1] = g[pick[k == 1], 3:]
    tang = d - (d * nrm).sum(1, keepdims=True) * nrm
    tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-12)
    graze = tang + nrm * rng.uniform(-1e-3, 1e-3, size=(N, 1))
    d[k == 2] = graze[k == 2]
    bad = ~np.isfinite(d).all(1) | (np.abs(d).sum(1) == 0)
    d[bad] = [0, 0, 1]
    return _finish(o, d)


def _outside(ctx, rng):
    """Origins 20 to 1000 scene radii away; every other ray points away from the scene (a miss)."""
    c, r = (ctx.lo + ctx.hi) / 2, np.linalg.norm(ctx.hi - ctx.lo) / 2
    u = _sphere(rng, N)
    o = c + u * r * np.exp(rng.uniform(np.log(20), np.log(1000), size=(N, 1)))
    t = _box_origins(ctx, rng, N, scale=1.0)
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1::2] *= -1
    return _finish(o, d)


def _stacked(ctx, rng):
    """Along +-z, the plates' axis, through all of them: exactly axial, and slightly tilted."""
    o = np.stack([rng.uniform(-0.95, 0.95, N), rng.uniform(-0.95, 0.95, N), np.where(np.arange(N) % 2, 4.0, -4.0)], 1)
    d = np.zeros((N, 3))
    d[:, 2] = np.where(np.arange(N) % 2, -1.0, 1.0)
    tilt = (np.arange(N) // 2) % 2 == 1
    d[tilt, :2] = rng.uniform(-1e-3, 1e-3, size=(int(tilt.sum()), 2))
    return _finish(o, d)


_rays = {}


def rays(ctx, cls, oracle=None):
    """The class's rays for the scene, (N, 6) float32 (o, d). `oracle` is needed by surface only."""
    key = (ctx.name, cls)
    if key not in _rays:
        rng = ctx.rng(cls)
        fn = {"generic": _generic, "axis": _axis, "planar": _planar, "tiny": _tiny, "edges": _edges, "outside": _outside,
              "stacked": _stacked}.get(cls)
        _rays[key] = _surface(ctx, rng, oracle) if cls == "surface" else fn(ctx, rng)
        _rays[key].setflags(write=False)
    return _rays[key]


def instance_ids(ctx):
    """The instance of ray i's instance query: the instances in turn."""
    return (np.arange(N) % ctx.ninst).astype(np.int32)


# ------------------------------------------------------------------------------ the device probe
class QueryProbe:
    """ctypes binding of libjt_query.so (tests/probe/jt_query.hip)."""

    def __init__(self, path=None):
        import os
        path = path or os.environ.get("JT_QUERY_LIB") or QUERY_LIB  # another build: the mutation record
        if not Path(path).exists():
            raise FileNotFoundError(f"{path} is missing: build it with make -C tests/probe (build() does)")
        self.lib = lib = C.CDLL(str(path))
        lib.jq_form_name.argtypes = [C.c_int]
        lib.jq_form_name.restype = C.c_char_p
        lib.jq_last_error.restype = C.c_char_p
        lib.jq_form_skip.argtypes = [C.c_void_p, C.c_int]
        lib.jq_form_skip.restype = C.c_char_p
        lib.jq_close.argtypes = [C.c_void_p]
        lib.jq_close.restype = None
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        lib.jq_info.argtypes = [C.c_void_p, i32p]
        lib.jq_leaf_roots.argtypes = [C.c_void_p, i32p]
        lib.jq_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, f32p, i32p, i32p]
        lib.jq_run_leaf.argtypes = [C.c_void_p, C.c_int, C.c_int64, f32p, i32p, i32p]
        self.forms = [lib.jq_form_name(k).decode() for k in range(lib.jq_form_count())]
        self.words, self.state_words = lib.jq_out_words(), lib.jq_state_words()

    def _scene_args(self, ctx, order):
        return ctx.sa.ref, C.byref(ctx.bvh.struct), C.byref(ctx.lights.struct), C.byref(ctx.params[order])

    def layout_info(self, ctx, order):
        """The host layout alone (no device): dict of need, feat, blob bytes."""
        info = (C.c_int32 * 3)()
        st = self.lib.jq_layout_info(*self._scene_args(ctx, order), info)
        if st != 0:
            raise RuntimeError(f"layout of {ctx.name}/{order}: {st} {self.lib.jq_last_error().decode()}")
        return {"need": info[0], "feat": info[1], "blob": info[2]}

    def open(self, ctx, order):
        h = C.c_void_p()
        st = self.lib.jq_open(*self._scene_args(ctx, order), C.byref(h))
        if st != 0:
            raise RuntimeError(f"jq_open {ctx.name}/{order}: {st} {self.lib.jq_last_error().decode()}")
        return DeviceScene(self, h, ctx)


class DeviceScene:
    def __init__(self, probe, h, ctx):
        self.probe, self.h, self.ctx = probe, h, ctx
        info = (C.c_int32 * 7)()
        probe.lib.jq_info(h, info)
        self.need, self.feat, self.wide, self.order_flip, self.blob, self.ninst, self.special = list(info)
        roots = np.zeros(max(self.ninst, 1), np.int32)
        probe.lib.jq_leaf_roots(h, roots.ctypes.data_as(C.POINTER(C.c_int32)))
        self.leaf_roots = np.flatnonzero(roots[:self.ninst])

    def close(self):
        if self.h:
            self.probe.lib.jq_close(self.h)
            self.h = None

    def skip_reason(self, form):
        r = self.probe.lib.jq_form_skip(self.h, self.probe.forms.index(form))
        return r.decode() if r else None

    def run(self, form, rays, inst=None, ring=16):
        """The rays through one traversal form: dict of inst, elem, hit, nh63, nodes, instances,
        prims, maxsp, flags (int32) and u, v, t (float32)."""
        rays = np.ascontiguousarray(rays, F32)
        n = len(rays)
        out = np.empty((n, self.probe.words), np.int32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        ip = np.ascontiguousarray(inst, np.int32).ctypes.data_as(i32p) if inst is not None else None
        st = self.probe.lib.jq_run(self.h, self.probe.forms.index(form), ring, n, rays.ctypes.data_as(f32p), ip,
                                   out.ctypes.data_as(i32p))
        if st != 0:
            what = "stack guard changed / step cap / sp above the bound, flags" if st >= 2000 else "status"
            raise RuntimeError(f"jq_run {form} ring={ring}: {what} {st - 2000 if st >= 2000 else st}")
        f = lambda k: out[:, k].copy().view(F32)
        return {"inst": out[:, 0].copy(), "elem": out[:, 1].copy(), "u": f(2), "v": f(3), "t": f(4), "hit": out[:, 5].copy(),
                "nh63": out[:, 6].copy(), "nodes": out[:, 7].copy(), "instances": out[:, 8].copy(), "prims": out[:, 9].copy(),
                "maxsp": out[:, 10].copy(), "flags": out[:, 11].copy()}

    def run_leaf(self, baked, rays, inst):
        """(state after query_start + node_step, state after inst_leaf_query), each (n, words) int32."""
        rays = np.ascontiguousarray(rays, F32)
        n, w = len(rays), self.probe.state_words
        out = np.empty((n, 2, w), np.int32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        st = self.probe.lib.jq_run_leaf(self.h, int(baked), n, rays.ctypes.data_as(f32p),
                                        np.ascontiguousarray(inst, np.int32).ctypes.data_as(i32p), out.ctypes.data_as(i32p))
        if st != 0:
            raise RuntimeError(f"jq_run_leaf baked={baked}: status {st}")
        return out[:, 0], out[:, 1]


def same_bits(a, b):
    return np.ascontiguousarray(a, F32).view(np.uint32) == np.ascontiguousarray(b, F32).view(np.uint32)
