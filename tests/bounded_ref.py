"""Bounded ray queries restated: intersect_scene_bvh / intersect_instance_bvh of
Ray3f(o, d, ray_eps, tmax) (src/bvh.jl:306-520) in the reference and the near child order, with the
near order's tie re-run and its one-leaf-instance exemption, over the oracle-built BVH arrays that
queries_ref.Tree exposes.

The oracle's or_query starts every ray at tmax = +inf, so a caller's bound needs a reference of its
own. This one has no arithmetic of its own: every box test is a row of or_probe's `bbox`
(intersect_bbox), every primitive test a row of `triangle` / `quad` (intersect_triangle,
intersect_quad, which apply tmin <= t <= tmax themselves), the instance-space ray is
or_instance_ray's, and 1 / d is a float32 division. What is restated is the control flow only: the
stack, the push order by the sign of d[axis], a TLAS leaf's instances and a BLAS leaf's primitives
in order, tmax shrinking at every accepted hit, and the tie note (t == tmax at an accepted hit).
tests/test_bounded_host.py holds it to or_query bit for bit at tmax = +inf before it judges anything.

Vectorised over the rays: one step of every ray in flight per iteration (a primitive test for a ray
inside a leaf, else one stack pop), one or_probe call per step kind. The scene query's recursion
into intersect_shape_bvh is flattened onto one stack: a shape's entries drain before anything below
them is popped, and the shape query's copy of tmax and the scene query's are always equal where
either is read (the scene's is set to the shape's result), so one tmax per ray serves both.

The wide order is not restated: its quantised boxes are made inside the product and the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

F32 = np.float32
RAY_EPS = F32(0.0001)  # src/geometry.jl:34
T_TLAS, T_INST, T_BLAS = 0, 1, 2
SHIFT = 1 << 32
DEPTH = 256  # entries of the flattened stack (or_query's two stacks hold 128 each)


class Flat:
    """A queries_ref.Context's scene and BVH as flat arrays: every BLAS's nodes, primitive slots and
    elements in one array each, addressed through per-shape offsets."""

    def __init__(self, ctx):
        sc = ctx.scene
        self.tl = ctx.tlas.nodes
        self.tl_prims = ctx.tlas.prims.astype(np.int64)
        self.shape = np.array([i.shape for i in sc.instances], np.int64)
        self.frames = [np.ascontiguousarray(np.asarray(i.frame, F32).reshape(12)) for i in sc.instances]
        nodes, prims, tris, quads = [], [], [np.zeros((0, 9), F32)], [np.zeros((0, 12), F32)]
        self.node_off, self.nnodes, self.root_internal, self.kind, self.elem_off = [], [], [], [], []
        nn = npr = nt = nq = 0
        for k, b in enumerate(ctx.blas):
            sh = sc.shapes[k]
            pos = np.asarray(sh.positions, F32).reshape(-1, 3)
            nd = b.nodes.copy()
            nd["start"] += np.where(nd["internal"] != 0, nn, npr).astype(np.int32)
            self.node_off.append(nn)
            self.nnodes.append(len(nd))
            self.root_internal.append(bool(len(nd) and nd["internal"][0]))
            nodes.append(nd)
            prims.append(b.prims.astype(np.int64))
            nn += len(nd)
            npr += len(b.prims)
            if len(sh.triangles):
                self.kind.append(0)
                self.elem_off.append(nt)
                tris.append(pos[np.asarray(sh.triangles, np.int64).reshape(-1, 3)].reshape(-1, 9))
                nt += len(tris[-1])
            elif len(sh.quads):
                self.kind.append(1)
                self.elem_off.append(nq)
                quads.append(pos[np.asarray(sh.quads, np.int64).reshape(-1, 4)].reshape(-1, 12))
                nq += len(quads[-1])
            else:
                self.kind.append(-1)
                self.elem_off.append(0)
        self.bl = np.concatenate(nodes) if nodes else self.tl[:0]
        self.prims = np.concatenate(prims) if prims else np.zeros(0, np.int64)
        self.tris, self.quads = np.concatenate(tris), np.concatenate(quads)
        for k in ("node_off", "nnodes", "root_internal", "kind", "elem_off"):
            setattr(self, k, np.asarray(getattr(self, k)))


_flat = {}


def flat(ctx):
    if ctx.name not in _flat:
        _flat[ctx.name] = Flat(ctx)
    return _flat[ctx.name]


class Probes:
    """or_probe rows by name, the op table read once."""

    def __init__(self, oracle):
        self.lib = oracle.lib
        self.ops = {name: (k, nin, nout) for k, (name, nin, nout) in enumerate(oracle.probe_ops())}
        assert self.ops["bbox"][1:] == (14, 1) and self.ops["triangle"][1:] == (17, 12) and self.ops["quad"][1:] == (20, 4)

    def __call__(self, op, x):
        k, nin, nout = self.ops[op]
        x = np.ascontiguousarray(x, F32)
        assert x.shape[1] == nin
        out = np.empty((len(x), nout), F32)
        f32p = C.POINTER(C.c_float)
        assert self.lib.or_probe(k, len(x), x.ctypes.data_as(f32p), out.ctypes.data_as(f32p)) == 0
        return out


def _col(n, v):
    return np.full((n, 1), v, F32)


def _run(F, probe, rays, inst, bound, flip):
    """One traversal of every ray: `flip` True visits the near child first. Returns or_query's
    fields (a miss is instance = element = -1, u = v = t = 0) and the tie flags."""
    n = len(rays)
    f32p = C.POINTER(C.c_float)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    with np.errstate(divide="ignore", over="ignore"):
        dinv = F32(1) / d
    wsign = ((d < 0) ^ bool(flip)).astype(np.int64)
    lo, ld, ldinv, lsign = o.copy(), d.copy(), dinv.copy(), wsign.copy()
    stack = np.zeros((n, DEPTH), np.int64)
    sp = np.zeros(n, np.int64)
    sq = inst < 0
    if len(F.tl):
        sp[sq] = 1  # entry 0: TLAS node 0
    stack[~sq, 0] = T_INST * SHIFT + inst[~sq]
    sp[~sq] = 1
    tmax = np.array(bound, F32)
    h_inst, h_elem = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    h_u, h_v = np.zeros(n, F32), np.zeros(n, F32)
    hit, tie = np.zeros(n, bool), np.zeros(n, bool)
    cur_inst = np.zeros(n, np.int64)
    pcur, pleft = np.zeros(n, np.int64), np.zeros(n, np.int64)
    local = np.empty(6, F32)
    while True:
        A = np.flatnonzero(pleft > 0)
        B = np.flatnonzero((pleft == 0) & (sp > 0))
        if not len(A) and not len(B):
            break
        # ---- the next primitive of the current leaf (src/bvh.jl:444-484)
        if len(A):
            kind = F.kind[F.shape[cur_inst[A]]]
            for k, op, verts in ((0, "triangle", F.tris), (1, "quad", F.quads)):
                S = A[kind == k]
                if not len(S):
                    continue
                elem = F.prims[pcur[S]]
                x = np.concatenate([lo[S], ld[S], _col(len(S), RAY_EPS), tmax[S, None], verts[elem + F.elem_off[F.shape[cur_inst[S]]]]], 1)
                y = probe(op, x)
                acc = y[:, 3] != 0
                Sa, t = S[acc], y[acc, 2]
                tie[Sa] |= t == tmax[Sa]
                h_inst[Sa], h_elem[Sa], h_u[Sa], h_v[Sa] = cur_inst[Sa], elem[acc], y[acc, 0], y[acc, 1]
                tmax[Sa] = t
                hit[Sa] = True
            pcur[A] += 1
            pleft[A] -= 1
        if not len(B):
            continue
        sp[B] -= 1
        e = stack[B, sp[B]]
        typ, idx = e // SHIFT, e % SHIFT
        # ---- an instance visit (src/bvh.jl:345-351, 502-506): the ray into its space, its BLAS root pushed
        I, ii = B[typ == T_INST], idx[typ == T_INST]
        for r, k in zip(I, ii):
            probe.lib.or_instance_ray(F.frames[k].ctypes.data_as(f32p), o[r].ctypes.data_as(f32p), d[r].ctypes.data_as(f32p),
                                      local.ctypes.data_as(f32p))
            lo[r], ld[r] = local[:3], local[3:]
        if len(I):
            with np.errstate(divide="ignore", over="ignore"):
                ldinv[I] = F32(1) / ld[I]
            lsign[I] = (ld[I] < 0) ^ bool(flip)
            cur_inst[I] = ii
            shp = F.shape[ii]
            has = F.nnodes[shp] > 0
            stack[I[has], sp[I[has]]] = T_BLAS * SHIFT + F.node_off[shp[has]]
            sp[I[has]] += 1
        # ---- a node: the box test, then the children by the sign of d[axis], or the leaf
        for tk, nodes, ro, rdinv, rsign in ((T_TLAS, F.tl, o, dinv, wsign), (T_BLAS, F.bl, lo, ldinv, lsign)):
            M, ni = B[typ == tk], idx[typ == tk]
            if not len(M):
                continue
            nd = nodes[ni]
            ok = probe("bbox", np.concatenate([ro[M], rdinv[M], _col(len(M), RAY_EPS), tmax[M, None], nd["bmin"], nd["bmax"]], 1))[:, 0] != 0
            M, nd = M[ok], nd[ok]
            internal = nd["internal"] != 0
            Mi, ndi = M[internal], nd[internal]
            s = rsign[Mi, ndi["axis"].astype(np.int64)]
            c0 = ndi["start"].astype(np.int64)
            stack[Mi, sp[Mi]] = tk * SHIFT + np.where(s == 0, c0, c0 + 1)
            stack[Mi, sp[Mi] + 1] = tk * SHIFT + np.where(s == 0, c0 + 1, c0)
            sp[Mi] += 2
            Ml, ndl = M[~internal], nd[~internal]
            start, num = ndl["start"].astype(np.int64), ndl["num"].astype(np.int64)
            if tk == T_BLAS:
                pcur[Ml], pleft[Ml] = start, num
            else:  # a TLAS leaf's instances, pushed last first so that they are visited in order
                for k in range(int(num.max()) if len(num) else 0):
                    sel = num > k
                    stack[Ml[sel], sp[Ml[sel]]] = T_INST * SHIFT + F.tl_prims[start[sel] + num[sel] - 1 - k]
                    sp[Ml[sel]] += 1
        assert sp.max() < DEPTH - 4, "stack of the restatement"
    return {"inst": h_inst, "elem": h_elem, "hit": hit.astype(np.int32), "u": h_u, "v": h_v,
            "t": np.where(hit, tmax, F32(0)).astype(F32), "tie": tie}


def query(ctx, oracle, order, rays, inst=None, tmax=None):
    """The bounded query of every ray in `order` ("reference" or "near"): or_query's fields (inst,
    elem, hit int32; u, v, t float32; a miss carries t = 0). inst: None, or per ray -1 / an instance
    id; tmax: None (+inf), a scalar or (n,)."""
    assert order in ("reference", "near"), order
    F, probe = flat(ctx), Probes(oracle)
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    n = len(rays)
    inst = np.full(n, -1, np.int64) if inst is None else np.asarray(inst, np.int64)
    bound = np.full(n, np.inf, F32) if tmax is None else np.broadcast_to(np.asarray(tmax, F32), (n,)).copy()
    near = order == "near"
    r = _run(F, probe, rays, inst, bound, near)
    if near:
        # the tie re-run in the reference's child order, with the same bound; an instance query of a
        # one-leaf BLAS tests its leaf in the same order either way and is never re-run
        again = r["tie"] & ((inst < 0) | F.root_internal[F.shape[np.maximum(inst, 0)]])
        k = np.flatnonzero(again)
        if len(k):
            r2 = _run(F, probe, rays[k], inst[k], bound[k], False)
            for f in ("inst", "elem", "hit", "u", "v", "t"):
                r[f][k] = r2[f]
    return r


# ------------------------------------------------------------------------------ the bound families
def miss_bounds(ctx, cls, family, n):
    """The seeded finite bound of a ray without a hit: 0.5 to 2 scene diagonals."""
    diag = float(np.linalg.norm(ctx.hi - ctx.lo))
    return (diag * np.exp(ctx.rng(f"{cls}/bound/{family}").uniform(np.log(0.5), np.log(2.0), n))).astype(F32)


def doubled_bounds(ctx, cls, free):
    """2 t_i of the order's own unbounded record `free` (or_query's fields); a miss: miss_bounds."""
    hit = np.asarray(free["hit"]) != 0
    return np.where(hit, F32(2) * np.asarray(free["t"], F32), miss_bounds(ctx, cls, "double", len(hit))).astype(F32)


def family_bounds(ctx, cls, family, free):
    """The bounds of families A, B, C from the order's own unbounded record: A the bits of t_i (a hit
    exactly on the bound), B nextafter(t_i, 0), C t_i * u with u seeded log-uniform in [0.25, 4]; a
    miss takes miss_bounds."""
    hit = np.asarray(free["hit"]) != 0
    t = np.asarray(free["t"], F32)
    n = len(t)
    if family == "A":
        b = t.copy()
    elif family == "B":
        b = np.nextafter(t, F32(0))
    else:
        u = np.exp(ctx.rng(f"{cls}/bound/u").uniform(np.log(0.25), np.log(4.0), n)).astype(F32)
        b = t * u
    return np.where(hit, b, miss_bounds(ctx, cls, family, n)).astype(F32)
