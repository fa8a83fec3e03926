"""The multi-hit queries restated (include/jtrace.h: jt_intersect_multi, jt_count_hits): the control
flow of bounded_ref._run with two changes, over the same flat arrays and the same or_probe rows.

  - a sorted list of at most k records per ray, ordered by the key (t, instance, element), replaces
    the single closest hit; the query's tmax is the caller's bound while the list holds fewer than k
    entries and the k-th entry's t afterwards; there is no tie pass;
  - a no-shrink mode (k = None) counts the accepted primitives with tmax held at the bound.

Beside it the brute force: every element of every instance through or_instance_ray and the
`triangle` / `quad` probe rows at tmax = +inf, sorted by the key. Neither has arithmetic of its own:
every box test is a `bbox` row, every primitive test a `triangle` / `quad` row, the instance-space
ray is or_instance_ray's and 1 / d a float32 division. The wide order is not restated.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from bounded_ref import DEPTH, F32, RAY_EPS, SHIFT, T_BLAS, T_INST, T_TLAS, Probes, _col, flat

INF = F32(np.inf)


def key_less(t, inst, elem, t2, inst2, elem2):
    """(t, instance, element) < (t2, instance2, element2): t as float32, all ascending."""
    return (t < t2) | ((t == t2) & ((inst < inst2) | ((inst == inst2) & (elem < elem2))))


class Lists:
    """Per ray the sorted list of at most k records and its length."""

    def __init__(self, n, k):
        self.k = k
        self.t = np.full((n, k), INF, F32)
        self.u, self.v = np.zeros((n, k), F32), np.zeros((n, k), F32)
        self.inst, self.elem = np.full((n, k), -1, np.int32), np.full((n, k), -1, np.int32)
        self.count = np.zeros(n, np.int64)

    def insert(self, rows, t, inst, elem, u, v):
        """One candidate for each of `rows` (distinct rays). It goes in front of every trailing entry
        it is smaller than, found from the end; a full list drops its last entry, or the candidate.
        Returns the rows whose list is full afterwards and was changed."""
        k, cnt = self.k, self.count[rows]
        j = np.arange(k)[None, :]
        less = key_less(t[:, None], inst[:, None], elem[:, None], self.t[rows], self.inst[rows], self.elem[rows])
        stop = (~less) & (j < cnt[:, None])  # entries the candidate is not smaller than
        pos = np.where(stop.any(1), k - np.argmax(stop[:, ::-1], axis=1), 0)  # one past the last of them
        ins = pos < k
        rows, pos, cnt = rows[ins], pos[ins], cnt[ins]
        src = np.where(j > pos[:, None], j - 1, j)  # entry j afterwards is entry j - 1 behind the new one
        here = j == pos[:, None]
        for name, val in (("t", t), ("inst", inst), ("elem", elem), ("u", u), ("v", v)):
            a = getattr(self, name)
            a[rows] = np.where(here, val[ins][:, None], np.take_along_axis(a[rows], src, axis=1))
        self.count[rows] = np.minimum(cnt + 1, k)
        return rows[self.count[rows] == k]

    def records(self, hit_dtype):
        out = np.zeros(self.t.shape, hit_dtype)
        filled = np.arange(self.k)[None, :] < self.count[:, None]
        out["instance"], out["element"] = np.where(filled, self.inst, -1), np.where(filled, self.elem, -1)
        out["u"], out["v"] = np.where(filled, self.u, F32(0)), np.where(filled, self.v, F32(0))
        out["t"], out["hit"] = np.where(filled, self.t, INF), filled
        return out


def _run(F, probe, rays, inst, bound, flip, k):
    """bounded_ref._run with the list (k: 1 .. 16) or the count (k None) at the accept."""
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
    L = Lists(n, k) if k is not None else None
    total = np.zeros(n, np.int64)
    cur_inst = np.zeros(n, np.int64)
    pcur, pleft = np.zeros(n, np.int64), np.zeros(n, np.int64)
    local = np.empty(6, F32)
    while True:
        A = np.flatnonzero(pleft > 0)
        B = np.flatnonzero((pleft == 0) & (sp > 0))
        if not len(A) and not len(B):
            break
        # ---- the next primitive of the current leaf, against the current tmax
        if len(A):
            kind = F.kind[F.shape[cur_inst[A]]]
            for kk, op, verts in ((0, "triangle", F.tris), (1, "quad", F.quads)):
                S = A[kind == kk]
                if not len(S):
                    continue
                elem = F.prims[pcur[S]]
                x = np.concatenate([lo[S], ld[S], _col(len(S), RAY_EPS), tmax[S, None], verts[elem + F.elem_off[F.shape[cur_inst[S]]]]], 1)
                y = probe(op, x)
                acc = y[:, 3] != 0
                Sa = S[acc]
                if L is None:
                    total[Sa] += 1
                    continue
                full = L.insert(Sa, y[acc, 2], cur_inst[Sa].astype(np.int32), elem[acc].astype(np.int32), y[acc, 0], y[acc, 1])
                tmax[full] = L.t[full, k - 1]
            pcur[A] += 1
            pleft[A] -= 1
        if not len(B):
            continue
        sp[B] -= 1
        e = stack[B, sp[B]]
        typ, idx = e // SHIFT, e % SHIFT
        # ---- an instance visit: the ray into its space, its BLAS root pushed
        I, ii = B[typ == T_INST], idx[typ == T_INST]
        for r, q in zip(I, ii):
            probe.lib.or_instance_ray(F.frames[q].ctypes.data_as(f32p), o[r].ctypes.data_as(f32p), d[r].ctypes.data_as(f32p),
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
                for q in range(int(num.max()) if len(num) else 0):
                    sel = num > q
                    stack[Ml[sel], sp[Ml[sel]]] = T_INST * SHIFT + F.tl_prims[start[sel] + num[sel] - 1 - q]
                    sp[Ml[sel]] += 1
        assert sp.max() < DEPTH - 4, "stack of the restatement"
    return L, total


def _args(rays, inst, tmax):
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    n = len(rays)
    inst = np.full(n, -1, np.int64) if inst is None else np.asarray(inst, np.int64)
    bound = np.full(n, np.inf, F32) if tmax is None else np.broadcast_to(np.asarray(tmax, F32), (n,)).copy()
    return rays, inst, bound


_memo = {}


def _key(ctx, what, rays, inst, tmax):
    return (ctx.name, what, rays.tobytes(), inst.tobytes(), tmax.tobytes())


def multi(ctx, oracle, order, rays, k, inst=None, tmax=None):
    """jt_intersect_multi restated in `order` ("reference" or "near"): (records (n, k) of
    abi.HIT_DTYPE, counts (n,) int32). Computed once per argument set and shared, read-only."""
    assert order in ("reference", "near") and 1 <= k <= 16
    rays, inst, bound = _args(rays, inst, tmax)
    key = _key(ctx, ("multi", order, k), rays, inst, bound)
    if key not in _memo:
        L, _ = _run(flat(ctx), Probes(oracle), rays, inst, bound, order == "near", k)
        out = (L.records(ctx.abi.HIT_DTYPE), L.count.astype(np.int32))
        for a in out:
            a.setflags(write=False)
        _memo[key] = out
    return _memo[key]


def count(ctx, oracle, order, rays, inst=None, tmax=None):
    """jt_count_hits restated: (n,) int32."""
    assert order in ("reference", "near")
    rays, inst, bound = _args(rays, inst, tmax)
    key = _key(ctx, ("count", order), rays, inst, bound)
    if key not in _memo:
        _, total = _run(flat(ctx), Probes(oracle), rays, inst, bound, order == "near", None)
        total = total.astype(np.int32)
        total.setflags(write=False)
        _memo[key] = total
    return _memo[key]


class Brute:
    """Every element of every instance against every ray, unbounded (tmax = +inf): per ray the
    accepted (t, instance, element, u, v), sorted by the key."""

    def __init__(self, ctx, oracle, rays, inst=None):
        F, probe = flat(ctx), Probes(oracle)
        rays, inst, _ = _args(rays, inst, None)
        n = len(rays)
        f32p = C.POINTER(C.c_float)
        o, d = rays[:, :3].copy(), rays[:, 3:].copy()
        local = np.empty(6, F32)
        rows, ts, insts, elems, us, vs = [], [], [], [], [], []
        for q in range(len(F.shape)):
            shp = F.shape[q]
            if F.kind[shp] < 0:
                continue
            sel = np.flatnonzero((inst < 0) | (inst == q))
            if not len(sel):
                continue
            lr = np.empty((len(sel), 6), F32)
            for a, r in enumerate(sel):
                probe.lib.or_instance_ray(F.frames[q].ctypes.data_as(f32p), o[r].ctypes.data_as(f32p), d[r].ctypes.data_as(f32p),
                                          local.ctypes.data_as(f32p))
                lr[a] = local
            op, verts = (("triangle", F.tris), ("quad", F.quads))[F.kind[shp]]
            # the shape's elements: those its BLAS lists (every element is in exactly one leaf)
            nelem = len(ctx.scene.shapes[shp].triangles) if F.kind[shp] == 0 else len(ctx.scene.shapes[shp].quads)
            head = np.concatenate([lr, _col(len(sel), RAY_EPS), _col(len(sel), np.inf)], 1)
            for e in range(nelem):
                y = probe(op, np.concatenate([head, np.broadcast_to(verts[e + F.elem_off[shp]], (len(sel), verts.shape[1]))], 1))
                acc = y[:, 3] != 0
                if acc.any():
                    rows.append(sel[acc]); ts.append(y[acc, 2]); us.append(y[acc, 0]); vs.append(y[acc, 1])
                    insts.append(np.full(int(acc.sum()), q, np.int32)); elems.append(np.full(int(acc.sum()), e, np.int32))
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
        row, t, ins, el = cat(rows, np.int64), cat(ts, F32), cat(insts, np.int32), cat(elems, np.int32)
        u, v = cat(us, F32), cat(vs, F32)
        order = np.lexsort((el, ins, t, row))  # by ray, then the key
        self.n = n
        self.row, self.t, self.inst, self.elem, self.u, self.v = row[order], t[order], ins[order], el[order], u[order], v[order]
        self.first = np.searchsorted(self.row, np.arange(n))
        self.total = np.bincount(self.row, minlength=n).astype(np.int64)

    def rank(self):
        """Each candidate's position in its ray's sorted list."""
        return np.arange(len(self.row)) - self.first[self.row]

    def multi(self, hit_dtype, k, tmax=None):
        """The k smallest keys per ray among the candidates with t <= tmax (None: all): (records, counts)."""
        keep = np.ones(len(self.row), bool) if tmax is None else self.t <= np.asarray(tmax, F32)[self.row]
        # a bound cuts a sorted list at its end, so the kept candidates keep their ranks
        rank = self.rank()
        counts = np.bincount(self.row[keep], minlength=self.n)
        assert (rank[keep] < counts[self.row[keep]]).all()
        out = np.zeros((self.n, k), hit_dtype)
        out["instance"], out["element"], out["t"] = -1, -1, INF
        w = keep & (rank < k)
        r, j = self.row[w], rank[w]
        out["instance"][r, j], out["element"][r, j] = self.inst[w], self.elem[w]
        out["u"][r, j], out["v"][r, j], out["t"][r, j], out["hit"][r, j] = self.u[w], self.v[w], self.t[w], 1
        return out, np.minimum(counts, k).astype(np.int32)

    def count(self, tmax=None):
        keep = np.ones(len(self.row), bool) if tmax is None else self.t <= np.asarray(tmax, F32)[self.row]
        return np.bincount(self.row[keep], minlength=self.n).astype(np.int32)

    def nth_t(self, j):
        """The t of each ray's entry j (0-based); +inf where the ray has fewer."""
        out = np.full(self.n, np.inf, F32)
        w = self.rank() == j
        out[self.row[w]] = self.t[w]
        return out


_brute = {}


def brute(ctx, oracle, rays, inst=None):
    rays_, inst_, _ = _args(rays, inst, None)
    key = (ctx.name, rays_.tobytes(), inst_.tobytes())
    if key not in _brute:
        _brute[key] = Brute(ctx, oracle, rays, inst)
    return _brute[key]


def differing(a, ca, b, cb):
    """Rays whose records or counts differ in any bit."""
    n = len(ca)
    return np.flatnonzero((a.view(np.uint8).reshape(n, -1) != b.view(np.uint8).reshape(n, -1)).any(axis=1) | (ca != cb))
