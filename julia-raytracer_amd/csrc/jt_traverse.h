// jt_traverse.h — the BVH traversals of the megakernel (src/bvh.jl:306-520): the resumable
// per-lane query (Trav), the exact-t tie rule, query start and restart, the primitive step, the
// stack, the node step of the binary and of the wide traversal, and the one-leaf instance query of
// the inline light chains. Per-lane device functions, included by jt_integrator.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_device.h"
#include "jt_launch.h"
#include "jt_push.h"

#ifndef JT_CHILD_PRETEST
#define JT_CHILD_PRETEST 1
#endif

namespace jtk {
using namespace jtd;

// ============================================================================ traversal (src/bvh.jl)
// The unified per-lane stack in LDS, its entry format and BLOCK, T_*, IDX_MASK, SNAP_NONE: jt_select.h.

struct Hit {
    int inst, elem;
    float u, v, t;
    bool hit;
};
struct Counters {  // diagnostic traversal counts (COUNT=1); paths / rays / light queries are per wave
    unsigned nodes, instances, prims, shades;
};

// A resumable BVH query per lane, for intersect_scene_bvh (root = TLAS node 0) and
// intersect_instance_bvh (root = one instance entry). node_step() / prim_step() do one unit of work: one
// node (box test + push), one instance entry (ray to instance space), or ONE primitive test of
// the current leaf (leaf cursor), so every step costs about the same whatever a lane is doing.
// Visit order — children per d[axis] sign (far-first as the reference, or near-first with
// JT_TRAVERSAL_NEAR), a TLAS leaf's instances in order, a BLAS leaf's primitives in order before
// anything else is popped — is the oracle's in either mode, so the closest hit and its
// tie-breaking (t == tmax replaces; only t > tmax rejects) match it.
struct Trav {
    v3 wo, wd, wdinv;  // world-space ray of the query
    v3 lo, ld, ldinv;  // the ray every node test uses: the world ray, or inside a BLAS the ray
                       // in the current instance's space (transform_ray, src/geometry.jl:107)
    float tmax;
    int sp;            // stack entries (all levels)
    int low;           // OVF: entries [low, sp) are in the LDS ring, [0, low) in HBM
    int inst_space;    // lo/ld/ldinv hold an instance-space ray (restore before a TLAS pop)
    int negmask;       // bit a set <=> ld[a] < 0 (the push order of src/bvh.jl:331-341, 424-434),
                       // every bit inverted for JT_TRAVERSAL_NEAR (S.order_flip)
    int cur_inst, cur_kind;
    int prim, nprim;   // leaf cursor: next primitive record, primitives left
    int h_inst, h_elem;  // closest hit so far (instance -1: none); its distance is tmax
    float h_u, h_v;
    int nh;              // bits 0-5: hits accepted so far (every tmax change), saturating at 63;
                         // TIE_SEEN, REF_RERUN (the tie rule below)
    unsigned nxt;        // wide traversal: the child word visited by the next node step (W_EMPTY: pop)
};

// Exact-t ties in the near-first orders (JT_TRAVERSAL_NEAR / WIDE). The reference accepts a hit
// at t == tmax (src/geometry.jl:226, only t > tmax rejects), so among equal-t hits the one it
// tests LAST wins, and which one that is depends on its child order (src/bvh.jl:331-341). A
// near-first query that accepts a hit at exactly its current tmax (TIE_SEEN) is therefore run
// again in the reference's child order (REF_RERUN: the same records, the children visited far
// first; with the wide records that is the binary far-first leaf sequence) and reports that
// query's hit instead: the reference's own tie resolution. Ties are rare (2e-5 of bathroom1's
// queries, none on cornellbox), so the hot path only records them (at an accepted hit), and the
// re-run runs where the query's hit is consumed (rerun_tie). A re-run is the same query: it is
// not counted as a ray or light query again; its node and primitive work is counted (COUNT=1).
#ifndef JT_TIE_RERUN
#define JT_TIE_RERUN 1  // 0: ties resolve in the near-first order's own sequence (A/B runs only)
#endif
constexpr int TIE_SEEN = 1 << 8, REF_RERUN = 1 << 9, NH_COUNT = 63;
// the child-order flip of the lane's current query: near-first, unless it is a tie's re-run
// (pb: push_bit of the kernel, below)
__device__ __forceinline__ int query_flip(const DScene& S, const Trav& T, int pb = 0) {
    return ((T.nh & REF_RERUN) ? 0 : S.order_flip) | pb;
}
// a hit accepted at t (t <= tmax): count it (child pre-test snapshots) and note an exact-t tie
__device__ __forceinline__ void hit_count(Trav& T, float t) {
    T.nh = (T.nh + ((T.nh & NH_COUNT) < NH_COUNT ? 1 : 0)) | (JT_TIE_RERUN && t == T.tmax ? TIE_SEEN : 0);
}

// The baked node form (jt_push.h): the LDS-mode FT_NONE kernels whose node step takes the
// straight-line push (binary, fixed stack: configurations 0 and 7) rewrite the nodes of their LDS
// copy once per launch (bake_nodes, jt_kernels.h) and step on push_plan_baked. The FT_ALL kernel of
// configuration 1 keeps push_plan: measured even to -0.2 % with the baked step.
// Every query of a baking kernel keeps BAKE_MASK_BIT set in its push mask: push_bit, folded into
// the constant neg_mask XORs in wherever a mask is made (the `pb` arguments below; 0 in every other
// kernel, whose code is unchanged).
// 0: every kernel keeps push_plan on the host's words (A/B runs).
#ifndef JT_NODE_BAKE
#define JT_NODE_BAKE 1
#endif
#ifndef JT_NODE_READ16
#define JT_NODE_READ16 0  // node_step's LDS arm
#endif
template <bool OVF, bool NCACHE, bool WIDE, int F>
__host__ __device__ constexpr bool node_baked() {
    return JT_NODE_BAKE && !OVF && !NCACHE && !WIDE && ft_none(F);
}
__host__ __device__ constexpr int push_bit(bool baked) { return baked ? BAKE_MASK_BIT : 0; }
// Baked shading (jt_bsdf.h BakedBasis; bake_shading, jt_kernels.h): the same kernels' bake pass also
// writes, per element of the LDS copy, the hemisphere basis of the element normal and, per material,
// color / pi, into bytes of the copy that an FT_NONE kernel never reads; their matte bounce reads
// them back instead of dividing. Every other kernel computes both per bounce, its code unchanged.
// 0: the baking kernels compute them too (A/B runs).
#ifndef JT_SHADE_BAKE
#define JT_SHADE_BAKE 1
#endif
template <bool OVF, bool NCACHE, bool WIDE, int F>
__host__ __device__ constexpr bool shade_baked() {
    return JT_SHADE_BAKE && node_baked<OVF, NCACHE, WIDE, F>();
}
// Instance roots (jt_push.h): the bake pass also writes a baked copy of every instance's BLAS root
// node into the LDS copy of inst_trav, and an instance's stack entry in a baking kernel is the
// copy's node index, so node_step reads its node at the popped index for every entry type and has
// no instance arm; inst_leaf_query reads the copy too. The baking kernels have neither FT_XFORM nor
// FT_QUAD, so an instance visit is only "the current instance is this one", a select.
// 0: instance entries carry the instance number and the step reads S.inst_blas first (A/B runs).
#ifndef JT_INST_ROOTS
#define JT_INST_ROOTS 1
#endif
// the node index of instance 0's root row in a kernel whose push bit is pb: wave-uniform, from two
// of the scene's blob offsets; 0 in every kernel that does not bake (pb 0), whose entries keep the
// instance number
__device__ __forceinline__ int inst_root_base(const DScene& S, int pb) {
    return JT_INST_ROOTS && pb ? instance_root_base(S.o_nodes, S.o_inst_trav) : 0;
}

__device__ __forceinline__ int neg_mask(v3 d, int flip) {
    return ((d.x < 0 ? 1 : 0) | (d.y < 0 ? 2 : 0) | (d.z < 0 ? 4 : 0)) ^ flip;
}

__device__ __forceinline__ void world_ray(const DScene& S, Trav& T, int pb = 0) {
    T.lo = T.wo;
    T.ld = T.wd;
    T.ldinv = T.wdinv;
    T.negmask = neg_mask(T.wd, query_flip(S, T, pb));
    T.inst_space = 0;
}

__device__ __forceinline__ Hit query_hit(const Trav& T) {
    return Hit{T.h_inst, T.h_elem, T.h_u, T.h_v, T.tmax, T.h_inst >= 0};
}

__device__ __forceinline__ bool query_busy(const Trav& T) { return T.sp > 0 || T.nprim > 0; }
// A lane's next step in either traversal: a primitive test (nprim > 0) or a node step (a stack
// entry, or in the wide traversal a pending child word); neither: its query is done (sp 0) or the
// lane has no samples left (sp < 0).
template <bool WIDE>
__device__ __forceinline__ bool wants_node(const Trav& T) {
    return T.nprim == 0 && (T.sp > 0 || (WIDE && T.nxt != W_EMPTY));
}
template <bool WIDE>
__device__ __forceinline__ bool query_done(const Trav& T) {
    return (T.sp | T.nprim) == 0 && (!WIDE || T.nxt == W_EMPTY);
}

// The start of every query, in two parts. The ray: query_begin and query_begin_wide compute 1/d
// (query_ray); query_restart and inst_leaf_query take the 1/d their caller kept and assign the six
// ray fields themselves. Then query_reset, what all four share: no hit so far (nh: 0, or REF_RERUN
// for a tie's re-run), an empty leaf cursor, no current instance. Each caller then sets what is its
// own: the push mask, the stack or the pending child word.
// (The ray is not query_reset's: as its parameters, 1/d is evaluated before T.wo and T.wd are
// assigned, and 33 kernels, the FT_NONE ones, compile to a reordered schedule, one of them to
// another spill count. This form compiles to the instructions of the four hand-written copies it
// replaces: profiles/kernel_split/isa_diff_step2.txt.)
__device__ __forceinline__ void query_ray(Trav& T, v3 o, v3 d) {
    T.wo = o;
    T.wd = d;
    T.wdinv = V3(jl_rcp(d.x), jl_rcp(d.y), jl_rcp(d.z));  // ray_dinv (src/bvh.jl:322), no guard
    T.lo = o;
    T.ld = d;
    T.ldinv = T.wdinv;
}
__device__ __forceinline__ void query_reset(Trav& T, int nh) {
    T.tmax = __builtin_inff();
    T.nh = nh;
    T.h_inst = -1;
    T.h_elem = -1;
    T.h_u = 0;
    T.h_v = 0;
    T.nprim = 0;
    T.prim = 0;
    T.cur_inst = -1;
    T.cur_kind = KIND_TRI;
    T.inst_space = 0;
}
__device__ __forceinline__ void query_begin(const DScene& S, Trav& T, v3 o, v3 d, unsigned root, int* stack, int rerun = 0,
                                            int pb = 0) {
    query_ray(T, o, d);
    query_reset(T, rerun);
    T.negmask = neg_mask(d, (rerun ? 0 : S.order_flip) | pb);
    stack[0] = (int)root;
    T.sp = 1;
    T.low = 0;
    T.nxt = W_EMPTY;
}
// query_begin of the wide traversal: the root is the first node step's child word (the TLAS
// root record, or an instance leaf of one instance for intersect_instance_bvh); the stack is empty
__device__ __forceinline__ void query_begin_wide(const DScene& S, Trav& T, v3 o, v3 d, unsigned root_word, int rerun = 0) {
    query_ray(T, o, d);
    query_reset(T, rerun);
    T.negmask = neg_mask(d, rerun ? 0 : S.order_flip);
    T.sp = 0;
    T.low = 0;
    T.nxt = root_word;
}
constexpr unsigned WROOT_SCENE = 0u;  // the TLAS root record
__device__ __forceinline__ unsigned wroot_instance(int inst) { return W_LEAF | W_INST | (unsigned)inst; }
// query_begin for either traversal: a closest-hit scene query, or (inst >= 0) the
// intersect_instance_bvh of sample_lights_pdf. In a baking kernel (pb set) the instance's entry
// carries its root row (instance_root_entry, jt_push.h: the instance number plus iroot0)
template <bool WIDE>
__device__ __forceinline__ void query_start(const DScene& S, Trav& T, v3 o, v3 d, int inst, int* stack, int rerun = 0,
                                            int pb = 0) {
    if (JT_INST_ROOTS && pb && inst >= 0) inst += inst_root_base(S, pb);
    if (WIDE) query_begin_wide(S, T, o, d, inst < 0 ? WROOT_SCENE : wroot_instance(inst), rerun);
    else query_begin(S, T, o, d, inst < 0 ? ((T_TLAS << 30) | SNAP_NONE) : ((T_INST << 30) | SNAP_NONE | (unsigned)inst), stack, rerun, pb);
}
// The scene query of a lane that has just run its bounce's light chains inline (light_chain with
// JT_CHAIN_TAIL) in the binary traversal: query_begin for the same direction d, whose world-space
// 1/d the chain left in T.wdinv and, in kernels without instance transforms, whose push mask it
// left in T.negmask. The instance-space values of a transformed light (T.ldinv, T.negmask with
// FT_XFORM) are never reused.
template <int F>
__device__ __forceinline__ void query_restart(const DScene& S, Trav& T, v3 o, v3 d, int* stack, int pb = 0) {
    T.wo = o;
    T.wd = d;
    T.lo = o;
    T.ld = d;
    T.ldinv = T.wdinv;
    query_reset(T, 0);
    if (F & FT_XFORM) T.negmask = neg_mask(d, S.order_flip | pb);
    stack[0] = (int)((T_TLAS << 30) | SNAP_NONE);
    T.sp = 1;
    T.low = 0;
    T.nxt = W_EMPTY;
}
// a finished near-first query that saw an exact-t tie: run it again in the reference's child order
// (the same world ray (o, d): every query is started on its path's (st.o, st.d), which do not
// change until its hit is consumed — so T.wo/T.wd stay dead in kernels without instance
// transforms; inst >= 0: the intersect_instance_bvh of that instance). Returns whether the lane
// re-runs (its query is then not done).
// An instance query of a one-leaf BLAS (INST_LEAF_ROOT) tests its leaf's primitives in the same
// order in every child order, so it is never re-run (the oracle's instance_query: the same rule).
constexpr int INST_LEAF_ROOT = 1 << 30;  // in the instance record's w (shape) word
template <bool WIDE>
__device__ __forceinline__ bool rerun_tie(const DScene& S, Trav& T, v3 o, v3 d, int inst, int* stack, int pb = 0) {
    if (!JT_TIE_RERUN || (T.nh & (TIE_SEEN | REF_RERUN)) != TIE_SEEN || S.order_flip == 0) return false;
    if (inst >= 0 && (S.inst_blas[inst].w & INST_LEAF_ROOT)) return false;
    query_start<WIDE>(S, T, o, d, inst, stack, REF_RERUN, pb);
    return true;
}

// An instance visit (src/bvh.jl:345,502), for the node step of either traversal and the one-leaf
// instance query: the ray every node test uses becomes the ray in the instance's space
// (inverse(frame, true) precomputed: S.inst_trav), and the instance is the current one. `ib` is the
// instance's S.inst_blas record: y its identity flag, z the kind of its shape's primitives.
// XF false (kernels without FT_XFORM): every instance ray is the world ray, no transform, no
// space switch.
template <bool XF>
__device__ __forceinline__ void enter_instance(const DScene& S, Trav& T, unsigned inst, const int4& ib, int pb = 0) {
    if (!XF || ib.y) {
        // inverse(identity) is exactly the identity: transform_ray returns the ray bit for bit
        if (XF && T.inst_space) world_ray(S, T, pb);
    } else {
        const DInstTrav it = S.inst_trav[inst];
        const fr3 inv = frame_from(it.i0, it.i1, it.i2);
        T.lo = transform_point(inv, T.wo);
        T.ld = transform_vector(inv, T.wd);
        T.ldinv = V3(jl_rcp(T.ld.x), jl_rcp(T.ld.y), jl_rcp(T.ld.z));
        T.negmask = neg_mask(T.ld, query_flip(S, T, pb));
        T.inst_space = 1;
    }
    T.cur_inst = (int)inst;
    T.cur_kind = ib.z;
}

// The current BLAS leaf's next primitive(s), in order (src/bvh.jl:444-484). Triangles go in
// pairs: both tests are computed side by side (the record after the leaf's last one exists: the
// array is padded), then accepted in order, the second against the tmax the first left. A
// second pair runs in the same step when some lane's leaf has more than two left.
// Triangle k of the current leaf and the next one come from one 80-B pair record (host layout:
// the two triangles' components interleaved, 5 loads instead of 6 for two separate records).
// k is 0 or 2.
template <int F>
__device__ __forceinline__ void tri_pair(const DScene& S, Trav& T, int k) {
    const float4* r = S.prims + 5 * (T.prim + (k >> 1));
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    const PrimHit p1 = intersect_triangle_pre(T.lo, T.ld, ray_eps, V3(r0.x, r0.z, r1.x), V3(r1.z, r2.x, r2.z),
                                              V3(r3.x, r3.z, r4.x));
    const PrimHit p2 = intersect_triangle_pre(T.lo, T.ld, ray_eps, V3(r0.y, r0.w, r1.y), V3(r1.w, r2.y, r2.w),
                                              V3(r3.y, r3.w, r4.y));
    if (tri_hit_before(p1, T.tmax)) {
        hit_count(T, p1.t);
        T.h_inst = T.cur_inst;
        T.h_elem = __float_as_int(r4.z);
        T.h_u = p1.u;
        T.h_v = p1.v;
        T.tmax = p1.t;
    }
    if (T.nprim >= k + 2 && tri_hit_before(p2, T.tmax)) {
        hit_count(T, p2.t);
        T.h_inst = T.cur_inst;
        T.h_elem = __float_as_int(r4.w);
        T.h_u = p2.u;
        T.h_v = p2.v;
        T.tmax = p2.t;
    }
}
template <int COUNT, int F>
__device__ __forceinline__ void prim_step(const DScene& S, Trav& T, Counters& cnt) {
    if (!(F & FT_QUAD) || T.cur_kind == KIND_TRI) {
        // a triangle leaf (<= 4 primitives, BVH_MAX_PRIMS, src/bvh.jl:32) is tested within this step
        tri_pair<F>(S, T, 0);
        const bool more = T.nprim > 2;
        if (__builtin_amdgcn_ballot_w64(more)) {
            if (more) tri_pair<F>(S, T, 2);
        }
        const int n = T.nprim < 4 ? T.nprim : 4;
        if (COUNT) cnt.prims += n;
        T.prim += 2;  // pair records (only read again when the leaf had more than four)
        T.nprim -= n;
        return;
    }
    if (COUNT) cnt.prims++;
    const float4* r = S.prims + 4 * T.prim;
    const float4 a = r[0], b = r[1], c = r[2], d = r[3];
    const PrimHit p = intersect_quad(T.lo, T.ld, ray_eps, T.tmax, xyz(a), xyz(b), xyz(c), xyz(d), d.w != 0.0f);
    if (p.hit) {
        hit_count(T, p.t);
        T.h_inst = T.cur_inst;
        T.h_elem = __float_as_int(a.w);
        T.h_u = p.u;
        T.h_v = p.v;
        T.tmax = p.t;
    }
    T.prim += 1;
    T.nprim -= 1;
}

template <int RING, bool OVF>
__device__ __forceinline__ void st_push(const DScene& S, Trav& T, int* stack, int pixel, unsigned e) {
    if (OVF) {
        if (T.sp - T.low == S.ring) {  // ring full: the oldest entry moves to HBM
            S.ovf[(size_t)pixel * S.ovf_stride + T.low] = stack[(T.low & (S.ring - 1)) * BLOCK];
            T.low += 1;
        }
        stack[(T.sp & (S.ring - 1)) * BLOCK] = (int)e;
    } else {
        stack[T.sp * BLOCK] = (int)e;
    }
    T.sp += 1;
}
template <int RING, bool OVF>
__device__ __forceinline__ unsigned st_pop(const DScene& S, Trav& T, const int* stack, int pixel) {
    T.sp -= 1;
    if (OVF) {
        // the ring slot is read unconditionally (its address is always valid; a relaxed atomic
        // load, which the compiler cannot merge with the HBM load) and the HBM entry only below
        // the ring: written as a choice of the two addresses, the compiler made every pop one
        // flat load waiting on both memory counters
        const unsigned r = (unsigned)__hip_atomic_load(stack + (T.sp & (S.ring - 1)) * BLOCK, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        if (T.sp < T.low) {  // below the ring: this entry was spilled
            T.low = T.sp;
            return (unsigned)S.ovf[(size_t)pixel * S.ovf_stride + T.sp];
        }
        return r;
    }
    return (unsigned)stack[T.sp * BLOCK];
}

// Pop one stack entry: an instance entry or a TLAS/BLAS node. An instance visit and the box
// test of its BLAS root are one step: the reference's instance visit pushes nothing but the
// root (src/bvh.jl:345-351, 502-506), which is then the very next pop, so testing it in the same
// step visits the same nodes in the same order.
template <int RING, bool OVF, int COUNT, bool NCACHE, int F>
__device__ __forceinline__ void node_step(const DScene& S, Trav& T, int* stack, int pixel, Counters& cnt) {
    // without FT_XFORM every instance ray is the world ray: no transform, no space switch
    constexpr bool XF = (F & FT_XFORM) != 0;
    constexpr bool BAKED = node_baked<OVF, NCACHE, false, F>();  // S.nodes holds the baked form (jt_push.h)
    constexpr int PB = push_bit(BAKED);
    const unsigned e = st_pop<RING, OVF>(S, T, stack, pixel);
    unsigned type = e >> 30, idx = e & IDX_MASK;
    if constexpr (BAKED && JT_INST_ROOTS) {
        // an instance entry is the node index of the instance's root row (jt_push.h): idx is the
        // node to read whatever the type, and the visit is a select
        if (COUNT) cnt.instances += type == T_INST ? 1u : 0u;
        T.cur_inst = type == T_INST ? instance_of_entry(inst_root_base(S, PB), e) : T.cur_inst;
    } else if (type == T_INST) {  // instance visit: inverse(frame, true) precomputed (src/bvh.jl:345,502)
        if (COUNT) cnt.instances++;
        const int4 ib = S.inst_blas[idx];  // blas_root, identity, kind, shape | leaf root (one load: x, y adjacent)
        enter_instance<XF>(S, T, idx, ib, PB);
        type = T_BLAS;
        idx = (unsigned)ib.x;
    } else if (XF && type == T_TLAS && T.inst_space) {
        world_ray(S, T, PB);  // back from an instance: TLAS nodes test the world ray
    }
    const bool blas = type == T_BLAS;
    if (COUNT) cnt.nodes++;
    // HBM mode: a child pre-tested at its parent with the tmax it still has (no hit since: its
    // snapshot equals the hit count) passes this pop's box test too — same ray, same box, same
    // tmax — so only its start/meta half is loaded
    const unsigned snap = (e >> 24) & 63u;
    float4 nb;
    if (NCACHE) {
        // The second half (z slab, start/meta) is one load for every lane, the first half only
        // for lanes that test the box: a gather costs one vector-memory wave-instruction whatever
        // the number of active lanes (scripts/td_lanes_bench.hip), so a load shared by both kinds
        // of pop is issued once per step instead of once per kind (bathroom1 +3 %, ecosys +2.8 %).
        nb = S.nodes[idx].b;
        // keep it one 16-B load: without this the compiler narrows it to the start/meta half and
        // sinks the z-slab half into the branch below (a second instruction in every mixed step)
        __asm__("" : "+v"(nb.x), "+v"(nb.y), "+v"(nb.z), "+v"(nb.w));
        if (snap == 63u || snap != (unsigned)(T.nh & NH_COUNT))
            if (!intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, S.nodes[idx].a, nb)) return;
    } else {  // LDS mode (no pre-test): the whole node, two LDS reads
        DNode nd = S.nodes[idx];
        // JT_NODE_READ16 (baking kernels): the node as two 16-B reads issued together, as the
        // NCACHE arm pins its nb, instead of 16 + 8 B and a dependent 8-B read of start/meta
        // behind the box test. Measured again on the step without an instance arm, per kernel
        // family, and not adopted: EXPERIMENTS.md ("Instance-root rows").
        if (JT_NODE_READ16 && BAKED) __asm__("" : "+v"(nd.b.x), "+v"(nd.b.y), "+v"(nd.b.z), "+v"(nd.b.w));
        if (!intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, nd.a, nd.b)) return;
        nb = nd.b;
    }
    const unsigned meta = __float_as_uint(nb.w);
    const int start = __float_as_int(nb.z);
    const int num = (int)(meta & 0xffffu);
    if (!OVF && !(JT_CHILD_PRETEST && NCACHE)) {
        // fixed stack, no pre-test: the entries of either arm are affine in the slot number
        // (jt_push.h), so every lane writes PUSH_SLOTS entries straight-line — the surplus ones
        // repeat the top entry, or land in the slot just popped — instead of a divergent branch
        // per arm and a loop per TLAS-leaf instance. The leaf cursor is set by selects.
        if constexpr (BAKED) {
            // the node's words already hold what push_plan derives from them (start is e0); the
            // writes are addressed from the slot just popped
            const PushPlan p = push_plan_baked((unsigned)start, meta, T.negmask, T.sp);
            int* const top = stack + T.sp * BLOCK;
#pragma unroll
            for (int j = 0; j < PUSH_SLOTS; j++) top[(p.slot[j] - T.sp) * BLOCK] = (int)p.value[j];
            T.sp += p.npush;
            T.prim = p.leaf ? start : T.prim;
            T.nprim = p.leaf ? num : T.nprim;
            return;
        }
        const PushPlan p = push_plan(meta, start, type, blas, T.negmask, T.sp);
#pragma unroll
        for (int j = 0; j < PUSH_SLOTS; j++) stack[p.slot[j] * BLOCK] = (int)p.value[j];
        T.sp += p.npush;
        T.prim = p.leaf ? start : T.prim;
        T.nprim = p.leaf ? num : T.nprim;
        return;
    }
    if (meta >> 24) {  // internal: for d[axis] >= 0 push start, start+1 (start+1 pops first)
        const int axis = (int)((meta >> 16) & 0xffu);
        // d[axis] < 0, or (JT_TRAVERSAL_NEAR) d[axis] >= 0: start+1 is pushed first, start pops first
        const bool neg = (T.negmask >> axis) & 1;
        const unsigned tag = type << 30 | SNAP_NONE;
        // c_second is pushed first and popped second, c_first popped first
        const unsigned c_second = (unsigned)(neg ? start + 1 : start), c_first = (unsigned)(neg ? start : start + 1);
        if (JT_CHILD_PRETEST && NCACHE) {
            // HBM mode: test both children (one 64-B pair) when their parent is visited. A child
            // whose box fails now fails when popped too (the slab test is monotone in tmax, which
            // only shrinks): count its pop and skip the push. A pushed child is tested again when
            // popped, with that moment's tmax, exactly as the reference does. (+10 % bathroom1,
            // +14 % ecosys; in LDS mode the extra tests cost more than the pops they save.)
            const DNode n0 = S.nodes[c_second];
            const DNode n1 = S.nodes[c_first];
            const bool k0 = intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, n0.a, n0.b);
            const bool k1 = intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, n1.a, n1.b);
            if (COUNT) cnt.nodes += (k0 ? 0 : 1) + (k1 ? 0 : 1);
            const unsigned ptag = type << 30 | (unsigned)(T.nh & NH_COUNT) << 24;  // pre-tested at hit count nh
            if (k0) st_push<RING, OVF>(S, T, stack, pixel, ptag | c_second);
            if (k1) st_push<RING, OVF>(S, T, stack, pixel, ptag | c_first);
        } else {
            st_push<RING, OVF>(S, T, stack, pixel, tag | c_second);
            st_push<RING, OVF>(S, T, stack, pixel, tag | c_first);
        }
    } else if (!blas) {  // TLAS leaf: instances start .. start+num-1, in order
        for (int k = num - 1; k >= 0; k--)
            st_push<RING, OVF>(S, T, stack, pixel, (T_INST << 30) | SNAP_NONE | (unsigned)(start + k));
    } else {  // BLAS leaf: its primitives are tested next, in order, before any other pop
        T.prim = start;
        T.nprim = num;

    }
}

// ============================================================================ wide traversal
// JT_TRAVERSAL_WIDE (DWide records, jt_device.h). The children of a record are visited in the
// binary tree's DFS order for the ray: the near pair first by N's axis a0, in each pair the near
// child by a1 / a2 — the same rule as the binary near-first order (S.order_flip folds the order
// into negmask), so leaves are reached in the binary near-first sequence. flips bit 0: the R pair
// first; bit 1 / 2: within L / R the second slot first. Visit index k -> slot:
__device__ __forceinline__ int wide_slot(unsigned flips, int k) {
    const int p = (k >> 1) ^ (int)(flips & 1u);
    return 2 * p + ((k & 1) ^ (int)((flips >> (p ? 2 : 1)) & 1u));
}
__device__ __forceinline__ unsigned wide_word(const uint4& r3, int slot) {
    return slot == 0 ? r3.x : slot == 1 ? r3.y : slot == 2 ? r3.z : r3.w;
}
// dequantised box of slot c (the record's origin + byte * scale, in float) as intersect_bbox's
// (bmin.x, bmax.x, bmin.y, bmax.y), (bmin.z, bmax.z). byte * scale is exact (a byte times a
// normal power of two), so the fused multiply-add rounds once exactly as origin + byte * scale
// does: one v_fma_f32 per plane, the same bits as the host's quantisation check.
__device__ __forceinline__ float deq(float o, unsigned w, int sh, float s) {
    return __builtin_fmaf((float)((w >> sh) & 255u), s, o);
}
__device__ __forceinline__ void wide_box(const float4& r0, const uint4& r1, const uint4& r2, float sx, float sy,
                                         float sz, int c, float4& a, float4& b) {
    const int sh = 8 * c;
    a = make_float4(deq(r0.x, r1.x, sh, sx), deq(r0.x, r1.y, sh, sx), deq(r0.y, r1.z, sh, sy), deq(r0.y, r1.w, sh, sy));
    b = make_float4(deq(r0.z, r2.x, sh, sz), deq(r0.z, r2.y, sh, sz), 0.0f, 0.0f);
}
// Stack entries of the wide traversal (32 bits): a group — the children of record `index` still
// to visit (bit 31 clear; bits 28-30 the record's flips for this ray, 24-27 the visit-order mask
// of children whose boxes passed, 0-23 the record) — or an instance range (bit 31 set; bits 24-25
// count - 1, 0-23 the first instance) of a TLAS leaf whose first instance is being visited.
// A child whose box passed is visited even if tmax has shrunk since (no re-test at pop).
// (Every field is written on both paths: as two branches storing to different fields, the
// compiler merged the stores into one through a selected address, and the Trav fields it addressed
// no longer fit in registers — they lived in scratch, stored per node step.)
template <int F>
__device__ __forceinline__ void wide_take(Trav& T, unsigned w) {
    const bool leaf = (w & (W_LEAF | W_INST)) == W_LEAF;  // a BLAS leaf: its primitives are tested next
    T.prim = leaf ? (int)(w & W_START) : T.prim;
    T.nprim = leaf ? (int)((w >> 28) & 3u) + 1 : T.nprim;

    T.nxt = leaf ? T.nxt : w;  // a record, or a TLAS leaf (its first instance is visited by the next step)
}
// one record visit: the up-to-four child boxes against the current ray and tmax; the first passing
// child (visit order) is taken at once, the others are pushed as one group entry
template <int RING, bool OVF, int COUNT, int F>
__device__ __forceinline__ void wide_visit(const DScene& S, Trav& T, int* stack, int pixel, Counters& cnt, unsigned idx) {
    if (COUNT) cnt.nodes++;
    const DWide& rec = S.wnodes[idx];
    const float4 r0 = rec.r0;
    const uint4 r1 = rec.r1, r2 = rec.r2, r3 = rec.r3;
    const unsigned meta = __float_as_uint(r0.w);
    const float sx = __uint_as_float((meta & 255u) << 23), sy = __uint_as_float(((meta >> 8) & 255u) << 23),
                sz = __uint_as_float(((meta >> 16) & 255u) << 23);
    unsigned hits = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float4 a, b;
        wide_box(r0, r1, r2, sx, sy, sz, c, a, b);
        const bool pass = intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, a, b);
        if (wide_word(r3, c) != W_EMPTY && pass) hits |= 1u << c;
    }
    if (!hits) return;
    const unsigned ax = meta >> 24;
    const unsigned flips = ((T.negmask >> (ax & 3u)) & 1u ? 0u : 1u) | ((T.negmask >> ((ax >> 2) & 3u)) & 1u ? 0u : 2u) |
                           ((T.negmask >> ((ax >> 4) & 3u)) & 1u ? 0u : 4u);
    unsigned vm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) vm |= ((hits >> wide_slot(flips, k)) & 1u) << k;
    const int k0 = __builtin_ctz(vm);
    const unsigned rest = vm & (vm - 1u);
    if (rest) st_push<RING, OVF>(S, T, stack, pixel, flips << 28 | rest << 24 | idx);
    wide_take<F>(T, wide_word(r3, wide_slot(flips, k0)));
}
// One node step of the wide traversal: the pending child word, or the next child of the group on
// top of the stack (its word: one 4-B load), or the next instance of a range. An instance visit
// (inverse frame precomputed, src/bvh.jl:345,502) and the visit of its BLAS root record are one
// step, as in the binary traversal.
template <int RING, bool OVF, int COUNT, int F>
__device__ __forceinline__ void node_step_wide(const DScene& S, Trav& T, int* stack, int pixel, Counters& cnt) {
    constexpr bool XF = (F & FT_XFORM) != 0;
    unsigned w = T.nxt;
    if (w == W_EMPTY) {
        const unsigned e = st_pop<RING, OVF>(S, T, stack, pixel);
        const unsigned idx = e & IDX_MASK;
        if (!(e >> 31)) {  // a group: its next child in visit order
            const unsigned m = (e >> 24) & 15u;
            const unsigned rest = m & (m - 1u);
            if (rest) st_push<RING, OVF>(S, T, stack, pixel, (e & ~(15u << 24)) | rest << 24);
            if (XF && T.inst_space && idx < (unsigned)S.tlas_wnodes) world_ray(S, T);  // back in the TLAS
            w = reinterpret_cast<const unsigned*>(S.wnodes + idx)[12 + wide_slot((e >> 28) & 7u, __builtin_ctz(m))];
            if ((w & (W_LEAF | W_INST)) == W_LEAF) {
                wide_take<F>(T, w);
                return;
            }
        } else {  // the rest of a TLAS leaf's instances
            w = W_LEAF | W_INST | ((e >> 24) & 3u) << 28 | idx;
        }
    } else {
        T.nxt = W_EMPTY;
    }
    if (w & W_LEAF) {  // a TLAS leaf: visit its first instance, keep the others as a range entry
        const unsigned inst = w & W_START, n1 = (w >> 28) & 3u;
        if (n1) st_push<RING, OVF>(S, T, stack, pixel, W_LEAF | (n1 - 1u) << 24 | (inst + 1u));
        if (COUNT) cnt.instances++;
        const int4 ib = S.inst_blas[inst];  // wide BLAS root record, identity, kind, shape | leaf root
        enter_instance<XF>(S, T, inst, ib);
        w = (unsigned)ib.x;
    }
    wide_visit<RING, OVF, COUNT, F>(S, T, stack, pixel, cnt, w);
}
// a node step in either traversal
template <bool WIDE, int RING, bool OVF, int COUNT, bool NCACHE, int F>
__device__ __forceinline__ void node_step_any(const DScene& S, Trav& T, int* stack, int pixel, Counters& cnt) {
    if (WIDE) node_step_wide<RING, OVF, COUNT, F>(S, T, stack, pixel, cnt);
    else node_step<RING, OVF, COUNT, NCACHE, F>(S, T, stack, pixel, cnt);
}

// One query of an inline chain in the binary fixed-stack LDS kernels: intersect_instance_bvh of an
// instance whose BLAS is one leaf (INST_LEAF_ROOT), without the stack round trip of query_start +
// node_step — the instance record and its root node are read directly, the root box is tested by
// the same intersect_bbox, and the leaf cursor is set by selects. dinv and negmask are those of
// query_begin for direction d: the direction is the same for every query of a bounce's chain, so
// the caller computes them once. The query's state ends as query_start + node_step leave it
// (sp 0; prim 0 when the box fails), and one instance and one node are counted.
template <int COUNT, int F>
__device__ __forceinline__ void inst_leaf_query(const DScene& S, Trav& T, v3 o, v3 d, v3 dinv, int negmask, int inst,
                                                Counters& cnt) {
    constexpr bool XF = (F & FT_XFORM) != 0;
    constexpr int PB = push_bit(node_baked<false, false, false, F>());  // chain_leaf_step's kernels: LDS mode, binary, fixed stack
    T.wo = o;
    T.wd = d;
    T.wdinv = dinv;
    T.lo = o;
    T.ld = d;
    T.ldinv = dinv;
    query_reset(T, 0);
    T.negmask = negmask;
    T.sp = 0;
    T.low = 0;
    T.nxt = W_EMPTY;
    if (COUNT) cnt.instances++;
    int root;
    if constexpr (JT_INST_ROOTS && PB != 0) {
        // the instance's root row (jt_push.h): no instance record is read. A one-leaf root's baked
        // words are its own: start, and the count in meta's low 16 bits
        T.cur_inst = inst;
        root = inst_root_base(S, PB) + inst;
    } else {
        const int4 ib = S.inst_blas[inst];
        // the query has just started in world space (inst_space 0), so enter_instance's return to the
        // world ray is dead here; this overwrites query_reset's cur_inst and cur_kind
        enter_instance<XF>(S, T, (unsigned)inst, ib, PB);
        root = ib.x;
    }
    if (COUNT) cnt.nodes++;
    const DNode nd = S.nodes[root];
    const bool pass = intersect_bbox(T.lo, T.ldinv, ray_eps, T.tmax, nd.a, nd.b);
    T.prim = pass ? __float_as_int(nd.b.z) : 0;
    T.nprim = pass ? (int)(__float_as_uint(nd.b.w) & 0xffffu) : 0;
}

}  // namespace jtk
