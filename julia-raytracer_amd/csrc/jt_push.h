// The stack entries one binary node step pushes, as an integer function of the node: plain C++
// (no HIP runtime), shared by jtk::node_step and the host check (tests/push_check.cpp).
//
// An internal node and a TLAS leaf both push a short run of entries whose indices are affine in
// the slot number j:
//   internal node   tag|c_second, tag|c_first   = tag | (first + step*j), j = 0, 1, with
//                   (first, step) = (start+1, -1) when the ray's negmask bit of the node's axis is
//                   set (start+1 is pushed first, start pops first), (start, +1) otherwise
//   TLAS leaf       INST|(start+num-1) .. INST|start: (first, step) = (start+num-1, -1), num <= 4
//                   (BVH_MAX_PRIMS, src/bvh.jl:32; the host layout rejects larger leaves)
//   BLAS leaf       nothing (its primitives are tested next)
// So the fixed-stack kernels write PUSH_SLOTS entries unconditionally instead of branching per
// arm and looping per entry: entry j goes to slot sp + min(j, max(npush,1)-1) with the value of
// entry min(j, max(npush,1)-1). Writes with j >= npush repeat the top entry; with npush == 0 they
// land in slot sp, which is the entry the step just popped, so it is free. No write leaves
// [sp, sp + max(npush,1)): the stack needs no slot more than the pushes themselves do.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JT_PUSH_HD __host__ __device__ inline
#else
#define JT_PUSH_HD inline
#endif

namespace jtk {

constexpr int PUSH_SLOTS = 4;  // the most entries one node step pushes (a full TLAS leaf)
// stack entry fields (jt_launch.h): type in bits 30-31, the child pre-test snapshot in 24-29
constexpr unsigned PUSH_T_INST = 1u, PUSH_SNAP_NONE = 63u << 24;

struct PushPlan {
    int npush;       // entries pushed: sp grows by this
    int first, step; // entry j's index is first + step*j
    unsigned tag;    // type and snapshot bits of every entry
    bool leaf;       // a BLAS leaf: the leaf cursor (prim, nprim) becomes (start, count)
    int slot[PUSH_SLOTS];       // stack slot of write j
    unsigned value[PUSH_SLOTS]; // entry of write j
};

// meta, start: the node's words (meta: bit 24 internal, bits 16-23 axis, bits 0-15 the leaf's
// count); type: the node's level (T_TLAS / T_BLAS) and blas = (type == T_BLAS); negmask: the
// query's push-order mask; sp: the stack size after this step's pop
JT_PUSH_HD PushPlan push_plan(unsigned meta, int start, unsigned type, bool blas, int negmask, int sp) {
    PushPlan p;
    const bool internal = (meta >> 24) != 0;
    const int num = (int)(meta & 0xffffu);
    const bool neg = ((negmask >> (int)((meta >> 16) & 3u)) & 1) != 0;  // axis 0..2
    p.npush = internal ? 2 : blas ? 0 : num;
    p.first = internal ? (neg ? start + 1 : start) : start + num - 1;
    p.step = internal && !neg ? 1 : -1;
    p.tag = (internal ? type << 30 : PUSH_T_INST << 30) | PUSH_SNAP_NONE;
    p.leaf = blas && !internal;
    const int last = (p.npush > 1 ? p.npush : 1) - 1;
    const unsigned e0 = p.tag | (unsigned)p.first;
    for (int j = 0; j < PUSH_SLOTS; j++) {
        const int k = j < last ? j : last;
        p.slot[j] = sp + k;
        p.value[j] = e0 + (unsigned)(p.step * k);  // = tag | (first + step*k): the index stays below 2^24
    }
    return p;
}

}  // namespace jtk
