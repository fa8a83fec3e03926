// The stack entries one binary node step pushes, as an integer function of the node: plain C++
// (no HIP runtime), shared by jtk::node_step and the host checks (tests/push_check.cpp,
// tests/push_baked_check.cpp). push_plan is the definition; the baked form below restates it.
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
// stack entry fields (jt_select.h): type in bits 30-31, the child pre-test snapshot in 24-29
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

// The baked node form. Everything push_plan derives from (meta, start, level) is a constant of the
// node, so a kernel that stages the nodes itself (trace_kernel_lds, jt_kernels.h) rewrites each
// node's two words once per launch and its node step runs push_plan_baked on them:
//   word z (e0): the stack entry of slot order 0, ready to store
//       internal node   level << 30 | SNAP_NONE | start
//       TLAS leaf       T_INST << 30 | SNAP_NONE | start
//       BLAS leaf       start, unchanged (the leaf cursor's primitive record)
//   word w: bits 0-15 the count, unchanged; 16-17 the axis whose push-mask bit reverses the run
//       (a leaf: BAKE_AXIS_SET); 24-26 npush (2 / the count / 0); bit 27 a BLAS leaf; 28-29
//       last = max(npush, 1) - 1; bit 30 min(1, last)
// With nlast = (the mask's bit of the axis) ? last : 0, entry j is e0 + |nlast - min(j, last)| in
// slot sp + min(j, last): the run start+1, start or start, start+1 of an internal node,
// start+num-1 .. start of a TLAS leaf — whose axis names bit 3 of the mask, BAKE_MASK_BIT, which
// the baking kernels keep set in every query's push mask, so a leaf needs no arm of its own. The
// same entries in the same slots as push_plan for every node (a TLAS leaf without instances, which
// pushes nothing, differs in the value of its dead write to slot sp); tests/push_baked_check.cpp
// enumerates both. `start` is e0's low 24 bits, the count w's low 16.
constexpr unsigned BAKE_AXIS_SET = 3u;  // the axis field of a leaf: reads BAKE_MASK_BIT
constexpr int BAKE_MASK_BIT = 8;        // set in the push mask of every query of a baking kernel
constexpr unsigned BAKE_LEAF = 1u << 27;

struct BakedNode {
    unsigned e0, meta;  // the node's words z and w
};
// iroot0 (instance roots, below): added to a TLAS leaf's start, whose run of instance entries then
// names the instances' root rows; the run stays affine in the slot number
JT_PUSH_HD BakedNode bake_node(unsigned meta, int start, unsigned level, int iroot0 = 0) {
    const bool internal = (meta >> 24) != 0;
    const bool blas = level != 0u;  // T_BLAS, against T_TLAS = 0
    const unsigned num = meta & 0xffffu;
    if (!internal && !blas) start += iroot0;
    const unsigned tag = (internal ? level << 30 : PUSH_T_INST << 30) | PUSH_SNAP_NONE;
    // (a TLAS leaf holds at most PUSH_SLOTS instances: the host layout rejects larger ones)
    const unsigned npush = internal ? 2u : blas ? 0u : (num < (unsigned)PUSH_SLOTS ? num : (unsigned)PUSH_SLOTS);
    const unsigned last = (npush > 1u ? npush : 1u) - 1u;
    BakedNode b;
    b.e0 = internal || !blas ? tag | (unsigned)start : (unsigned)start;
    b.meta = num | (internal ? (meta >> 16) & 3u : BAKE_AXIS_SET) << 16 | npush << 24 | (!internal && blas ? BAKE_LEAF : 0u) |
             last << 28 | (last ? 1u : 0u) << 30;
    return b;
}
// c + |a - b|: one instruction on the device (the compiler does not form it from the C++ below)
JT_PUSH_HD unsigned add_absdiff(unsigned a, unsigned b, unsigned c) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned r;
    __asm__("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return c + (a > b ? a - b : b - a);
#endif
}
// The plan of a baked node: npush, slot, value and leaf as push_plan's; first, step and tag are
// folded into e0 and stay zero. negmask carries BAKE_MASK_BIT.
JT_PUSH_HD PushPlan push_plan_baked(unsigned e0, unsigned meta, int negmask, int sp) {
    PushPlan p;
    p.npush = (int)((meta >> 24) & 7u);
    p.first = 0;
    p.step = 0;
    p.tag = 0u;
    p.leaf = (meta & BAKE_LEAF) != 0;
    const unsigned neg = ((unsigned)negmask >> ((meta >> 16) & 3u)) & 1u;
    const unsigned last = (meta >> 28) & 3u;
    const unsigned nlast = last * neg;  // neg ? last : 0
    for (int j = 0; j < PUSH_SLOTS; j++) {
        const unsigned k = j == 1 ? (meta >> 30) & 1u : (unsigned)j < last ? (unsigned)j : last;  // min(j, last)
        p.slot[j] = sp + (int)k;
        p.value[j] = j == 0 ? e0 + nlast : add_absdiff(nlast, k, e0);
    }
    return p;
}

// Instance roots (JT_INST_ROOTS, jt_traverse.h). The baking kernels read one word of an instance's
// record while they traverse, the index of its BLAS root node, and that node is a constant of the
// scene. So the bake pass also writes, for every instance i, a baked copy of its root node, and an
// instance's stack entry carries the copy's node index: a pop reads its node at the entry's index
// whatever the entry's type, without reading the instance record first.
// The copies live in the LDS copy of the blob's inst_trav array (64 B per instance, read only with
// instance transforms, which no baking kernel has): copy i is node iroot0 + i, counted in 32-B nodes
// from the node array's base. o_nodes and o_inst_trav are the arrays' blob offsets in 16-B units;
// iroot0 is the first whole node at or after inst_trav's first byte. The last copy ends at most
// 16 + 32 n bytes into the n instances' 64 n: tests/instance_root_check.cpp enumerates it.
JT_PUSH_HD int instance_root_base(int o_nodes, int o_inst_trav) { return (o_inst_trav - o_nodes + 1) >> 1; }
constexpr unsigned PUSH_IDX_MASK = (1u << 24) - 1;  // IDX_MASK (jt_select.h)
// the stack entry of instance inst in a baking kernel, and the instance of such an entry
JT_PUSH_HD unsigned instance_root_entry(int iroot0, int inst) {
    return PUSH_T_INST << 30 | PUSH_SNAP_NONE | (unsigned)(iroot0 + inst);
}
JT_PUSH_HD int instance_of_entry(int iroot0, unsigned e) { return (int)(e & PUSH_IDX_MASK) - iroot0; }

}  // namespace jtk
