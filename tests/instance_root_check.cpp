// instance_root_check.cpp — the instance-root rows of the baking kernels (csrc/jt_push.h:
// instance_root_base, instance_root_entry, instance_of_entry, bake_node's iroot0), enumerated on the
// host. tests/test_instance_roots_host.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
// A blob is modelled by its offsets in 16-B units, as pack_blob (csrc/jt_layout.cpp) makes them:
// the nodes at o_nodes (two units each), then `gap` units of wide records and primitives, then
// inst_trav at o_inst_trav (four units per instance). Cases: o_nodes 0..3 and gap 1..6, 9, 100, 101
// (both parities of o_nodes and of o_inst_trav - o_nodes), 1..64 nodes, 1..64 instances. For each:
//   - row i occupies bytes [16 o_nodes + 32 (iroot0 + i), + 32): every row lies inside
//     [16 o_inst_trav, 16 o_inst_trav + 64 ninst), so behind every real node and inside the array
//     no baking kernel reads; the rows are consecutive nodes from iroot0
//   - instance_root_entry(iroot0, i) is an instance entry whose index is iroot0 + i, fits IDX_MASK,
//     and instance_of_entry gives i back
//   - a TLAS leaf of num = 1..4 instances at the first two and the last two starts: push_plan_baked on
//     bake_node(meta, start, T_TLAS, iroot0) pushes, for every ray mask 0..7 (with the baking
//     kernels' bit set, and also clear: the run then ascends), the entries push_plan pushes for the
//     unbaked words with iroot0 added to each instance index, in the same slots. With the bit clear
//     the reference is the same run reversed.
//   - bake_node of an internal node and of a BLAS leaf does not depend on iroot0
#include <cstdio>

#include "../julia-raytracer_amd/csrc/jt_push.h"

namespace {

constexpr unsigned T_TLAS = 0u, T_INST = 1u, T_BLAS = 2u;
constexpr unsigned IDX_MASK = (1u << 24) - 1, SNAP_NONE = 63u << 24;

long cases = 0, bad = 0;

void fail(const char* what, int o_nodes, int o_inst_trav, int ninst, int a, int b) {
    if (bad++ < 10) std::fprintf(stderr, "instance_root_check: %s: o_nodes=%d o_inst_trav=%d ninst=%d (%d, %d)\n", what, o_nodes, o_inst_trav, ninst, a, b);
}

void check(int o_nodes, int nnodes, int gap, int ninst) {
    const int o_inst_trav = o_nodes + 2 * nnodes + gap;
    const int iroot0 = jtk::instance_root_base(o_nodes, o_inst_trav);
    const long lo = 16L * o_inst_trav, hi = lo + 64L * ninst;
    cases++;
    if (iroot0 < nnodes) fail("a row is a real node", o_nodes, o_inst_trav, ninst, iroot0, nnodes);
    for (int i = 0; i < ninst; i++) {
        const unsigned e = jtk::instance_root_entry(iroot0, i);
        const long at = 16L * o_nodes + 32L * (long)(e & IDX_MASK);  // where node_step reads the entry's node
        if (at < lo || at + 32 > hi) fail("row outside inst_trav", o_nodes, o_inst_trav, ninst, i, (int)(at - lo));
        if ((e & IDX_MASK) != (unsigned)(iroot0 + i) || e >> 30 != T_INST || (e & SNAP_NONE) != SNAP_NONE)
            fail("entry fields", o_nodes, o_inst_trav, ninst, i, (int)e);
        if (jtk::instance_of_entry(iroot0, e) != i) fail("entry decode", o_nodes, o_inst_trav, ninst, i, jtk::instance_of_entry(iroot0, e));
    }
    if ((unsigned)(iroot0 + ninst - 1) > IDX_MASK) fail("index above IDX_MASK", o_nodes, o_inst_trav, ninst, iroot0, 0);
    // TLAS leaves over the instances
    for (int num = 1; num <= 4 && num <= ninst; num++)
    for (int start = 0; start + num <= ninst; start += (start < 1 || start + num + 1 >= ninst ? 1 : ninst - num - 1 - start))
    for (int negmask = 0; negmask < 8; negmask++)
    for (int bit = 0; bit < 2; bit++) {
        const int sp = (start + negmask) % 12;
        const jtk::BakedNode b = jtk::bake_node((unsigned)num, start, T_TLAS, iroot0);
        const jtk::PushPlan got = jtk::push_plan_baked(b.e0, b.meta, negmask | (bit ? jtk::BAKE_MASK_BIT : 0), sp);
        const jtk::PushPlan ref = jtk::push_plan((unsigned)num, start, T_TLAS, false, negmask, sp);
        bool ok = got.npush == ref.npush && !got.leaf && (b.e0 & IDX_MASK) == (unsigned)(iroot0 + start);
        for (int j = 0; j < jtk::PUSH_SLOTS; j++) {
            // write j of the reference names entry min(j, num - 1) of the run; with the bit clear the
            // baked run ascends from start: the same entries, slot by slot in the opposite order
            const int k = j < num - 1 ? j : num - 1;
            const unsigned want = bit ? ref.value[j] + (unsigned)iroot0 : ref.value[num - 1 - k] + (unsigned)iroot0;
            ok = ok && got.slot[j] == ref.slot[j] && got.value[j] == want && got.value[j] >> 30 == T_INST &&
                 jtk::instance_of_entry(iroot0, got.value[j]) == (int)((bit ? ref.value[j] : ref.value[num - 1 - k]) & IDX_MASK);
        }
        cases++;
        if (!ok) fail("TLAS leaf run", o_nodes, o_inst_trav, ninst, start, num << 8 | negmask << 1 | bit);
    }
}

}  // namespace

int main() {
    const int gaps[] = {1, 2, 3, 4, 5, 6, 9, 100, 101};
    for (int o_nodes = 0; o_nodes < 4; o_nodes++)
        for (int gap : gaps)
            for (int nnodes = 1; nnodes <= 64; nnodes++)
                for (int ninst = 1; ninst <= 64; ninst++) check(o_nodes, nnodes, gap, ninst);
    // iroot0 moves a TLAS leaf's start and nothing else
    const int bases[] = {1, 7, 4096};
    for (int iroot0 : bases) {
        for (unsigned level = T_TLAS; level <= T_BLAS; level += T_BLAS)
            for (unsigned axis = 0; axis < 3; axis++) {
                const jtk::BakedNode a = jtk::bake_node(1u << 24 | axis << 16, 5, level), b = jtk::bake_node(1u << 24 | axis << 16, 5, level, iroot0);
                cases++;
                if (a.e0 != b.e0 || a.meta != b.meta) fail("internal node moved", 0, 0, 0, iroot0, (int)level);
            }
        for (unsigned num = 1; num <= 4; num++) {
            const jtk::BakedNode a = jtk::bake_node(num, 5, T_BLAS), b = jtk::bake_node(num, 5, T_BLAS, iroot0);
            cases++;
            if (a.e0 != b.e0 || a.meta != b.meta || b.e0 != 5u) fail("BLAS leaf moved", 0, 0, 0, iroot0, (int)num);
        }
    }
    std::printf("instance_root_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
