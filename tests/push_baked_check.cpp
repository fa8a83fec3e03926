// push_baked_check.cpp — the baked node form (csrc/jt_push.h: bake_node, push_plan_baked) against
// push_plan, the reference definition of the binary node step's pushes, enumerated on the host.
// tests/test_push_baked.py builds it with the host compiler under -fsanitize=address,undefined and
// runs it. No Python, no HIP runtime, no GPU.
//
// Cases: internal nodes at both levels with axis 0..2; TLAS leaves of 1..4 instances; BLAS leaves
// of 1..4 and of 65535 primitives; start 0, 1, 2^24-5, 2^24-2; every ray mask 0..7 with the baking
// kernels' bit (BAKE_MASK_BIT) set in the mask the baked plan gets; stack size sp 0..28. For each,
// push_plan_baked(bake_node(meta, start, level)) must equal push_plan(meta, start, level) in
// npush, every slot, every value and the leaf flag, and `start` and the count must be recoverable
// from the baked words as jtk::node_step and jtk::inst_leaf_query read them: the count is w's low
// 16 bits, start is e0's low 24 bits, and a BLAS leaf's e0 is start itself.
// One exception, which that last property forces: a BLAS leaf pushes nothing, its four writes all
// land in slot sp (the entry the step just popped: free) and are dead. push_plan writes an
// instance-tagged start+num-1 there, the baked plan the leaf's e0, which must stay `start` for the
// leaf cursor. For npush 0 the values are therefore not compared; the slots (all sp) are.
#include <cstdio>

#include "../julia-raytracer_amd/csrc/jt_push.h"

namespace {

constexpr unsigned T_TLAS = 0u, T_BLAS = 2u;
constexpr unsigned IDX_MASK = (1u << 24) - 1;

long cases = 0, bad = 0;

void check(unsigned meta, int start, unsigned level) {
    const bool blas = level == T_BLAS;
    const jtk::BakedNode b = jtk::bake_node(meta, start, level);
    const bool blas_leaf = blas && !(meta >> 24);
    bool words = (b.meta & 0xffffu) == (meta & 0xffffu) && (b.e0 & IDX_MASK) == (unsigned)start;
    if (blas_leaf) words = words && b.e0 == (unsigned)start;
    for (int negmask = 0; negmask < 8; negmask++)
    for (int sp = 0; sp <= 28; sp++) {
        const jtk::PushPlan ref = jtk::push_plan(meta, start, level, blas, negmask, sp);
        const jtk::PushPlan got = jtk::push_plan_baked(b.e0, b.meta, negmask | jtk::BAKE_MASK_BIT, sp);
        cases++;
        bool ok = words && got.npush == ref.npush && got.leaf == ref.leaf;
        for (int j = 0; j < jtk::PUSH_SLOTS; j++) ok = ok && got.slot[j] == ref.slot[j] && (ref.npush == 0 ? got.slot[j] == sp : got.value[j] == ref.value[j]);
        if (!ok && bad++ < 10)
            std::fprintf(stderr, "push_baked_check: meta=%08x start=%d level=%u negmask=%d sp=%d: npush %d (%d) leaf %d (%d) "
                         "values %08x %08x %08x %08x (%08x %08x %08x %08x) words %d\n",
                         meta, start, level, negmask, sp, got.npush, ref.npush, (int)got.leaf, (int)ref.leaf, got.value[0],
                         got.value[1], got.value[2], got.value[3], ref.value[0], ref.value[1], ref.value[2], ref.value[3],
                         (int)words);
    }
}

}  // namespace

int main() {
    const int starts[] = {0, 1, (1 << 24) - 5, (1 << 24) - 2};
    const unsigned blas_counts[] = {1, 2, 3, 4, 65535};
    for (int start : starts) {
        for (unsigned level = T_TLAS; level <= T_BLAS; level += T_BLAS)
            for (unsigned axis = 0; axis < 3; axis++) check(1u << 24 | axis << 16, start, level);
        // (a TLAS leaf's instances start .. start+num-1 are 24-bit indices: the host layout rejects a
        // scene with more, and push_plan's `tag | index` is not defined past them)
        for (unsigned num = 1; num <= 4; num++)
            if ((unsigned)start + num - 1u <= IDX_MASK) check(num, start, T_TLAS);
        for (unsigned num : blas_counts) check(num, start, T_BLAS);
    }
    std::printf("push_baked_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
