// push_check.cpp — the push plan of the binary node step (csrc/jt_push.h) against the branch-and-
// loop form it replaces, enumerated on the host. tests/test_push_plan.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
// For every node kind (internal, TLAS leaf, BLAS leaf), level (TLAS, BLAS), axis, negmask, leaf
// count 0..4, start and stack size sp 0..15 it runs the reference arms (restated below from
// jtk::node_step as it was: two pushes for an internal node, a loop over a TLAS leaf's instances,
// the leaf cursor for a BLAS leaf) and the plan's four unconditional writes on sentinel-filled
// stacks, and checks that
//   - slots [sp, sp + npush) hold the reference's entries, in its order,
//   - no slot outside [sp, sp + max(npush, 1)) changed (slot sp is the entry just popped: free),
//   - sp, prim and nprim end as the reference leaves them.
// The stack has 16 slots; 4 guard slots behind it let the combinations with sp + npush > 16, which
// stack_bound excludes on the device, run through the same checks.
#include <cstdio>

#include "../julia-raytracer_amd/csrc/jt_push.h"

namespace {

constexpr unsigned T_TLAS = 0u, T_INST = 1u, T_BLAS = 2u;
constexpr unsigned SNAP_NONE = 63u << 24;
constexpr int SLOTS = 16, GUARD = 4;
constexpr unsigned SENTINEL = 0xdeadbeefu;

struct Lane {
    unsigned stack[SLOTS + GUARD];
    int sp, prim, nprim;
};

void ref_push(Lane& L, unsigned e) {
    L.stack[L.sp] = e;
    L.sp += 1;
}
// the arms of jtk::node_step before the push plan (fixed stack, no child pre-test)
void ref_step(Lane& L, unsigned meta, int start, unsigned type, int negmask) {
    const bool blas = type == T_BLAS;
    const int num = (int)(meta & 0xffffu);
    if (meta >> 24) {
        const int axis = (int)((meta >> 16) & 0xffu);
        const bool neg = (negmask >> axis) & 1;
        const unsigned tag = type << 30 | SNAP_NONE;
        const unsigned c_second = (unsigned)(neg ? start + 1 : start), c_first = (unsigned)(neg ? start : start + 1);
        ref_push(L, tag | c_second);
        ref_push(L, tag | c_first);
    } else if (!blas) {
        for (int k = num - 1; k >= 0; k--) ref_push(L, (T_INST << 30) | SNAP_NONE | (unsigned)(start + k));
    } else {
        L.prim = start;
        L.nprim = num;
    }
}
// the straight-line form, as jtk::node_step applies the plan
int new_step(Lane& L, unsigned meta, int start, unsigned type, int negmask) {
    const jtk::PushPlan p = jtk::push_plan(meta, start, type, type == T_BLAS, negmask, L.sp);
    for (int j = 0; j < jtk::PUSH_SLOTS; j++) {
        if (p.slot[j] < 0 || p.slot[j] >= SLOTS + GUARD) return -1;
        L.stack[p.slot[j]] = p.value[j];
    }
    L.sp += p.npush;
    L.prim = p.leaf ? start : L.prim;
    L.nprim = p.leaf ? (int)(meta & 0xffffu) : L.nprim;
    return p.npush;
}

}  // namespace

int main() {
    long cases = 0, bad = 0;
    const int starts[] = {0, 1, 7, 4093, (1 << 24) - 6};
    for (int internal = 0; internal < 2; internal++)
    for (unsigned type = T_TLAS; type <= T_BLAS; type += T_BLAS)
    for (int axis = 0; axis < 3; axis++)
    for (int negmask = 0; negmask < 8; negmask++)
    for (int num = 0; num <= 4; num++)
    for (int start : starts)
    for (int sp = 0; sp < SLOTS; sp++) {
        const unsigned meta = (unsigned)internal << 24 | (unsigned)(internal ? axis : 0) << 16 | (unsigned)num;
        Lane ref, got;
        for (int k = 0; k < SLOTS + GUARD; k++) ref.stack[k] = got.stack[k] = SENTINEL;
        ref.sp = got.sp = sp;
        ref.prim = got.prim = 12345;
        ref.nprim = got.nprim = 0;
        ref_step(ref, meta, start, type, negmask);
        const int npush = new_step(got, meta, start, type, negmask);
        cases++;
        bool ok = npush == ref.sp - sp && got.sp == ref.sp && got.prim == ref.prim && got.nprim == ref.nprim;
        const int end = sp + (npush > 1 ? npush : 1);
        for (int k = 0; ok && k < SLOTS + GUARD; k++) {
            if (k >= sp && k < sp + npush) ok = got.stack[k] == ref.stack[k];  // the entries, in order
            else if (k < sp || k >= end) ok = got.stack[k] == SENTINEL;        // nothing else written
        }
        if (!ok && bad++ < 10)
            std::fprintf(stderr, "push_check: internal=%d type=%u axis=%d negmask=%d num=%d start=%d sp=%d: npush %d (reference %d)\n",
                         internal, type, axis, negmask, num, start, sp, npush, ref.sp - sp);
    }
    std::printf("push_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
