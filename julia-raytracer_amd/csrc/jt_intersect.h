// jt_intersect.h — the integer rules of a ray queries' launch (include/jtrace.h: jt_intersect,
// jt_occluded; the kernel and the context's half are in jt_intersect.hip): the persistent grid for n
// rays, the size of its stack overflow area, a wave's reserve of claimed rays (the refill of
// jt_feed.h runs it), the growth of the host variants' staging buffers.
// Plain C++ (no HIP runtime), shared by the kernels and the host check (tests/query_plan_check.cpp).
// Not part of the ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "jt_select.h"  // BLOCK

namespace jtq {

constexpr int64_t QUERY_MAX_RAYS = (int64_t)1 << 30;  // rays of one call (the ray counter is 32 bits)
constexpr int QUERY_WG_PER_CU = 8;  // workgroups per compute unit of the persistent grid, at most
constexpr int QUERY_RING = 16;      // entries of the LDS stack ring: 16 KiB per workgroup
// a wave hands new rays to its finished lanes once this many of them have none: fewer and a
// refill's ray loads serve few lanes, more and finished lanes idle longer
constexpr int QUERY_REFILL_LANES = 16;
// the step-kind vote: one lane that wants a primitive test outvotes this many that want a node step
// (the megakernel's JT_VOTE_P)
constexpr int QUERY_VOTE_P = 3;

// Workgroups of the launch for n >= 1 rays: one lane per ray up to the persistent grid of
// cus * QUERY_WG_PER_CU workgroups, whose waves then claim the other rays as their lanes finish.
inline int query_grid(int64_t n, int cus) {
    const int64_t full = (int64_t)(cus < 1 ? 1 : cus) * QUERY_WG_PER_CU;
    const int64_t want = (n + jtk::BLOCK - 1) / jtk::BLOCK;
    return (int)(want < 1 ? 1 : want < full ? want : full);
}

// Entries (ints) of the grid's HBM stack overflow area: the scene's stack bound `need` per lane;
// a lane's slot is blockIdx.x * BLOCK + threadIdx.x.
inline size_t query_ovf_entries(int grid, int need) { return (size_t)grid * jtk::BLOCK * (size_t)need; }

// Rays a wave claims with one atomicAdd on the launch's ray counter, its reserve for the next
// refills: QUERY_CLAIM_MAX when every wave of the grid can have that many (one same-address
// atomic per refill bound a launch of 2^22 rays to 2.4 ms), down to 64, a ray per lane, for a
// small call, so that its rays spread over all its waves; a power of two.
constexpr int QUERY_CLAIM_MAX = 256;
inline int query_claim_rays(int64_t n, int grid) {
    const int64_t waves = (int64_t)grid * (jtk::BLOCK / 64);
    int claim = 64;
    while (claim < QUERY_CLAIM_MAX && (int64_t)claim * 2 * waves <= n) claim *= 2;
    return claim;
}

// The most the ray counter reaches: the last claim that starts below n ends below n +
// QUERY_CLAIM_MAX, and every wave stops claiming at its first claim that starts at or past n: one
// more claim per wave of the grid (< 2^32: the counter is 32 bits).
inline uint64_t query_counter_bound(int64_t n, int grid) {
    return (uint64_t)n + (uint64_t)QUERY_CLAIM_MAX * ((uint64_t)grid * (jtk::BLOCK / 64) + 1);
}

// A wave's reserve of claimed rays [next, end), and what the refill does to it (feed_refill,
// jt_feed.h; replayed on the host by tests/query_plan_check.cpp). constexpr: device code runs the
// members too.
struct WaveReserve {
    unsigned next = 0, end = 0;
    bool drained = false;  // every ray of the launch is claimed: the wave claims no more
    constexpr bool empty() const { return next >= end; }
    // the wave's atomicAdd of `claim` on the ray counter of a launch of n rays returned `base`
    constexpr void claimed(unsigned base, unsigned claim, unsigned n) {
        next = base;
        end = base + claim < n ? base + claim : n;  // < 2^32: query_counter_bound
        drained = base >= n;
    }
    // rays that nidle idle lanes take; the k-th of them takes ray next + k, then next += take
    constexpr unsigned take(unsigned nidle) const { return nidle < end - next ? nidle : end - next; }
};

// n of a call outside 0 .. QUERY_MAX_RAYS: the message (`most`: the family's words for the upper
// bound), else nullptr
constexpr const char* query_count_error(int64_t n, const char* most) {
    return n < 0 ? "n must be at least 0" : n > QUERY_MAX_RAYS ? most : nullptr;
}

// Where a query's starting tmax comes from (query_kernel's BOUND): +inf as every query of the
// integrator (jt_intersect, jt_occluded), the caller's per-ray array (jt_intersect_bounded,
// jt_occluded_bounded), or the segment form of jt_visible: the record is (a, b), the ray
// (a, b - a) and the bound SEGMENT_TMAX for every ray
enum : int { BOUND_NONE = 0, BOUND_ARRAY = 1, BOUND_SEGMENT = 2 };
// jt_visible's bound in units of the segment: 1 - ray_eps in float32 (jt_device.h's ray_eps; the
// kernel's unit asserts the two agree), so both ends keep the same relative epsilon
constexpr float SEGMENT_TMAX = 1.0f - 0.0001f;

// Rays the staging buffers hold after a call of n rays when they held `have`: unchanged while n
// fits; else at least twice as many (so m growing calls copy O(m) buffers' worth), rounded up to
// 1024 rays, at most QUERY_MAX_RAYS.
inline int64_t query_stage_rays(int64_t have, int64_t n) {
    if (n <= have) return have;
    int64_t want = n > 2 * have ? n : 2 * have;
    want = (want + 1023) / 1024 * 1024;
    return want > QUERY_MAX_RAYS ? QUERY_MAX_RAYS : want;
}

}  // namespace jtq
