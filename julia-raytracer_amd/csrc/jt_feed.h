// jt_feed.h — the ray hand-out of a persistent grid over the caller's rays (query_kernel,
// jt_intersect.hip; radiance_kernel, jt_radiance.hip): a launch's ray counter and a wave's refill of
// its idle lanes from it. The integer rules are jtq::WaveReserve's (jt_intersect.h), which the host
// check replays. A per-wave device function, beside jt_traverse.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_intersect.h"

namespace jtk {

struct DFeed {
    unsigned* counter;  // the next ray to claim (zeroed before the launch)
    int n;              // rays of the launch
    unsigned claim;     // rays a wave claims with one atomic (query_claim_rays)
};

// One refill, at the top of every iteration of a wave (wave-uniform control). false: every ray is
// claimed and no lane of the wave has one, the wave is done. Once QUERY_REFILL_LANES lanes have no
// ray (has_ray false), the k-th of them takes the k-th ray of the wave's reserve, take(ray); an
// empty reserve is first refilled with F.claim consecutive rays, claimed by the wave's first lane
// with one atomicAdd.
template <class Take>
__device__ __forceinline__ bool feed_refill(const DFeed& F, jtq::WaveReserve& w, bool has_ray, Take&& take) {
    const unsigned long long idle = __builtin_amdgcn_ballot_w64(!has_ray);
    const int nidle = __popcll(idle);
    if (nidle == 64 && w.drained) return false;
    if (!w.drained && nidle >= jtq::QUERY_REFILL_LANES) {
        if (w.empty()) {
            unsigned base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(F.counter, F.claim);
            w.claimed(__builtin_amdgcn_readfirstlane(base), F.claim, (unsigned)F.n);
        }
        if (!w.drained) {
            const unsigned ntake = w.take((unsigned)nidle);
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
            if (!has_ray && rank < ntake) take((int)(w.next + rank));
            w.next += ntake;
        }
    }
    return true;
}

}  // namespace jtk
