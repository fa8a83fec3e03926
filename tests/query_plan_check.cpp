// query_plan_check.cpp — the integer rules of a ray-query launch (csrc/jt_intersect.h) enumerated on the
// host. tests/test_query_plan.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
//   - query_grid: at least one workgroup, one lane per ray up to the persistent grid, never more
//     than cus * QUERY_WG_PER_CU workgroups, monotone in n;
//   - query_ovf_entries: every lane's area [slot * need, slot * need + need) of the grid lies inside
//     it, also at the largest grid and bound (no 32-bit wrap);
//   - query_claim_rays: a power of two in [64, QUERY_CLAIM_MAX], above 64 only while every wave of
//     the grid can have a claim; and the refill's hand-out, run on jtq::WaveReserve, the struct the
//     kernels' refill runs (csrc/jt_feed.h): waves that claim that many consecutive rays with one
//     add, hand them to their idle lanes and stop at the first claim starting at or past n hand
//     every ray out exactly once, whatever the order of the refills, and the counter stays below
//     query_counter_bound (< 2^32);
//   - query_stage_rays: enough for the call, unchanged while the call fits, at least doubling when
//     it grows, a multiple of 1024, never above QUERY_MAX_RAYS.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_intersect.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "query_plan_check: %s (%lld %lld %lld)\n", what, a, b, c);
}

constexpr int BLOCK = jtk::BLOCK;

void check_grid() {
    const int64_t ns[] = {1, 2, 63, 64, 65, 255, 256, 257, 4099, 65536, 524287, 524288, 524289, 2623360, jtq::QUERY_MAX_RAYS};
    for (int cus : {1, 2, 8, 64, 104, 256, 304}) {
        int prev = 0;
        for (int64_t n : ns) {
            const int g = jtq::query_grid(n, cus);
            check(g >= 1 && g <= cus * jtq::QUERY_WG_PER_CU, "grid outside [1, cus * 8]", n, cus, g);
            check((int64_t)g * BLOCK >= n || g == cus * jtq::QUERY_WG_PER_CU, "a partial grid with fewer lanes than rays", n, cus, g);
            check((int64_t)(g - 1) * BLOCK < n, "a workgroup without a first ray", n, cus, g);
            check(g >= prev, "grid not monotone in n", n, cus, g);
            prev = g;
        }
    }
    check(jtq::query_grid(5, 0) == 1 && jtq::query_grid(5, -3) == 1, "no compute units reported");
}

void check_ovf() {
    for (int grid : {1, 3, 2048, 304 * 8})
        for (int need : {17, 28, 46, 128}) {
            const size_t entries = jtq::query_ovf_entries(grid, need);
            const size_t last_slot = (size_t)grid * BLOCK - 1;
            check(last_slot * (size_t)need + (size_t)need == entries, "the last lane's area does not end the overflow area", grid, need);
            check((unsigned long long)entries == (unsigned long long)grid * BLOCK * (unsigned long long)need, "overflow area size wraps", grid, need);
        }
}

// the waves of query_grid(n, cus) claim query_claim_rays rays at a time and hand them to between
// QUERY_REFILL_LANES and 64 idle lanes per refill, until each has seen a claim start at or past n:
// jtq::WaveReserve's members, called as feed_refill (csrc/jt_feed.h) calls them. The next wave to
// refill and its idle lanes come from a small generator (every order is a valid run)
void check_claims(int64_t n, int cus, unsigned seed) {
    const int grid = jtq::query_grid(n, cus), waves = grid * (BLOCK / 64);
    const int claim = jtq::query_claim_rays(n, grid);
    check(claim >= 64 && claim <= jtq::QUERY_CLAIM_MAX && (claim & (claim - 1)) == 0, "claim size", n, cus, claim);
    check(claim == 64 || (int64_t)claim * waves <= n, "a claim that leaves waves without rays", n, cus, claim);
    std::vector<int> taken((size_t)n, 0);
    std::vector<jtq::WaveReserve> reserve((size_t)waves);
    uint64_t counter = 0;  // 64 bits here, so that a wrap of the kernels' 32-bit counter shows against its bound
    int left = waves;
    unsigned s = seed;
    auto rnd = [&]() { return (s = s * 1664525u + 1013904223u) >> 8; };
    while (left > 0) {
        size_t w = rnd() % (unsigned)waves;
        while (reserve[w].drained) w = (w + 1) % (size_t)waves;
        jtq::WaveReserve& r = reserve[w];
        const unsigned idle = (unsigned)jtq::QUERY_REFILL_LANES + rnd() % (unsigned)(64 - jtq::QUERY_REFILL_LANES + 1);
        if (r.empty()) {  // feed_refill's atomicAdd
            r.claimed((unsigned)counter, (unsigned)claim, (unsigned)n);
            counter += (uint64_t)claim;
            if (r.drained) {
                left--;
                continue;
            }
        }
        const unsigned take = r.take(idle);
        for (unsigned k = 0; k < take; k++) taken[(size_t)(r.next + k)]++;
        r.next += take;
    }
    long wrong = 0;
    for (int v : taken) wrong += v != 1;
    check(wrong == 0, "rays not claimed exactly once", n, waves, wrong);
    check(counter <= jtq::query_counter_bound(n, grid), "ray counter above its bound", n, waves, (long long)counter);
}

void check_stage() {
    const int64_t ns[] = {1, 63, 1024, 1025, 4099, 2623360, jtq::QUERY_MAX_RAYS - 1, jtq::QUERY_MAX_RAYS};
    for (int64_t have : {(int64_t)0, (int64_t)1024, (int64_t)5120, (int64_t)1 << 22, jtq::QUERY_MAX_RAYS})
        for (int64_t n : ns) {
            const int64_t cap = jtq::query_stage_rays(have, n);
            check(cap >= n && cap >= have, "staging too small", have, n, cap);
            check(cap <= jtq::QUERY_MAX_RAYS, "staging above the largest call", have, n, cap);
            if (n <= have) check(cap == have, "staging regrown though the call fits", have, n, cap);
            else check(cap % 1024 == 0 && (cap >= 2 * have || cap == jtq::QUERY_MAX_RAYS), "staging growth", have, n, cap);
        }
}

}  // namespace

int main() {
    check_grid();
    check_ovf();
    for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)257, (int64_t)4099, (int64_t)100003})
        for (int cus : {1, 2, 64, 256, 304})
            for (unsigned seed : {1u, 2u, 3u}) check_claims(n, cus, seed);
    check_claims((int64_t)1 << 22, 256, 4u);
    check(jtq::query_claim_rays((int64_t)1 << 22, jtq::query_grid((int64_t)1 << 22, 256)) == jtq::QUERY_CLAIM_MAX, "the measured launch's claim");
    check(jtq::query_claim_rays(4099, jtq::query_grid(4099, 256)) == 64, "a small call's claim");
    // the largest call on the largest grid: the counter's bound fits the kernel's 32-bit counter
    check(jtq::query_counter_bound(jtq::QUERY_MAX_RAYS, 304 * jtq::QUERY_WG_PER_CU) < ((uint64_t)1 << 32), "counter bound above 2^32");
    check_stage();
    std::printf("query_plan_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
