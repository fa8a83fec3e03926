// radiance_plan_check.cpp — the integer rules of a jt_radiance launch (csrc/jt_radiance.h) enumerated
// on the host. tests/test_radiance_host.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
//   - radiance_step, for every (np, nn, ns) a wave of 64 lanes can vote: the kind chosen has a lane
//     that takes part whenever some lane wants a step (so every iteration advances a lane: the
//     kernel's termination argument), a shading step runs exactly when lanes wait for one and either
//     RADIANCE_SHADE_LANES of them do or no lane can traverse, and the traversal kinds follow the ray
//     queries' vote;
//   - a replay of that vote on lanes with random query lengths: every lane finishes all its
//     queries in a bounded number of iterations;
//   - the lane's LDS slots: the mean, the sample and the parked path state do not overlap, and the
//     workgroup's static LDS is what the kernel declares;
//   - radiance_range_error: each rule at its boundary, in the header's order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_radiance.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "radiance_plan_check: %s (%lld %lld %lld)\n", what, a, b, c);
}

void check_step() {
    for (int np = 0; np <= 64; np++)
        for (int nn = 0; np + nn <= 64; nn++)
            for (int ns = 0; np + nn + ns <= 64; ns++) {
                const int k = jtr::radiance_step(np, nn, ns);
                check(k == jtr::STEP_PRIM || k == jtr::STEP_NODE || k == jtr::STEP_SHADE, "no step kind", np, nn, ns);
                const int lanes = k == jtr::STEP_PRIM ? np : k == jtr::STEP_NODE ? nn : ns;
                if (np + nn + ns > 0) check(lanes > 0, "a step without a lane", np, nn, ns);
                const bool shade = ns > 0 && (np + nn == 0 || ns >= jtr::RADIANCE_SHADE_LANES);
                check((k == jtr::STEP_SHADE) == shade, "the shading gate", np, nn, ns);
                if (!shade && np + nn > 0)
                    check((k == jtr::STEP_PRIM) == (np * jtq::QUERY_VOTE_P >= nn), "the traversal vote is not the ray queries'", np, nn, ns);
            }
}

// 64 lanes, each with a number of queries of random lengths (node steps with primitive steps among
// them), advanced by the vote as the kernel's loop does: all finish within three times the steps and
// shading steps they have in all (an iteration advances at least one lane)
void check_replay() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&] {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    for (int round = 0; round < 200; round++) {
        struct Lane {
            int queries, steps;  // queries left; steps left of the current one
            bool prim;           // the next step's kind
        };
        std::vector<Lane> lanes(64);
        for (Lane& l : lanes) {
            l.queries = (int)(next() % 6);
            l.steps = l.queries ? (int)(next() % 40) : 0;
            l.prim = next() & 1;
        }
        long long budget = 0;
        for (const Lane& l : lanes) budget += (long long)l.queries * 41 + 1;
        budget *= 3;
        long long it = 0;
        for (;; it++) {
            int np = 0, nn = 0, ns = 0;
            for (const Lane& l : lanes) {
                if (!l.queries) continue;
                if (l.steps == 0) ns++;
                else if (l.prim) np++;
                else nn++;
            }
            if (np + nn + ns == 0) break;
            if (it > budget) break;
            const int k = jtr::radiance_step(np, nn, ns);
            for (Lane& l : lanes) {
                if (!l.queries) continue;
                if (k == jtr::STEP_SHADE && l.steps == 0) {
                    l.queries--;
                    l.steps = l.queries ? (int)(next() % 40) : 0;
                    l.prim = next() & 1;
                } else if (l.steps > 0 && ((k == jtr::STEP_PRIM && l.prim) || (k == jtr::STEP_NODE && !l.prim))) {
                    l.steps--;
                    l.prim = next() & 1;
                }
            }
        }
        check(it <= budget, "the replay did not finish within its bound", round, it, budget);
    }
}

void check_slots() {
    check(jtr::RADIANCE_ACC == 0 && jtr::RADIANCE_SAMPLE == jtr::RADIANCE_ACC + 4, "the mean's four slots, then the sample");
    check(jtr::RADIANCE_PARK == jtr::RADIANCE_SAMPLE + 1, "the parked state follows the sample");
    check(jtr::RADIANCE_SLOTS == jtr::RADIANCE_PARK + jtk::PARK_SLOTS && jtk::park(jtd::FT_ALL), "PARK_SLOTS parked slots");
    check(jtr::RADIANCE_LDS_BYTES == (size_t)(16 + jtr::RADIANCE_SLOTS) * 256 * 4 + 2048, "the workgroup's static LDS", (long long)jtr::RADIANCE_LDS_BYTES);
    check(jtr::RADIANCE_LDS_BYTES <= 64 * 1024 && 160 * 1024 / jtr::RADIANCE_LDS_BYTES >= 4, "at least four workgroups per compute unit by LDS");
}

void check_range() {
    const int64_t M = jtq::QUERY_MAX_RAYS, S = jtr::RADIANCE_MAX_STREAM;
    auto has = [](const char* msg, const char* word) { return msg && std::strstr(msg, word) != nullptr; };
    check(jtr::radiance_range_error(0, 0, 0, 1) == nullptr, "n = 0 is in range");
    check(jtr::radiance_range_error(M, S - M, 0, 1) == nullptr, "the largest call is in range");
    check(jtr::radiance_range_error(1, 0, 0, 1 << 24) == nullptr, "2^24 samples are in range");
    check(jtr::radiance_range_error(1, 0, INT32_MAX - 1, INT32_MAX) == nullptr, "the last sample is in range");
    check(has(jtr::radiance_range_error(-1, 0, 0, 1), "n must"), "n < 0");
    check(has(jtr::radiance_range_error(M + 1, 0, 0, 1), "n must"), "n > 2^30");
    check(has(jtr::radiance_range_error(1, -1, 0, 1), "stream_base must"), "stream_base < 0");
    check(has(jtr::radiance_range_error(M, S - M + 1, 0, 1), "stream_base + n"), "stream_base + n > 2^31");
    check(has(jtr::radiance_range_error(1, INT64_MAX, 0, 1), "stream_base + n"), "stream_base + n does not wrap");
    check(has(jtr::radiance_range_error(1, 0, -1, 1), "sample_begin"), "sample_begin < 0");
    check(has(jtr::radiance_range_error(1, 0, 3, 3), "sample_end must"), "an empty range");
    check(has(jtr::radiance_range_error(1, 0, 3, 2), "sample_end must"), "a reversed range");
    check(has(jtr::radiance_range_error(1, 0, 0, (1 << 24) + 1), "2^24"), "more than 2^24 samples");
    // the order: the first failing rule of the list is the one named
    check(has(jtr::radiance_range_error(-1, -1, -1, -1), "n must"), "n before stream_base");
    check(has(jtr::radiance_range_error(1, -1, -1, -1), "stream_base must"), "stream_base before sample_begin");
    check(has(jtr::radiance_range_error(1, 0, -1, -2), "sample_begin"), "sample_begin before sample_end");
    check(has(jtr::radiance_range_error(1, 0, 0, 0), "sample_end must"), "sample_end before the count");
}

}  // namespace

int main() {
    check_step();
    check_replay();
    check_slots();
    check_range();
    std::printf("radiance_plan_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
