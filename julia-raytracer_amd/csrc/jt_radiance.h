// jt_radiance.h — the integer rules of a jt_radiance or jt_irradiance launch (include/jtrace.h; the
// kernel and the context's half are in jt_radiance.hip): the argument bounds, the lane's LDS slots
// and the step-kind vote of a wave. The grid, the claim size and the overflow area are the ray
// queries' (jt_intersect.h). Plain C++ (no HIP runtime), shared by jt_radiance.hip and the host
// check (tests/radiance_plan_check.cpp). Not part of the ABI.
#pragma once

#include <stdint.h>

#include "jt_intersect.h"

namespace jtr {

constexpr int64_t RADIANCE_MAX_STREAM = (int64_t)1 << 31;  // stream_base + n at most: rng_init's stream is 32 bits
constexpr int64_t RADIANCE_MAX_SAMPLES = (int64_t)1 << 24;  // samples of one call: (float)(c + 1) is exact

// Per-lane LDS slots (slot k of a lane at [k * BLOCK]): the running mean rgba, the sample in
// flight, then Path::pk's parked path state (PARK_SLOTS: park(FT_ALL) is true).
constexpr int RADIANCE_ACC = 0, RADIANCE_SAMPLE = 4, RADIANCE_PARK = 5;
constexpr int RADIANCE_SLOTS = RADIANCE_PARK + jtk::PARK_SLOTS;
// static LDS of a workgroup: the stack ring, the lane slots and the texel-decode LUTs (tex_lut)
constexpr size_t RADIANCE_LDS_BYTES = (size_t)(jtq::QUERY_RING + RADIANCE_SLOTS) * jtk::BLOCK * 4 + 2048;

// Tuning knobs, measured on cornellbox and features2 at 1280x720x16 (EXPERIMENTS.md, "Radiance along
// the caller's rays"; -D overrides are for A/B builds). Waves per SIMD the kernel is compiled for
// (0: the compiler's choice, 190 VGPRs and 2 waves): 3 waves (168 VGPRs, 17 spilled) +15 % and
// +9 %; 4 waves (128 VGPRs, 231 spilled) a third of the rate. Node pops per node iteration, the
// megakernel's JT_NODE_REPEAT: 3 against 1 +10 % and +11 %.
#ifndef JT_RADIANCE_WAVES
#define JT_RADIANCE_WAVES 3
#endif
#ifndef JT_RADIANCE_NODE_REPEAT
#define JT_RADIANCE_NODE_REPEAT 3
#endif
constexpr int RADIANCE_NODE_REPEAT = JT_RADIANCE_NODE_REPEAT;
// Where jt_probe_sh's 36 running sums live (EXPERIMENTS.md, "The sphere source and the SH
// projection"): 0, the lane's own output record in HBM, read and written per finished sample; 1
// (an A/B build), 36 more LDS slots per lane, which takes the workgroup from 31 744 to 68 608 B
// and the CU from three workgroups to two.
#ifndef JT_PROBE_LDS
#define JT_PROBE_LDS 0
#endif

// The step kind of a wave's iteration, from the lanes that want each: np a primitive test, nn a
// node step, ns a shading step (their query is done). Traversal steps are picked by the ray
// queries' biased vote; a shading step, whose code is by far the longest, runs once
// RADIANCE_SHADE_LANES lanes wait for it (32: +15 % and +5 % over 16, 48 slower than 32), or when
// no lane can do anything else. Some lane takes
// part in the step chosen whenever np + nn + ns > 0, so every iteration advances a lane.
#ifndef JT_RADIANCE_SHADE_LANES
#define JT_RADIANCE_SHADE_LANES 32
#endif
constexpr int RADIANCE_SHADE_LANES = JT_RADIANCE_SHADE_LANES;
enum : int { STEP_PRIM = 0, STEP_NODE = 1, STEP_SHADE = 2 };
constexpr int radiance_step(int np, int nn, int ns) {
    return ns > 0 && (np + nn == 0 || ns >= RADIANCE_SHADE_LANES) ? STEP_SHADE
           : np * jtq::QUERY_VOTE_P >= nn                          ? STEP_PRIM
                                                                   : STEP_NODE;
}

// Where a sample's ray comes from (radiance_kernel's SOURCE): the caller's ray record as it stands
// (jt_radiance), or the caller's point record (position, normal) and a cosine-weighted direction
// about the normal drawn from the sample's own stream (jt_irradiance, jt_hemisphere_rays)
enum : int { SOURCE_RAY = 0, SOURCE_HEMISPHERE = 1, SOURCE_SPHERE = 2 };
// SOURCE_SPHERE: the caller's record is a position alone and the direction a uniform draw over the
// whole sphere from the sample's stream (jt_probe_sh, jt_sphere_rays). The floats of a source's
// record, a compile-time property of the source: whoever reads record i reads it at this stride.
constexpr int source_stride(int source) { return source == SOURCE_SPHERE ? 3 : 6; }

// jt_probe_sh's host variant runs the caller's array in chunks of at most this many points, each
// staged and copied out on its own (a probe's record is 144 bytes): stream_base advances with the
// chunks, which the contract makes bit-identical to one call. The option test_probe_chunk (tests
// only) lowers it.
constexpr int64_t PROBE_MAX_CHUNK = (int64_t)1 << 22;
constexpr int64_t probe_chunk(int64_t option) { return option >= 1 && option < PROBE_MAX_CHUNK ? option : PROBE_MAX_CHUNK; }

// the argument rules of jt_radiance that do not need the context, in the header's order; nullptr:
// all hold, else the message
constexpr const char* radiance_range_error(int64_t n, int64_t stream_base, int32_t sample_begin, int32_t sample_end) {
    return n < 0                                                          ? "n must be at least 0"
           : n > jtq::QUERY_MAX_RAYS                                      ? "n must be at most 2^30 rays"
           : stream_base < 0                                              ? "stream_base must be at least 0"
           : stream_base > RADIANCE_MAX_STREAM - n                        ? "stream_base + n must be at most 2^31"
           : sample_begin < 0                                             ? "sample_begin must be at least 0"
           : sample_end <= sample_begin                                   ? "sample_end must be greater than sample_begin"
           : (int64_t)sample_end - sample_begin > RADIANCE_MAX_SAMPLES    ? "sample_end - sample_begin must be at most 2^24 samples"
                                                                          : nullptr;
}

// jt_ambient_occlusion's rules after jt_radiance's range. The radius: greater than 0, +inf allowed
// (an unbounded query); NaN fails the comparison and is refused with 0 and the negatives.
constexpr const char* occlusion_radius_error(float radius) {
    return radius > 0.0f ? nullptr : "radius must be greater than 0 (+inf: unbounded)";
}
// The visibility of a point: the samples whose query found nothing over the samples of the call,
// both exact in float32 (at most RADIANCE_MAX_SAMPLES), one float32 division: a value that does
// not depend on the order in which the samples finished.
constexpr float occlusion_visibility(int visible, int samples) { return (float)visible / (float)samples; }

}  // namespace jtr
