// jt_error.h — the per-pixel error estimate's launch and its context entry; the kernel and the
// context's half (jt_get_variance, jt_get_noise) are in jt_error.hip. Not part of the ABI; only
// .hip units include it (wave_sum_f is device code).
#pragma once

#include <hip/hip_runtime.h>

#include "jt_records.h"

namespace jt {

constexpr int ERR_BLOCK = 256;  // threads per workgroup: four 8x8 tiles, as combine_kernel's

// One launch over the slots of a context's stream means (DAccum::part_img, jt_launch.h): thread
// g is launch slot g (slot_pixel, jt_plan.h), stream j's record of its pixel is
// part_img[j * nslot + g]. The launch's share of the tiles is carried here rather than as the
// context's DParams: the kernel's arguments stay these few words.
struct DError {
    const float4* part_img;
    const float4* image;      // the combined means, as combine_kernel wrote them
    float4* var;              // float4[width * height]: the variance of the mean per channel
    float2* block_sums;       // one (V, M) pair per workgroup
    int nslot;
    int width, height;
    int tiles;                // launch tiles (launch_tiles)
    int tile_stride, tile_offset;
    int ns;                   // streams that hold a sample, >= 2
    float w[JT_MAX_STREAMS];  // their weights n_j / n: the last launch's DCombine
};

// workgroups of the launch: every slot of the launch's tiles
inline int error_blocks(int tiles) { return (int)(((long long)tiles * 64 + ERR_BLOCK - 1) / ERR_BLOCK); }

// Enqueues the kernel on `stream`; nothing waits, the caller synchronises.
hipError_t error_launch(hipStream_t stream, const DError& E);

}  // namespace jt

namespace jtk {

// the wave's sum in lane 0, in a fixed order: for off = 32, 16, ..., 1: v[l] += v[l + off]
// (error_kernel's sums and adapt_kernel's tile sums, jt_adapt.hip; restated in tests/adapt_ref.py)
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum
}

}  // namespace jtk

struct jt_ctx;

namespace jtc {

// The error estimate of a context's current samples, into jt_ctx::err_var / err_noise: every check
// of jt_get_variance (include/jtrace.h) in its order, the flush, then one launch unless the
// result is already valid for these samples. Its readers: jt_get_variance, jt_get_noise and
// jt_denoise_guided (jt_denoise.hip).
int estimate_error(jt_ctx* c);

}  // namespace jtc
