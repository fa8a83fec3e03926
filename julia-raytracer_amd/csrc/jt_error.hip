// jt_error.hip — the per-pixel error estimate (include/jtrace.h: jt_get_variance, jt_get_noise):
// the between-stream variance of a context's k > 1 sample streams (DESIGN.md §Error estimate).
//
// One pixel per lane over the launch's tile slots, as combine_kernel (jt_trace.hip) reads them:
// stream j's records of neighbouring slots are contiguous, so every load is a coalesced 16 B per
// lane, and the unrolled pass keeps eight streams' loads in flight. The image is read, not
// recombined: the estimate is about the pixel the caller gets. Each workgroup also sums its
// pixels' (V, M) contributions — shuffles within a wave, LDS across the four waves — and writes
// one pair; the host adds the pairs in double. No atomics: the result does not depend on the
// order the workgroups run in.
#include <hip/hip_runtime.h>

#include "jt_error.h"

namespace jtk {

using jt::DError;
using jt::ERR_BLOCK;

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum
}

__global__ __launch_bounds__(ERR_BLOCK) void error_kernel(DError E) {
    const int tiles_x = (E.width + 7) / 8;
    const int g = (int)(blockIdx.x * ERR_BLOCK + threadIdx.x);  // < 2^26 + 256 (jt_create's tile limit)
    // slots past the launch's tiles and pixels of an edge tile outside the image add 0 to the sums
    float v = 0.0f, m = 0.0f;
    if (g < E.tiles * 64) {
        const int t = (g >> 6) * E.tile_stride + E.tile_offset, l = g & 63;
        const int i = (t % tiles_x) * 8 + (l & 7), j = (t / tiles_x) * 8 + (l >> 3);
        if (i < E.width && j < E.height) {
            const size_t pixel = (size_t)j * E.width + i, ns = (size_t)E.nslot;
            const float4 mu = E.image[pixel];
            float ax = 0.0f, ay = 0.0f, az = 0.0f, aw = 0.0f;
            // acc = acc + (d * d) * w_j in stream order (-ffp-contract=off: no FMA)
#pragma unroll 8
            for (int s = 0; s < E.ns; s++) {
                const float w = E.w[s];
                const float4 a = E.part_img[s * ns + g];
                const float dx = a.x - mu.x, dy = a.y - mu.y, dz = a.z - mu.z, dw = a.w - mu.w;
                ax = ax + (dx * dx) * w, ay = ay + (dy * dy) * w, az = az + (dz * dz) * w, aw = aw + (dw * dw) * w;
            }
            const float den = (float)(E.ns - 1);
            const float4 var = make_float4(ax / den, ay / den, az / den, aw / den);
            E.var[pixel] = var;
            v = (var.x + var.y) + var.z;
            m = (mu.x + mu.y) + mu.z;
        }
    }
    __shared__ float2 wsum[ERR_BLOCK / 64];
    v = wave_sum_f(v);
    m = wave_sum_f(m);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = make_float2(v, m);
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 r = wsum[0];
#pragma unroll
        for (int k = 1; k < ERR_BLOCK / 64; k++) r = make_float2(r.x + wsum[k].x, r.y + wsum[k].y);
        E.block_sums[blockIdx.x] = r;
    }
}

}  // namespace jtk

namespace jt {

hipError_t error_launch(hipStream_t stream, const DError& E) {
    const int nblk = error_blocks(E.tiles);
    if (nblk > 0) hipLaunchKernelGGL(jtk::error_kernel, dim3(nblk), dim3(ERR_BLOCK), 0, stream, E);
    return hipGetLastError();
}

}  // namespace jt
