// jt_adapt.hip — adaptive sampling (include/jtrace.h: jt_adapt, jt_get_sample_counts): 8x8 tiles
// whose error estimate meets the image-level noise target handed down to them freeze, and the
// megakernel's hand-out skips their units from then on (DAccum::frozen, jt_kernels.h; DESIGN.md
// §6d "Adaptive sampling").
//
// One wave per tile over the launch's tile slots, as error_kernel (jt_error.hip) reads them: each
// lane loads its pixel's variance (16 B, rows of 128 B), the wave sums the channel sums in the
// order of wave_sum_f (jt_error.h), and lane 0 compares and records the sample count for a tile
// that newly freezes (an ordinary vector store). Each workgroup writes its count of tiles still active as
// one word; the host adds the words. No atomics: the result does not depend on the order the
// workgroups run in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "jt_adapt.h"
#include "jt_context.h"
#include "jt_error.h"

namespace jtk {

using jt::ADAPT_BLOCK;
using jt::DAdapt;

__global__ __launch_bounds__(ADAPT_BLOCK) void adapt_kernel(DAdapt D) {
    const int g = (int)(blockIdx.x * ADAPT_BLOCK + threadIdx.x);  // < 2^26 + 256 (jt_create's tile limit)
    const bool traced = g < D.tiles * 64;  // wave-uniform: a wave is one launch tile
    // pixels of an edge tile outside the image add 0 and are not counted in N_t
    float v = 0.0f;
    bool inside = false;
    if (traced) {
        const SlotPixel px = slot_pixel(g, D.width, D.height, D.tile_stride, D.tile_offset);
        inside = px.inside;
        if (inside) {
            const float4 var = D.var[(size_t)px.j * D.width + px.i];
            v = (var.x + var.y) + var.z;
        }
    }
    const float vt = wave_sum_f(v);
    const int nt = __popcll(__builtin_amdgcn_ballot_w64(inside));
    __shared__ unsigned wact[ADAPT_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        unsigned act = 0;
        if (traced) {
            const int t = (g >> 6) * D.tile_stride + D.tile_offset;  // < the image's tiles (plan_tiles)
            if (D.frozen_at[t] == 0u) {  // frozen tiles stay frozen
                if (vt <= (float)nt * D.vmax)
                    D.frozen_at[t] = D.n;
                else
                    act = 1;
            }
        }
        wact[threadIdx.x >> 6] = act;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = wact[0];
#pragma unroll
        for (int k = 1; k < ADAPT_BLOCK / 64; k++) r += wact[k];
        D.active[blockIdx.x] = r;
    }
}

}  // namespace jtk

namespace jt {

hipError_t adapt_launch(hipStream_t stream, const DAdapt& D) {
    const int nblk = adapt_blocks(D.tiles);
    if (nblk > 0) hipLaunchKernelGGL(jtk::adapt_kernel, dim3(nblk), dim3(ADAPT_BLOCK), 0, stream, D);
    return hipGetLastError();
}

}  // namespace jt

// ---- the context's half (jt_context.h)
using namespace jtc;

extern "C" {

int jt_adapt(jt_ctx* c, double noise_target, int32_t* active_tiles) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (!std::isfinite(noise_target) || !(noise_target > 0))
        return jt::fail(JT_ERR_INVALID, "noise_target must be finite and > 0");
    // every check of jt_get_variance, the flush, and the estimate of these samples (a valid one is reused)
    if (const int st = estimate_error(c)) return st;
    const long long n = c->next - c->first, k = 1LL << c->lk;
    if (n % k != 0)
        return jt::fail(JT_ERR_STATE, "jt_adapt needs every stream to hold the same number of samples: n = " +
                                          std::to_string(n) + " samples is not a multiple of k = " + std::to_string(k) +
                                          " streams");
    (void)hipSetDevice(c->device);
    const int tiles = jtk::launch_tiles(c->P), nblk = jt::adapt_blocks(tiles);
    int st;
    hipError_t e;
    if (!c->frozen_at) {
        void *mask = nullptr, *words = nullptr;
        const size_t mask_bytes = std::max<size_t>(1, (size_t)c->tiles) * sizeof(unsigned);
        if ((st = device_alloc(c, mask_bytes, "adaptive mask", &mask)) ||
            (st = device_alloc(c, std::max<size_t>(1, (size_t)nblk) * sizeof(unsigned), "adaptive mask", &words)))
            return st;
        if ((e = hipMemsetAsync(mask, 0, mask_bytes, c->stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
        c->frozen_at = (unsigned*)mask;
        c->adapt_words = (unsigned*)words;
        c->A.frozen = c->frozen_at;  // every later trace launch skips the frozen tiles
    }
    const long long N = jtk::traced_pixels(c->width, c->height, c->P.tile_stride, c->P.tile_offset);
    jt::DAdapt D{};
    D.var = c->err_var;
    D.frozen_at = c->frozen_at;
    D.active = c->adapt_words;
    D.vmax = N > 0 ? jt::adapt_vmax(noise_target, c->err_M, N) : 0.0f;
    D.n = (unsigned)n;
    D.width = c->width;
    D.height = c->height;
    D.tiles = tiles;
    D.tile_stride = c->P.tile_stride;
    D.tile_offset = c->P.tile_offset;
    // on the context's stream, after the flush: no trace launch overlaps a mask write
    std::vector<unsigned> words((size_t)nblk);
    if ((e = jt::adapt_launch(c->stream, D)) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess ||
        (nblk > 0 && (e = hipMemcpy(words.data(), c->adapt_words, words.size() * sizeof(unsigned), hipMemcpyDeviceToHost)) != hipSuccess))
        return hip_fail(e, "adaptive mask");
    long long active = 0;
    for (const unsigned w : words) active += w;
    c->adapt_active = (int)active;
    c->adapted = true;
    if (active_tiles) *active_tiles = (int32_t)active;
    return JT_OK;
}

int jt_get_sample_counts(jt_ctx* c, int32_t* counts) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (!counts) return jt::fail(JT_ERR_INVALID, "counts is NULL");
    if (const int st = flush(c)) return st;
    const int32_t n = c->first < 0 ? 0 : c->next - c->first;
    const size_t np = (size_t)c->width * c->height;
    if (c->multi) {  // never adapts: every device's share adds up to n samples of every pixel
        std::fill(counts, counts + np, n);
        return JT_OK;
    }
    std::vector<unsigned> frozen((size_t)c->tiles, 0u);
    if (c->frozen_at) {
        (void)hipSetDevice(c->device);
        const hipError_t e = hipMemcpy(frozen.data(), c->frozen_at, frozen.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy adaptive mask");
    }
    const int tiles_x = (c->width + 7) / 8, stride = c->P.tile_stride, offset = c->P.tile_offset;
    for (int j = 0; j < c->height; j++)
        for (int i = 0; i < c->width; i++) {
            const int t = (j / 8) * tiles_x + i / 8;
            const bool traced = t >= offset && (t - offset) % stride == 0;
            counts[(size_t)j * c->width + i] = !traced ? 0 : frozen[t] ? (int32_t)frozen[t] : n;
        }
    return JT_OK;
}

}  // extern "C"
