// jt_error.hip — the per-pixel error estimate (include/jtrace.h: jt_get_variance, jt_get_noise):
// the between-stream variance of a context's k > 1 sample streams (DESIGN.md §Error estimate).
//
// One pixel per lane over the launch's tile slots, as combine_kernel (jt_accum.hip) reads them:
// stream j's records of neighbouring slots are contiguous, so every load is a coalesced 16 B per
// lane, and the unrolled pass keeps eight streams' loads in flight. The image is read, not
// recombined: the estimate is about the pixel the caller gets. Each workgroup also sums its
// pixels' (V, M) contributions — shuffles within a wave, LDS across the four waves — and writes
// one pair; the host adds the pairs in double. No atomics: the result does not depend on the
// order the workgroups run in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jt_context.h"
#include "jt_error.h"

namespace jtk {

using jt::DError;
using jt::ERR_BLOCK;

__global__ __launch_bounds__(ERR_BLOCK) void error_kernel(DError E) {
    const int g = (int)(blockIdx.x * ERR_BLOCK + threadIdx.x);  // < 2^26 + 256 (jt_create's tile limit)
    // slots past the launch's tiles and pixels of an edge tile outside the image add 0 to the sums
    float v = 0.0f, m = 0.0f;
    if (g < E.tiles * 64) {
        const SlotPixel px = slot_pixel(g, E.width, E.height, E.tile_stride, E.tile_offset);
        if (px.inside) {
            const size_t pixel = (size_t)px.j * E.width + px.i, ns = (size_t)E.nslot;
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

// ---- the context's half (jt_context.h)
using namespace jtc;

// The error estimate of the current samples (include/jtrace.h jt_get_variance): checks, the flush,
// then one launch of error_kernel over the stream means the last combine read, unless the
// result of these samples is already there. Neither counted in jt_counters nor touching an
// accumulator or a stream mean.
int jtc::estimate_error(jt_ctx* c) {
    if (c->multi)
        return jt::fail(JT_ERR_UNSUPPORTED,
                        "the error estimate is not available on a multi-device context (jt_create_multi): "
                        "query one context per device");
    if (c->failed) return jt::fail(JT_ERR_STATE, "a previous launch failed; jt_reset the context");
    const char* need = "the error estimate needs two sample streams that hold a sample";
    if (c->lk == 0)
        return jt::fail(JT_ERR_STATE, std::string(need) + ": this context has one (create it with batch >= 2 or "
                                                          "the option streams)");
    if (const int st = flush(c)) return st;
    const long long n = c->first < 0 ? 0 : c->next - c->first;
    if (n < 1) return jt::fail(JT_ERR_STATE, "no sample has been traced");
    if (n < 2)
        return jt::fail(JT_ERR_STATE, std::string(need) + ": one sample has been traced (batch >= 2 or the option "
                                                          "streams, and two samples)");
    if (c->err_valid) return JT_OK;
    (void)hipSetDevice(c->device);
    const size_t np = (size_t)c->width * c->height;
    const int tiles = jtk::launch_tiles(c->P), nblk = jt::error_blocks(tiles);
    int st;
    hipError_t e;
    if (!c->err_var) {
        void *var = nullptr, *sums = nullptr;
        if ((st = device_alloc(c, np * 16, "error estimate", &var)) ||
            (st = device_alloc(c, std::max<size_t>(1, (size_t)nblk) * sizeof(float2), "error estimate", &sums)))
            return st;
        // a tile share's other pixels stay 0
        if ((e = hipMemsetAsync(var, 0, np * 16, c->stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
        c->err_var = (float4*)var;
        c->err_sums = (float2*)sums;
    }
    if ((st = zero_if_stale(c))) return st;
    jt::DError E{};
    E.part_img = c->A.part_img;
    E.image = c->A.image;
    E.var = c->err_var;
    E.block_sums = c->err_sums;
    E.nslot = c->A.nslot;
    E.width = c->width;
    E.height = c->height;
    E.tiles = tiles;
    E.tile_stride = c->P.tile_stride;
    E.tile_offset = c->P.tile_offset;
    E.ns = c->last_cw.ns;  // min(n, k) >= 2, with the weights the image was combined with
    std::memcpy(E.w, c->last_cw.w, sizeof E.w);
    std::vector<float2> sums((size_t)nblk);
    if ((e = jt::error_launch(c->stream, E)) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess ||
        (nblk > 0 && (e = hipMemcpy(sums.data(), c->err_sums, sums.size() * sizeof(float2), hipMemcpyDeviceToHost)) != hipSuccess))
        return hip_fail(e, "error estimate");
    double V = 0, M = 0;
    for (const float2& s : sums) V += (double)s.x, M += (double)s.y;
    // N: the traced pixels inside the image (edge tiles are clipped)
    const long long N = jtk::traced_pixels(c->width, c->height, c->P.tile_stride, c->P.tile_offset);
    c->err_noise = M == 0 ? 0.0 : std::sqrt(3.0 * (double)N * V) / M;
    c->err_M = M;  // jt_adapt's threshold (jt_adapt.hip)
    c->err_valid = true;
    return JT_OK;
}

extern "C" {

int jt_get_variance(jt_ctx* c, float* var_rgba) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (!var_rgba) return jt::fail(JT_ERR_INVALID, "var_rgba is NULL");
    if (const int st = estimate_error(c)) return st;
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemcpy(var_rgba, c->err_var, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy variance");
}

int jt_get_noise(jt_ctx* c, double* noise) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (!noise) return jt::fail(JT_ERR_INVALID, "noise is NULL");
    if (const int st = estimate_error(c)) return st;
    *noise = c->err_noise;
    return JT_OK;
}

}  // extern "C"
