// jt_denoise.hip — the denoiser (include/jtrace.h: jt_denoise, jt_denoise_image): the
// edge-avoiding a-trous wavelet filter of Dammertz et al. (HPG 2010) on albedo-demodulated
// radiance, guided by the tracer's albedo and normal means.
//
// One pixel per lane, every buffer float4. A workgroup is 64 x 4 pixels and a wave one row of 64
// consecutive x, so each of a pixel's 24 taps is one coalesced 16-B-per-lane load per array, and
// whether a tap's row lies inside the image is the same for the whole wave. The taps of
// neighbouring rows and iterations overlap, so all but the compulsory 64 B per pixel and
// iteration (d, albedo, normal read, d written) comes from the caches. The iterations ping-pong
// between two scratch buffers; the last one multiplies the albedo back in and writes the result.
// The variance-guided filter (jt_denoise_guided, jt_denoise_guided_image) has kernels of its own
// in the same shape, below the plain ones.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "jt_context.h"
#include "jt_denoise.h"
#include "jt_error.h"

namespace jtk {

constexpr int DN_BX = 64, DN_BY = 4;

struct DDenoise {
    const float4* src;     // d_i
    const float4* image;   // mean radiance (alpha, and d_0 for the demodulation)
    const float4* albedo;
    const float4* normal;
    float4* dst;           // d_{i+1}, or the result from the last iteration
    int width, height, step;
    float inv_sc2, inv_sn2, inv_sa2;  // 1 / sc_i^2, 1 / sigma_normal^2, 1 / sigma_albedo^2
    float floor;
};

__device__ __forceinline__ float dist2(float4 a, float4 b) {
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return (x * x + y * y) + z * z;
}
__device__ __forceinline__ float4 modulation(float4 a, float floor) {
    return make_float4(fmaxf(a.x, floor), fmaxf(a.y, floor), fmaxf(a.z, floor), 0.0f);
}

// d_0 = c.rgb / max(a, albedo_floor)
__global__ __launch_bounds__(256) void demodulate_kernel(DDenoise D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;  // width * height < 2^26 (denoise_check_size)
    const float4 c = D.image[p], m = modulation(D.albedo[p], D.floor);
    D.dst[p] = make_float4(c.x / m.x, c.y / m.y, c.z / m.z, 0.0f);
}

// one a-trous iteration with step s: the 5 x 5 taps p + s * (dx, dy), those outside the image
// skipped; the centre tap's weight is k[2] * k[2] * exp(-0) = 9/64 whatever the sigmas, so the
// sums start from it and the denominator is never 0
template <bool LAST>
__global__ __launch_bounds__(256) void atrous_kernel(DDenoise D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;
    const float4 dp = D.src[p], np = D.normal[p], ap = D.albedo[p];
    constexpr float k[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    float wsum = k[2] * k[2];
    float sx = dp.x * wsum, sy = dp.y * wsum, sz = dp.z * wsum;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * D.step;
        if (qy < 0 || qy >= D.height) continue;  // the same for every lane of the wave
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx * D.step;
            if (qx < 0 || qx >= D.width) continue;
            const int q = qy * D.width + qx;
            const float4 dq = D.src[q], nq = D.normal[q], aq = D.albedo[q];
            const float e = (dist2(dp, dq) * D.inv_sc2 + dist2(np, nq) * D.inv_sn2) + dist2(ap, aq) * D.inv_sa2;
            const float w = (k[dy + 2] * k[dx + 2]) * expf(-e);
            sx += w * dq.x, sy += w * dq.y, sz += w * dq.z;
            wsum += w;
        }
    }
    float4 r = make_float4(sx / wsum, sy / wsum, sz / wsum, 0.0f);
    if constexpr (LAST) {  // out.rgb = d_I * m, out.a = c.a
        const float4 m = modulation(ap, D.floor);
        r = make_float4(r.x * m.x, r.y * m.y, r.z * m.z, D.image[p].w);
    }
    D.dst[p] = r;
}

// ---- the variance-guided filter (jt_denoise_guided): the same window, buffers and launch shape;
// the colour term of a tap is scaled by the two pixels' own variance instead of a global sigma.
// V_i, the variance of |d_i| summed over the channels, rides in the .w of the d_i buffer, so
// V(q) arrives with the d(q) load the tap makes anyway: 72 tap loads per pixel, as above.
struct DGuided {
    const float4* src;       // (d_i, V_i)
    const float4* image;     // mean radiance (alpha, and d_0 for the demodulation)
    const float4* variance;  // variance of the mean per channel (w ignored); the demodulation only
    const float4* albedo;
    const float4* normal;
    float4* dst;             // (d_{i+1}, V_{i+1}), or the result from the last iteration
    int width, height, step;
    float sv2, inv_sn2, inv_sa2;  // sigma_variance^2, 1 / sigma_normal^2, 1 / sigma_albedo^2
    float floor, vfloor;          // albedo_floor, variance_floor
};

// d_0 = c.rgb / m, V_0 = sum over the channels of v / (m * m), m = max(a, albedo_floor)
__global__ __launch_bounds__(256) void guided_demodulate_kernel(DGuided D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;  // width * height < 2^26 (denoise_check_size)
    const float4 c = D.image[p], v = D.variance[p], m = modulation(D.albedo[p], D.floor);
    const float ux = v.x / (m.x * m.x), uy = v.y / (m.y * m.y), uz = v.z / (m.z * m.z);
    D.dst[p] = make_float4(c.x / m.x, c.y / m.y, c.z / m.z, (ux + uy) + uz);
}

// one guided iteration with step s. The centre tap weighs 9/64 whatever the variances, so the
// sums start from it; the last iteration has no use for V_{i+1} and does not sum it
template <bool LAST>
__global__ __launch_bounds__(256) void guided_atrous_kernel(DGuided D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;
    const float4 dp = D.src[p], np = D.normal[p], ap = D.albedo[p];
    constexpr float k[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    float wsum = k[2] * k[2];
    float sx = dp.x * wsum, sy = dp.y * wsum, sz = dp.z * wsum, sv = (wsum * wsum) * dp.w;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * D.step;
        if (qy < 0 || qy >= D.height) continue;  // the same for every lane of the wave
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx * D.step;
            if (qx < 0 || qx >= D.width) continue;
            const int q = qy * D.width + qx;
            const float4 dq = D.src[q], nq = D.normal[q], aq = D.albedo[q];
            const float tol = D.sv2 * fmaxf(dp.w + dq.w, D.vfloor);  // > 0 (denoise_guided_check_params)
            const float e = (dist2(dp, dq) / tol + dist2(np, nq) * D.inv_sn2) + dist2(ap, aq) * D.inv_sa2;
            const float w = (k[dy + 2] * k[dx + 2]) * expf(-e);
            sx += w * dq.x, sy += w * dq.y, sz += w * dq.z;
            if constexpr (!LAST) sv += (w * w) * dq.w;
            wsum += w;
        }
    }
    float4 r = make_float4(sx / wsum, sy / wsum, sz / wsum, 0.0f);
    if constexpr (LAST) {  // out.rgb = d_I * m, out.a = c.a
        const float4 m = modulation(ap, D.floor);
        r = make_float4(r.x * m.x, r.y * m.y, r.z * m.z, D.image[p].w);
    } else {
        r.w = sv / (wsum * wsum);
    }
    D.dst[p] = r;
}

}  // namespace jtk

namespace jt {

namespace {
// 1 / v^2 as a float, finite: a tap whose guide differs then gets exp(-inf) = 0 and one whose
// guide is equal exp(-0) = 1 however small the sigma, never 0 * inf
float inv_square(float v) {
    const double r = 1.0 / ((double)v * (double)v);
    return r > (double)FLT_MAX ? FLT_MAX : (float)r;
}
bool positive_finite(float v) { return std::isfinite(v) && v > 0; }
}  // namespace

int denoise_check_params(const jt_denoise_params* p) {
    if (!p) return fail(JT_ERR_INVALID, "params is NULL");
    if (p->iterations < 1 || p->iterations > 8) return fail(JT_ERR_INVALID, "iterations must be in [1, 8]");
    if (!positive_finite(p->sigma_color)) return fail(JT_ERR_INVALID, "sigma_color must be finite and > 0");
    if (!positive_finite(p->sigma_normal)) return fail(JT_ERR_INVALID, "sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_albedo)) return fail(JT_ERR_INVALID, "sigma_albedo must be finite and > 0");
    if (!positive_finite(p->albedo_floor)) return fail(JT_ERR_INVALID, "albedo_floor must be finite and > 0");
    return JT_OK;
}

int denoise_check_size(int32_t width, int32_t height) {
    if (width < 1) return fail(JT_ERR_INVALID, "width must be at least 1");
    if (height < 1) return fail(JT_ERR_INVALID, "height must be at least 1");
    // jt_create's limit (alloc_accumulators): pixel indices stay below 2^26
    if ((long long)((width + 7LL) / 8) * ((height + 7LL) / 8) >= (1LL << 20))
        return fail(JT_ERR_INVALID, "width*height above 2^20 8x8 tiles (67 Mpixels)");
    return JT_OK;
}

hipError_t denoise_launch(hipStream_t stream, const float4* image, const float4* albedo, const float4* normal, int width,
                          int height, const jt_denoise_params& p, float4* ping, float4* pong, float4* out) {
    using namespace jtk;
    const dim3 block(DN_BX, DN_BY), grid((width + DN_BX - 1) / DN_BX, (height + DN_BY - 1) / DN_BY);
    DDenoise D{};
    D.image = image;
    D.albedo = albedo;
    D.normal = normal;
    D.width = width;
    D.height = height;
    D.inv_sn2 = inv_square(p.sigma_normal);
    D.inv_sa2 = inv_square(p.sigma_albedo);
    D.floor = p.albedo_floor;
    D.dst = ping;
    hipLaunchKernelGGL(demodulate_kernel, grid, block, 0, stream, D);
    float4* buf[2] = {ping, pong};
    for (int i = 0; i < p.iterations; i++) {
        const bool last = i + 1 == p.iterations;
        D.src = buf[i & 1];
        D.dst = last ? out : buf[(i + 1) & 1];
        D.step = 1 << i;
        D.inv_sc2 = inv_square(p.sigma_color / (float)D.step);  // sc_i = sigma_color / 2^i
        if (last) hipLaunchKernelGGL(atrous_kernel<true>, grid, block, 0, stream, D);
        else hipLaunchKernelGGL(atrous_kernel<false>, grid, block, 0, stream, D);
    }
    return hipGetLastError();
}

int denoise_guided_check_params(const jt_denoise_guided_params* p) {
    if (!p) return fail(JT_ERR_INVALID, "params is NULL");
    if (p->iterations < 1 || p->iterations > 8) return fail(JT_ERR_INVALID, "iterations must be in [1, 8]");
    if (!positive_finite(p->sigma_variance)) return fail(JT_ERR_INVALID, "sigma_variance must be finite and > 0");
    if (!positive_finite(p->sigma_normal)) return fail(JT_ERR_INVALID, "sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_albedo)) return fail(JT_ERR_INVALID, "sigma_albedo must be finite and > 0");
    if (!positive_finite(p->albedo_floor)) return fail(JT_ERR_INVALID, "albedo_floor must be finite and > 0");
    if (!positive_finite(p->variance_floor)) return fail(JT_ERR_INVALID, "variance_floor must be finite and > 0");
    // the smallest colour tolerance a tap divides by: a normal float, so no tap computes 0 / 0
    if (!((p->sigma_variance * p->sigma_variance) * p->variance_floor >= FLT_MIN))
        return fail(JT_ERR_INVALID, "sigma_variance^2 * variance_floor underflows");
    return JT_OK;
}

hipError_t denoise_guided_launch(hipStream_t stream, const float4* image, const float4* variance, const float4* albedo,
                                 const float4* normal, int width, int height, const jt_denoise_guided_params& p,
                                 float4* ping, float4* pong, float4* out) {
    using namespace jtk;
    const dim3 block(DN_BX, DN_BY), grid((width + DN_BX - 1) / DN_BX, (height + DN_BY - 1) / DN_BY);
    DGuided D{};
    D.image = image;
    D.variance = variance;
    D.albedo = albedo;
    D.normal = normal;
    D.width = width;
    D.height = height;
    D.sv2 = p.sigma_variance * p.sigma_variance;
    D.inv_sn2 = inv_square(p.sigma_normal);
    D.inv_sa2 = inv_square(p.sigma_albedo);
    D.floor = p.albedo_floor;
    D.vfloor = p.variance_floor;
    D.dst = ping;
    hipLaunchKernelGGL(guided_demodulate_kernel, grid, block, 0, stream, D);
    float4* buf[2] = {ping, pong};
    for (int i = 0; i < p.iterations; i++) {
        const bool last = i + 1 == p.iterations;
        D.src = buf[i & 1];
        D.dst = last ? out : buf[(i + 1) & 1];
        D.step = 1 << i;  // the colour tolerance is not halved: V_i shrinks where the filter has averaged
        if (last) hipLaunchKernelGGL(guided_atrous_kernel<true>, grid, block, 0, stream, D);
        else hipLaunchKernelGGL(guided_atrous_kernel<false>, grid, block, 0, stream, D);
    }
    return hipGetLastError();
}

}  // namespace jt

extern "C" {

int jt_denoise_defaults(int32_t samples, jt_denoise_params* out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    out->iterations = 5;
    // the noise level falls as 1 / sqrt(spp), and the colour sigma with it
    out->sigma_color = 8.0f / sqrtf((float)(samples > 1 ? samples : 1));
    out->sigma_normal = 0.3f;
    out->sigma_albedo = 0.1f;
    out->albedo_floor = 0.01f;
    return JT_OK;
}

}  // extern "C"

namespace {
// The host-array filters' device half, after their argument checks: uploads the arrays to `device`,
// runs launch(stream, image, variance, albedo, normal, ping, pong, out) and copies the result
// back. variance NULL (the plain filter): no such buffer, the launch gets nullptr.
template <class Launch>
int filter_host_arrays(const float* rgba, const float* variance, const float* albedo, const float* normal, int32_t width,
                       int32_t height, int32_t device, float* out_rgba, Launch launch) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return jt::fail(JT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    const size_t np = (size_t)width * (size_t)height;
    // image, albedo, normal, ping, pong, out and the variance: one allocation, freed on every path
    struct Dev {
        float4* p = nullptr;
        hipStream_t stream = nullptr;
        ~Dev() {
            if (stream) (void)hipStreamDestroy(stream);
            if (p) (void)hipFree(p);
        }
    } dev;
    if (hipMalloc((void**)&dev.p, np * 16 * (variance ? 7 : 6)) != hipSuccess) {
        (void)hipGetLastError();
        return jt::fail(JT_ERR_NOMEM, "hipMalloc denoise buffers");
    }
    if ((e = hipStreamCreateWithFlags(&dev.stream, hipStreamNonBlocking)) != hipSuccess)
        return jt::fail(JT_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    std::vector<float4> host(np * 2);
    for (size_t k = 0; k < np; k++) {
        host[k] = make_float4(albedo[3 * k], albedo[3 * k + 1], albedo[3 * k + 2], 0.0f);
        host[np + k] = make_float4(normal[3 * k], normal[3 * k + 1], normal[3 * k + 2], 0.0f);
    }
    float4* d = dev.p;
    if ((e = hipMemcpy(d, rgba, np * 16, hipMemcpyHostToDevice)) == hipSuccess &&
        (e = hipMemcpy(d + np, host.data(), np * 32, hipMemcpyHostToDevice)) == hipSuccess &&
        (!variance || (e = hipMemcpy(d + 6 * np, variance, np * 16, hipMemcpyHostToDevice)) == hipSuccess) &&
        (e = launch(dev.stream, d, variance ? d + 6 * np : nullptr, d + np, d + 2 * np, d + 3 * np, d + 4 * np,
                    d + 5 * np)) == hipSuccess &&
        (e = hipStreamSynchronize(dev.stream)) == hipSuccess)
        e = hipMemcpy(out_rgba, d + 5 * np, np * 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return jt::fail(JT_ERR_DEVICE, std::string("denoise: ") + hipGetErrorString(e));
    return JT_OK;
}
}  // namespace

extern "C" {

int jt_denoise_image(const float* rgba, const float* albedo, const float* normal, int32_t width, int32_t height,
                     const jt_denoise_params* params, int32_t device, float* out_rgba) {
    if (!rgba) return jt::fail(JT_ERR_INVALID, "rgba is NULL");
    if (!albedo) return jt::fail(JT_ERR_INVALID, "albedo is NULL");
    if (!normal) return jt::fail(JT_ERR_INVALID, "normal is NULL");
    if (!out_rgba) return jt::fail(JT_ERR_INVALID, "out_rgba is NULL");
    int st;
    if ((st = jt::denoise_check_params(params)) || (st = jt::denoise_check_size(width, height))) return st;
    if (device < 0) return jt::fail(JT_ERR_INVALID, "device must not be negative");
    return filter_host_arrays(rgba, nullptr, albedo, normal, width, height, device, out_rgba,
                              [&](hipStream_t s, const float4* img, const float4*, const float4* alb, const float4* nrm,
                                  float4* ping, float4* pong, float4* out) {
                                  return jt::denoise_launch(s, img, alb, nrm, width, height, *params, ping, pong, out);
                              });
}

int jt_denoise_guided_defaults(jt_denoise_guided_params* out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    out->iterations = 5;
    out->sigma_variance = 2.0f;
    out->sigma_normal = 0.3f;
    out->sigma_albedo = 0.1f;
    out->albedo_floor = 0.01f;
    out->variance_floor = 1e-10f;
    return JT_OK;
}

int jt_denoise_guided_image(const float* rgba, const float* variance, const float* albedo, const float* normal,
                            int32_t width, int32_t height, const jt_denoise_guided_params* params, int32_t device,
                            float* out_rgba) {
    if (!rgba) return jt::fail(JT_ERR_INVALID, "rgba is NULL");
    if (!variance) return jt::fail(JT_ERR_INVALID, "variance is NULL");
    if (!albedo) return jt::fail(JT_ERR_INVALID, "albedo is NULL");
    if (!normal) return jt::fail(JT_ERR_INVALID, "normal is NULL");
    if (!out_rgba) return jt::fail(JT_ERR_INVALID, "out_rgba is NULL");
    int st;
    if ((st = jt::denoise_guided_check_params(params)) || (st = jt::denoise_check_size(width, height))) return st;
    if (device < 0) return jt::fail(JT_ERR_INVALID, "device must not be negative");
    return filter_host_arrays(rgba, variance, albedo, normal, width, height, device, out_rgba,
                              [&](hipStream_t s, const float4* img, const float4* var, const float4* alb,
                                  const float4* nrm, float4* ping, float4* pong, float4* out) {
                                  return jt::denoise_guided_launch(s, img, var, alb, nrm, width, height, *params, ping,
                                                                   pong, out);
                              });
}

// ---- the context's half (jt_context.h): the filter of a context's running means, kept in jt_ctx::dn
int jt_denoise(jt_ctx* c, const jt_denoise_params* params) {
    using namespace jtc;
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    jt_denoise_params p{};
    if (params) {
        if (const int st = jt::denoise_check_params(params)) return st;
        p = *params;
    }
    if (c->failed) return jt::fail(JT_ERR_STATE, "a previous launch failed; jt_reset the context");
    if (const int st = flush(c)) return st;
    const int samples = c->first < 0 ? 0 : c->next - c->first;
    if (samples < 1) return jt::fail(JT_ERR_STATE, "no sample has been traced");
    if (!params) (void)jt_denoise_defaults(samples, &p);
    c->denoised = false;
    if (c->multi) return multi_denoise(c, p);
    const size_t np = (size_t)c->width * c->height;
    int st;
    if ((st = zero_if_stale(c)) || (st = finish_aovs(c))) return st;
    (void)hipSetDevice(c->device);
    for (int k = 0; k < 3; k++)
        if (!c->dn[k] && (st = device_alloc(c, np * 16, "denoise buffers", (void**)&c->dn[k]))) return st;
    // neither counted in jt_counters (launches, kernel_ms) nor touching an accumulator
    hipError_t e = jt::denoise_launch(c->stream, c->A.image, c->A.albedo, c->A.normal, c->width, c->height, p, c->dn[0],
                                      c->dn[1], c->dn[2]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "denoise");
    c->denoised = true;
    return JT_OK;
}

// The variance-guided filter of a context's running means into the same jt_ctx::dn: the error
// estimate of these samples (jt_error.hip; computed here unless already valid, and then valid
// for jt_get_variance / jt_get_noise too), then the launches, which only read it.
int jt_denoise_guided(jt_ctx* c, const jt_denoise_guided_params* params) {
    using namespace jtc;
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    jt_denoise_guided_params p{};
    if (params) {
        if (const int st = jt::denoise_guided_check_params(params)) return st;
        p = *params;
    } else {
        (void)jt_denoise_guided_defaults(&p);
    }
    int st;
    if ((st = estimate_error(c))) return st;  // every check of jt_get_variance, and the flush
    c->denoised = false;
    const size_t np = (size_t)c->width * c->height;
    if ((st = zero_if_stale(c)) || (st = finish_aovs(c))) return st;
    (void)hipSetDevice(c->device);
    for (int k = 0; k < 3; k++)
        if (!c->dn[k] && (st = device_alloc(c, np * 16, "denoise buffers", (void**)&c->dn[k]))) return st;
    // neither counted in jt_counters (launches, kernel_ms) nor touching an accumulator
    hipError_t e = jt::denoise_guided_launch(c->stream, c->A.image, c->err_var, c->A.albedo, c->A.normal, c->width,
                                             c->height, p, c->dn[0], c->dn[1], c->dn[2]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "denoise");
    c->denoised = true;
    return JT_OK;
}

int jt_get_denoised(jt_ctx* c, float* rgba) {
    if (!c || !rgba) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (!c->denoised) return jt::fail(JT_ERR_STATE, "no jt_denoise or jt_denoise_guided since the last sample was traced or jt_reset");
    if (c->multi) return jtc::multi_get_denoised(c, rgba);
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemcpy(rgba, c->dn[2], (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : jtc::hip_fail(e, "hipMemcpy denoised");
}

}  // extern "C"
