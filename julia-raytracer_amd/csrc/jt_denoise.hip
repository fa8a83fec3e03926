// jt_denoise.hip — the denoisers (include/jtrace.h: jt_denoise, jt_denoise_image, jt_denoise_guided,
// jt_denoise_guided_image): the edge-avoiding a-trous wavelet filter of Dammertz et al. (HPG 2010)
// on albedo-demodulated radiance, guided by the tracer's albedo and normal means (DESIGN.md
// §Denoiser).
//
// One pixel per lane, every buffer float4. A workgroup is 64 x 4 pixels and a wave one row of 64
// consecutive x, so each of a pixel's 24 taps is one coalesced 16-B-per-lane load per array, and
// whether a tap's row lies inside the image is the same for the whole wave. The taps of
// neighbouring rows and iterations overlap, so all but the compulsory 64 B per pixel and
// iteration (d, albedo, normal read, d written) comes from the caches. The iterations ping-pong
// between two scratch buffers; the last one multiplies the albedo back in and writes the result.
//
// The plain and the variance-guided filter are one set of kernels, one launch loop, one parameter
// check and one entry of each kind, templated on GUIDED or on the parameter record. The guided
// filter scales the colour term of a tap by the two pixels' own variance instead of a global
// sigma: V_i, the variance of |d_i| summed over the channels, rides in the .w of the d_i buffer,
// so V(q) arrives with the d(q) load the tap makes anyway: 72 tap loads per pixel in both.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "jt_context.h"
#include "jt_denoise.h"
#include "jt_error.h"

namespace jtk {

constexpr int DN_BX = 64, DN_BY = 4;

struct DFilter {
    const float4* src;       // d_i; guided: (d_i, V_i)
    const float4* image;     // mean radiance (alpha, and d_0 for the demodulation)
    const float4* variance;  // guided: variance of the mean per channel (w ignored); the demodulation only
    const float4* albedo;
    const float4* normal;
    float4* dst;             // d_{i+1} (guided: with V_{i+1}), or the result from the last iteration
    int width, height, step;
    float colour;            // 1 / sc_i^2; guided: sigma_variance^2
    float inv_sn2, inv_sa2;  // 1 / sigma_normal^2, 1 / sigma_albedo^2
    float floor, vfloor;     // albedo_floor; guided: variance_floor
};

__device__ __forceinline__ float dist2(float4 a, float4 b) {
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return (x * x + y * y) + z * z;
}
__device__ __forceinline__ float4 modulation(float4 a, float floor) {
    return make_float4(fmaxf(a.x, floor), fmaxf(a.y, floor), fmaxf(a.z, floor), 0.0f);
}

// d_0 = c.rgb / m, m = max(a, albedo_floor); guided: V_0 = sum over the channels of v / (m * m)
template <bool GUIDED>
__global__ __launch_bounds__(256) void demodulate_kernel(DFilter D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;  // width * height < 2^26 (denoise_check_size)
    const float4 c = D.image[p], m = modulation(D.albedo[p], D.floor);
    float v0 = 0.0f;
    if constexpr (GUIDED) {
        const float4 v = D.variance[p];
        const float ux = v.x / (m.x * m.x), uy = v.y / (m.y * m.y), uz = v.z / (m.z * m.z);
        v0 = (ux + uy) + uz;
    }
    D.dst[p] = make_float4(c.x / m.x, c.y / m.y, c.z / m.z, v0);
}

// one a-trous iteration with step s: the 5 x 5 taps p + s * (dx, dy), those outside the image
// skipped; the centre tap's weight is k[2] * k[2] * exp(-0) = 9/64 whatever the sigmas and the
// variances, so the sums start from it and the denominator is never 0. The guided filter's last
// iteration has no use for V_{i+1} and does not sum it
template <bool GUIDED, bool LAST>
__global__ __launch_bounds__(256) void atrous_kernel(DFilter D) {
    const int x = (int)(blockIdx.x * DN_BX + threadIdx.x), y = (int)(blockIdx.y * DN_BY + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int p = y * D.width + x;
    const float4 dp = D.src[p], np = D.normal[p], ap = D.albedo[p];
    constexpr float k[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    float wsum = k[2] * k[2];
    float sx = dp.x * wsum, sy = dp.y * wsum, sz = dp.z * wsum, sv = 0.0f;
    if constexpr (GUIDED && !LAST) sv = (wsum * wsum) * dp.w;
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
            float ec;
            if constexpr (GUIDED) {
                const float tol = D.colour * fmaxf(dp.w + dq.w, D.vfloor);  // > 0 (check_params)
                ec = dist2(dp, dq) / tol;
            } else {
                ec = dist2(dp, dq) * D.colour;
            }
            const float e = (ec + dist2(np, nq) * D.inv_sn2) + dist2(ap, aq) * D.inv_sa2;
            const float w = (k[dy + 2] * k[dx + 2]) * expf(-e);
            sx += w * dq.x, sy += w * dq.y, sz += w * dq.z;
            if constexpr (GUIDED && !LAST) sv += (w * w) * dq.w;
            wsum += w;
        }
    }
    float4 r = make_float4(sx / wsum, sy / wsum, sz / wsum, 0.0f);
    if constexpr (LAST) {  // out.rgb = d_I * m, out.a = c.a
        const float4 m = modulation(ap, D.floor);
        r = make_float4(r.x * m.x, r.y * m.y, r.z * m.z, D.image[p].w);
    } else if constexpr (GUIDED) {
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
int check_positive(float v, const char* field) {
    if (std::isfinite(v) && v > 0) return JT_OK;
    return fail(JT_ERR_INVALID, std::string(field) + " must be finite and > 0");
}

template <class P>
constexpr bool is_guided = std::is_same_v<P, jt_denoise_guided_params>;

// The check of either parameter record, P jt_denoise_params or jt_denoise_guided_params
template <class P>
int check_params(const P* p) {
    if (!p) return fail(JT_ERR_INVALID, "params is NULL");
    if (p->iterations < 1 || p->iterations > 8) return fail(JT_ERR_INVALID, "iterations must be in [1, 8]");
    int st;
    if constexpr (is_guided<P>) st = check_positive(p->sigma_variance, "sigma_variance");
    else st = check_positive(p->sigma_color, "sigma_color");
    if (st || (st = check_positive(p->sigma_normal, "sigma_normal")) ||
        (st = check_positive(p->sigma_albedo, "sigma_albedo")) || (st = check_positive(p->albedo_floor, "albedo_floor")))
        return st;
    if constexpr (is_guided<P>) {
        if ((st = check_positive(p->variance_floor, "variance_floor"))) return st;
        // the smallest colour tolerance a tap divides by: a normal float, so no tap computes 0 / 0
        if (!((p->sigma_variance * p->sigma_variance) * p->variance_floor >= FLT_MIN))
            return fail(JT_ERR_INVALID, "sigma_variance^2 * variance_floor underflows");
    }
    return JT_OK;
}

// The launches of either filter: the demodulation into ping, then p.iterations a-trous kernels.
// `variance` is read by the guided filter only
template <class P>
hipError_t filter_launch(hipStream_t stream, const float4* image, const float4* variance, const float4* albedo,
                         const float4* normal, int width, int height, const P& p, float4* ping, float4* pong,
                         float4* out) {
    using namespace jtk;
    constexpr bool GUIDED = is_guided<P>;
    const dim3 block(DN_BX, DN_BY), grid((width + DN_BX - 1) / DN_BX, (height + DN_BY - 1) / DN_BY);
    DFilter D{};
    D.image = image;
    D.albedo = albedo;
    D.normal = normal;
    D.width = width;
    D.height = height;
    D.inv_sn2 = inv_square(p.sigma_normal);
    D.inv_sa2 = inv_square(p.sigma_albedo);
    D.floor = p.albedo_floor;
    if constexpr (GUIDED) {
        D.variance = variance;
        // not halved per iteration: V_i shrinks where the filter has averaged
        D.colour = p.sigma_variance * p.sigma_variance;
        D.vfloor = p.variance_floor;
    }
    D.dst = ping;
    hipLaunchKernelGGL(demodulate_kernel<GUIDED>, grid, block, 0, stream, D);
    float4* buf[2] = {ping, pong};
    for (int i = 0; i < p.iterations; i++) {
        const bool last = i + 1 == p.iterations;
        D.src = buf[i & 1];
        D.dst = last ? out : buf[(i + 1) & 1];
        D.step = 1 << i;
        if constexpr (!GUIDED) D.colour = inv_square(p.sigma_color / (float)D.step);  // sc_i = sigma_color / 2^i
        if (last) hipLaunchKernelGGL((atrous_kernel<GUIDED, true>), grid, block, 0, stream, D);
        else hipLaunchKernelGGL((atrous_kernel<GUIDED, false>), grid, block, 0, stream, D);
    }
    return hipGetLastError();
}
}  // namespace

int denoise_check_params(const jt_denoise_params* p) { return check_params(p); }
int denoise_guided_check_params(const jt_denoise_guided_params* p) { return check_params(p); }

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
    return filter_launch(stream, image, nullptr, albedo, normal, width, height, p, ping, pong, out);
}

hipError_t denoise_guided_launch(hipStream_t stream, const float4* image, const float4* variance, const float4* albedo,
                                 const float4* normal, int width, int height, const jt_denoise_guided_params& p,
                                 float4* ping, float4* pong, float4* out) {
    return filter_launch(stream, image, variance, albedo, normal, width, height, p, ping, pong, out);
}

}  // namespace jt

namespace {
// The host-array filters (jt_denoise_image, jt_denoise_guided_image): the argument checks, then the
// device half, which uploads the arrays to `device`, runs the launches and copies the result
// back. The plain filter passes variance NULL and gets no such buffer.
template <class P>
int filter_host_arrays(const float* rgba, const float* variance, const float* albedo, const float* normal, int32_t width,
                       int32_t height, const P* params, int32_t device, float* out_rgba) {
    if (!rgba) return jt::fail(JT_ERR_INVALID, "rgba is NULL");
    if (jt::is_guided<P> && !variance) return jt::fail(JT_ERR_INVALID, "variance is NULL");
    if (!albedo) return jt::fail(JT_ERR_INVALID, "albedo is NULL");
    if (!normal) return jt::fail(JT_ERR_INVALID, "normal is NULL");
    if (!out_rgba) return jt::fail(JT_ERR_INVALID, "out_rgba is NULL");
    int st;
    if ((st = jt::check_params(params)) || (st = jt::denoise_check_size(width, height))) return st;
    if (device < 0) return jt::fail(JT_ERR_INVALID, "device must not be negative");
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
        (e = jt::filter_launch(dev.stream, d, variance ? d + 6 * np : nullptr, d + np, d + 2 * np, width, height, *params,
                               d + 3 * np, d + 4 * np, d + 5 * np)) == hipSuccess &&
        (e = hipStreamSynchronize(dev.stream)) == hipSuccess)
        e = hipMemcpy(out_rgba, d + 5 * np, np * 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return jt::fail(JT_ERR_DEVICE, std::string("denoise: ") + hipGetErrorString(e));
    return JT_OK;
}

// The context filters' shared tail, after their own checks: either filter of a context's running
// means into jt_ctx::dn. `variance` is read by the guided filter only
template <class P>
int filter_context(jt_ctx* c, const float4* variance, const P& p) {
    using namespace jtc;
    c->denoised = false;
    const size_t np = (size_t)c->width * c->height;
    int st;
    if ((st = zero_if_stale(c)) || (st = finish_aovs(c))) return st;
    (void)hipSetDevice(c->device);
    for (int k = 0; k < 3; k++)
        if (!c->dn[k] && (st = device_alloc(c, np * 16, "denoise buffers", (void**)&c->dn[k]))) return st;
    // neither counted in jt_counters (launches, kernel_ms) nor touching an accumulator
    hipError_t e = jt::filter_launch(c->stream, c->A.image, variance, c->A.albedo, c->A.normal, c->width, c->height, p,
                                     c->dn[0], c->dn[1], c->dn[2]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "denoise");
    c->denoised = true;
    return JT_OK;
}
}  // namespace

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

int jt_denoise_image(const float* rgba, const float* albedo, const float* normal, int32_t width, int32_t height,
                     const jt_denoise_params* params, int32_t device, float* out_rgba) {
    return filter_host_arrays(rgba, nullptr, albedo, normal, width, height, params, device, out_rgba);
}

int jt_denoise_guided_image(const float* rgba, const float* variance, const float* albedo, const float* normal,
                            int32_t width, int32_t height, const jt_denoise_guided_params* params, int32_t device,
                            float* out_rgba) {
    return filter_host_arrays(rgba, variance, albedo, normal, width, height, params, device, out_rgba);
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
    if (c->multi) {
        c->denoised = false;
        return multi_denoise(c, p);
    }
    return filter_context(c, nullptr, p);
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
    if (const int st = estimate_error(c)) return st;  // every check of jt_get_variance, and the flush
    return filter_context(c, c->err_var, p);
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
