// jt_trace.hip — the C-ABI device context of the MI355X path tracer (include/jtrace.h): scene
// upload, launches, the multi-device split and its RCCL reduce. The scene's validation and host
// layout are in jt_layout.cpp (no HIP runtime); the kernels are in jt_kernels.h (instantiated by
// jt_kv.hip, one translation unit per configuration).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "jt_denoise.h"
#include "jt_error.h"
#include "jt_internal.h"
#include "jt_kernels.h"
#include "jt_layout.h"

using namespace jtd;
using namespace jtk;

namespace jtk {
// every configuration is compiled in its own translation unit (jt_kv.hip)
JT_KV_FOR(0, extern template)
JT_KV_FOR(1, extern template)
JT_KV_FOR(2, extern template)
JT_KV_FOR(3, extern template)
JT_KV_FOR(4, extern template)
JT_KV_FOR(5, extern template)
JT_KV_FOR(6, extern template)
JT_KV_FOR(7, extern template)
JT_KV_FOR(8, extern template)
JT_KV_FOR(9, extern template)
JT_KV_FOR(10, extern template)
JT_KV_FOR(11, extern template)
JT_KV_FOR(12, extern template)
JT_KV_FOR(13, extern template)
JT_KV_FOR(14, extern template)
JT_KV_FOR(15, extern template)

// configuration ID of the binary traversal, or its wide twin (ID + NUM_BASE_CONFIGS)
template <int ID, int SAMPLER, int COUNT>
hipError_t launch_tw(bool wide, const DScene& S, const DParams& P, int s0, int s1, const DAccum& A, hipStream_t st, int cus) {
    return wide ? launch_cfg<ID + NUM_BASE_CONFIGS, SAMPLER, COUNT>(S, P, s0, s1, A, st, cus)
                : launch_cfg<ID, SAMPLER, COUNT>(S, P, s0, s1, A, st, cus);
}
// Stack configurations: the whole bound in a 16-entry LDS ring, or a RING-entry ring + HBM.
template <int SAMPLER, int COUNT>
hipError_t launch_s(int need, int ring, int kmask, bool wide, const DScene& S, const DParams& P, int s0, int s1,
                    const DAccum& A, hipStream_t st, int cus) {
    if (need <= 16) {
        if (kmask == (FT_NONE | FT_LINL)) return launch_tw<0, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
        if (kmask == FT_NONE) return launch_tw<7, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
        return launch_tw<1, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
    }
    if (ring <= 16) {
        switch (kmask) {
            case FT_MESH | FT_LINL: return launch_tw<2, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
            case FT_MESH_ENV | FT_NOIL: return launch_tw<3, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
            case FT_MESH_ENV_QUAD | FT_LINL: return launch_tw<4, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
            default: return launch_tw<5, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
        }
    }
    return launch_tw<6, SAMPLER, COUNT>(wide, S, P, s0, s1, A, st, cus);
}
}  // namespace jtk

// ============================================================================ C-ABI context
struct jt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DScene S{};
    DParams P{};
    DAccum A{};
    std::vector<void*> allocations;
    int width = 0, height = 0;
    int total_samples = 0, batch = 1, sampler = 1;
    int cus = 256;   // compute units of the device (persistent grid size)
    int lk = 0;      // log2 of the sample streams per pixel (DParams::lk; fixed at jt_create)
    int tiles = 0;   // 8x8 pixel tiles
    int stack = 16;  // stack bound of the scene (entries); > 16: LDS ring of `ring` + HBM overflow
    int ring = 16;
    int feat = FT_ALL;   // scene feature bits (jt_records.h)
    int kmask = FT_ALL;  // feature mask of the kernel specialisation the scene runs
    bool wide = false;   // JT_TRAVERSAL_WIDE: the wide-record kernels (configurations 8-15)
    int traversal = 0;   // jt_params.traversal as resolved (JT_TRAVERSAL_AUTO: near or wide)
    int first = -1, next = 0;  // running-mean origin and next expected sample (deferred ones included)
    // Deferred samples [pend0, pend1): jt_trace_range / jt_trace_samples queue their range and
    // trace it, merged with the ranges queued before it, once JT_DEFER_SAMPLES are queued or when
    // anything reads the context (flush). A render split into calls gives the bits of one call
    // (jt_trace_range's contract), so merging changes only the launch count: the reference's
    // default --batch 1 (one call per sample) runs as launches of many samples each.
    int pend0 = 0, pend1 = 0;
    // one-stream contexts (lk == 0): a flushed range of m > 1 samples runs as chunks of up to
    // `chunk` samples, each traced as one-sample streams into the stream-mean buffers (allocated at
    // the first such flush) and folded into the running mean by chain_kernel in sample order
    int chunk = 0;
    // two sets of chunk buffers: chunk i traces into set i & 1 on `stream` while chain_kernel folds
    // chunk i - 1 on `stream2` (the chains stay in sample order on stream2; a trace reuses a set
    // only after the chain that read it, chain_done)
    float4* cpart[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    hipStream_t stream2 = nullptr;
    hipEvent_t trace_done[2] = {nullptr, nullptr}, chain_done[2] = {nullptr, nullptr};
    bool exported = false;  // jt_get_device_buffers handed out the accumulators' device pointers
    int count = 1;             // 1: all traversal counters (diagnostic), 0: paths/rays/light queries only
    bool failed = false;       // a launch failed: the running means are unusable
    bool stale = true;         // the accumulators are not yet zeroed or overwritten since jt_reset
    // k > 1: the last launch combined the image only; albedo, normal and hits are combined from
    // the stream means (weights aov_cw) when first read (finish_aovs)
    bool aov_pending = false;
    DCombine aov_cw{};
    bool env_alias = false;    // JT_ENV_ALIAS=1: environment lights sample through alias tables
                               // until jt_reset
    size_t lds_scene_bytes = 0;  // > 0: small-scene LDS mode
    unsigned long long launches = 0;
    double kernel_ms = 0;
    // multi-device context (jt_create_multi): one sub-context per device, each tracing its share
    // of every batch into its own running mean; RCCL communicators for the reduce of jt_get_image
    std::vector<jt_ctx*> sub;
    std::vector<ncclComm_t> comms;
    std::vector<long long> nsub;  // samples accumulated by each device
    // split of every batch: false = contiguous sample shares (device d's mean weighted n_d / N in
    // the reduce), true = interleaved 8x8 pixel tiles (tile t on device t mod D, every sample of
    // the batch; disjoint pixels, so the reduce is a plain sum). Tiles when params.batch < D:
    // the reference's default --batch 1 would leave all but one device idle under a sample split
    bool tile_split = false;
    float* red = nullptr;         // device 0: reduce target, W*H float4
    long long* red_hits = nullptr;
    // the denoiser (jt_denoise, jt_denoise.hip): two scratch buffers and the result, float4[W*H]
    // each, allocated by the first jt_denoise and kept across jt_reset. A multi-device context
    // filters the reduced host arrays on device 0 and keeps the result on the host instead
    float4* dn[3] = {nullptr, nullptr, nullptr};
    std::vector<float> dn_host;
    bool denoised = false;  // the result is the filter of the current running means
    // the error estimate (jt_get_variance, jt_get_noise; jt_error.hip): the per-pixel variance of
    // the mean, float4[W*H], and one (V, M) pair per workgroup; allocated (the variance zeroed) by
    // the first call and kept across jt_reset. err_noise is the scalar of the current samples
    float4* err_var = nullptr;
    float2* err_sums = nullptr;
    double err_noise = 0;
    bool err_valid = false;  // err_var and err_noise are those of the current running means
};

namespace jtk {
// the combine of every pixel's stream means (DCombine, jt_kernels.h), one thread per pixel of
// the launch's tiles (slot g); stream j's records of neighbouring pixels are contiguous (coalesced).
// Two kernels over the same streams: the image after every launch (16 B per pixel and stream),
// the AOVs and hits (32 B per pixel and stream) only when they are read (jt_ctx::aov_pending):
// the stream means stay in place until the next launch appends to them, so the deferred AOV
// combine reads exactly what an eager one would have
template <bool AOV>
__global__ __launch_bounds__(256) void combine_kernel(DParams P, DAccum A, DCombine Cw) {
    const int tiles_x = (P.width + 7) / 8, tiles = launch_tiles(P);
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= tiles * 64) return;
    const int t = (g >> 6) * P.tile_stride + P.tile_offset, l = g & 63;
    const int i = (t % tiles_x) * 8 + (l & 7), j = (t / tiles_x) * 8 + (l >> 3);
    if (i >= P.width || j >= P.height) return;
    const size_t pixel = (size_t)j * P.width + i, ns = (size_t)A.nslot;
    const float w0 = Cw.w[0];
    if constexpr (!AOV) {
        float4 im = A.part_img[g];
        im = make_float4(im.x * w0, im.y * w0, im.z * w0, im.w * w0);
        // unrolled: eight streams' loads in flight per thread (the sums stay in stream order)
#pragma unroll 8
        for (int s = 1; s < Cw.ns; s++) {
            const float w = Cw.w[s];
            const float4 a = A.part_img[s * ns + g];
            im = make_float4(im.x + a.x * w, im.y + a.y * w, im.z + a.z * w, im.w + a.w * w);
        }
        A.image[pixel] = im;
    } else {
        float4 al = A.part_alb[g], nr = A.part_nrm[g];
        long long h = __float_as_int(al.w);
        al = make_float4(al.x * w0, al.y * w0, al.z * w0, 0.0f);
        nr = make_float4(nr.x * w0, nr.y * w0, nr.z * w0, 0.0f);
#pragma unroll 4
        for (int s = 1; s < Cw.ns; s++) {
            const float w = Cw.w[s];
            const float4 b = A.part_alb[s * ns + g], c = A.part_nrm[s * ns + g];
            al = make_float4(al.x + b.x * w, al.y + b.y * w, al.z + b.z * w, 0.0f);
            nr = make_float4(nr.x + c.x * w, nr.y + c.y * w, nr.z + c.z * w, 0.0f);
            h += __float_as_int(b.w);
        }
        A.albedo[pixel] = al;
        A.normal[pixel] = nr;
        A.hits[pixel] = h;
    }
}

// A chunk of a one-stream context (k = 1, the reference's single running mean): the chunk's
// samples x .. x+m-1 were traced as m one-sample streams (each record = that sample's value:
// 0 * 0 + value * 1), and are folded into the running mean here one by one, in sample order, with
// the epilogue's own operations (mean * (1 - w) + value * w, w = 1 / (n0 + j + 1): src/trace.jl:
// 631-648, src/math.jl:89-93) — bit for bit the image of tracing the samples one launch each.
// n0: the context's samples before the chunk (0: the mean starts from zero, as after jt_reset).
// At most 32 VGPRs: the trace kernel of the next chunk (5 waves/SIMD of 96 VGPRs in LDS mode)
// leaves 32 per SIMD free, so chain waves run on the same CUs beside it (stream2).
__global__ __launch_bounds__(256) void chain_kernel(DParams P, DAccum A, int n0, int m) {
    const int tiles_x = (P.width + 7) / 8, tiles = launch_tiles(P);
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= tiles * 64) return;
    const int t = (g >> 6) * P.tile_stride + P.tile_offset, l = g & 63;
    const int i = (t % tiles_x) * 8 + (l & 7), j = (t / tiles_x) * 8 + (l >> 3);
    if (i >= P.width || j >= P.height) return;
    const unsigned pixel = (unsigned)j * (unsigned)P.width + (unsigned)i;  // jt_create: < 2^26 pixels
    float ix = 0, iy = 0, iz = 0, iw = 0, ax = 0, ay = 0, az = 0, nx = 0, ny = 0, nz = 0;
    int h = 0;  // the chunk's hits (< 2^31 samples)
    if (n0 > 0) {
        const float4 a = A.image[pixel], b = A.albedo[pixel], c = A.normal[pixel];
        ix = a.x, iy = a.y, iz = a.z, iw = a.w, ax = b.x, ay = b.y, az = b.z, nx = c.x, ny = c.y, nz = c.z;
    }
    // few live registers (byte offsets below 4 GiB: 2^27 records of 16 B at most per buffer set
    // and array, jt_ctx::chunk), so the waves fit beside the next chunk's trace kernel
    const char* pi = reinterpret_cast<const char*>(A.part_img);
    const char* pa = reinterpret_cast<const char*>(A.part_alb);
    const char* pn = reinterpret_cast<const char*>(A.part_nrm);
    const unsigned step = (unsigned)A.nslot * 16u;
    unsigned off = (unsigned)g * 16u;
#pragma unroll 1
    for (int s = 0; s < m; s++, off += step) {
        const float w = 1.0f / (float)(n0 + s + 1), omw = 1 - w;
        const float4 a = *reinterpret_cast<const float4*>(pi + off);
        ix = ix * omw + a.x * w, iy = iy * omw + a.y * w, iz = iz * omw + a.z * w, iw = iw * omw + a.w * w;
        const float4 b = *reinterpret_cast<const float4*>(pa + off);
        ax = ax * omw + b.x * w, ay = ay * omw + b.y * w, az = az * omw + b.z * w;
        h += __float_as_int(b.w);
        const float4 c = *reinterpret_cast<const float4*>(pn + off);
        nx = nx * omw + c.x * w, ny = ny * omw + c.y * w, nz = nz * omw + c.z * w;
    }
    A.image[pixel] = make_float4(ix, iy, iz, iw);
    A.albedo[pixel] = make_float4(ax, ay, az, 0.0f);
    A.normal[pixel] = make_float4(nx, ny, nz, 0.0f);
    A.hits[pixel] = (n0 > 0 ? A.hits[pixel] : 0LL) + h;
}

}  // namespace jtk

namespace {

int hip_fail(hipError_t e, const char* what) {
    return jt::fail(JT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
int zero_if_stale(jt_ctx* c);

// RCCL, loaded on first use by a multi-device context (dlopen of the ROCm install's
// librccl.so.1): single-device contexts never touch it, and a process that already loaded an
// RCCL (e.g. torch's) shares that one instead of a second copy
struct Rccl {
    bool ok = false;
    decltype(&ncclCommInitAll) CommInitAll;
    decltype(&ncclCommDestroy) CommDestroy;
    decltype(&ncclReduce) Reduce;
    decltype(&ncclGroupStart) GroupStart;
    decltype(&ncclGroupEnd) GroupEnd;
    decltype(&ncclRedOpCreatePreMulSum) RedOpCreatePreMulSum;
    decltype(&ncclRedOpDestroy) RedOpDestroy;
    decltype(&ncclGetErrorString) GetErrorString;
};
const Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return x;
        x.CommInitAll = (decltype(x.CommInitAll))dlsym(h, "ncclCommInitAll");
        x.CommDestroy = (decltype(x.CommDestroy))dlsym(h, "ncclCommDestroy");
        x.Reduce = (decltype(x.Reduce))dlsym(h, "ncclReduce");
        x.GroupStart = (decltype(x.GroupStart))dlsym(h, "ncclGroupStart");
        x.GroupEnd = (decltype(x.GroupEnd))dlsym(h, "ncclGroupEnd");
        x.RedOpCreatePreMulSum = (decltype(x.RedOpCreatePreMulSum))dlsym(h, "ncclRedOpCreatePreMulSum");
        x.RedOpDestroy = (decltype(x.RedOpDestroy))dlsym(h, "ncclRedOpDestroy");
        x.GetErrorString = (decltype(x.GetErrorString))dlsym(h, "ncclGetErrorString");
        x.ok = x.CommInitAll && x.CommDestroy && x.Reduce && x.GroupStart && x.GroupEnd && x.RedOpCreatePreMulSum &&
               x.RedOpDestroy && x.GetErrorString;
        return x;
    }();
    return r;
}
int nccl_fail(ncclResult_t r, const char* what) {
    return jt::fail(JT_ERR_DEVICE, std::string(what) + ": " + rccl().GetErrorString(r));
}

template <class T>
int upload(jt_ctx* c, const std::vector<T>& host, const T** dptr) {
    size_t bytes = std::max<size_t>(sizeof(T), host.size() * sizeof(T));
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return jt::fail(JT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    c->allocations.push_back(p);
    if (!host.empty()) {
        e = hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    }
    *dptr = (const T*)p;
    return JT_OK;
}

// the launch schedule: a unit counter per XCD band
constexpr size_t SCHED_BYTES = (size_t)NBANDS * BAND_STRIDE * 4;

// Sample streams per pixel (DESIGN.md §2 "Sample streams"), fixed at jt_create from the pixels
// the context traces and the batch only (never from the scene's memory mode, so every option
// that picks LDS or HBM mode keeps the image bits): 1 for the reference's default one-sample
// batches (its single running mean); otherwise at least 16 — 32 from a batch of 64 (two samples
// per stream) — and enough for 2^22 (pixel, stream) items (a context tracing few pixels — a tile
// share, a small image — still fills the GPU), at most 64, the batch, and 2^27 items of stream
// means (6.4 GB).
// Measured (gpurun_out/r05i, r05j): bathroom1 1024 spp 8 -> 16 streams +0.8 %, features2 512 spp
// +2 %, ecosys 64 spp 2 -> 16 +2.6 %, its 1/8 share (512 spp) +3.7 %; a 1/8 tile share of the
// headline 32 streams 9265, 64 streams 9794 Mrays/s. A context whose scene runs from HBM starts
// from 32 streams when the batch gives each at least two samples (gpurun_out/r05sk, r05sk2:
// features2 +0.6 %, bathroom1 +0.5 %; cornellbox +1.0 %, round 5, when 32 streams were the
// HBM-mode rule only). The option "streams" overrides.
int stream_log2(long long pixels, int batch) {
    if (batch <= 1) return 0;
    long long want = batch >= 2 * JT_STREAMS_WIDE ? JT_STREAMS_WIDE : JT_STREAMS_MIN;
    while (pixels * want < JT_STREAM_ITEMS) want *= 2;
    int lk = 0;
    while (lk < 6 && (2LL << lk) <= want && (2 << lk) <= batch && (2 << lk) <= JT_MAX_STREAMS &&
           pixels * (2LL << lk) <= JT_STREAM_ITEMS_MAX)
        lk++;
    return lk;
}

// ------------------------------------------------------------------------ the steps of jt_create
static_assert(jt::IDX_MASK == jtk::IDX_MASK, "the layout's index limit is the kernels'");

// A scene ready for upload: its host layout (jt_layout.h) and what depends on the kernels' LDS use
struct PreparedScene {
    jt::HostScene hs;
    int ring = 16;               // entries of the overflow kernels' LDS stack ring (option lds_stack)
    size_t lds_scene_bytes = 0;  // > 0: small-scene LDS mode, the bytes of the blob
    int traversal = 0;           // jt_params.traversal, JT_TRAVERSAL_AUTO resolved to near or wide
};

// The bytes of the LDS blob when the scene runs from it, 0 for HBM mode.
// LDS mode only when the blob does not cost workgroups per CU: the kernel holds at most
// 4 workgroups per CU (4 waves/SIMD), so the blob + stack + accumulators may use up to
// 160 KiB / 4, or as much as HBM mode's stack + accumulators already cost. Override
// with the option lds_scene=0 (off) or a byte budget for the blob.
size_t lds_mode_bytes(const jt::HostScene& hs, int ring, const jt::Options& opts) {
    size_t budget = 48 * 1024;
    if (const char* v = jt::opt(opts, "lds_scene")) budget = (size_t)std::atoll(v);
    // HBM mode's stack is the kernel's static ring (16 or 32 entries); LDS mode's, without
    // overflow, just the scene's bound
    // + the texel-decode LUTs a texture kernel keeps in LDS (trace_body)
    const size_t acc_bytes = (size_t)ACC_SLOTS * BLOCK * 4 + ((hs.feat & FT_TEX) ? 2048 : 0);
    const size_t base_bytes = (size_t)(hs.need <= 16 ? 16 : ring) * BLOCK * 4 + acc_bytes;
    const size_t lds_base = lds_stack_bytes(hs.need > 16, ring, hs.need) + acc_bytes;
    const size_t bytes = hs.blob.size() * 16;
    const size_t lds_cu = 160 * 1024;
    const size_t wg_hbm = std::min<size_t>(4, lds_cu / base_bytes), wg_lds = lds_cu / (lds_base + bytes);
    return bytes <= budget && wg_lds >= wg_hbm ? bytes : 0;
}

// Host only: the layout, the LDS / HBM decision and the traversal JT_TRAVERSAL_AUTO resolves to.
int prepare_scene(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                  const jt::Options& opts, PreparedScene& ps) {
    jt::HostScene& hs = ps.hs;
    int st = jt::layout_scene(scene, bvh, lights, params, opts, hs);
    if (st != JT_OK) return st;
    if (const char* r = jt::opt(opts, "lds_stack")) ps.ring = std::atoi(r) > 16 ? 32 : 16;
    ps.lds_scene_bytes = lds_mode_bytes(hs, ps.ring, opts);
    // auto: wide for a scene in HBM mode whose BVH is deep (a stack bound above 32: bathroom1 46,
    // ecosys 43: +20 %, +30 % over near); near otherwise — features2 (bound 24) runs 2737/2742
    // Mrays/s near vs 2677/2646 wide at 512 spp (gpurun_out/r04m), cornellbox runs from LDS
    if (params->traversal == JT_TRAVERSAL_AUTO && !ps.lds_scene_bytes && hs.need > JT_AUTO_WIDE_MIN_STACK) {
        // HBM mode: the wide records (the binary nodes stay uploaded, unused); the instances'
        // BLAS roots become root records
        if ((st = jt::make_wide(hs, scene, bvh)) != JT_OK) return st;
    }
    ps.traversal = params->traversal == JT_TRAVERSAL_AUTO ? (hs.wide ? JT_TRAVERSAL_WIDE : JT_TRAVERSAL_NEAR)
                                                          : params->traversal;
    return JT_OK;
}

// every array of the list (jt_layout.h), and the blob in LDS mode
int upload_scene(jt_ctx* c, const PreparedScene& ps) {
    const jt::HostScene& hs = ps.hs;
    DScene& S = c->S;
    S = hs.S;
    int st;
#define JT_UPLOAD(T, name) \
    if ((st = upload(c, hs.name, &S.name)) != JT_OK) return st;
    JT_SCENE_ARRAYS(JT_UPLOAD, JT_UPLOAD)
#undef JT_UPLOAD
    S.blob = nullptr;
    S.blob_n16 = 0;
    if (ps.lds_scene_bytes) {
        if ((st = upload(c, hs.blob, &S.blob)) != JT_OK) return st;
        S.blob_n16 = (int)hs.blob.size();
    }
    return JT_OK;
}

int device_alloc(jt_ctx* c, size_t bytes, const char* what, void** p) {
    *p = nullptr;
    if (hipMalloc(p, bytes) != hipSuccess) return jt::fail(JT_ERR_NOMEM, std::string("hipMalloc ") + what);
    c->allocations.push_back(*p);
    return JT_OK;
}

// the stack members of the device scene and, for a bound above the LDS ring, its HBM overflow
int alloc_stack_overflow(jt_ctx* c, const jt::Options& opts) {
    DScene& S = c->S;
    const int need = c->stack;
    S.ovf = nullptr;
    S.ovf_stride = 0;
    S.ring = c->ring;
    S.stack_need = c->stack;
    // option test_lds_ring (tests only): use fewer ring entries than allocated, to exercise the overflow
    if (const char* r = jt::opt(opts, "test_lds_ring")) {
        int v = std::atoi(r);
        if (v >= 1 && v <= 16 && (v & (v - 1)) == 0) {
            S.ring = v;
            c->stack = std::max(c->stack, 17);  // force the overflow-capable kernel
            c->ring = 16;
        }
    }
    if (c->stack > 16) {  // HBM overflow of the LDS stack ring: `need` entries per lane of the
        // persistent grid (at most 8 workgroups of BLOCK lanes per CU resident; kernel slot
        // blockIdx.x * BLOCK + threadIdx.x: a query never outlives its lane)
        void* p = nullptr;
        const int st = device_alloc(c, (size_t)c->cus * 8 * BLOCK * (size_t)need * 4, "stack overflow", &p);
        if (st != JT_OK) return st;
        S.ovf = (int*)p;
        S.ovf_stride = need;
    }
    return JT_OK;
}

// DParams: camera, tile share, sample streams, wait lanes and light lanes; the kernel mask.
// forced_streams: the option "streams" set the stream count
int make_params(jt_ctx* c, const jt_scene* scene, const jt_params* params, const jt::Options& opts, bool inst_light,
                bool& forced_streams) {
    DParams& P = c->P;
    const int W = c->width, H = c->height;
    const jt_camera& cam = scene->cameras[params->camera];
    std::memcpy(P.cam.frame, cam.frame, sizeof(P.cam.frame));
    P.cam.orthographic = cam.orthographic;
    P.cam.lens = cam.lens;
    P.cam.film = cam.film;
    P.cam.aspect = (params->width > 0 && params->height > 0) ? (float)W / (float)H : cam.aspect;
    // film = aspect >= 1 ? (film, film / aspect) : (film * aspect, film) (src/scene.jl:377-378)
    P.cam.film_x = P.cam.aspect >= 1 ? cam.film : cam.film * P.cam.aspect;
    P.cam.film_y = P.cam.aspect >= 1 ? cam.film / P.cam.aspect : cam.film;
    P.cam.focus = cam.focus;
    P.cam.aperture = cam.aperture;
    P.cam.pinhole = (std::signbit(cam.aperture) == 0 && cam.aperture == 0.0f) ? 1 : 0;
    P.width = W;
    P.height = H;
    P.bounces = params->bounces;
    P.sampler = params->sampler;
    P.clamp = (float)params->clamp;
    P.envhidden = params->envhidden;
    P.tentfilter = params->tentfilter;
    P.nocaustics = params->nocaustics;
    P.first = 0;
    P.seed = params->seed;
    P.tile_stride = 1;  // every tile (jt_create_multi may split by tiles)
    P.tile_offset = 0;
    // option tile_share "stride,offset": trace only tiles offset, offset + stride, ... — one
    // process's share of a render split by tiles over one process per GPU (bench.py), or one
    // device's share of jt_create_multi's tile split reproduced on one GPU (tests)
    if (const char* ts = jt::opt(opts, "tile_share")) {
        int k = 0, o = 0;
        if (std::sscanf(ts, "%d,%d", &k, &o) == 2 && k >= 1 && o >= 0 && o < k) {
            P.tile_stride = k;
            P.tile_offset = o;
        }
    }
    // sample streams: from the pixels this context traces (a tile share traces 1/stride of them)
    c->lk = stream_log2(((long long)W * H + P.tile_stride - 1) / P.tile_stride, std::max(1, params->batch));
    forced_streams = false;
    if (const char* ks = jt::opt(opts, "streams")) {
        forced_streams = true;
        const int k = std::atoi(ks);
        if (k < 1 || k > JT_MAX_STREAMS || (k & (k - 1)) != 0)
            return jt::fail(JT_ERR_INVALID, "option streams: a power of two in [1, " + std::to_string(JT_MAX_STREAMS) + "]");
        c->lk = 0;
        while ((1 << c->lk) < k) c->lk++;
    }
    P.lk = c->lk;
    // measured best (cornellbox): 40 waiting lanes per shading phase; 48 with
    // light-hit steps in the traversal phase (they take the light queries out of the phases)
    c->kmask = kernel_mask(c->feat, c->stack, c->ring, c->lds_scene_bytes > 0, c->S.light_inline != 0, inst_light);
    // light queries leave the shading phase's waiting lanes early (light-hit steps) or never wait
    // there at all (inline chains): the gate then waits for more lanes
    const int smp = c->sampler == JT_SAMPLER_NAIVE ? 2 : 1;
    const bool lstep = inst_light && smp == 1 && (light_steps(smp, c->kmask) || c->S.light_inline);
    // deep BVHs (stack bound > 32: bathroom1, ecosys) shade sooner: their lanes finish queries far
    // apart, so waiting for many leaves the wave idle. Re-swept in round 4 (per-lane work items,
    // short chunks, auto traversal; profiles/r04_ab/wait_lanes_r04o.txt): cornellbox 56 (52
    // even, 48 / 60 -1.3 %, 64 -6 %), features2 56 (60 -2.9 %, 48 -0.5 %, 64 -9 %), bathroom1 40
    // (48 even, 24 -10 %), ecosys (no instance lights) 24 (16 -1.2 %, 32 -2.2 %, 8 -11 %)
    const bool deep = c->stack > 32;
    P.wait_lanes = lstep ? (deep ? 40 : 56) : deep ? 24 : 40;
    if (const char* wl = jt::opt(opts, "wait_lanes")) P.wait_lanes = std::max(1, std::min(64, std::atoi(wl)));
    P.light_lanes = 2;
    if (const char* ll = jt::opt(opts, "light_lanes")) P.light_lanes = std::max(1, std::min(65, std::atoi(ll)));
    return JT_OK;
}

// accumulators (make_trace_state: zeroed) + counters, the schedule and the stream means
int alloc_accumulators(jt_ctx* c, bool forced_streams) {
    DParams& P = c->P;
    const int W = c->width, H = c->height;
    const size_t np = (size_t)W * (size_t)H;
    void *img, *alb, *nrmb, *hits, *cnt, *sched;
    int st;
    if ((st = device_alloc(c, np * 16, "accumulators", &img)) || (st = device_alloc(c, np * 16, "accumulators", &alb)) ||
        (st = device_alloc(c, np * 16, "accumulators", &nrmb)) || (st = device_alloc(c, np * 8, "accumulators", &hits)) ||
        (st = device_alloc(c, 32 * 8, "counters", &cnt)))
        return st;
    // persistent scheduling: unit counters (zeroed before each launch)
    c->tiles = ((W + 7) / 8) * ((H + 7) / 8);
    if (c->tiles >= (1 << 20))  // the per-lane work items address a pixel as tile * 64 + l
        return jt::fail(JT_ERR_UNSUPPORTED, "image above 2^20 8x8 tiles (67 Mpixels)");
    if ((st = device_alloc(c, SCHED_BYTES, "schedule", &sched)) != JT_OK) return st;
    // the sample streams' means (k > 1): image, albedo + hits, normal per (stream, slot of the
    // launch's tiles: a tile share holds only its own pixels). Too little memory for k streams
    // halves k (the image bits then follow the smaller k, jt_get_streams) unless the option
    // "streams" asked for this k.
    void* part[3] = {nullptr, nullptr, nullptr};
    const size_t nslot = (size_t)launch_tiles(P) * 64;
    while (c->lk > 0) {
        const size_t mark = c->allocations.size();
        bool ok = true;
        for (int k = 0; k < 3 && ok; k++) ok = device_alloc(c, nslot * 16 << c->lk, "stream means", &part[k]) == JT_OK;
        if (ok) break;
        (void)hipGetLastError();
        for (; c->allocations.size() > mark; c->allocations.pop_back()) (void)hipFree(c->allocations.back());
        part[0] = part[1] = part[2] = nullptr;
        if (forced_streams) return JT_ERR_NOMEM;  // "hipMalloc stream means"
        c->lk--;
    }
    P.lk = c->lk;
    c->A = DAccum{(float4*)img, (float4*)alb, (float4*)nrmb, (long long*)hits, (unsigned long long*)cnt, (unsigned*)sched,
                  (float4*)part[0], (float4*)part[1], (float4*)part[2], (int)nslot};
    return JT_OK;
}

unsigned long long fnv1a64(const void* data, size_t n) {
    unsigned long long h = 14695981039346656037ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)data)[i]) * 1099511628211ull;
    return h;
}

}  // namespace

extern "C" {

int jt_device_count(int32_t* out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *out = n;
    return JT_OK;
}

void jt_destroy(jt_ctx* c) {
    if (!c) return;
    if (!c->sub.empty() || !c->comms.empty()) {
        for (ncclComm_t m : c->comms) (void)rccl().CommDestroy(m);
        if (!c->sub.empty()) {
            (void)hipSetDevice(c->sub[0]->device);
            if (c->red) (void)hipFree(c->red);
            if (c->red_hits) (void)hipFree(c->red_hits);
        }
        for (jt_ctx* s : c->sub) jt_destroy(s);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (void* p : c->allocations) (void)hipFree(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int k = 0; k < 2; k++) {
        if (c->trace_done[k]) (void)hipEventDestroy(c->trace_done[k]);
        if (c->chain_done[k]) (void)hipEventDestroy(c->chain_done[k]);
    }
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int jt_create(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
              jt_ctx** out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    // the run-time options (jt_set_option) this context is created with
    const jt::Options opts = jt::options_snapshot();
    PreparedScene ps;
    int st = prepare_scene(scene, bvh, lights, params, opts, ps);
    if (st != JT_OK) return st;

    hipError_t e = hipSetDevice(params->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    jt_ctx* c = new jt_ctx();
    c->device = params->device;
    c->width = ps.hs.width;
    c->height = ps.hs.height;
    c->total_samples = params->samples;
    c->batch = params->batch;
    c->sampler = params->sampler;
    c->stack = ps.hs.need;
    c->ring = ps.ring;
    c->feat = ps.hs.feat;
    c->wide = ps.hs.wide;
    c->traversal = ps.traversal;
    c->env_alias = ps.hs.env_alias;
    c->lds_scene_bytes = ps.lds_scene_bytes;
    auto bail = [&](int status) {
        jt_destroy(c);
        return status;
    };
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail(hip_fail(e, "hipStreamCreate"));
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess)
        return bail(hip_fail(e, "hipEventCreate"));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, params->device) == hipSuccess && cus > 0) c->cus = cus;

    bool forced_streams = false;
    if ((st = upload_scene(c, ps)) || (st = alloc_stack_overflow(c, opts)) ||
        (st = make_params(c, scene, params, opts, ps.hs.inst_light, forced_streams)) ||
        (st = alloc_accumulators(c, forced_streams)) || (st = jt_reset(c)))
        return bail(st);
    *out = c;
    return JT_OK;
}

// The host layout jt_create would upload, as text (tests/test_layout.py; like jt_debug_stamps not
// part of include/jtrace.h). Touches no device. One line "name length fnv1a64" per array of the
// list (jt_layout.h) and for the blob (empty in HBM mode), then the scalars.
int jt_debug_layout_digest(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                           char* buf, int32_t n) {
    if (!buf || n <= 0) return jt::fail(JT_ERR_INVALID, "NULL argument");
    PreparedScene ps;
    const int st = prepare_scene(scene, bvh, lights, params, jt::options_snapshot(), ps);
    if (st != JT_OK) return st;
    const jt::HostScene& hs = ps.hs;
    const DScene& S = hs.S;
    std::string text;
    char line[1024];
    auto item = [&](const char* name, size_t len, const void* data, size_t bytes) {
        std::snprintf(line, sizeof line, "%s %zu %016llx\n", name, len, fnv1a64(data, bytes));
        text += line;
    };
#define JT_DIGEST(T, name) item(#name, hs.name.size(), hs.name.data(), hs.name.size() * sizeof(T));
    JT_SCENE_ARRAYS(JT_DIGEST, JT_DIGEST)
#undef JT_DIGEST
    const size_t blob_n16 = ps.lds_scene_bytes ? hs.blob.size() : 0;
    item("blob", blob_n16, hs.blob.data(), blob_n16 * 16);
    std::snprintf(line, sizeof line,
                  "scalars need=%d feat=%d traversal=%d tlas_nnodes=%d tlas_wnodes=%d order_flip=%d light_inline=%d "
                  "o_nodes=%d o_wnodes=%d o_prims=%d o_inst_trav=%d o_inst_blas=%d o_inst_shade=%d o_shapes=%d o_pos=%d o_nrm=%d "
                  "o_tc=%d o_col=%d o_elems=%d o_enrm=%d o_enrm_id=%d o_materials=%d o_lights=%d o_cdf=%d o_light_hit=%d "
                  "o_light_elems=%d blob_n16=%d\n",
                  hs.need, hs.feat, ps.traversal, S.tlas_nnodes, S.tlas_wnodes, S.order_flip, S.light_inline, S.o_nodes, S.o_wnodes,
                  S.o_prims, S.o_inst_trav, S.o_inst_blas, S.o_inst_shade, S.o_shapes, S.o_pos, S.o_nrm, S.o_tc, S.o_col, S.o_elems,
                  S.o_enrm, S.o_enrm_id, S.o_materials, S.o_lights, S.o_cdf, S.o_light_hit, S.o_light_elems, (int)blob_n16);
    text += line;
    if (text.size() + 1 > (size_t)n) return jt::fail(JT_ERR_INVALID, "layout digest: buffer too small");
    std::memcpy(buf, text.c_str(), text.size() + 1);
    return JT_OK;
}

// The raw bytes of one array of the list, by name, for the structural checks of tests/test_layout.py:
// *nbytes is its size; it is copied to `data` when that is not NULL and holds `cap` >= *nbytes bytes.
int jt_debug_layout_array(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                          const char* name, void* data, int64_t cap, int64_t* nbytes) {
    if (!name || !nbytes) return jt::fail(JT_ERR_INVALID, "NULL argument");
    PreparedScene ps;
    const int st = prepare_scene(scene, bvh, lights, params, jt::options_snapshot(), ps);
    if (st != JT_OK) return st;
    const void* src = nullptr;
    *nbytes = -1;
#define JT_FIND(T, member) \
    if (std::strcmp(name, #member) == 0) src = ps.hs.member.data(), *nbytes = (int64_t)(ps.hs.member.size() * sizeof(T));
    JT_SCENE_ARRAYS(JT_FIND, JT_FIND)
#undef JT_FIND
    if (*nbytes < 0) return jt::fail(JT_ERR_INVALID, std::string("layout array: no array named ") + name);
    if (data && cap < *nbytes) return jt::fail(JT_ERR_INVALID, "layout array: buffer too small");
    if (data && *nbytes) std::memcpy(data, src, (size_t)*nbytes);
    return JT_OK;
}

int jt_create_multi(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                    const int32_t* devices, int32_t ndevices, jt_ctx** out) {
    if (!out) return jt::fail(JT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!params) return jt::fail(JT_ERR_INVALID, "NULL argument");
    int avail = 0;
    if (hipGetDeviceCount(&avail) != hipSuccess) avail = 0;
    if (ndevices < 1 || ndevices > avail)
        return jt::fail(JT_ERR_INVALID, "ndevices must be in [1, " + std::to_string(avail) + "]");
    std::vector<int> devs(ndevices);
    for (int d = 0; d < ndevices; d++) {
        devs[d] = devices ? devices[d] : d;
        if (devs[d] < 0 || devs[d] >= avail) return jt::fail(JT_ERR_INVALID, "device id out of range");
        for (int k = 0; k < d; k++)
            if (devs[k] == devs[d]) return jt::fail(JT_ERR_INVALID, "a device is listed twice");
    }
    if (!rccl().ok) return jt::fail(JT_ERR_UNSUPPORTED, "librccl.so.1 (RCCL) could not be loaded");
    jt_ctx* c = new jt_ctx();
    for (int d = 0; d < ndevices; d++) {
        jt_params p = *params;
        p.device = devs[d];
        jt_ctx* s = nullptr;
        const int st = jt_create(scene, bvh, lights, &p, &s);
        if (st != JT_OK) {
            jt_destroy(c);
            return st;
        }
        c->sub.push_back(s);
    }
    c->nsub.assign(ndevices, 0);
    // split mode (jt_ctx::tile_split); the option multi_split=tiles|samples overrides
    c->tile_split = params->batch < ndevices;
    {
        const auto opts = jt::options_snapshot();
        const auto m = opts.find("multi_split");
        if (m != opts.end() && m->second == "tiles") c->tile_split = true;
        if (m != opts.end() && m->second == "samples") c->tile_split = false;
    }
    // every sub-context traces every tile under the sample split (a tile_share option never
    // leaves tiles out of the reduced image), its interleaved share under the tile split
    for (int d = 0; d < ndevices; d++) {
        c->sub[d]->P.tile_stride = c->tile_split ? ndevices : 1;
        c->sub[d]->P.tile_offset = c->tile_split ? d : 0;
        // a device's share leaves the other devices' tiles at zero for the summing reduce
        const int st = c->tile_split ? zero_if_stale(c->sub[d]) : JT_OK;
        if (st != JT_OK) {
            jt_destroy(c);
            return st;
        }
    }
    c->comms.resize(ndevices);
    ncclResult_t r = rccl().CommInitAll(c->comms.data(), ndevices, devs.data());
    if (r != ncclSuccess) {
        c->comms.clear();
        jt_destroy(c);
        return nccl_fail(r, "ncclCommInitAll");
    }
    jt_ctx* s0 = c->sub[0];
    c->device = s0->device;
    c->width = s0->width;
    c->height = s0->height;
    c->total_samples = s0->total_samples;
    c->batch = s0->batch;
    c->sampler = s0->sampler;
    (void)hipSetDevice(s0->device);
    const size_t np = (size_t)c->width * c->height;
    if (hipMalloc(&c->red, np * 16) != hipSuccess || hipMalloc(&c->red_hits, np * 8) != hipSuccess) {
        jt_destroy(c);
        return jt::fail(JT_ERR_NOMEM, "hipMalloc reduce buffers");
    }
    *out = c;
    return JT_OK;
}

namespace {
int zero_if_stale(jt_ctx* c) {
    if (!c->stale) return JT_OK;
    (void)hipSetDevice(c->device);
    const size_t np = (size_t)c->width * (size_t)c->height;
    hipError_t e;
    if ((e = hipMemsetAsync(c->A.image, 0, np * 16, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->A.albedo, 0, np * 16, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->A.normal, 0, np * 16, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->A.hits, 0, np * 8, c->stream)) != hipSuccess)
        return hip_fail(e, "hipMemsetAsync");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    c->stale = false;
    return JT_OK;
}
// the deferred AOV combine of the last launch (jt_ctx::aov_pending), before albedo, normal or
// hits are read: jt_get_aovs, jt_synchronize, jt_get_device_buffers
int finish_aovs(jt_ctx* c) {
    if (!c->aov_pending) return JT_OK;
    (void)hipSetDevice(c->device);
    const int nblk = (int)(((long long)launch_tiles(c->P) * 64 + 255) / 256);
    hipLaunchKernelGGL(jtk::combine_kernel<true>, dim3(nblk), dim3(256), 0, c->stream, c->P, c->A, c->aov_cw);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->failed = true;
        return hip_fail(e, "AOV combine");
    }
    c->aov_pending = false;
    return JT_OK;
}
}  // namespace

int jt_reset(jt_ctx* c) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    c->denoised = false;
    c->err_valid = false;
    if (!c->sub.empty()) {
        for (jt_ctx* s : c->sub) {
            const int st = jt_reset(s);
            if (st != JT_OK) return st;
        }
        std::fill(c->nsub.begin(), c->nsub.end(), 0LL);
        c->pend0 = c->pend1 = 0;  // deferred samples are dropped with the state
        c->first = -1;
        c->next = 0;
        c->failed = false;
        c->launches = 0;
        c->kernel_ms = 0;
        return JT_OK;
    }
    (void)hipSetDevice(c->device);
    hipError_t e;
    // a failed flush may have left chains queued on stream2 (a complete one ends on `stream`)
    if (c->stream2 && (e = hipStreamSynchronize(c->stream2)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    if ((e = hipMemsetAsync(c->A.counters, 0, 256, c->stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    // make_trace_state's zeroed buffers (src/trace.jl:189-213). A context that traces every tile
    // overwrites every pixel in its first launch without reading it (a stream's first sample
    // starts from zero), so they are zeroed only if read before that launch (zero_if_stale); a
    // tile share keeps the other tiles' pixels at zero for the reduce, and a context whose device
    // buffers were handed out is read in place, so those zero them now.
    c->stale = true;
    c->aov_pending = false;
    c->pend0 = c->pend1 = 0;  // deferred samples are dropped with the state
    // a caller holding the device pointers (jt_get_device_buffers) sees the zeros at once
    if (c->P.tile_stride != 1 || c->exported) {
        const int st = zero_if_stale(c);
        if (st != JT_OK) return st;
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    c->first = -1;
    c->next = 0;
    c->failed = false;
    c->launches = 0;
    c->kernel_ms = 0;
    return JT_OK;
}

}  // extern "C"

namespace {
// the chunk size of a one-stream context: as many one-sample streams as two sets of stream-mean
// buffers hold, at most 64 (JT_MAX_STREAMS) and 2^27 (stream, slot) records in all (6.4 GB);
// allocated at the first multi-sample range, halved on NOMEM. 0 after jt_create (none yet), 1:
// none possible (the range then runs as one launch of long items).
int ensure_chunk(jt_ctx* c) {
    if (c->chunk) return JT_OK;
    const long long nslot = (long long)launch_tiles(c->P) * 64;
    int m = JT_MAX_STREAMS;
    while (m > 1 && 2 * nslot * m > JT_STREAM_ITEMS_MAX) m >>= 1;
    (void)hipSetDevice(c->device);
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) {
        c->stream2 = nullptr;
        m = 1;
    }
    for (int k = 0; k < 2 && m > 1; k++)
        if (hipEventCreateWithFlags(&c->trace_done[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->chain_done[k], hipEventDisableTiming) != hipSuccess)
            m = 1;
    for (; m > 1; m >>= 1) {
        void* part[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool ok = true;
        for (int k = 0; k < 6 && ok; k++) ok = hipMalloc(&part[k], (size_t)nslot * 16 * (size_t)m) == hipSuccess;
        if (ok) {
            for (int k = 0; k < 6; k++) {
                c->allocations.push_back(part[k]);
                c->cpart[k / 3][k % 3] = (float4*)part[k];
            }
            break;
        }
        (void)hipGetLastError();
        for (int k = 0; k < 6; k++)
            if (part[k]) (void)hipFree(part[k]);
    }
    c->chunk = m;
    return JT_OK;
}

// enqueue the trace launch of global samples [s0, s1) for local samples starting at `first`
// (stream t & (k-1) of local sample t = s - first, DParams::lk), then — with k > 1 — the combine
// of every pixel's stream means into the image and AOV buffers
int launch_range(jt_ctx* c, const DParams& P, const DAccum& A, int32_t s0, int32_t s1) {
    hipError_t e = hipMemsetAsync(c->A.work, 0, SCHED_BYTES, c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync schedule");
    if (c->sampler == JT_SAMPLER_NAIVE)
        e = c->count ? launch_s<2, 1>(c->stack, c->ring, c->kmask, c->wide, c->S, P, s0, s1, A, c->stream, c->cus)
                     : launch_s<2, 0>(c->stack, c->ring, c->kmask, c->wide, c->S, P, s0, s1, A, c->stream, c->cus);
    else
        e = c->count ? launch_s<1, 1>(c->stack, c->ring, c->kmask, c->wide, c->S, P, s0, s1, A, c->stream, c->cus)
                     : launch_s<1, 0>(c->stack, c->ring, c->kmask, c->wide, c->S, P, s0, s1, A, c->stream, c->cus);
    if (e != hipSuccess) return hip_fail(e, "trace kernel launch");
    return JT_OK;
}

// enqueue the launches of global samples [s0, s1) of a context whose local samples start at
// `first`. k > 1 streams: one trace launch + the combine. k = 1 (the reference's single running
// mean): one launch for one sample; a longer range in chunks (jt_ctx::chunk) of one-sample streams,
// each folded into the running mean by chain_kernel — the bits of one launch per sample, with
// m times the items per launch
int trace_launch(jt_ctx* c, int32_t s0, int32_t s1, int32_t first) {
    (void)hipSetDevice(c->device);
    hipError_t e;
    if ((e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    const int tiles = launch_tiles(c->P);
    const int nblk = (int)(((long long)tiles * 64 + 255) / 256);
    int launches = 0;
    if (c->lk == 0 && s1 - s0 > 1 && ensure_chunk(c) == JT_OK && c->chunk > 1) {
        // chunk i traces into buffer set i & 1 on `stream`; its chain runs on `stream2` after that
        // trace and after chain i - 1 (stream order), overlapping trace i + 1; trace i + 2 reuses
        // the set once chain i has read it. `stream` then waits for the last chain (ev1 covers it).
        int i = 0;
        for (int32_t x = s0; x < s1; x += c->chunk, i++) {
            const int32_t y = std::min(s1, x + c->chunk);
            const int set = i & 1;
            DParams P = c->P;  // the chunk's samples as one-sample streams x .. y-1
            P.first = x;
            P.lk = 0;
            while ((1 << P.lk) < y - x) P.lk++;
            DAccum A = c->A;
            A.part_img = c->cpart[set][0];
            A.part_alb = c->cpart[set][1];
            A.part_nrm = c->cpart[set][2];
            A.nslot = tiles * 64;
            if (i >= 2 && (e = hipStreamWaitEvent(c->stream, c->chain_done[set], 0)) != hipSuccess)
                return hip_fail(e, "hipStreamWaitEvent");
            if (const int st = launch_range(c, P, A, x, y)) return st;
            if ((e = hipEventRecord(c->trace_done[set], c->stream)) != hipSuccess ||
                (e = hipStreamWaitEvent(c->stream2, c->trace_done[set], 0)) != hipSuccess)
                return hip_fail(e, "hipEventRecord");
            if (nblk > 0) hipLaunchKernelGGL(chain_kernel, dim3(nblk), dim3(256), 0, c->stream2, c->P, A, x - first, y - x);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "chain kernel launch");
            if ((e = hipEventRecord(c->chain_done[set], c->stream2)) != hipSuccess) return hip_fail(e, "hipEventRecord");
            launches++;
        }
        if ((e = hipStreamWaitEvent(c->stream, c->chain_done[(i - 1) & 1], 0)) != hipSuccess)
            return hip_fail(e, "hipStreamWaitEvent");
    } else {
        c->P.first = first;
        if (const int st = launch_range(c, c->P, c->A, s0, s1)) return st;
        launches = 1;
        if (c->lk > 0) {
            // weights n_j / n of the streams after this launch: n local samples, stream j holds
            // those t < n with t mod k == j (include/jtrace.h jt_get_streams restates the rule)
            const long long n = (long long)s1 - first, k = 1LL << c->lk;
            DCombine cw{};
            cw.ns = (int)std::min(n, k);
            for (int j = 0; j < cw.ns; j++) cw.w[j] = (float)((double)((n - 1 - j) / k + 1) / (double)n);
            if (nblk > 0) hipLaunchKernelGGL(combine_kernel<false>, dim3(nblk), dim3(256), 0, c->stream, c->P, c->A, cw);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "combine kernel launch");
            c->aov_pending = nblk > 0;
            c->aov_cw = cw;
        }
    }
    if ((e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    c->launches += launches - 1;  // trace_finish counts one
    c->stale = false;  // every pixel of the launch's tiles was written (tile shares were zeroed at reset)
    return JT_OK;
}
// wait for the launch; its device time in *ms
int trace_finish(jt_ctx* c, float* ms) {
    (void)hipSetDevice(c->device);
    hipError_t e;
    if ((e = hipEventSynchronize(c->ev1)) != hipSuccess) return hip_fail(e, "trace kernel");
    *ms = 0;
    (void)hipEventElapsedTime(ms, c->ev0, c->ev1);
    c->kernel_ms += *ms;
    c->launches++;
    return JT_OK;
}

// multi-device trace_samples step. Sample split: [s0, s1) in contiguous shares, one per device,
// each appended to that device's own running mean (weight 1/(n_d + k + 1) for its k-th new
// sample). Tile split: every device traces all of [s0, s1) on its own tiles (the running-mean
// weights are the single-device ones: first = the context's first sample).
int multi_trace_range(jt_ctx* c, int32_t s0, int32_t s1) {
    const int D = (int)c->sub.size();
    const long long L = s1 - s0;
    std::vector<int> a(D), b(D);
    std::vector<char> launched(D, 0);
    int status = JT_OK;
    for (int d = 0; d < D && status == JT_OK; d++) {
        a[d] = c->tile_split ? s0 : s0 + (int)(L * d / D);
        b[d] = c->tile_split ? s1 : s0 + (int)(L * (d + 1) / D);
        if (a[d] < b[d]) {
            const int32_t first = c->tile_split ? c->first : (int32_t)(a[d] - c->nsub[d]);
            status = trace_launch(c->sub[d], a[d], b[d], first);
            launched[d] = status == JT_OK;
        }
    }
    // wait for every launch already queued, even after a failed one: they add to their devices'
    // running means, so the context is unusable (failed) unless all of them ran
    float wall = 0;
    for (int d = 0; d < D; d++) {
        if (!launched[d]) continue;
        float ms = 0;
        const int st = trace_finish(c->sub[d], &ms);
        if (st != JT_OK && status == JT_OK) status = st;
        c->nsub[d] += b[d] - a[d];
        wall = std::max(wall, ms);
    }
    if (status != JT_OK) {
        c->failed = true;
        return status;
    }
    c->kernel_ms += wall;  // the launches run concurrently: the slowest device's time
    c->launches++;
    c->next = s1;
    return JT_OK;
}

// the reduce of the devices' running means onto device 0, then to the host. Sample split: one
// RCCL reduce with a per-rank premultiplied sum, sum_d mean_d * n_d / N; tile split: the devices'
// pixels are disjoint (zero elsewhere), so a plain sum. which: 0 image, 1 albedo, 2 normal
// (float4 buffers); hits (int64) are summed.
int multi_reduce(jt_ctx* c, int which, float* out4, int64_t* hits) {
    const int D = (int)c->sub.size();
    const size_t np = (size_t)c->width * c->height;
    long long N = 0;
    for (long long n : c->nsub) N += n;
    // the premultiplied-sum ops created so far, destroyed on every exit path
    struct Ops {
        jt_ctx* c;
        std::vector<ncclRedOp_t> op;
        ~Ops() {
            for (size_t d = 0; d < op.size(); d++) (void)rccl().RedOpDestroy(op[d], c->comms[d]);
        }
    } ops{c, {}};
    std::vector<float> w(D);
    ncclResult_t r;
    if (out4 && !c->tile_split) {
        for (int d = 0; d < D; d++) {
            w[d] = N > 0 ? (float)((double)c->nsub[d] / (double)N) : (d == 0 ? 1.0f : 0.0f);
            ncclRedOp_t op;
            if ((r = rccl().RedOpCreatePreMulSum(&op, &w[d], ncclFloat32, ncclScalarHostImmediate, c->comms[d])) != ncclSuccess)
                return nccl_fail(r, "ncclRedOpCreatePreMulSum");
            ops.op.push_back(op);
        }
    }
    if ((r = rccl().GroupStart()) != ncclSuccess) return nccl_fail(r, "ncclGroupStart");
    for (int d = 0; d < D; d++) {
        jt_ctx* s = c->sub[d];
        (void)hipSetDevice(s->device);
        if (out4) {
            const float4* src = which == 0 ? s->A.image : which == 1 ? s->A.albedo : s->A.normal;
            r = rccl().Reduce(src, d == 0 ? (void*)c->red : (void*)src, np * 4, ncclFloat32,
                              c->tile_split ? ncclSum : ops.op[d], 0, c->comms[d], s->stream);
        } else {
            r = rccl().Reduce(s->A.hits, d == 0 ? (void*)c->red_hits : (void*)s->A.hits, np, ncclInt64, ncclSum, 0, c->comms[d],
                              s->stream);
        }
        if (r != ncclSuccess) {
            (void)rccl().GroupEnd();
            return nccl_fail(r, "ncclReduce");
        }
    }
    if ((r = rccl().GroupEnd()) != ncclSuccess) return nccl_fail(r, "ncclGroupEnd");
    hipError_t e;
    for (int d = 0; d < D; d++) {
        (void)hipSetDevice(c->sub[d]->device);
        if ((e = hipStreamSynchronize(c->sub[d]->stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    }
    (void)hipSetDevice(c->sub[0]->device);
    if (out4) e = hipMemcpy(out4, c->red, np * 16, hipMemcpyDeviceToHost);
    else e = hipMemcpy(hits, c->red_hits, np * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy reduce");
}

// trace the deferred samples [pend0, pend1) (jt_ctx) and wait for them; every call that reads
// the context's results or device buffers runs this first
int flush(jt_ctx* c) {
    if (c->pend1 <= c->pend0) return JT_OK;
    const int32_t s0 = c->pend0, s1 = c->pend1;
    c->pend0 = c->pend1 = 0;
    if (!c->sub.empty()) return multi_trace_range(c, s0, s1);
    int st = trace_launch(c, s0, s1, c->first);
    float ms = 0;
    if (st == JT_OK) st = trace_finish(c, &ms);
    if (st != JT_OK) c->failed = true;
    return st;
}
}  // namespace

extern "C" {

int jt_trace_range(jt_ctx* c, int32_t s0, int32_t s1) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (s0 < 0 || s1 < s0) return jt::fail(JT_ERR_STATE, "invalid sample range");
    if (s0 == s1) return JT_OK;
    if (c->failed) return jt::fail(JT_ERR_STATE, "a previous launch failed; jt_reset the context");
    if (c->first >= 0 && s0 != c->next)
        return jt::fail(JT_ERR_STATE, "samples must be accumulated in order (expected " + std::to_string(c->next) + ")");
    if (c->first < 0) c->first = s0;
    c->denoised = false;  // jt_get_denoised never returns the filter of fewer samples
    c->err_valid = false;
    // queue the range behind the deferred ones (jt_ctx::pend0); trace them all once enough are
    // queued, the render is complete (params.samples: the end of Jtrace.main's loop), or a caller
    // reads the accumulators in place (jt_get_device_buffers: it sees every range at once)
    if (c->pend1 <= c->pend0) c->pend0 = s0;
    c->pend1 = s1;
    c->next = s1;
    const bool in_place = c->exported || (!c->sub.empty() && c->sub[0]->exported);
    if (in_place || c->pend1 - c->pend0 >= JT_DEFER_SAMPLES || c->next >= c->total_samples) return flush(c);
    return JT_OK;
}

int jt_trace_samples(jt_ctx* c) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    const int n = c->first < 0 ? 0 : c->next;
    if (n >= c->total_samples) return JT_OK;  // state.samples >= params.samples
    const int target = std::min(n + c->batch, c->total_samples);
    return jt_trace_range(c, n, target);
}

int jt_get_streams(const jt_ctx* c, int32_t* streams) {
    if (!c || !streams) return jt::fail(JT_ERR_INVALID, "NULL argument");
    *streams = 1 << (c->sub.empty() ? c->lk : c->sub[0]->lk);
    return JT_OK;
}

int jt_get_samples(const jt_ctx* c, int32_t* samples) {
    if (!c || !samples) return jt::fail(JT_ERR_INVALID, "NULL argument");
    *samples = c->first < 0 ? 0 : c->next - c->first;
    return JT_OK;
}

int jt_get_size(const jt_ctx* c, int32_t* w, int32_t* h) {
    if (!c || !w || !h) return jt::fail(JT_ERR_INVALID, "NULL argument");
    *w = c->width;
    *h = c->height;
    return JT_OK;
}

int jt_get_image(jt_ctx* c, float* rgba) {
    if (!c || !rgba) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (const int st = flush(c)) return st;
    if (c->failed) return jt::fail(JT_ERR_STATE, "the running means are corrupt (a launch failed); jt_reset the context");
    if (!c->sub.empty()) {
        for (jt_ctx* s : c->sub)
            if (const int st = zero_if_stale(s)) return st;
        return multi_reduce(c, 0, rgba, nullptr);
    }
    if (const int st = zero_if_stale(c)) return st;
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemcpy(rgba, c->A.image, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy image");
}

int jt_get_aovs(jt_ctx* c, float* albedo, float* normal, int64_t* hits) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (const int st = flush(c)) return st;
    if (c->failed) return jt::fail(JT_ERR_STATE, "the running means are corrupt (a launch failed); jt_reset the context");
    for (jt_ctx* s : c->sub)
        if (const int st = zero_if_stale(s)) return st;
    for (jt_ctx* s : c->sub)
        if (const int st = finish_aovs(s)) return st;
    if (c->sub.empty()) {
        if (const int st = zero_if_stale(c)) return st;
        if (const int st = finish_aovs(c)) return st;
    }
    (void)hipSetDevice(c->device);
    const size_t np = (size_t)c->width * c->height;
    std::vector<float4> tmp(np);
    hipError_t e;
    const bool multi = !c->sub.empty();
    int st;
    if (albedo) {
        if (multi) {
            if ((st = multi_reduce(c, 1, reinterpret_cast<float*>(tmp.data()), nullptr)) != JT_OK) return st;
        } else if ((e = hipMemcpy(tmp.data(), c->A.albedo, np * 16, hipMemcpyDeviceToHost)) != hipSuccess) {
            return hip_fail(e, "hipMemcpy");
        }
        for (size_t k = 0; k < np; k++) {
            albedo[3 * k] = tmp[k].x;
            albedo[3 * k + 1] = tmp[k].y;
            albedo[3 * k + 2] = tmp[k].z;
        }
    }
    if (normal) {
        if (multi) {
            if ((st = multi_reduce(c, 2, reinterpret_cast<float*>(tmp.data()), nullptr)) != JT_OK) return st;
        } else if ((e = hipMemcpy(tmp.data(), c->A.normal, np * 16, hipMemcpyDeviceToHost)) != hipSuccess) {
            return hip_fail(e, "hipMemcpy");
        }
        for (size_t k = 0; k < np; k++) {
            normal[3 * k] = tmp[k].x;
            normal[3 * k + 1] = tmp[k].y;
            normal[3 * k + 2] = tmp[k].z;
        }
    }
    if (hits) {
        if (multi) {
            if ((st = multi_reduce(c, 0, nullptr, hits)) != JT_OK) return st;
        } else if ((e = hipMemcpy(hits, c->A.hits, np * 8, hipMemcpyDeviceToHost)) != hipSuccess) {
            return hip_fail(e, "hipMemcpy");
        }
    }
    return JT_OK;
}

int jt_denoise(jt_ctx* c, const jt_denoise_params* params) {
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
    const size_t np = (size_t)c->width * c->height;
    if (!c->sub.empty()) {
        // the devices' means reduced as jt_get_image / jt_get_aovs do, filtered on device 0
        std::vector<float> img(np * 4), alb(np * 3), nrm(np * 3);
        int st;
        if ((st = jt_get_image(c, img.data())) || (st = jt_get_aovs(c, alb.data(), nrm.data(), nullptr))) return st;
        c->dn_host.resize(np * 4);
        if ((st = jt_denoise_image(img.data(), alb.data(), nrm.data(), c->width, c->height, &p, c->sub[0]->device,
                                   c->dn_host.data())))
            return st;
        c->denoised = true;
        return JT_OK;
    }
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

int jt_get_denoised(jt_ctx* c, float* rgba) {
    if (!c || !rgba) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (!c->denoised) return jt::fail(JT_ERR_STATE, "no jt_denoise since the last sample was traced or jt_reset");
    const size_t np = (size_t)c->width * c->height;
    if (!c->sub.empty()) {
        std::memcpy(rgba, c->dn_host.data(), np * 16);
        return JT_OK;
    }
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemcpy(rgba, c->dn[2], np * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy denoised");
}

namespace {
// The error estimate of the current samples (include/jtrace.h jt_get_variance): checks, the flush,
// then one launch of error_kernel over the stream means the last combine read, unless the
// result of these samples is already there. Neither counted in jt_counters nor touching an
// accumulator or a stream mean.
int estimate_error(jt_ctx* c) {
    if (!c->sub.empty())
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
    const int tiles = launch_tiles(c->P), nblk = jt::error_blocks(tiles);
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
    E.ns = c->aov_cw.ns;  // min(n, k) >= 2, with the weights the image was combined with
    std::memcpy(E.w, c->aov_cw.w, sizeof E.w);
    std::vector<float2> sums((size_t)nblk);
    if ((e = jt::error_launch(c->stream, E)) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess ||
        (nblk > 0 && (e = hipMemcpy(sums.data(), c->err_sums, sums.size() * sizeof(float2), hipMemcpyDeviceToHost)) != hipSuccess))
        return hip_fail(e, "error estimate");
    double V = 0, M = 0;
    for (const float2& s : sums) V += (double)s.x, M += (double)s.y;
    // N: the traced pixels inside the image (edge tiles are clipped)
    const int tiles_x = (c->width + 7) / 8;
    long long N = 0;
    for (int u = 0; u < tiles; u++) {
        const int t = u * c->P.tile_stride + c->P.tile_offset;
        const int x0 = (t % tiles_x) * 8, y0 = (t / tiles_x) * 8;
        N += (long long)std::min(8, c->width - x0) * std::min(8, c->height - y0);
    }
    c->err_noise = M == 0 ? 0.0 : std::sqrt(3.0 * (double)N * V) / M;
    c->err_valid = true;
    return JT_OK;
}
}  // namespace

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

int jt_get_counters(jt_ctx* c, jt_counters* out) {
    if (!c || !out) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (const int st = flush(c)) return st;
    if (!c->sub.empty()) {  // summed over the devices; kernel_ms: per launch the slowest device
        jt_counters sum{};
        for (jt_ctx* s : c->sub) {
            jt_counters k{};
            const int st = jt_get_counters(s, &k);
            if (st != JT_OK) return st;
            sum.paths += k.paths;
            sum.rays += k.rays;
            sum.light_queries += k.light_queries;
            sum.nodes += k.nodes;
            sum.instances += k.instances;
            sum.prims += k.prims;
            sum.shades += k.shades;
        }
        sum.launches = c->launches;
        sum.kernel_ms = c->kernel_ms;
        *out = sum;
        return JT_OK;
    }
    (void)hipSetDevice(c->device);
    unsigned long long v[8] = {0};
    hipError_t e = hipMemcpy(v, c->A.counters, 7 * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy counters");
    out->paths = v[0];
    out->rays = v[1];
    out->light_queries = v[2];
    out->nodes = v[3];
    out->instances = v[4];
    out->prims = v[5];
    out->shades = v[6];
    out->launches = c->launches;
    out->kernel_ms = c->kernel_ms;
    return JT_OK;
}

int jt_get_device_buffers(jt_ctx* c, jt_device_buffers* out) {
    if (!c || !out) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (const int st = flush(c)) return st;
    if (!c->sub.empty()) return jt_get_device_buffers(c->sub[0], out);  // device 0's share
    if (const int st = zero_if_stale(c)) return st;
    if (const int st = finish_aovs(c)) return st;
    c->exported = true;  // jt_reset now zeroes the buffers at once (the caller may read them)
    out->image = c->A.image;
    out->albedo = c->A.albedo;
    out->normal = c->A.normal;
    out->hits = c->A.hits;
    out->width = c->width;
    out->height = c->height;
    out->stream = c->stream;
    return JT_OK;
}

// diagnostic build only (JT_STAMPS=1): per-phase wave clocks and shading-phase material coherence
// (24 u64), read by scripts/stamps.py
extern "C" int jt_debug_stamps(jt_ctx* c, unsigned long long* out8) {
    if (!c || !out8) return jt::fail(JT_ERR_INVALID, "NULL argument");
    hipError_t e = hipMemcpy(out8, c->A.counters + 8, 24 * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy stamps");
}

int jt_describe(const jt_ctx* c, char* buf, int32_t n) {
    if (!c || !buf || n <= 0) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (!c->sub.empty()) {
        char tmp[640];
        const int st = jt_describe(c->sub[0], tmp, sizeof tmp);
        if (st != JT_OK) return st;
        std::snprintf(buf, (size_t)n, "%s devices=%d split=%s", tmp, (int)c->sub.size(), c->tile_split ? "tiles" : "samples");
        return JT_OK;
    }
    const bool ovf = c->stack > 16;
    const int ring = ovf ? c->ring : 16;
    // test-only options in effect (jt_set_option): a tile filter, a shortened LDS ring
    char filt[96] = "";
    if (c->P.tile_stride != 1 || c->S.ring != c->ring)
        std::snprintf(filt, sizeof filt, " tile_filter=%d/%d ring_used=%d", c->P.tile_offset, c->P.tile_stride, c->S.ring);
    char tmp[640];
    std::snprintf(tmp, sizeof tmp,
                  "kernel=%s<%d,%d,%s,%d,%d,%s> mode=%s scene_lds_bytes=%zu stack_bound=%d lds_ring=%d hbm_overflow=%d "
                  "wait_lanes=%d light_lanes=%d streams=%d tiles=%d block=%d env_alias=%d light_inline=%d "
                  "traversal=%s%s",
                  c->lds_scene_bytes ? "trace_kernel_lds" : "trace_kernel", c->sampler == JT_SAMPLER_NAIVE ? 2 : 1,
                  ring, ovf ? "true" : "false", c->count, c->kmask, c->wide ? "true" : "false",
                  c->lds_scene_bytes ? "lds" : "hbm", c->lds_scene_bytes,
                  c->stack, ring, ovf ? 1 : 0, c->P.wait_lanes, c->P.light_lanes, 1 << c->lk, c->tiles, BLOCK,
                  c->env_alias ? 1 : 0, c->S.light_inline,
                  c->traversal == JT_TRAVERSAL_REFERENCE ? "reference" : c->traversal == JT_TRAVERSAL_NEAR ? "near" : "wide",
                  filt);
    std::snprintf(buf, (size_t)n, "%s", tmp);
    return JT_OK;
}

int jt_set_counters(jt_ctx* c, int32_t level) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (level != 0 && level != 1) return jt::fail(JT_ERR_INVALID, "counter level must be 0 or 1");
    if (const int st = flush(c)) return st;  // queued samples are traced at the level they were queued at
    for (jt_ctx* s : c->sub) s->count = level;
    c->count = level;
    return JT_OK;
}

int jt_synchronize(jt_ctx* c) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (const int st = flush(c)) return st;
    for (jt_ctx* s : c->sub) {
        const int st = jt_synchronize(s);
        if (st != JT_OK) return st;
    }
    if (!c->sub.empty()) return JT_OK;
    if (const int st = finish_aovs(c)) return st;
    (void)hipSetDevice(c->device);
    hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipStreamSynchronize");
}

}  // extern "C"
