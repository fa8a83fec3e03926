// jt_context.h — the device context behind include/jtrace.h's jt_ctx and the few functions its
// pieces share: jt_trace.hip (creation, the sample queue, the getters), jt_multi.hip (the
// multi-device context), jt_denoise.hip, jt_error.hip, jt_adapt.hip, jt_intersect.hip,
// jt_surface.hip and jt_radiance.hip (their context halves). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>
#include <vector>

#include "jt_internal.h"
#include "jt_launch.h"

namespace jtc {
struct MultiCtx;  // jt_multi.hip
}

struct jt_ctx {
    // ---- launch state: the device, the scene and what selects and feeds the trace kernel
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    jtd::DScene S{};
    jtd::DParams P{};
    jtk::DAccum A{};
    std::vector<void*> allocations;
    int width = 0, height = 0;
    int total_samples = 0, batch = 1, sampler = 1;
    int cus = 256;   // compute units of the device (persistent grid size)
    int lk = 0;      // log2 of the sample streams per pixel (DParams::lk; fixed at jt_create)
    int tiles = 0;   // 8x8 pixel tiles
    // the kernel configuration the scene runs, its memory mode, stack and gates (select_kernel,
    // jt_select.h), fixed at jt_create
    jtk::KernelChoice choice{};
    bool env_alias = false;    // JT_ENV_ALIAS=1: environment lights sample through alias tables
                               // until jt_reset
    int count = 1;             // 1: all traversal counters (diagnostic), 0: paths/rays/light queries only
    bool exported = false;  // jt_get_device_buffers handed out the accumulators' device pointers
    bool failed = false;       // a launch failed: the running means are unusable
    bool stale = true;         // the accumulators are not yet zeroed or overwritten since jt_reset
    // k > 1: the last launch combined the image only; albedo, normal and hits are combined from
    // the stream means (weights last_cw) when first read (finish_aovs)
    bool aov_pending = false;
    jtk::DCombine last_cw{};  // the weights of the last combine (finish_aovs, the error estimate)
    unsigned long long launches = 0;
    double kernel_ms = 0;

    // ---- deferred queue
    int first = -1, next = 0;  // running-mean origin and next expected sample (deferred ones included)
    // Deferred samples [pend0, pend1): jt_trace_range / jt_trace_samples queue their range and
    // trace it, merged with the ranges queued before it, once JT_DEFER_SAMPLES are queued or when
    // anything reads the context (flush). A render split into calls gives the bits of one call
    // (jt_trace_range's contract), so merging changes only the launch count: the reference's
    // default --batch 1 (one call per sample) runs as launches of many samples each.
    int pend0 = 0, pend1 = 0;

    // ---- one-stream chunks
    // one-stream contexts (lk == 0): a flushed range of m > 1 samples runs as chunks of up to
    // `chunk` samples, each traced as one-sample streams into the stream-mean buffers (allocated at
    // the first such flush) and folded into the running mean by chain_kernel in sample order
    int chunk = 0;
    int trace_chunk = 0;  // option test_trace_chunk (tests only; 0: unset): a cap on `chunk`
    // two sets of chunk buffers: chunk i traces into set i & 1 on `stream` while chain_kernel folds
    // chunk i - 1 on `stream2` (the chains stay in sample order on stream2; a trace reuses a set
    // only after the chain that read it, chain_done)
    float4* cpart[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    hipStream_t stream2 = nullptr;
    hipEvent_t trace_done[2] = {nullptr, nullptr}, chain_done[2] = {nullptr, nullptr};

    // ---- denoise
    // the denoiser (jt_denoise, jt_denoise_guided; jt_denoise.hip): two scratch buffers and the
    // result, float4[W*H] each, allocated by the first call of either and kept across jt_reset;
    // the result is that of the last to run. A multi-device context (jt_denoise only) filters the
    // reduced host arrays on device 0 and keeps the result on the host instead
    float4* dn[3] = {nullptr, nullptr, nullptr};
    bool denoised = false;  // the result is the filter of the current running means

    // ---- error
    // the error estimate (jt_get_variance, jt_get_noise; jt_error.hip): the per-pixel variance of
    // the mean, float4[W*H], and one (V, M) pair per workgroup; allocated (the variance zeroed) by
    // the first call and kept across jt_reset. err_noise is the scalar of the current samples
    float4* err_var = nullptr;
    float2* err_sums = nullptr;
    double err_noise = 0;
    double err_M = 0;        // the sum of (mu.x + mu.y) + mu.z over the traced pixels behind err_noise
    bool err_valid = false;  // err_var, err_noise and err_M are those of the current running means

    // ---- adaptive sampling
    // jt_adapt, jt_get_sample_counts (jt_adapt.hip): per image tile the local sample count at
    // which it froze (0: active; DAccum::frozen points here) and one word per workgroup of the
    // adapt launch; allocated (the mask zeroed) by the first jt_adapt, kept across jt_reset, which
    // zeroes the mask again
    unsigned* frozen_at = nullptr;
    unsigned* adapt_words = nullptr;
    int adapt_active = 0;   // traced tiles still active after the last jt_adapt (all after jt_reset)
    bool adapted = false;   // jt_adapt has run on this context (jt_describe)

    // ---- ray queries
    // jt_intersect, jt_occluded (jt_intersect.hip). inst_new: the caller's instance id -> the device's
    // (layout_scene's permutation, kept by jt_create). Uploaded by the first query, in
    // `allocations`: that permutation and its inverse, and the launch's ray counter. q_grow: the
    // buffers that grow with the calls — the query grid's own stack overflow area (q_ovf_entries
    // ints) and the host variants' staging of rays, instance ids and results (q_stage_rays
    // rays) — kept across jt_reset, freed by jt_destroy (query_free). The surface calls
    // (jt_eval_hits, jt_camera_rays, jt_gbuffer; jt_surface.hip) stage rays and hits in the same
    // buffers and their jt_surface records in Q_SURF (q_stage_surf records); jt_radiance
    // (jt_radiance.hip) launches on the same counter and overflow area and stages its rays in
    // Q_RAYS and its means in Q_OUT; the bounded queries (jt_intersect_bounded, jt_occluded_bounded)
    // stage their per-ray bounds in Q_TMAX, grown with the rays; jt_probe_sh's host variant stages a
    // chunk's 144-byte records in Q_SH (q_stage_sh records; at most probe_chunk points a chunk,
    // jtr::PROBE_MAX_CHUNK unless the option test_probe_chunk lowers it); jt_intersect_multi's host
    // variant (jt_multihit.hip) stages a chunk's n x k jt_hit records in Q_MULTI (q_stage_multi
    // records; the rays of a chunk: jtm::multi_chunk of k and the option test_multi_chunk) and,
    // like jt_count_hits, its counts in Q_OUT
    std::vector<int> inst_new;
    int* q_to_dev = nullptr;
    int* q_to_ref = nullptr;
    unsigned* q_counter = nullptr;
    enum { Q_OVF = 0, Q_RAYS, Q_INST, Q_OUT, Q_SURF, Q_TMAX, Q_SH, Q_MULTI, Q_NGROW };
    void* q_grow[Q_NGROW] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t q_ovf_entries = 0;
    long long q_stage_rays = 0;
    long long q_stage_surf = 0;
    long long q_stage_sh = 0;
    long long q_stage_multi = 0;
    long long probe_chunk = (long long)1 << 22;
    long long multi_chunk = 0;  // option test_multi_chunk (tests only; 0: unset)
    // inst_nelem: the elements of each instance's shape, in the caller's numbering (jt_create);
    // uploaded by the first surface call (s_nelem, in `allocations`): surface_kernel's range check
    std::vector<int> inst_nelem;
    int* s_nelem = nullptr;

    // ---- a multi-device context (jt_create_multi) owns its sub-contexts and reduce state here
    // and uses, of the fields above, only the size, the sample counts, the queue, `failed`,
    // `denoised`, the counters' totals, and device 0's `lk` and `exported`
    jtc::MultiCtx* multi = nullptr;
};

namespace jtc {

int hip_fail(hipError_t e, const char* what);
// hipMalloc owned by the context (freed by jt_destroy); JT_ERR_NOMEM "hipMalloc <what>"
int device_alloc(jt_ctx* c, size_t bytes, const char* what, void** p);
// zeroes the accumulators if nothing has since jt_reset (jt_ctx::stale)
int zero_if_stale(jt_ctx* c);
// the deferred AOV combine of the last launch (jt_ctx::aov_pending), before albedo, normal or
// hits are read: jt_get_aovs, jt_synchronize, jt_get_device_buffers
int finish_aovs(jt_ctx* c);
// enqueue the launches of global samples [s0, s1) of a context whose local samples start at `first`
int trace_launch(jt_ctx* c, int32_t s0, int32_t s1, int32_t first);
// wait for the launch; its device time in *ms
int trace_finish(jt_ctx* c, float* ms);
// trace the deferred samples [pend0, pend1) (jt_ctx) and wait for them; every call that reads
// the context's results or device buffers runs this first
int flush(jt_ctx* c);
// frees the ray queries' growing buffers (jt_ctx::q_grow; jt_intersect.hip), for jt_destroy
void query_free(jt_ctx* c);
// the ray queries' pieces the surface calls and jt_radiance share (jt_intersect.hip). query_setup: the first call's
// uploads (q_to_dev, q_to_ref, q_counter). query_grow: buffer `which` of q_grow replaced by one of
// at least `bytes` (its content is not kept); JT_ERR_NOMEM "hipMalloc <what>". query_stage: the
// staging of rays, instance ids and jt_hit records grown to hold n rays
int query_setup(jt_ctx* c);
int query_grow(jt_ctx* c, int which, size_t bytes, const char* what);
int query_stage(jt_ctx* c, int64_t n);
// the scene a persistent query grid of `grid` workgroups traverses (query_kernel, and jt_radiance.hip's
// radiance_kernel): the context's HBM scene with the ring entries in use and, when the scene's stack
// bound exceeds them (*ovf), an overflow area of the grid's own in q_grow[Q_OVF], grown to fit
int query_scene(jt_ctx* c, int grid, jtd::DScene* S, bool* ovf);

// ---- what the calls on the caller's own records share (jt_intersect, jt_occluded; jt_eval_hits,
// jt_camera_rays, jt_gbuffer; jt_radiance; defined in jt_intersect.hip)
// The argument checks, in the order include/jtrace.h documents: ctx NULL, each of `args` NULL
// ("<name> is NULL"), range_error and misaligned (the message of an argument out of range, of a
// device variant's misaligned pointer; nullptr: none), `empty` (n == 0: *done = true, JT_OK), a
// multi-device context (JT_ERR_UNSUPPORTED multi_error), a previous launch failed. A call without n
// passes neither empty nor done.
struct NamedArg {
    const void* p;
    const char* name;
};
int ray_call_check(const jt_ctx* c, std::initializer_list<NamedArg> args, const char* range_error, const char* misaligned,
                   const char* multi_error, bool empty = false, bool* done = nullptr);
// after a kernel launch on the context's stream: the launch's error ("<what> launch"), then the
// stream's once it is idle ("<what>"), which marks the context failed
int launch_finish(jt_ctx* c, const char* what);
// a blocking hipMemcpy to and from the device; `what` names it in the error
int copy_in(void* dst, const void* src, size_t bytes, const char* what);
int copy_out(void* dst, const void* src, size_t bytes, const char* what);
// f(A, B, C) with a, b, c as std::true_type / std::false_type: three runtime booleans to template
// arguments (kernel<A(), B(), C()>)
template <class F>
void with_bools(bool a, bool b, bool c, F&& f) {
    const auto pick = [](bool v, auto&& g) { !v ? g(std::false_type{}) : g(std::true_type{}); };
    pick(a, [&](auto A) { pick(b, [&](auto B) { pick(c, [&](auto C) { f(A, B, C); }); }); });
}

// xyz of np float4 to np x 3 floats (the AOV getters)
inline void unpack3(const std::vector<float4>& src, float* dst) {
    for (size_t k = 0; k < src.size(); k++) {
        dst[3 * k] = src[k].x;
        dst[3 * k + 1] = src[k].y;
        dst[3 * k + 2] = src[k].z;
    }
}

// the multi-device branch of the ABI functions (jt_multi.hip), each called as
// `if (c->multi) return multi_...`, after the checks both kinds of context share
void multi_destroy(jt_ctx* c);
int multi_reset(jt_ctx* c);
int multi_trace_range(jt_ctx* c, int32_t s0, int32_t s1);
int multi_get_image(jt_ctx* c, float* rgba);
int multi_get_aovs(jt_ctx* c, float* albedo, float* normal, int64_t* hits);
int multi_denoise(jt_ctx* c, const jt_denoise_params& p);
int multi_get_denoised(jt_ctx* c, float* rgba);
int multi_get_counters(jt_ctx* c, jt_counters* out);
int multi_get_device_buffers(jt_ctx* c, jt_device_buffers* out);
int multi_describe(const jt_ctx* c, char* buf, int32_t n);
int multi_set_counters(jt_ctx* c, int32_t level);
int multi_synchronize(jt_ctx* c);

}  // namespace jtc
