// jt_radiance.hip — the path integrator on the caller's own rays (include/jtrace.h: jt_radiance and
// its device-pointer variant; DESIGN.md §6g "Radiance along the caller's rays") and at the caller's
// own points, every sample along a cosine-weighted direction of its own (jt_irradiance,
// jt_hemisphere_rays and their device-pointer variants), or along a uniform direction
// over the whole sphere with every sample projected onto nine spherical harmonics (jt_probe_sh,
// jt_sphere_rays and their device-pointer variants; jt_sh.h): the megakernel's
// integrator (jt_integrator.h: Path, path_hit, naive_hit, light_hit) driven by the ray queries'
// persistent, refilling grid instead of the megakernel's pixel hand-out: query_kernel's refill itself
// (feed_refill, jt_feed.h), its grid, claim size, ray counter and scene (jt_intersect.h; query_setup,
// query_scene, jt_context.h), and the argument checks, launch tail and staging copies every call on
// the caller's records shares (ray_call_check, launch_finish, copy_in, copy_out; jt_intersect.hip).
//
// The scene is the context's HBM copy (NCACHE) with the general feature mask, no counters, the
// 16-entry LDS stack ring and, for a scene whose bound exceeds it, the query grid's own HBM overflow
// area: query_kernel's configuration. A lane takes a ray and keeps it for all its samples: the mean
// is defined in sample order, so a lane that owns its ray needs no atomics and no second pass. Its
// running mean, its sample index and the parked path state (Path::pk) live in the lane's LDS slots
// (jt_radiance.h), the stack ring beside them. Where a sample's ray comes from is the kernel's
// compile-time SOURCE (radiance_ray, jt_sample_ray.h): the record as it stands, or the hemisphere draw about the
// record's normal; nothing else differs, and hemisphere_kernel writes that same ray out. The third
// source, the sphere draw at the record's position (sphere_kernel writes it out), also changes where
// the mean lives: a probe's 36 running sums are its own output record, not LDS slots.
//
// Each iteration of a wave runs one step kind, chosen by a lane vote (radiance_step):
//   a primitive step   prim_step
//   a node step        node_step_any, RADIANCE_NODE_REPEAT pops for a lane whose next step is a pop again
//   a shading step     for the lanes whose query is done: rerun_tie (a light query's instance passed
//                      to it, as the megakernel's shading phase does), then light_hit when the path
//                      waits on a light query, else path_hit or naive_hit, then query_start of the
//                      next scene query or of the next light-instance query. A finished path runs
//                      trace_sample's epilogue into the lane's mean and starts the ray's next
//                      sample, or writes rgba[ray] and frees the lane.
// Light queries go through the traversal loop: the megakernel's path without inline light chains,
// which gives the bits of the inline chain. Every value a path computes depends on its ray, its
// stream and its sample only, never on the lane that runs it or on when.
//
// Termination: every traversal step pops an entry of a finite tree or tests primitives of a leaf's
// finite cursor; a tie's re-run happens once per query (REF_RERUN); a path has at most
// params.bounces bounces, each with at most 129 opacity retries and, per light, a chain of fewer
// than 100 hits over a finite light list; the sample count of a ray is finite and so is the number
// of rays. Every iteration advances some lane that has a ray (radiance_step), so every lane frees in
// a bounded number of steps for any input, non-finite rays included; for those the result is
// unspecified.
#include <hip/hip_runtime.h>

#include "jt_context.h"
#include "jt_feed.h"
#include "jt_integrator.h"
#include "jt_radiance.h"
#include "jt_sample_ray.h"
#include "jt_sh.h"

namespace jtk {

using jtq::QUERY_RING;

struct DRadiance {
    const float* rays;      // n x (o, d); SOURCE_HEMISPHERE: n x (position, normal); SOURCE_SPHERE: n x position
    float4* rgba;           // n means; SOURCE_SPHERE: n probes of nine float4 (jt_sh.h)
    long long stream_base;  // ray i draws from stream stream_base + i
    int s_begin, s_end;     // the samples of every ray, in order
    DFeed feed;             // the n rays' hand-out
};

// trace_sample's prologue (start_path) for ray `ray`: the sample's ray (radiance_ray) and the path state
template <int F, int SOURCE>
__device__ __forceinline__ void radiance_start(const DParams& P, const DRadiance& Q, int ray, int sample, Path& st) {
    radiance_ray<SOURCE>(P, Q.rays, Q.stream_base, ray, sample, st.rng, st.o, st.d);
    st.set_radiance<F>(V3(0, 0, 0));
    st.set_weight<F>(V3(1, 1, 1));
    st.set_max_roughness<F>(0.0f);
    st.ctl = 0u;
    st.phase = PH_SCENE;
}

// the instance of the path's pending query: a light's (sample_lights_pdf), or -1 for the scene
__device__ __forceinline__ int radiance_query_instance(const DScene& S, const Path& st) {
    return st.phase == PH_LIGHT ? S.lights[st.li].instance : -1;
}

#if JT_RADIANCE_WAVES > 0
#define JT_RADIANCE_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(JT_RADIANCE_WAVES, JT_RADIANCE_WAVES)))
#else
#define JT_RADIANCE_WAVES_ATTR
#endif

template <bool WIDE, bool OVF, int SAMPLER, int SOURCE>
__global__ __launch_bounds__(BLOCK) JT_RADIANCE_WAVES_ATTR void radiance_kernel(DScene S, DParams P, DRadiance Q) {
    constexpr int F = FT_ALL;
    __shared__ int ring[QUERY_RING * BLOCK];
    __shared__ float lane_lds[jtr::RADIANCE_SLOTS * BLOCK];
    stage_tex_lut(S);
    int* const stack = ring + threadIdx.x;
    float* const acc = lane_lds + jtr::RADIANCE_ACC * BLOCK + threadIdx.x;
    int* const cur = reinterpret_cast<int*>(lane_lds + jtr::RADIANCE_SAMPLE * BLOCK + threadIdx.x);
    const int slot = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // the lane's HBM stack-overflow area
    Counters cnt{0, 0, 0, 0};
    const NoAov aov{};
    Path st;
    st.pk = lane_lds + jtr::RADIANCE_PARK * BLOCK + threadIdx.x;
    st.phase = PH_SCENE;
    st.li = 0;
    Trav T;
    T.sp = 0;
    T.nprim = 0;
    T.nxt = W_EMPTY;
    T.nh = 0;
    int ray = -1;  // the lane's ray; -1: none
    jtq::WaveReserve reserve;
    // ---- refill (jt_feed.h): a lane without a ray takes one of the wave's reserve and starts its first sample
    while (feed_refill(Q.feed, reserve, ray >= 0, [&](int r) {
        ray = r;
        if constexpr (SOURCE != jtr::SOURCE_SPHERE) {  // a probe's sums live in its output record
            acc[0] = 0.0f;
            acc[BLOCK] = 0.0f;
            acc[2 * BLOCK] = 0.0f;
            acc[3 * BLOCK] = 0.0f;
        }
        *cur = Q.s_begin;
        radiance_start<F, SOURCE>(P, Q, ray, Q.s_begin, st);
        query_start<WIDE>(S, T, st.o, st.d, -1, stack);
    })) {
        // ---- one step kind for the wave (radiance_step); a lane's own sequence of steps is
        // unchanged, it only waits while another kind runs
        const bool wantp = ray >= 0 && T.nprim > 0, wantn = ray >= 0 && wants_node<WIDE>(T);
        const bool wants = ray >= 0 && query_done<WIDE>(T);
        const int np = __popcll(__builtin_amdgcn_ballot_w64(wantp)), nn = __popcll(__builtin_amdgcn_ballot_w64(wantn));
        const int ns = __popcll(__builtin_amdgcn_ballot_w64(wants));
        const int kind = jtr::radiance_step(np, nn, ns);
        if (kind == jtr::STEP_PRIM) {
            if (wantp) prim_step<0, F>(S, T, cnt);
        } else if (kind == jtr::STEP_NODE) {
            // RADIANCE_NODE_REPEAT pops per node iteration: a lane whose next step is again a
            // stack pop takes it at once (the megakernel's JT_NODE_REPEAT: the same steps in the same
            // per-lane order, fewer votes)
#pragma unroll
            for (int k = 0; k < jtr::RADIANCE_NODE_REPEAT; k++)
                if (ray >= 0 && wants_node<WIDE>(T)) node_step_any<WIDE, QUERY_RING, OVF, 0, true, F>(S, T, stack, slot, cnt);
        } else if (wants && !rerun_tie<WIDE>(S, T, st.o, st.d, radiance_query_instance(S, st), stack)) {
            // ---- shading step: the lane consumes its hit and issues its next query
            bool done;
            if (SAMPLER == 1 && st.phase == PH_LIGHT) done = light_hit<F>(S, P, st, query_hit(T));
            else if (SAMPLER == 2) done = naive_hit<F>(S, P, st, query_hit(T), aov, cnt.shades);
            else done = path_hit<F>(S, P, st, query_hit(T), aov, cnt.shades);
            if (done) {
                // trace_sample's epilogue (src/trace.jl:625-648), into the ray's running mean
                v3 radiance = st.radiance<F>();
                if (!all_finite(radiance)) radiance = V3(0, 0, 0);
                const float mr = max3(radiance);
                if (mr > P.clamp) radiance = radiance * (P.clamp / mr);
                const int sample = *cur;
                const float w = jl_rcp_weight((float)(sample - Q.s_begin + 1));
                const float omw = 1 - w;
                const bool hit = st.flag(F_HIT);
                const bool env = !hit && !P.envhidden && S.nenvs != 0;
                const v4 target = (hit || env) ? V4(radiance.x, radiance.y, radiance.z, 1) : V4(0, 0, 0, 0);
                if constexpr (SOURCE == jtr::SOURCE_SPHERE) {
                    // The projection (jt_sh.h): the 36 running sums are the lane's own output record,
                    // nine float4 at rgba + 9 ray, which no other lane touches; a read-modify-write
                    // with plain vector loads and stores. The first sample folds from zero without
                    // reading the record (and turns a product of -0 into +0). The sample's initial
                    // direction is drawn again by the arm that started it: the same function, the
                    // same bits, and nothing parked across the path.
                    Rng rng0;
                    v3 o0, d0;
                    radiance_ray<SOURCE>(P, Q.rays, Q.stream_base, ray, sample, rng0, o0, d0);
                    const jtsh::Basis Y = jtsh::sh_basis(d0.x, d0.y, d0.z);
                    float4* const rec = Q.rgba + (size_t)ray * jtsh::SH_COEFFS;
                    const bool first = sample == Q.s_begin;
#if JT_PROBE_LDS
                    // A/B build (EXPERIMENTS.md): the sums in 36 more LDS slots per lane, 36 KiB per
                    // workgroup (two workgroups per CU instead of three), the record written once
                    __shared__ float sums[jtsh::SH_RECORD * BLOCK];
                    float* const mine = sums + threadIdx.x;
                    const bool last = sample + 1 >= Q.s_end;
#pragma unroll
                    for (int k = 0; k < jtsh::SH_COEFFS; k++) {
                        float* const m = mine + 4 * k * BLOCK;
                        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (!first) a = make_float4(m[0], m[BLOCK], m[2 * BLOCK], m[3 * BLOCK]);
                        a.x = jtsh::sh_fold(a.x, target.x, Y.y[k], w, omw);
                        a.y = jtsh::sh_fold(a.y, target.y, Y.y[k], w, omw);
                        a.z = jtsh::sh_fold(a.z, target.z, Y.y[k], w, omw);
                        a.w = jtsh::sh_fold(a.w, target.w, Y.y[k], w, omw);
                        m[0] = a.x;
                        m[BLOCK] = a.y;
                        m[2 * BLOCK] = a.z;
                        m[3 * BLOCK] = a.w;
                        if (last) rec[k] = a;
                    }
#else
#pragma unroll
                    for (int k = 0; k < jtsh::SH_COEFFS; k++) {
                        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (!first) a = rec[k];
                        a.x = jtsh::sh_fold(a.x, target.x, Y.y[k], w, omw);
                        a.y = jtsh::sh_fold(a.y, target.y, Y.y[k], w, omw);
                        a.z = jtsh::sh_fold(a.z, target.z, Y.y[k], w, omw);
                        a.w = jtsh::sh_fold(a.w, target.w, Y.y[k], w, omw);
                        rec[k] = a;
                    }
#endif
                } else {
                    acc[0] = acc[0] * omw + target.x * w;
                    acc[BLOCK] = acc[BLOCK] * omw + target.y * w;
                    acc[2 * BLOCK] = acc[2 * BLOCK] * omw + target.z * w;
                    acc[3 * BLOCK] = acc[3 * BLOCK] * omw + target.w * w;
                }
                if (sample + 1 >= Q.s_end) {
                    if constexpr (SOURCE != jtr::SOURCE_SPHERE)
                        Q.rgba[ray] = make_float4(acc[0], acc[BLOCK], acc[2 * BLOCK], acc[3 * BLOCK]);
                    ray = -1;
                } else {
                    *cur = sample + 1;
                    radiance_start<F, SOURCE>(P, Q, ray, sample + 1, st);
                }
            }
            if (ray >= 0) query_start<WIDE>(S, T, st.o, st.d, radiance_query_instance(S, st), stack);
        }
    }
}

// jt_hemisphere_rays: one point per thread on a plain grid, as jt_surface.hip's camera_kernel; the
// ray radiance_kernel<.., SOURCE_HEMISPHERE> starts sample `sample` of point i with, from the same arm.
// A thread reads its record before it writes, so rays may be the points' own array.
__global__ __launch_bounds__(BLOCK) void hemisphere_kernel(DParams P, const float* points, long long stream_base, int sample, int n,
                                                           float2* rays) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // n <= 2^30 (QUERY_MAX_RAYS)
    if (i >= n) return;
    Rng rng;
    v3 o, d;
    radiance_ray<jtr::SOURCE_HEMISPHERE>(P, points, stream_base, i, sample, rng, o, d);
    float2* const y = rays + (size_t)i * 3;
    y[0] = make_float2(o.x, o.y);
    y[1] = make_float2(o.z, d.x);
    y[2] = make_float2(d.y, d.z);
}

// jt_sphere_rays: the same for radiance_kernel<.., SOURCE_SPHERE>, whose record is a position alone
// (3 floats in, 6 out: rays must not be the points' own array)
__global__ __launch_bounds__(BLOCK) void sphere_kernel(DParams P, const float* points, long long stream_base, int sample, int n,
                                                       float2* rays) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // n <= 2^30 (QUERY_MAX_RAYS)
    if (i >= n) return;
    Rng rng;
    v3 o, d;
    radiance_ray<jtr::SOURCE_SPHERE>(P, points, stream_base, i, sample, rng, o, d);
    float2* const y = rays + (size_t)i * 3;
    y[0] = make_float2(o.x, o.y);
    y[1] = make_float2(o.z, d.x);
    y[2] = make_float2(d.y, d.z);
}

}  // namespace jtk

// ---- the context's half (jt_context.h)
using namespace jtc;
using jtd::DScene;

namespace {

constexpr int BLOCK = jtk::BLOCK;

constexpr const char* RADIANCE_MULTI =
    "jt_radiance, jt_irradiance and jt_hemisphere_rays are not available on a multi-device context (jt_create_multi): use one "
    "context per device";

// the checks jt_radiance's and jt_irradiance's entry points share (`in`: the rays or the points); *done: n == 0, nothing to do
int radiance_check(const jt_ctx* c, int64_t n, const void* in, const char* in_name, int64_t stream_base, int32_t s0, int32_t s1,
                   const void* out, const char* out_name, bool device, bool* done) {
    return ray_call_check(c, {{in, in_name}, {out, out_name}}, jtr::radiance_range_error(n, stream_base, s0, s1),
                          device && ((uintptr_t)out & 15) ? "d_rgba must be aligned to 16 bytes" : nullptr, RADIANCE_MULTI, n == 0, done);
}

// jt_hemisphere_rays': one sample, which only has to be a stream's (sample >= 0), in the place of jt_radiance's range
int hemisphere_check(const jt_ctx* c, int64_t n, const void* points, const char* points_name, int64_t stream_base, int32_t sample,
                     const void* out, const char* out_name, bool device, bool* done) {
    const char* range = jtr::radiance_range_error(n, stream_base, 0, 1);
    if (!range && sample < 0) range = "sample must be at least 0";
    return ray_call_check(c, {{points, points_name}, {out, out_name}}, range,
                          device && ((uintptr_t)out & 7) ? "d_rays must be aligned to 8 bytes" : nullptr, RADIANCE_MULTI, n == 0, done);
}

// jt_probe_sh's and jt_sphere_rays': the same rules in the same order, the messages their own
constexpr const char* PROBE_MULTI =
    "jt_probe_sh and jt_sphere_rays are not available on a multi-device context (jt_create_multi): use one context per device";

int probe_check(const jt_ctx* c, int64_t n, const void* points, const char* points_name, int64_t stream_base, int32_t s0, int32_t s1,
                const void* out, const char* out_name, bool device, bool* done) {
    return ray_call_check(c, {{points, points_name}, {out, out_name}}, jtr::radiance_range_error(n, stream_base, s0, s1),
                          device && ((uintptr_t)out & 15) ? "d_sh must be aligned to 16 bytes" : nullptr, PROBE_MULTI, n == 0, done);
}

int sphere_check(const jt_ctx* c, int64_t n, const void* points, const char* points_name, int64_t stream_base, int32_t sample,
                 const void* out, const char* out_name, bool device, bool* done) {
    const char* range = jtr::radiance_range_error(n, stream_base, 0, 1);
    if (!range && sample < 0) range = "sample must be at least 0 (jt_sphere_rays)";
    return ray_call_check(c, {{points, points_name}, {out, out_name}}, range,
                          device && ((uintptr_t)out & 7) ? "d_rays must be aligned to 8 bytes (jt_sphere_rays)" : nullptr, PROBE_MULTI,
                          n == 0, done);
}

// n >= 1 records (SOURCE_RAY: rays, SOURCE_HEMISPHERE: points, SOURCE_SPHERE: positions, d_rgba then
// the probes' records) from device pointers, on the context's stream; returns once the stream is idle
template <int SOURCE>
int radiance_run(jt_ctx* c, int64_t n, const void* d_recs, int64_t stream_base, int32_t s0, int32_t s1, void* d_rgba) {
    (void)hipSetDevice(c->device);
    int st = query_setup(c);
    if (st != JT_OK) return st;
    const int grid = jtq::query_grid(n, c->cus);
    DScene S;
    bool ovf;
    if ((st = query_scene(c, grid, &S, &ovf)) != JT_OK) return st;
    jtk::DRadiance Q{};
    Q.rays = (const float*)d_recs;
    Q.rgba = (float4*)d_rgba;
    Q.stream_base = (long long)stream_base;
    Q.s_begin = s0;
    Q.s_end = s1;
    Q.feed = {c->q_counter, (int)n, (unsigned)jtq::query_claim_rays(n, grid)};
    const hipError_t e = hipMemsetAsync(c->q_counter, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync radiance ray counter");
    with_bools(c->choice.wide, ovf, c->sampler == 2, [&](auto wide, auto over, auto naive) {
        hipLaunchKernelGGL((jtk::radiance_kernel<wide(), over(), naive() ? 2 : 1, SOURCE>), dim3((unsigned)grid), dim3(BLOCK), 0, c->stream,
                           S, c->P, Q);
    });
    return launch_finish(c, SOURCE == jtr::SOURCE_RAY          ? "radiance kernel"
                            : SOURCE == jtr::SOURCE_HEMISPHERE ? "irradiance kernel"
                                                               : "probe kernel");
}

// the host variants of both: the records staged in Q_RAYS, the means in Q_OUT, whose jt_hit slot
// (24 bytes) has room for a 16-byte mean
template <int SOURCE>
int radiance_host(jt_ctx* c, int64_t n, const float* recs, int64_t stream_base, int32_t s0, int32_t s1, float* rgba) {
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)n;
    int st;
    if ((st = query_stage(c, n))) return st;
    void* const d_recs = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_out = c->q_grow[jt_ctx::Q_OUT];
    if ((st = copy_in(d_recs, recs, N * 6 * sizeof(float), "hipMemcpy radiance rays")) ||
        (st = radiance_run<SOURCE>(c, n, d_recs, stream_base, s0, s1, d_out)))
        return st;
    return copy_out(rgba, d_out, N * 4 * sizeof(float), "hipMemcpy radiance results");
}

int hemisphere_run(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample, void* d_rays) {
    (void)hipSetDevice(c->device);
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(jtk::hemisphere_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, c->P, (const float*)d_points, (long long)stream_base,
                       (int)sample, (int)n, (float2*)d_rays);
    return launch_finish(c, "hemisphere kernel");
}

int sphere_run(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample, void* d_rays) {
    (void)hipSetDevice(c->device);
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(jtk::sphere_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, c->P, (const float*)d_points, (long long)stream_base,
                       (int)sample, (int)n, (float2*)d_rays);
    return launch_finish(c, "sphere kernel");
}

// jt_probe_sh's host variant: chunks of at most c->probe_chunk points, the positions staged in
// Q_RAYS (a 12-byte record in a 24-byte slot), the records in Q_SH, grown to the chunk; a chunk's
// streams start where the last one's ended, which gives the bits of one call. (A template like
// radiance_host, so the kernel's SOURCE_SPHERE instances follow the others in the object.)
template <int SOURCE>
int probe_host(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t s0, int32_t s1, float* sh) {
    (void)hipSetDevice(c->device);
    const int64_t chunk = n < c->probe_chunk ? n : c->probe_chunk;
    int st;
    if ((st = query_stage(c, chunk))) return st;
    if (chunk > c->q_stage_sh) {
        const size_t cap = (size_t)jtq::query_stage_rays(c->q_stage_sh, chunk);
        c->q_stage_sh = 0;
        if ((st = query_grow(c, jt_ctx::Q_SH, cap * jtsh::SH_RECORD * sizeof(float), "probe records"))) return st;
        c->q_stage_sh = (long long)cap;
    }
    void* const d_points = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_sh = c->q_grow[jt_ctx::Q_SH];
    for (int64_t at = 0; at < n; at += chunk) {
        const size_t m = (size_t)(n - at < chunk ? n - at : chunk);
        if ((st = copy_in(d_points, points + (size_t)at * 3, m * 3 * sizeof(float), "hipMemcpy probe points")) ||
            (st = radiance_run<SOURCE>(c, (int64_t)m, d_points, stream_base + at, s0, s1, d_sh)) ||
            (st = copy_out(sh + (size_t)at * jtsh::SH_RECORD, d_sh, m * jtsh::SH_RECORD * sizeof(float), "hipMemcpy probe records")))
            return st;
    }
    return JT_OK;
}

}  // namespace

static_assert(jtr::RADIANCE_LDS_BYTES <= 64 * 1024, "radiance_kernel's static LDS");
static_assert(sizeof(jt_hit) >= 6 * sizeof(float), "the host variants stage a mean (16 bytes) or a ray (24) in a jt_hit slot of Q_OUT");

extern "C" {

int jt_radiance_device(jt_ctx* c, int64_t n, const void* d_rays, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                       void* d_rgba) {
    bool done;
    if (const int st = radiance_check(c, n, d_rays, "d_rays", stream_base, sample_begin, sample_end, d_rgba, "d_rgba", true, &done))
        return st;
    return done ? JT_OK : radiance_run<jtr::SOURCE_RAY>(c, n, d_rays, stream_base, sample_begin, sample_end, d_rgba);
}

int jt_radiance(jt_ctx* c, int64_t n, const float* rays, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                float* rgba) {
    bool done;
    if (const int st = radiance_check(c, n, rays, "rays", stream_base, sample_begin, sample_end, rgba, "rgba", false, &done)) return st;
    return done ? JT_OK : radiance_host<jtr::SOURCE_RAY>(c, n, rays, stream_base, sample_begin, sample_end, rgba);
}

int jt_irradiance_device(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                         void* d_rgba) {
    bool done;
    if (const int st = radiance_check(c, n, d_points, "d_points", stream_base, sample_begin, sample_end, d_rgba, "d_rgba", true, &done))
        return st;
    return done ? JT_OK : radiance_run<jtr::SOURCE_HEMISPHERE>(c, n, d_points, stream_base, sample_begin, sample_end, d_rgba);
}

int jt_irradiance(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                  float* rgba) {
    bool done;
    if (const int st = radiance_check(c, n, points, "points", stream_base, sample_begin, sample_end, rgba, "rgba", false, &done))
        return st;
    return done ? JT_OK : radiance_host<jtr::SOURCE_HEMISPHERE>(c, n, points, stream_base, sample_begin, sample_end, rgba);
}

int jt_hemisphere_rays_device(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample, void* d_rays) {
    bool done;
    if (const int st = hemisphere_check(c, n, d_points, "d_points", stream_base, sample, d_rays, "d_rays", true, &done)) return st;
    return done ? JT_OK : hemisphere_run(c, n, d_points, stream_base, sample, d_rays);
}

int jt_hemisphere_rays(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t sample, float* rays) {
    bool done;
    if (const int st = hemisphere_check(c, n, points, "points", stream_base, sample, rays, "rays", false, &done)) return st;
    if (done) return JT_OK;
    (void)hipSetDevice(c->device);
    // the points staged in Q_RAYS, the rays in Q_OUT: a ray record fits its 24-byte jt_hit slot
    int st;
    if ((st = query_stage(c, n))) return st;
    void* const d_points = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_rays = c->q_grow[jt_ctx::Q_OUT];
    const size_t bytes = (size_t)n * 6 * sizeof(float);
    if ((st = copy_in(d_points, points, bytes, "hipMemcpy hemisphere points")) ||
        (st = hemisphere_run(c, n, d_points, stream_base, sample, d_rays)))
        return st;
    return copy_out(rays, d_rays, bytes, "hipMemcpy hemisphere rays");
}

int jt_probe_sh_device(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                       void* d_sh) {
    bool done;
    if (const int st = probe_check(c, n, d_points, "d_points", stream_base, sample_begin, sample_end, d_sh, "d_sh", true, &done)) return st;
    return done ? JT_OK : radiance_run<jtr::SOURCE_SPHERE>(c, n, d_points, stream_base, sample_begin, sample_end, d_sh);
}

int jt_probe_sh(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t sample_begin, int32_t sample_end, float* sh) {
    bool done;
    if (const int st = probe_check(c, n, points, "points", stream_base, sample_begin, sample_end, sh, "sh", false, &done)) return st;
    return done ? JT_OK : probe_host<jtr::SOURCE_SPHERE>(c, n, points, stream_base, sample_begin, sample_end, sh);
}

int jt_sphere_rays_device(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample, void* d_rays) {
    bool done;
    if (const int st = sphere_check(c, n, d_points, "d_points", stream_base, sample, d_rays, "d_rays", true, &done)) return st;
    return done ? JT_OK : sphere_run(c, n, d_points, stream_base, sample, d_rays);
}

int jt_sphere_rays(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t sample, float* rays) {
    bool done;
    if (const int st = sphere_check(c, n, points, "points", stream_base, sample, rays, "rays", false, &done)) return st;
    if (done) return JT_OK;
    (void)hipSetDevice(c->device);
    // the positions staged in Q_RAYS (12 bytes in a 24-byte slot), the rays in Q_OUT as jt_hemisphere_rays'
    int st;
    if ((st = query_stage(c, n))) return st;
    void* const d_points = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_rays = c->q_grow[jt_ctx::Q_OUT];
    if ((st = copy_in(d_points, points, (size_t)n * 3 * sizeof(float), "hipMemcpy sphere points")) ||
        (st = sphere_run(c, n, d_points, stream_base, sample, d_rays)))
        return st;
    return copy_out(rays, d_rays, (size_t)n * 6 * sizeof(float), "hipMemcpy sphere rays");
}

}  // extern "C"
