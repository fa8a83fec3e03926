// jt_intersect.hip — ray queries on a context's scene (include/jtrace.h: jt_intersect, jt_occluded and
// their device-pointer variants; DESIGN.md §6e "Ray queries"): the megakernel's own traversal
// (jt_traverse.h) over the caller's rays. The context's half below also holds what every call on
// the caller's own records shares (jt_context.h; jt_surface.hip and jt_radiance.hip use it): the
// argument checks, the launch tail, the staging copies, the first call's uploads and the grid's scene.
//
// The scene is the context's HBM copy — every array of JT_SCENE_ARRAYS is uploaded in both scene
// modes, so an LDS-mode context queries through HBM pointers too (NCACHE) — with the general feature
// mask (the traversal tells masks apart by FT_XFORM and FT_QUAD only), no counters, the 16-entry
// LDS stack ring, and for a scene whose bound exceeds the ring an HBM overflow area of the query
// grid's own. Per lane the loop is
//     query_start<WIDE>; until query_done<WIDE>: prim_step if nprim > 0, else node_step_any;
//     then rerun_tie<WIDE>, and the loop again if it re-runs
// and an any-hit query (ANY) leaves it at its first accepted hit instead. A ray's result depends
// on the ray and the scene only, never on the lane that runs it or on when.
//
// Work distribution: query lengths diverge by orders of magnitude (a miss from outside costs one
// box test, a ray through a deep scene hundreds of nodes), so the grid is persistent — at most
// QUERY_WG_PER_CU workgroups per compute unit (jt_intersect.h) — and a wave refills its finished lanes
// once QUERY_REFILL_LANES of them have no ray (feed_refill, jt_feed.h, which radiance_kernel runs
// too): a ballot of those lanes, and the k-th of them takes the k-th ray of the wave's reserve (the
// megakernel's hand-out pattern, jt_kernels.h). The reserve (jtq::WaveReserve, jt_intersect.h) is
// query_claim_rays consecutive rays (64 to 256), claimed by the wave's first lane with one atomicAdd on the
// launch's ray counter: a claim per refill (a fifth of a million same-address atomics for 2^22
// rays) bound the whole launch to 2.4 ms whatever the scene (EXPERIMENTS.md). Each iteration then
// runs one step kind, primitive tests or node steps, picked by the megakernel's biased lane vote.
// A lane writes its ray's record when its query ends.
//
// Bounded queries (jt_intersect_bounded, jt_occluded_bounded, jt_visible): the loop's
// compile-time BOUND (jt_intersect.h). A bounded query is the same query started at the caller's
// tmax instead of +inf: T.tmax is per-lane state that every step already reads, so the bound is one
// assignment after query_start (query_take), and one more after a tie's re-run, whose query_start
// resets it. The bound is the current tmax for the tie rule too: a near-first query that accepts a
// hit exactly on it re-runs like any other exact-t tie. The segment form builds d = b - a in the
// lane and writes the flag inverted (visible). query_kernel keeps its three parameters and its
// name, query_bounded_kernel is the same loop (query_loop) with a bound.
//
// Ambient occlusion (jt_ambient_occlusion): occlusion_kernel, the any-hit loop on the hemisphere
// draws of jt_irradiance (radiance_ray, jt_sample_ray.h), bounded by the call's radius. A lane keeps
// its point for all its samples, as radiance_kernel does, and counts the samples whose query found
// nothing in a register: no atomics, no second pass, no shading, no per-lane LDS slots.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "jt_context.h"
#include "jt_feed.h"
#include "jt_sample_ray.h"
#include "jt_traverse.h"

namespace jtk {

using jtq::QUERY_VOTE_P;
using jtq::QUERY_RING;

struct DQuery {
    const float* rays;     // n x (o, d)
    const int* inst;       // nullptr, or per ray -1 / an instance id in the caller's numbering
    int* hits;             // closest hit: n jt_hit records as 6 words each
    unsigned char* occ;    // any hit: n flags
    const int* to_dev;     // the caller's instance id -> the device's (TLAS leaf order)
    const int* to_ref;     // and back
    int ninst;
    DFeed feed;            // the n rays' hand-out
};

constexpr int Q_BAD_INSTANCE = -2;
// the device instance of ray `ray`'s query: -1 a scene query, Q_BAD_INSTANCE an id out of range
__device__ __forceinline__ int query_instance(const DQuery& Q, int ray) {
    if (!Q.inst) return -1;
    const int id = Q.inst[ray];
    if (id == -1) return -1;
    return id >= 0 && id < Q.ninst ? Q.to_dev[id] : Q_BAD_INSTANCE;
}

__device__ __forceinline__ void write_hit(const DQuery& Q, int ray, const Hit& h) {
    int* const y = Q.hits + (size_t)ray * 6;
    y[0] = h.hit ? Q.to_ref[h.inst] : -1;
    y[1] = h.elem;
    y[2] = __float_as_int(h.u);
    y[3] = __float_as_int(h.v);
    y[4] = __float_as_int(h.t);
    y[5] = h.hit ? 1 : 0;
}

static_assert(jtq::SEGMENT_TMAX == 1.0f - ray_eps, "jt_visible's bound is 1 - ray_eps");
// the tmax ray `ray`'s bounded query starts at: the caller's, or the segment form's constant
template <int BOUND>
__device__ __forceinline__ float query_bound(const float* tmax, int ray) {
    return BOUND == jtq::BOUND_SEGMENT ? jtq::SEGMENT_TMAX : tmax[ray];
}

// the lane starts ray `ray`'s query; false: its instance id is out of range, a miss is recorded
template <bool WIDE, bool ANY, int BOUND>
__device__ __forceinline__ bool query_take(const DScene& S, const DQuery& Q, const float* tmax, Trav& T, int ray, int* stack) {
    const int q = query_instance(Q, ray);
    if (q == Q_BAD_INSTANCE) {
        if (ANY) Q.occ[ray] = 0;
        else write_hit(Q, ray, Hit{-1, -1, 0.0f, 0.0f, __builtin_inff(), false});
        return false;
    }
    const float* const r = Q.rays + (size_t)ray * 6;
    if constexpr (BOUND == jtq::BOUND_NONE) {
        query_start<WIDE>(S, T, V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5]), q, stack);
    } else {
        const v3 o = V3(r[0], r[1], r[2]);
        v3 d = V3(r[3], r[4], r[5]);
        if constexpr (BOUND == jtq::BOUND_SEGMENT) d = d - o;  // the record is (a, b): one float32 subtraction per component
        query_start<WIDE>(S, T, o, d, q, stack);
        T.tmax = query_bound<BOUND>(tmax, ray);
    }
    return true;
}

// the loop of query_kernel and query_bounded_kernel; tmax: BOUND_ARRAY's per-ray bounds
template <bool WIDE, bool OVF, bool ANY, int BOUND>
__device__ __forceinline__ void query_loop(const DScene& S, const DQuery& Q, const float* tmax) {
    constexpr int F = FT_ALL;
    __shared__ int ring[QUERY_RING * BLOCK];
    int* const stack = ring + threadIdx.x;
    const int slot = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // the lane's HBM stack-overflow area
    Counters cnt{0, 0, 0, 0};
    Trav T;
    int ray = -1;  // the lane's ray; -1: none
    jtq::WaveReserve reserve;
    // ---- refill (jt_feed.h): a lane without a ray takes one of the wave's reserve
    while (feed_refill(Q.feed, reserve, ray >= 0, [&](int r) {
        if (query_take<WIDE, ANY, BOUND>(S, Q, tmax, T, r, stack)) ray = r;
    })) {
        // ---- one step of every lane with a query in flight: one step kind per iteration, by a
        // biased lane vote (the megakernel's, jt_kernels.h), so the SIMD runs one code path; a lane's
        // own sequence of steps is unchanged, it only waits while the other kind runs
        const bool wantp = ray >= 0 && T.nprim > 0, wantn = ray >= 0 && T.nprim == 0;
        const int np = __popcll(__builtin_amdgcn_ballot_w64(wantp)), nn = __popcll(__builtin_amdgcn_ballot_w64(wantn));
        if (np * QUERY_VOTE_P >= nn) {
            if (wantp) prim_step<0, F>(S, T, cnt);
        } else {
            if (wantn) node_step_any<WIDE, QUERY_RING, OVF, 0, true, F>(S, T, stack, slot, cnt);
        }
        // ---- a lane whose query has ended records it
        if (ray >= 0) {
            if (ANY) {  // the first accepted hit ends the query; never re-run for a tie
                if (T.h_inst >= 0 || query_done<WIDE>(T)) {
                    // the segment form reports visible: nothing hit
                    if constexpr (BOUND == jtq::BOUND_SEGMENT) Q.occ[ray] = T.h_inst >= 0 ? 0 : 1;
                    else Q.occ[ray] = T.h_inst >= 0 ? 1 : 0;
                    ray = -1;
                }
            } else if constexpr (BOUND == jtq::BOUND_NONE) {
                if (query_done<WIDE>(T) && !rerun_tie<WIDE>(S, T, T.wo, T.wd, query_instance(Q, ray), stack)) {
                    write_hit(Q, ray, query_hit(T));
                    ray = -1;
                }
            } else if (query_done<WIDE>(T)) {
                if (rerun_tie<WIDE>(S, T, T.wo, T.wd, query_instance(Q, ray), stack)) {
                    // the re-run is the same bounded query: its query_start has reset tmax
                    T.tmax = query_bound<BOUND>(tmax, ray);
                } else {
                    // a miss is the unbounded miss record: tmax still holds the bound, t is +inf
                    Hit h = query_hit(T);
                    h.t = h.hit ? h.t : __builtin_inff();
                    write_hit(Q, ray, h);
                    ray = -1;
                }
            }
        }
    }
}

template <bool WIDE, bool OVF, bool ANY>
__global__ __launch_bounds__(BLOCK) void query_kernel(DScene S, DQuery Q) {
    query_loop<WIDE, OVF, ANY, jtq::BOUND_NONE>(S, Q, nullptr);
}

template <bool WIDE, bool OVF, bool ANY, int BOUND>
__global__ __launch_bounds__(BLOCK) void query_bounded_kernel(DScene S, DQuery Q, const float* tmax) {
    query_loop<WIDE, OVF, ANY, BOUND>(S, Q, tmax);
}

struct DOcclusion {
    const float* points;    // n x (position, normal)
    float* visibility;      // n quotients
    long long stream_base;  // point i draws from stream stream_base + i
    int s_begin, s_end;     // the samples of every point
    float radius;           // every query's bound; +inf: unbounded
    DFeed feed;             // the n points' hand-out
};

// jt_ambient_occlusion: per point and sample the any-hit query of query_loop on jt_hemisphere_rays'
// ray, bounded by the radius. A sample's outcome is one bit and the quotient is taken once, of two
// integers, so the value does not depend on when a sample ran.
template <bool WIDE, bool OVF>
__global__ __launch_bounds__(BLOCK) void occlusion_kernel(DScene S, DParams P, DOcclusion Q) {
    constexpr int F = FT_ALL;
    __shared__ int ring[QUERY_RING * BLOCK];
    int* const stack = ring + threadIdx.x;
    const int slot = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // the lane's HBM stack-overflow area
    Counters cnt{0, 0, 0, 0};
    Trav T;
    int ray = -1;     // the lane's point; -1: none
    int sample = 0;   // its sample in flight
    int visible = 0;  // its samples so far whose query found nothing
    jtq::WaveReserve reserve;
    // the lane's point starts sample s: the hemisphere draw, then the bounded scene query
    const auto start = [&](int s) {
        Rng rng;
        v3 o, d;
        radiance_ray<jtr::SOURCE_HEMISPHERE>(P, Q.points, Q.stream_base, ray, s, rng, o, d);
        query_start<WIDE>(S, T, o, d, -1, stack);
        T.tmax = Q.radius;
    };
    while (feed_refill(Q.feed, reserve, ray >= 0, [&](int r) {
        ray = r;
        sample = Q.s_begin;
        visible = 0;
        start(sample);
    })) {
        // one step kind per iteration, by query_loop's vote
        const bool wantp = ray >= 0 && T.nprim > 0, wantn = ray >= 0 && T.nprim == 0;
        const int np = __popcll(__builtin_amdgcn_ballot_w64(wantp)), nn = __popcll(__builtin_amdgcn_ballot_w64(wantn));
        if (np * QUERY_VOTE_P >= nn) {
            if (wantp) prim_step<0, F>(S, T, cnt);
        } else {
            if (wantn) node_step_any<WIDE, QUERY_RING, OVF, 0, true, F>(S, T, stack, slot, cnt);
        }
        // the first accepted hit ends a sample's query; then the next sample, or the quotient
        if (ray >= 0 && (T.h_inst >= 0 || query_done<WIDE>(T))) {
            visible += T.h_inst >= 0 ? 0 : 1;
            sample += 1;
            if (sample >= Q.s_end) {
                Q.visibility[ray] = jtr::occlusion_visibility(visible, Q.s_end - Q.s_begin);
                ray = -1;
            } else {
                start(sample);
            }
        }
    }
}

}  // namespace jtk

// ---- the context's half (jt_context.h)
using namespace jtc;
using jtd::DScene;

namespace {

constexpr int BLOCK = jtk::BLOCK;

// the checks every entry point shares; *done: n == 0, nothing to do
int query_check(const jt_ctx* c, int64_t n, const void* rays, const char* rays_name, const void* out, const char* out_name,
                bool* done) {
    return ray_call_check(c, {{rays, rays_name}, {out, out_name}}, jtq::query_count_error(n, "n must be at most 2^30 rays"), nullptr,
                          "ray queries are not available on a multi-device context (jt_create_multi): query one context per device",
                          n == 0, done);
}

// n >= 1 rays from device pointers, on the context's stream; returns once the stream is idle.
// bound (jt_intersect.h): BOUND_ARRAY reads d_tmax, BOUND_SEGMENT (any-hit only) takes d_rays as
// segments and writes visible flags
int query_run(jt_ctx* c, int64_t n, const void* d_rays, const void* d_inst, void* d_out, bool any, int bound = jtq::BOUND_NONE,
              const void* d_tmax = nullptr) {
    (void)hipSetDevice(c->device);
    int st = query_setup(c);
    if (st != JT_OK) return st;
    const int grid = jtq::query_grid(n, c->cus);
    DScene S;
    bool ovf;
    if ((st = query_scene(c, grid, &S, &ovf)) != JT_OK) return st;
    jtk::DQuery Q{};
    Q.rays = (const float*)d_rays;
    Q.inst = (const int*)d_inst;
    Q.hits = any ? nullptr : (int*)d_out;
    Q.occ = any ? (unsigned char*)d_out : nullptr;
    Q.to_dev = c->q_to_dev;
    Q.to_ref = c->q_to_ref;
    Q.ninst = (int)c->inst_new.size();
    Q.feed = {c->q_counter, (int)n, (unsigned)jtq::query_claim_rays(n, grid)};
    const hipError_t e = hipMemsetAsync(c->q_counter, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync query ray counter");
    with_bools(c->choice.wide, ovf, any, [&](auto wide, auto over, auto occ) {
        const dim3 g((unsigned)grid), b(BLOCK);
        if (bound == jtq::BOUND_NONE) {
            hipLaunchKernelGGL((jtk::query_kernel<wide(), over(), occ()>), g, b, 0, c->stream, S, Q);
        } else if (bound == jtq::BOUND_ARRAY) {
            hipLaunchKernelGGL((jtk::query_bounded_kernel<wide(), over(), occ(), jtq::BOUND_ARRAY>), g, b, 0, c->stream, S, Q,
                               (const float*)d_tmax);
        } else if constexpr (occ()) {
            hipLaunchKernelGGL((jtk::query_bounded_kernel<wide(), over(), true, jtq::BOUND_SEGMENT>), g, b, 0, c->stream, S, Q,
                               (const float*)nullptr);
        }
    });
    return launch_finish(c, bound == jtq::BOUND_NONE ? "query kernel" : "bounded query kernel");
}

// the host variants: rays (and instance ids, and bounds) staged to the device, the results copied back
int query_host(jt_ctx* c, int64_t n, const float* rays, const int32_t* instance, void* out, bool any, int bound = jtq::BOUND_NONE,
               const float* tmax = nullptr) {
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)n;
    if (const int st = query_stage(c, n)) return st;
    void* const d_rays = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_inst = instance ? c->q_grow[jt_ctx::Q_INST] : nullptr;
    void* const d_tmax = tmax ? c->q_grow[jt_ctx::Q_TMAX] : nullptr;
    void* const d_out = c->q_grow[jt_ctx::Q_OUT];
    int st;
    if ((st = copy_in(d_rays, rays, N * 6 * sizeof(float), "hipMemcpy query rays")) ||
        (instance && (st = copy_in(d_inst, instance, N * sizeof(int32_t), "hipMemcpy query rays"))) ||
        (tmax && (st = copy_in(d_tmax, tmax, N * sizeof(float), "hipMemcpy query bounds"))))
        return st;
    if (bound != jtq::BOUND_NONE) st = query_run(c, n, d_rays, d_inst, d_out, any, bound, d_tmax);
    else st = any ? jt_occluded_device(c, n, d_rays, d_out) : jt_intersect_device(c, n, d_rays, d_inst, d_out);
    if (st) return st;
    return copy_out(out, d_out, any ? N : N * sizeof(jt_hit), "hipMemcpy query results");
}

constexpr const char* OCCLUSION_MULTI =
    "jt_ambient_occlusion is not available on a multi-device context (jt_create_multi): use one context per device";

// jt_ambient_occlusion's checks: jt_radiance's ladder with the radius after the sample range
int occlusion_check(const jt_ctx* c, int64_t n, const void* points, const char* points_name, int64_t stream_base, int32_t s0, int32_t s1,
                    float radius, const void* out, const char* out_name, bool device, bool* done) {
    const char* range = jtr::radiance_range_error(n, stream_base, s0, s1);
    if (!range) range = jtr::occlusion_radius_error(radius);
    return ray_call_check(c, {{points, points_name}, {out, out_name}}, range,
                          device && ((uintptr_t)out & 3) ? "d_visibility must be aligned to 4 bytes" : nullptr, OCCLUSION_MULTI, n == 0, done);
}

// n >= 1 points from device pointers, on the context's stream; returns once the stream is idle
int occlusion_run(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t s0, int32_t s1, float radius, void* d_vis) {
    (void)hipSetDevice(c->device);
    int st = query_setup(c);
    if (st != JT_OK) return st;
    const int grid = jtq::query_grid(n, c->cus);
    DScene S;
    bool ovf;
    if ((st = query_scene(c, grid, &S, &ovf)) != JT_OK) return st;
    jtk::DOcclusion Q{};
    Q.points = (const float*)d_points;
    Q.visibility = (float*)d_vis;
    Q.stream_base = (long long)stream_base;
    Q.s_begin = s0;
    Q.s_end = s1;
    Q.radius = radius;
    Q.feed = {c->q_counter, (int)n, (unsigned)jtq::query_claim_rays(n, grid)};
    const hipError_t e = hipMemsetAsync(c->q_counter, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync occlusion point counter");
    with_bools(c->choice.wide, ovf, false, [&](auto wide, auto over, auto) {
        hipLaunchKernelGGL((jtk::occlusion_kernel<wide(), over()>), dim3((unsigned)grid), dim3(BLOCK), 0, c->stream, S, c->P, Q);
    });
    return launch_finish(c, "occlusion kernel");
}

}  // namespace

// ---- what every call on the caller's own records shares (jt_surface.hip, jt_radiance.hip too)
int jtc::ray_call_check(const jt_ctx* c, std::initializer_list<NamedArg> args, const char* range_error, const char* misaligned,
                        const char* multi_error, bool empty, bool* done) {
    if (done) *done = false;
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    for (const NamedArg& a : args)
        if (!a.p) return jt::fail(JT_ERR_INVALID, std::string(a.name) + " is NULL");
    if (range_error) return jt::fail(JT_ERR_INVALID, range_error);
    if (misaligned) return jt::fail(JT_ERR_INVALID, misaligned);
    if (empty) {
        *done = true;
        return JT_OK;
    }
    if (c->multi) return jt::fail(JT_ERR_UNSUPPORTED, multi_error);
    if (c->failed) return jt::fail(JT_ERR_STATE, "a previous launch failed; jt_reset the context");
    return JT_OK;
}

int jtc::launch_finish(jt_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, (std::string(what) + " launch").c_str());
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->failed = true;
        return hip_fail(e, what);
    }
    return JT_OK;
}

int jtc::copy_in(void* dst, const void* src, size_t bytes, const char* what) {
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? JT_OK : hip_fail(e, what);
}

int jtc::copy_out(void* dst, const void* src, size_t bytes, const char* what) {
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, what);
}

// a buffer of jt_ctx::q_grow of at least `bytes` (the old one is freed first: its content is not kept)
int jtc::query_grow(jt_ctx* c, int which, size_t bytes, const char* what) {
    if (c->q_grow[which]) (void)hipFree(c->q_grow[which]);
    c->q_grow[which] = nullptr;
    if (hipMalloc(&c->q_grow[which], bytes) != hipSuccess) {
        c->q_grow[which] = nullptr;
        (void)hipGetLastError();
        return jt::fail(JT_ERR_NOMEM, std::string("hipMalloc ") + what);
    }
    return JT_OK;
}

// the first query's uploads: the instance permutation both ways and the ray counter
int jtc::query_setup(jt_ctx* c) {
    if (c->q_counter) return JT_OK;
    const size_t ni = c->inst_new.size();
    std::vector<int> to_ref(ni, -1);
    for (size_t k = 0; k < ni; k++) to_ref[(size_t)c->inst_new[k]] = (int)k;
    void *a = nullptr, *b = nullptr, *w = nullptr;
    int st;
    const size_t bytes = (ni ? ni : 1) * sizeof(int);
    if ((st = device_alloc(c, bytes, "query instance ids", &a)) || (st = device_alloc(c, bytes, "query instance ids", &b)) ||
        (st = device_alloc(c, sizeof(unsigned), "query ray counter", &w)))
        return st;
    hipError_t e;
    if (ni && ((e = hipMemcpy(a, c->inst_new.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess ||
               (e = hipMemcpy(b, to_ref.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess))
        return hip_fail(e, "hipMemcpy query instance ids");
    c->q_to_dev = (int*)a;
    c->q_to_ref = (int*)b;
    c->q_counter = (unsigned*)w;
    return JT_OK;
}

int jtc::query_scene(jt_ctx* c, int grid, DScene* out, bool* ovf) {
    DScene S = c->S;
    // the context's ring entries in use (option test_lds_ring shortens it), within this kernel's ring
    S.ring = c->S.ring < jtq::QUERY_RING ? c->S.ring : jtq::QUERY_RING;
    const int need = c->S.stack_need;
    *ovf = need > S.ring;
    S.ovf = nullptr;
    S.ovf_stride = 0;
    if (*ovf) {  // an overflow area of this grid's own (the trace kernel's belongs to its grid)
        const size_t entries = jtq::query_ovf_entries(grid, need);
        if (entries > c->q_ovf_entries) {
            c->q_ovf_entries = 0;
            if (const int st = query_grow(c, jt_ctx::Q_OVF, entries * sizeof(int), "query stack overflow")) return st;
            c->q_ovf_entries = entries;
        }
        S.ovf = (int*)c->q_grow[jt_ctx::Q_OVF];
        S.ovf_stride = need;
    }
    *out = S;
    return JT_OK;
}

// the host variants' staging of rays, instance ids, bounds and jt_hit records, grown to hold n rays
int jtc::query_stage(jt_ctx* c, int64_t n) {
    if (n <= c->q_stage_rays) return JT_OK;
    const size_t cap = (size_t)jtq::query_stage_rays(c->q_stage_rays, n);
    c->q_stage_rays = 0;
    int st;
    if ((st = query_grow(c, jt_ctx::Q_RAYS, cap * 6 * sizeof(float), "query rays")) ||
        (st = query_grow(c, jt_ctx::Q_INST, cap * sizeof(int32_t), "query instance ids")) ||
        (st = query_grow(c, jt_ctx::Q_TMAX, cap * sizeof(float), "query bounds")) ||
        (st = query_grow(c, jt_ctx::Q_OUT, cap * sizeof(jt_hit), "query results")))
        return st;
    c->q_stage_rays = (long long)cap;
    return JT_OK;
}

void jtc::query_free(jt_ctx* c) {
    for (void*& p : c->q_grow) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    c->q_ovf_entries = 0;
    c->q_stage_rays = 0;
    c->q_stage_surf = 0;
    c->q_stage_sh = 0;
    c->q_stage_multi = 0;
}

static_assert(sizeof(jt_hit) == 24, "the query kernel writes a jt_hit as six 32-bit words");

// the host variants' check of instance (NULL: none): every id within -1 .. ninstances-1
static int instance_range_check(const jt_ctx* c, int64_t n, const int32_t* instance) {
    if (!instance) return JT_OK;
    const int64_t ni = (int64_t)c->inst_new.size();
    for (int64_t i = 0; i < n; i++)
        if (instance[i] < -1 || instance[i] >= ni)
            return jt::fail(JT_ERR_INVALID, "instance[" + std::to_string(i) + "] = " + std::to_string(instance[i]) +
                                                " is outside -1 .. " + std::to_string(ni - 1));
    return JT_OK;
}

extern "C" {

int jt_intersect_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_instance, void* d_hits) {
    bool done;
    if (const int st = query_check(c, n, d_rays, "d_rays", d_hits, "d_hits", &done)) return st;
    return done ? JT_OK : query_run(c, n, d_rays, d_instance, d_hits, false);
}

int jt_occluded_device(jt_ctx* c, int64_t n, const void* d_rays, void* d_occluded) {
    bool done;
    if (const int st = query_check(c, n, d_rays, "d_rays", d_occluded, "d_occluded", &done)) return st;
    return done ? JT_OK : query_run(c, n, d_rays, nullptr, d_occluded, true);
}

int jt_intersect(jt_ctx* c, int64_t n, const float* rays, const int32_t* instance, jt_hit* hits) {
    bool done;
    if (const int st = query_check(c, n, rays, "rays", hits, "hits", &done)) return st;
    if (done) return JT_OK;
    if (const int st = instance_range_check(c, n, instance)) return st;
    return query_host(c, n, rays, instance, hits, false);
}

int jt_occluded(jt_ctx* c, int64_t n, const float* rays, uint8_t* occluded) {
    bool done;
    if (const int st = query_check(c, n, rays, "rays", occluded, "occluded", &done)) return st;
    return done ? JT_OK : query_host(c, n, rays, nullptr, occluded, true);
}

// ---- bounded queries: a NULL bound array is the unbounded call itself
int jt_intersect_bounded_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance, void* d_hits) {
    if (!d_tmax) return jt_intersect_device(c, n, d_rays, d_instance, d_hits);
    bool done;
    if (const int st = query_check(c, n, d_rays, "d_rays", d_hits, "d_hits", &done)) return st;
    return done ? JT_OK : query_run(c, n, d_rays, d_instance, d_hits, false, jtq::BOUND_ARRAY, d_tmax);
}

int jt_occluded_bounded_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_tmax, void* d_occluded) {
    if (!d_tmax) return jt_occluded_device(c, n, d_rays, d_occluded);
    bool done;
    if (const int st = query_check(c, n, d_rays, "d_rays", d_occluded, "d_occluded", &done)) return st;
    return done ? JT_OK : query_run(c, n, d_rays, nullptr, d_occluded, true, jtq::BOUND_ARRAY, d_tmax);
}

int jt_visible_device(jt_ctx* c, int64_t n, const void* d_segments, void* d_visible) {
    bool done;
    if (const int st = query_check(c, n, d_segments, "d_segments", d_visible, "d_visible", &done)) return st;
    return done ? JT_OK : query_run(c, n, d_segments, nullptr, d_visible, true, jtq::BOUND_SEGMENT);
}

int jt_intersect_bounded(jt_ctx* c, int64_t n, const float* rays, const float* tmax, const int32_t* instance, jt_hit* hits) {
    if (!tmax) return jt_intersect(c, n, rays, instance, hits);
    bool done;
    if (const int st = query_check(c, n, rays, "rays", hits, "hits", &done)) return st;
    if (done) return JT_OK;
    if (const int st = instance_range_check(c, n, instance)) return st;
    return query_host(c, n, rays, instance, hits, false, jtq::BOUND_ARRAY, tmax);
}

int jt_occluded_bounded(jt_ctx* c, int64_t n, const float* rays, const float* tmax, uint8_t* occluded) {
    if (!tmax) return jt_occluded(c, n, rays, occluded);
    bool done;
    if (const int st = query_check(c, n, rays, "rays", occluded, "occluded", &done)) return st;
    return done ? JT_OK : query_host(c, n, rays, nullptr, occluded, true, jtq::BOUND_ARRAY, tmax);
}

int jt_visible(jt_ctx* c, int64_t n, const float* segments, uint8_t* visible) {
    bool done;
    if (const int st = query_check(c, n, segments, "segments", visible, "visible", &done)) return st;
    return done ? JT_OK : query_host(c, n, segments, nullptr, visible, true, jtq::BOUND_SEGMENT);
}

// ---- ambient occlusion
int jt_ambient_occlusion_device(jt_ctx* c, int64_t n, const void* d_points, int64_t stream_base, int32_t sample_begin,
                                int32_t sample_end, float radius, void* d_visibility) {
    bool done;
    if (const int st = occlusion_check(c, n, d_points, "d_points", stream_base, sample_begin, sample_end, radius, d_visibility,
                                       "d_visibility", true, &done))
        return st;
    return done ? JT_OK : occlusion_run(c, n, d_points, stream_base, sample_begin, sample_end, radius, d_visibility);
}

int jt_ambient_occlusion(jt_ctx* c, int64_t n, const float* points, int64_t stream_base, int32_t sample_begin, int32_t sample_end,
                         float radius, float* visibility) {
    bool done;
    if (const int st = occlusion_check(c, n, points, "points", stream_base, sample_begin, sample_end, radius, visibility, "visibility",
                                       false, &done))
        return st;
    if (done) return JT_OK;
    (void)hipSetDevice(c->device);
    // the points staged in Q_RAYS, the quotients in Q_OUT, whose jt_hit slot has room for one float
    int st;
    if ((st = query_stage(c, n))) return st;
    void* const d_points = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_vis = c->q_grow[jt_ctx::Q_OUT];
    if ((st = copy_in(d_points, points, (size_t)n * 6 * sizeof(float), "hipMemcpy occlusion points")) ||
        (st = occlusion_run(c, n, d_points, stream_base, sample_begin, sample_end, radius, d_vis)))
        return st;
    return copy_out(visibility, d_vis, (size_t)n * sizeof(float), "hipMemcpy occlusion results");
}

}  // extern "C"
