// jt_multihit.hip — all hits along a ray (include/jtrace.h: jt_intersect_multi, jt_count_hits and
// their device-pointer variants): the ray queries' traversal (jt_traverse.h) and
// persistent grid (jt_feed.h) with another accept rule in the primitive step. Where the closest-hit
// query keeps "the closest so far" in the lane, this one keeps the k smallest keys (t, instance,
// element) so far, sorted, and the query's tmax is the k-th entry's t once the list is full
// (jt_multihit.h holds the list's rules, which the host checks).
//
// Per lane the loop is query_loop's (jt_intersect.hip):
//     query_start<WIDE>, T.tmax = the ray's bound; until query_done<WIDE>: multi_prim_step if
//     nprim > 0, else node_step_any; then the count and the padding are written
// with no tie re-run: among the primitives a traversal tests the list does not depend on the order
// in which they are tested (the ids decide an equal t).
//
// The list lives in the ray's own output records, hits + ray * k: a lane owns its ray for the whole
// query and is the only one that reads or writes them, with plain loads and stores; the count and
// the current tmax stay in registers. No LDS beside the 16 KiB stack ring, which already sets the
// workgroups per compute unit. hit_count (jt_traverse.h) runs at every change of T.tmax: the node
// step's child pre-test snapshots are valid only while T.nh counts them all.
//
// jt_count_hits (COUNT): no list and nothing shrinks; every accepted primitive adds one.
#include <hip/hip_runtime.h>

#include <string>

#include "jt_context.h"
#include "jt_feed.h"
#include "jt_multihit.h"
#include "jt_traverse.h"

static_assert(jtm::MULTI_MAX_HITS == JT_MULTI_MAX_HITS, "jt_multihit.h restates the header's constant");
static_assert(sizeof(jt_hit) == sizeof(jtm::MultiRec) && sizeof(jt_hit) == 24, "a list entry is a jt_hit: three 8-byte words");

namespace jtk {

using jtq::QUERY_VOTE_P;
using jtq::QUERY_RING;

struct DMulti {
    const float* rays;   // n x (o, d)
    const float* tmax;   // nullptr (+inf), or per ray the bound
    const int* inst;     // nullptr, or per ray -1 / an instance id in the caller's numbering
    int2* hits;          // n x k jt_hit records as three 8-byte words each (COUNT: unused)
    int* counts;         // n
    const int* to_dev;   // the caller's instance id -> the device's (TLAS leaf order)
    const int* to_ref;   // and back
    int ninst;
    int k;
    DFeed feed;          // the n rays' hand-out
};

constexpr int M_BAD_INSTANCE = -2;
// the device instance of ray `ray`'s query: -1 a scene query, M_BAD_INSTANCE an id out of range
__device__ __forceinline__ int multi_instance(const DMulti& Q, int ray) {
    if (!Q.inst) return -1;
    const int id = Q.inst[ray];
    if (id == -1) return -1;
    return id >= 0 && id < Q.ninst ? Q.to_dev[id] : M_BAD_INSTANCE;
}

// a ray's list: records [0, k) at hits + ray * k, read and written by the ray's lane alone
struct RayList {
    int2* rec;
    __device__ __forceinline__ jtm::MultiRec load(int j) const {
        const int2 a = rec[3 * j], b = rec[3 * j + 1], c = rec[3 * j + 2];
        return jtm::MultiRec{a.x, a.y, __int_as_float(b.x), __int_as_float(b.y), __int_as_float(c.x), c.y};
    }
    __device__ __forceinline__ void store(int j, const jtm::MultiRec& r) const {
        rec[3 * j] = make_int2(r.inst, r.elem);
        rec[3 * j + 1] = make_int2(__float_as_int(r.u), __float_as_int(r.v));
        rec[3 * j + 2] = make_int2(__float_as_int(r.t), r.hit);
    }
};
__device__ __forceinline__ RayList ray_list(const DMulti& Q, int ray) { return RayList{Q.hits + (size_t)ray * (size_t)Q.k * 3}; }

// the query ends: the count, and the miss record in every slot the list does not fill
template <bool COUNT>
__device__ __forceinline__ void multi_finish(const DMulti& Q, int ray, int count) {
    Q.counts[ray] = count;
    if constexpr (!COUNT) {
        const RayList L = ray_list(Q, ray);
        for (int j = count; j < Q.k; j++) L.store(j, jtm::multi_miss());
    }
}

// A primitive of the current leaf accepted at the current tmax (ray_eps <= t <= T.tmax).
// COUNT: one more. Else the candidate meets the ray's list (multi_insert, jt_multihit.h); where that
// leaves a full list, tmax becomes its last entry's t and the change is counted.
template <bool COUNT>
__device__ __forceinline__ void multi_accept(const DMulti& Q, Trav& T, int ray, int& count, const PrimHit& p, int elem) {
    if constexpr (COUNT) {
        count += 1;
    } else {
        RayList L = ray_list(Q, ray);
        float last;
        const int pos = jtm::multi_insert(L, Q.k, count, jtm::MultiRec{Q.to_ref[T.cur_inst], elem, p.u, p.v, p.t, 1}, &last);
        count = jtm::multi_count_after(Q.k, count, pos);
        if (pos < Q.k && count == Q.k) {
            const float tm = jtm::multi_tmax_after(Q.k, count, pos, last, T.tmax);
            hit_count(T, tm);
            T.tmax = tm;
        }
    }
}

// prim_step's tests (jt_traverse.h) with multi_accept in place of "the closest so far": the current
// leaf's next primitives in order, each against the tmax the one before it left. Triangles come from
// the 80-byte pair records, both tests of a pair computed side by side; k is 0 or 2.
template <bool COUNT>
__device__ __forceinline__ void multi_tri_pair(const DScene& S, const DMulti& Q, Trav& T, int ray, int& count, int k) {
    const float4* r = S.prims + 5 * (T.prim + (k >> 1));
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    const PrimHit p1 = intersect_triangle_pre(T.lo, T.ld, ray_eps, V3(r0.x, r0.z, r1.x), V3(r1.z, r2.x, r2.z),
                                              V3(r3.x, r3.z, r4.x));
    const PrimHit p2 = intersect_triangle_pre(T.lo, T.ld, ray_eps, V3(r0.y, r0.w, r1.y), V3(r1.w, r2.y, r2.w),
                                              V3(r3.y, r3.w, r4.y));
    if (tri_hit_before(p1, T.tmax)) multi_accept<COUNT>(Q, T, ray, count, p1, __float_as_int(r4.z));
    if (T.nprim >= k + 2 && tri_hit_before(p2, T.tmax)) multi_accept<COUNT>(Q, T, ray, count, p2, __float_as_int(r4.w));
}
template <bool COUNT, int F>
__device__ __forceinline__ void multi_prim_step(const DScene& S, const DMulti& Q, Trav& T, int ray, int& count) {
    if (!(F & FT_QUAD) || T.cur_kind == KIND_TRI) {
        multi_tri_pair<COUNT>(S, Q, T, ray, count, 0);
        const bool more = T.nprim > 2;
        if (__builtin_amdgcn_ballot_w64(more)) {
            if (more) multi_tri_pair<COUNT>(S, Q, T, ray, count, 2);
        }
        const int n = T.nprim < 4 ? T.nprim : 4;
        T.prim += 2;  // pair records
        T.nprim -= n;
        return;
    }
    const float4* r = S.prims + 4 * T.prim;
    const float4 a = r[0], b = r[1], c = r[2], d = r[3];
    const PrimHit p = intersect_quad(T.lo, T.ld, ray_eps, T.tmax, xyz(a), xyz(b), xyz(c), xyz(d), d.w != 0.0f);
    if (p.hit) multi_accept<COUNT>(Q, T, ray, count, p, __float_as_int(a.w));
    T.prim += 1;
    T.nprim -= 1;
}

// the lane starts ray `ray`'s query; false: its instance id is out of range, an empty list is recorded
template <bool WIDE, bool COUNT>
__device__ __forceinline__ bool multi_take(const DScene& S, const DMulti& Q, Trav& T, int ray, int* stack) {
    const int q = multi_instance(Q, ray);
    if (q == M_BAD_INSTANCE) {
        multi_finish<COUNT>(Q, ray, 0);
        return false;
    }
    const float* const r = Q.rays + (size_t)ray * 6;
    query_start<WIDE>(S, T, V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5]), q, stack);
    T.tmax = Q.tmax ? Q.tmax[ray] : __builtin_inff();
    return true;
}

template <bool WIDE, bool OVF, bool COUNT>
__global__ __launch_bounds__(BLOCK) void multi_kernel(DScene S, DMulti Q) {
    constexpr int F = FT_ALL;
    __shared__ int ring[QUERY_RING * BLOCK];
    int* const stack = ring + threadIdx.x;
    const int slot = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // the lane's HBM stack-overflow area
    Counters cnt{0, 0, 0, 0};
    Trav T;
    int ray = -1;   // the lane's ray; -1: none
    int count = 0;  // entries of its list (COUNT: candidates so far)
    jtq::WaveReserve reserve;
    // ---- refill (jt_feed.h): a lane without a ray takes one of the wave's reserve
    while (feed_refill(Q.feed, reserve, ray >= 0, [&](int r) {
        if (multi_take<WIDE, COUNT>(S, Q, T, r, stack)) {
            ray = r;
            count = 0;
        }
    })) {
        // ---- one step kind per iteration, by query_loop's biased lane vote
        const bool wantp = ray >= 0 && T.nprim > 0, wantn = ray >= 0 && T.nprim == 0;
        const int np = __popcll(__builtin_amdgcn_ballot_w64(wantp)), nn = __popcll(__builtin_amdgcn_ballot_w64(wantn));
        if (np * QUERY_VOTE_P >= nn) {
            if (wantp) multi_prim_step<COUNT, F>(S, Q, T, ray, count);
        } else {
            if (wantn) node_step_any<WIDE, QUERY_RING, OVF, 0, true, F>(S, T, stack, slot, cnt);
        }
        // ---- a lane whose query has ended records it
        if (ray >= 0 && query_done<WIDE>(T)) {
            multi_finish<COUNT>(Q, ray, count);
            ray = -1;
        }
    }
}

}  // namespace jtk

// ---- the context's half (jt_context.h)
using namespace jtc;
using jtd::DScene;

namespace {

constexpr int BLOCK = jtk::BLOCK;
constexpr const char* MULTI_CTX =
    "ray queries are not available on a multi-device context (jt_create_multi): query one context per device";

// the checks of the four entry points, in jt_intersect_bounded's order with k after n; hits NULL
// with count_only. *done: n == 0, nothing to do
int multi_check(const jt_ctx* c, int64_t n, const void* rays, const char* rays_name, bool count_only, int32_t k, const void* hits,
                const char* hits_name, const void* counts, const char* counts_name, bool device, bool* done) {
    const char* range = jtq::query_count_error(n, "n must be at most 2^30 rays");
    if (!range && !count_only) range = jtm::multi_k_error(n, k);
    const char* misaligned = !device                                    ? nullptr
                             : !count_only && ((uintptr_t)hits & 7)     ? "d_hits must be aligned to 8 bytes"
                             : ((uintptr_t)counts & 3)                  ? "d_counts must be aligned to 4 bytes"
                                                                        : nullptr;
    if (count_only) return ray_call_check(c, {{rays, rays_name}, {counts, counts_name}}, range, misaligned, MULTI_CTX, n == 0, done);
    return ray_call_check(c, {{rays, rays_name}, {hits, hits_name}, {counts, counts_name}}, range, misaligned, MULTI_CTX, n == 0, done);
}

// n >= 1 rays from device pointers, on the context's stream; returns once the stream is idle.
// d_hits nullptr: jt_count_hits
int multi_run(jt_ctx* c, int64_t n, const void* d_rays, const void* d_tmax, const void* d_inst, int32_t k, void* d_hits, void* d_counts) {
    (void)hipSetDevice(c->device);
    int st = query_setup(c);
    if (st != JT_OK) return st;
    const int grid = jtq::query_grid(n, c->cus);
    DScene S;
    bool ovf;
    if ((st = query_scene(c, grid, &S, &ovf)) != JT_OK) return st;
    const bool count_only = d_hits == nullptr;
    jtk::DMulti Q{};
    Q.rays = (const float*)d_rays;
    Q.tmax = (const float*)d_tmax;
    Q.inst = (const int*)d_inst;
    Q.hits = (int2*)d_hits;
    Q.counts = (int*)d_counts;
    Q.to_dev = c->q_to_dev;
    Q.to_ref = c->q_to_ref;
    Q.ninst = (int)c->inst_new.size();
    Q.k = count_only ? 0 : k;
    Q.feed = {c->q_counter, (int)n, (unsigned)jtq::query_claim_rays(n, grid)};
    const hipError_t e = hipMemsetAsync(c->q_counter, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync multi-hit ray counter");
    with_bools(c->choice.wide, ovf, count_only, [&](auto wide, auto over, auto count) {
        hipLaunchKernelGGL((jtk::multi_kernel<wide(), over(), count()>), dim3((unsigned)grid), dim3(BLOCK), 0, c->stream, S, Q);
    });
    return launch_finish(c, count_only ? "hit count kernel" : "multi-hit kernel");
}

// the host variants' check of instance (NULL: none): every id within -1 .. ninstances-1
int multi_instance_check(const jt_ctx* c, int64_t n, const int32_t* instance) {
    if (!instance) return JT_OK;
    const int64_t ni = (int64_t)c->inst_new.size();
    for (int64_t i = 0; i < n; i++)
        if (instance[i] < -1 || instance[i] >= ni)
            return jt::fail(JT_ERR_INVALID, "instance[" + std::to_string(i) + "] = " + std::to_string(instance[i]) +
                                                " is outside -1 .. " + std::to_string(ni - 1));
    return JT_OK;
}

// The host variants: chunks of at most `chunk` rays staged in the ray queries' buffers (the counts
// in Q_OUT, whose 24-byte slot per ray has room for one), a chunk's records in Q_MULTI, grown to
// chunk * k. A ray's result does not depend on the other rays of its launch, so the chunks give the
// bits of one call. hits nullptr: jt_count_hits, one chunk.
int multi_host(jt_ctx* c, int64_t n, const float* rays, const float* tmax, const int32_t* instance, int32_t k, jt_hit* hits,
               int32_t* counts) {
    (void)hipSetDevice(c->device);
    const int64_t most = hits ? jtm::multi_chunk(k, c->multi_chunk) : n;
    const int64_t chunk = n < most ? n : most;
    int st;
    if ((st = query_stage(c, chunk))) return st;
    if (hits && chunk * k > c->q_stage_multi) {
        const size_t cap = (size_t)jtq::query_stage_rays(c->q_stage_multi, chunk * k);
        c->q_stage_multi = 0;
        if ((st = query_grow(c, jt_ctx::Q_MULTI, cap * sizeof(jt_hit), "multi-hit records"))) return st;
        c->q_stage_multi = (long long)cap;
    }
    void* const d_rays = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_inst = instance ? c->q_grow[jt_ctx::Q_INST] : nullptr;
    void* const d_tmax = tmax ? c->q_grow[jt_ctx::Q_TMAX] : nullptr;
    void* const d_counts = c->q_grow[jt_ctx::Q_OUT];
    void* const d_hits = hits ? c->q_grow[jt_ctx::Q_MULTI] : nullptr;
    for (int64_t at = 0; at < n; at += chunk) {
        const size_t m = (size_t)(n - at < chunk ? n - at : chunk);
        if ((st = copy_in(d_rays, rays + (size_t)at * 6, m * 6 * sizeof(float), "hipMemcpy multi-hit rays")) ||
            (instance && (st = copy_in(d_inst, instance + at, m * sizeof(int32_t), "hipMemcpy multi-hit instance ids"))) ||
            (tmax && (st = copy_in(d_tmax, tmax + at, m * sizeof(float), "hipMemcpy multi-hit bounds"))) ||
            (st = multi_run(c, (int64_t)m, d_rays, d_tmax, d_inst, k, d_hits, d_counts)) ||
            (hits && (st = copy_out(hits + (size_t)at * (size_t)k, d_hits, m * (size_t)k * sizeof(jt_hit), "hipMemcpy multi-hit records"))) ||
            (st = copy_out(counts + at, d_counts, m * sizeof(int32_t), "hipMemcpy multi-hit counts")))
            return st;
    }
    return JT_OK;
}

}  // namespace

extern "C" {

int jt_intersect_multi_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance, int32_t k,
                              void* d_hits, void* d_counts) {
    bool done;
    if (const int st = multi_check(c, n, d_rays, "d_rays", false, k, d_hits, "d_hits", d_counts, "d_counts", true, &done)) return st;
    return done ? JT_OK : multi_run(c, n, d_rays, d_tmax, d_instance, k, d_hits, d_counts);
}

int jt_count_hits_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance, void* d_counts) {
    bool done;
    if (const int st = multi_check(c, n, d_rays, "d_rays", true, 0, nullptr, "", d_counts, "d_counts", true, &done)) return st;
    return done ? JT_OK : multi_run(c, n, d_rays, d_tmax, d_instance, 0, nullptr, d_counts);
}

int jt_intersect_multi(jt_ctx* c, int64_t n, const float* rays, const float* tmax, const int32_t* instance, int32_t k, jt_hit* hits,
                       int32_t* counts) {
    bool done;
    if (const int st = multi_check(c, n, rays, "rays", false, k, hits, "hits", counts, "counts", false, &done)) return st;
    if (done) return JT_OK;
    if (const int st = multi_instance_check(c, n, instance)) return st;
    return multi_host(c, n, rays, tmax, instance, k, hits, counts);
}

int jt_count_hits(jt_ctx* c, int64_t n, const float* rays, const float* tmax, const int32_t* instance, int32_t* counts) {
    bool done;
    if (const int st = multi_check(c, n, rays, "rays", true, 0, nullptr, "", counts, "counts", false, &done)) return st;
    if (done) return JT_OK;
    if (const int st = multi_instance_check(c, n, instance)) return st;
    return multi_host(c, n, rays, tmax, instance, 0, nullptr, counts);
}

}  // extern "C"
