// jt_trace.hip — the C-ABI device context of the MI355X path tracer (include/jtrace.h, jt_ctx in
// jt_context.h): the kernel dispatch, scene upload (the steps of jt_create), the sample queue
// and its launches, the single-device getters. The scene's validation and host layout are in
// jt_layout.cpp (no HIP runtime), the launch plan's integer rules in jt_plan.h, the choice of the
// scene's kernel configuration in jt_select.h (select_kernel), the trace kernels in jt_kernels.h (instantiated by jt_kv.hip, one translation unit per configuration; this unit
// sees only their declarations and the argument records, jt_launch.h), the
// combine and chain kernels in jt_accum.hip, the multi-device context in jt_multi.hip, and the
// denoiser's, the error estimate's and adaptive sampling's entry points beside their kernels
// (jt_denoise.hip, jt_error.hip, jt_adapt.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "jt_accum.h"
#include "jt_context.h"
#include "jt_layout.h"
#include "jt_radiance.h"

using namespace jtd;
using namespace jtk;
using namespace jtc;

namespace {
// The launch functions of every configuration (jt_kv.hip compiles each in its own translation
// unit), indexed [KernelChoice::id] and then [adapted][sampler - 1][counter level]; adapted: the
// context has a frozen-tile mask (DAccum::frozen set)
using LaunchFn = hipError_t (*)(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int);
struct LaunchRow {
    LaunchFn fn[2][2][2];
};
template <int ID, bool... ADAPT>
constexpr LaunchRow launch_row(std::integer_sequence<bool, ADAPT...>) {
    return {{{{launch_cfg<ID, 1, 0, ADAPT>, launch_cfg<ID, 1, 1, ADAPT>}, {launch_cfg<ID, 2, 0, ADAPT>, launch_cfg<ID, 2, 1, ADAPT>}}...}};
}
template <int... ID>
constexpr std::array<LaunchRow, sizeof...(ID)> launch_table(std::integer_sequence<int, ID...>) {
    return {{launch_row<ID>(std::integer_sequence<bool, false, true>{})...}};
}
constexpr auto LAUNCH = launch_table(std::make_integer_sequence<int, NUM_LAUNCH_CONFIGS>{});
}  // namespace

int jtc::hip_fail(hipError_t e, const char* what) {
    return jt::fail(JT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
int jtc::device_alloc(jt_ctx* c, size_t bytes, const char* what, void** p) {
    *p = nullptr;
    if (hipMalloc(p, bytes) != hipSuccess) return jt::fail(JT_ERR_NOMEM, std::string("hipMalloc ") + what);
    c->allocations.push_back(*p);
    return JT_OK;
}

namespace {

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

// ------------------------------------------------------------------------ the steps of jt_create
// A scene ready for upload: its host layout (jt_layout.h) and the kernel it runs (jt_select.h)
struct PreparedScene {
    jt::HostScene hs;
    KernelChoice choice;
};

// the options that bear on the kernel choice, as select_kernel's integer inputs
void select_options(const jt::Options& opts, SelectIn& in) {
    if (const char* v = jt::opt(opts, "lds_scene")) in.lds_scene = (size_t)std::atoll(v);
    if (const char* r = jt::opt(opts, "lds_stack")) in.lds_stack = std::atoi(r) > 16 ? 32 : 16;
    if (const char* r = jt::opt(opts, "test_lds_ring")) in.test_lds_ring = std::atoi(r);
    if (const char* wl = jt::opt(opts, "wait_lanes")) in.wait_lanes = given_lanes(std::atoi(wl), 64);
    if (const char* ll = jt::opt(opts, "light_lanes")) in.light_lanes = given_lanes(std::atoi(ll), 65);
}

// Host only: the layout and the kernel choice, with the wide records when it is a wide kernel.
int prepare_scene(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                  const jt::Options& opts, PreparedScene& ps) {
    jt::HostScene& hs = ps.hs;
    int st = jt::layout_scene(scene, bvh, lights, params, opts, hs);
    if (st != JT_OK) return st;
    SelectIn in;
    in.feat = hs.feat;
    in.need = hs.need;
    in.blob_bytes = hs.blob.size() * 16;
    in.inst_light = hs.inst_light;
    in.light_inline = hs.S.light_inline != 0;
    in.traversal = params->traversal;
    in.sampler = params->sampler;
    select_options(opts, in);
    ps.choice = select_kernel(in);
    // JT_TRAVERSAL_AUTO resolved to wide (HBM mode): the wide records (the binary nodes stay
    // uploaded, unused); the instances' BLAS roots become root records
    if (ps.choice.wide && !hs.wide && (st = jt::make_wide(hs, scene, bvh)) != JT_OK) return st;
    assert(ps.choice.wide == hs.wide);
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
    if (ps.choice.lds_scene_bytes) {
        if ((st = upload(c, hs.blob, &S.blob)) != JT_OK) return st;
        S.blob_n16 = (int)hs.blob.size();
    }
    return JT_OK;
}

// the stack members of the device scene and, for a bound above the LDS ring, its HBM overflow
int alloc_stack_overflow(jt_ctx* c) {
    DScene& S = c->S;
    const int need = c->choice.stack_need;
    S.ovf = nullptr;
    S.ovf_stride = 0;
    S.ring = c->choice.ring_used;
    S.stack_need = need;
    if (c->choice.ovf) {  // HBM overflow of the LDS stack ring: `need` entries per lane of the
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

// DParams: camera, tile share, sample streams, the kernel choice's wait lanes and light lanes.
// forced_streams: the option "streams" set the stream count
int make_params(jt_ctx* c, const jt_scene* scene, const jt_params* params, const jt::Options& opts, bool& forced_streams) {
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
    P.tile_stride_rcp = tile_stride_rcp(P.tile_stride);
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
    P.wait_lanes = c->choice.wait_lanes;
    P.light_lanes = c->choice.light_lanes;
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
    if (c->tiles >= (1 << 20))  // an item's slot: the float quotient of its tile (item_slot, jt_plan.h)
        return jt::fail(JT_ERR_UNSUPPORTED, "image above 2^20 8x8 tiles (67 Mpixels)");
    if (W > JT_ITEM_MAX_DIM || H > JT_ITEM_MAX_DIM)  // the per-lane work items hold a pixel as (j << 16) | i
        return jt::fail(JT_ERR_UNSUPPORTED, "image wider or higher than 32768 pixels");
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
    if (c->multi) return multi_destroy(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (void* p : c->allocations) (void)hipFree(p);
    query_free(c);
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
    // option test_trace_chunk (tests only): a cap on a one-stream context's chunk (ensure_chunk), a
    // power of two in [1, 64] (chunk_cap, jt_plan.h); 1: no chunks, as when their buffers fail
    int trace_chunk = 0;
    if (const char* tc = jt::opt(opts, "test_trace_chunk"))
        if (!(trace_chunk = chunk_cap(std::atoll(tc))))
            return jt::fail(JT_ERR_INVALID, "option test_trace_chunk: not a power of two in [1, 64]");

    hipError_t e = hipSetDevice(params->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    jt_ctx* c = new jt_ctx();
    c->device = params->device;
    c->width = ps.hs.width;
    c->height = ps.hs.height;
    c->total_samples = params->samples;
    c->batch = params->batch;
    c->sampler = params->sampler;
    c->choice = ps.choice;
    c->env_alias = ps.hs.env_alias;
    c->inst_new = ps.hs.inst_new;  // the ray queries' instance numbering (jt_intersect.hip)
    c->inst_nelem.resize((size_t)scene->ninstances);  // and the surface calls' element ranges (jt_surface.hip)
    for (int k = 0; k < scene->ninstances; k++) {
        const jt_shape& sh = scene->shapes[scene->instances[k].shape];
        c->inst_nelem[(size_t)k] = sh.ntriangles ? sh.ntriangles : sh.nquads;  // flatten_shape's kind
    }
    // option test_probe_chunk (tests only): the points of a chunk of jt_probe_sh's host variant
    if (const char* pc = jt::opt(opts, "test_probe_chunk")) c->probe_chunk = jtr::probe_chunk(std::atoll(pc));
    // option test_multi_chunk (tests only): the rays of a chunk of jt_intersect_multi's host variant
    if (const char* mc = jt::opt(opts, "test_multi_chunk")) c->multi_chunk = std::atoll(mc);
    c->trace_chunk = trace_chunk;
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
    if ((st = upload_scene(c, ps)) || (st = alloc_stack_overflow(c)) ||
        (st = make_params(c, scene, params, opts, forced_streams)) ||
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
    const size_t blob_n16 = ps.choice.lds_scene_bytes ? hs.blob.size() : 0;
    item("blob", blob_n16, hs.blob.data(), blob_n16 * 16);
    std::snprintf(line, sizeof line,
                  "scalars need=%d feat=%d traversal=%d tlas_nnodes=%d tlas_wnodes=%d order_flip=%d light_inline=%d "
                  "o_nodes=%d o_wnodes=%d o_prims=%d o_inst_trav=%d o_inst_blas=%d o_inst_shade=%d o_shapes=%d o_pos=%d o_nrm=%d "
                  "o_tc=%d o_col=%d o_elems=%d o_enrm=%d o_enrm_id=%d o_materials=%d o_lights=%d o_cdf=%d o_light_hit=%d "
                  "o_light_elems=%d blob_n16=%d\n",
                  hs.need, hs.feat, ps.choice.traversal, S.tlas_nnodes, S.tlas_wnodes, S.order_flip, S.light_inline, S.o_nodes, S.o_wnodes,
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

}  // extern "C"

namespace jtc {
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
int finish_aovs(jt_ctx* c) {
    if (!c->aov_pending) return JT_OK;
    (void)hipSetDevice(c->device);
    hipError_t e = jt::combine_launch(c->stream, c->P, c->A, c->last_cw, true);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->failed = true;
        return hip_fail(e, "AOV combine");
    }
    c->aov_pending = false;
    return JT_OK;
}
}  // namespace jtc

extern "C" int jt_reset(jt_ctx* c) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    c->denoised = false;
    c->err_valid = false;
    if (c->multi) return multi_reset(c);
    (void)hipSetDevice(c->device);
    hipError_t e;
    // a failed flush may have left chains queued on stream2 (a complete one ends on `stream`)
    if (c->stream2 && (e = hipStreamSynchronize(c->stream2)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    if ((e = hipMemsetAsync(c->A.counters, 0, 256, c->stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    // adaptive sampling (jt_adapt): every tile is active again; the mask's buffer is kept
    if (c->frozen_at) {
        if ((e = hipMemsetAsync(c->frozen_at, 0, (size_t)c->tiles * sizeof(unsigned), c->stream)) != hipSuccess)
            return hip_fail(e, "hipMemsetAsync");
        c->adapt_active = launch_tiles(c->P);
    }
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

namespace {
// the chunk buffers of a one-stream context (chunk_samples, jt_plan.h), allocated at the first
// multi-sample range, the chunk halved on NOMEM. jt_ctx::chunk: 0 after jt_create (none yet), 1:
// none possible (the range then runs as one launch of long items). The option test_trace_chunk
// (tests only, jt_ctx::trace_chunk) lowers the size chunk_samples gives; at 1 it takes the path of
// a second stream, an event or an allocation that failed.
int ensure_chunk(jt_ctx* c) {
    if (c->chunk) return JT_OK;
    const long long nslot = (long long)launch_tiles(c->P) * 64;
    int m = chunk_samples(nslot);
    if (c->trace_chunk && c->trace_chunk < m) m = c->trace_chunk;  // option test_trace_chunk: lowers it only
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
    const LaunchFn fn = LAUNCH[c->choice.id].fn[A.frozen != nullptr][c->sampler == JT_SAMPLER_NAIVE ? 1 : 0][c->count ? 1 : 0];
    e = fn(c->S, P, s0, s1, A, c->stream, c->cus);
    if (e != hipSuccess) return hip_fail(e, "trace kernel launch");
    return JT_OK;
}
}  // namespace

namespace jtc {
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
    int launches = 0;
    if (c->lk == 0 && s1 - s0 > 1 && ensure_chunk(c) == JT_OK && c->chunk > 1) {
        // chunk i traces into buffer set i & 1 on `stream`; its chain runs on `stream2` after that
        // trace and after chain i - 1 (stream order), overlapping trace i + 1; trace i + 2 reuses
        // the set once chain i has read it. `stream` then waits for the last chain (ev1 covers it).
        // Which samples, which stream count and which set: chunk_plan (jt_plan.h). A one-sample
        // tail goes through the chunk buffers like every other chunk (lk >= 1) rather than as a plain
        // lk == 0 launch behind a wait for the last chain: one code path and one launch shape, and
        // no launch that stores into the running mean while a chain is writing it.
        const int nchunk = chunk_count(s0, s1, c->chunk);
        for (int i = 0; i < nchunk; i++) {
            const ChunkPlan cp = chunk_plan(s0, s1, c->chunk, i);
            const int32_t x = cp.x, y = cp.y;
            const int set = cp.set;
            DParams P = c->P;  // the chunk's samples as one-sample streams x .. y-1
            P.first = x;
            P.lk = cp.lk;
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
            if ((e = jt::chain_launch(c->stream2, c->P, A, x - first, y - x)) != hipSuccess)
                return hip_fail(e, "chain kernel launch");
            if ((e = hipEventRecord(c->chain_done[set], c->stream2)) != hipSuccess) return hip_fail(e, "hipEventRecord");
            launches++;
        }
        if ((e = hipStreamWaitEvent(c->stream, c->chain_done[(nchunk - 1) & 1], 0)) != hipSuccess)
            return hip_fail(e, "hipStreamWaitEvent");
    } else {
        c->P.first = first;
        if (const int st = launch_range(c, c->P, c->A, s0, s1)) return st;
        launches = 1;
        if (c->lk > 0) {
            // the streams' weights after this launch: n = s1 - first local samples
            DCombine cw;
            combine_weights((long long)s1 - first, c->lk, cw);
            if ((e = jt::combine_launch(c->stream, c->P, c->A, cw, false)) != hipSuccess)
                return hip_fail(e, "combine kernel launch");
            c->aov_pending = tiles > 0;
            c->last_cw = cw;
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

// trace the deferred samples [pend0, pend1) (jt_ctx) and wait for them; every call that reads
// the context's results or device buffers runs this first
int flush(jt_ctx* c) {
    if (c->pend1 <= c->pend0) return JT_OK;
    const int32_t s0 = c->pend0, s1 = c->pend1;
    c->pend0 = c->pend1 = 0;
    if (c->multi) return multi_trace_range(c, s0, s1);
    int st = trace_launch(c, s0, s1, c->first);
    float ms = 0;
    if (st == JT_OK) st = trace_finish(c, &ms);
    if (st != JT_OK) c->failed = true;
    return st;
}
}  // namespace jtc

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
    if (c->exported || c->pend1 - c->pend0 >= JT_DEFER_SAMPLES || c->next >= c->total_samples) return flush(c);
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
    *streams = 1 << c->lk;
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
    if (c->multi) return multi_get_image(c, rgba);
    if (const int st = zero_if_stale(c)) return st;
    (void)hipSetDevice(c->device);
    hipError_t e = hipMemcpy(rgba, c->A.image, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipMemcpy image");
}

int jt_get_aovs(jt_ctx* c, float* albedo, float* normal, int64_t* hits) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (const int st = flush(c)) return st;
    if (c->failed) return jt::fail(JT_ERR_STATE, "the running means are corrupt (a launch failed); jt_reset the context");
    if (c->multi) return multi_get_aovs(c, albedo, normal, hits);
    if (const int st = zero_if_stale(c)) return st;
    if (const int st = finish_aovs(c)) return st;
    (void)hipSetDevice(c->device);
    const size_t np = (size_t)c->width * c->height;
    std::vector<float4> tmp(np);
    hipError_t e;
    if (albedo) {
        if ((e = hipMemcpy(tmp.data(), c->A.albedo, np * 16, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy");
        unpack3(tmp, albedo);
    }
    if (normal) {
        if ((e = hipMemcpy(tmp.data(), c->A.normal, np * 16, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy");
        unpack3(tmp, normal);
    }
    if (hits && (e = hipMemcpy(hits, c->A.hits, np * 8, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy");
    return JT_OK;
}

int jt_get_counters(jt_ctx* c, jt_counters* out) {
    if (!c || !out) return jt::fail(JT_ERR_INVALID, "NULL argument");
    if (const int st = flush(c)) return st;
    if (c->multi) return multi_get_counters(c, out);
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
    if (c->multi) return multi_get_device_buffers(c, out);
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
    if (c->multi) return multi_describe(c, buf, n);
    const KernelChoice& k = c->choice;
    // test-only options in effect (jt_set_option): a tile filter, a shortened LDS ring
    char filt[96] = "";
    if (c->P.tile_stride != 1 || k.ring_shortened())
        std::snprintf(filt, sizeof filt, " tile_filter=%d/%d ring_used=%d", c->P.tile_offset, c->P.tile_stride, c->S.ring);
    // adaptive sampling, once jt_adapt has run: the traced tiles still active / the traced tiles
    char adaptive[48] = "";
    if (c->adapted) std::snprintf(adaptive, sizeof adaptive, " adaptive=%d/%d", c->adapt_active, launch_tiles(c->P));
    char tmp[704];
    std::snprintf(tmp, sizeof tmp,
                  "kernel=%s<%d,%d,%s,%d,%d,%s> mode=%s scene_lds_bytes=%zu stack_bound=%d lds_ring=%d hbm_overflow=%d "
                  "wait_lanes=%d light_lanes=%d streams=%d tiles=%d block=%d env_alias=%d light_inline=%d "
                  "traversal=%s%s%s",
                  k.lds_scene_bytes ? "trace_kernel_lds" : "trace_kernel", c->sampler == JT_SAMPLER_NAIVE ? 2 : 1,
                  k.ring, k.ovf ? "true" : "false", c->count, k.kmask, k.wide ? "true" : "false",
                  k.lds_scene_bytes ? "lds" : "hbm", k.lds_scene_bytes,
                  k.stack, k.ring, k.ovf ? 1 : 0, c->P.wait_lanes, c->P.light_lanes, 1 << c->lk, c->tiles, BLOCK,
                  c->env_alias ? 1 : 0, c->S.light_inline,
                  k.traversal == JT_TRAVERSAL_REFERENCE ? "reference" : k.traversal == JT_TRAVERSAL_NEAR ? "near" : "wide",
                  filt, adaptive);
    std::snprintf(buf, (size_t)n, "%s", tmp);
    return JT_OK;
}

int jt_set_counters(jt_ctx* c, int32_t level) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (level != 0 && level != 1) return jt::fail(JT_ERR_INVALID, "counter level must be 0 or 1");
    if (const int st = flush(c)) return st;  // queued samples are traced at the level they were queued at
    if (c->multi) return multi_set_counters(c, level);
    c->count = level;
    return JT_OK;
}

int jt_synchronize(jt_ctx* c) {
    if (!c) return jt::fail(JT_ERR_INVALID, "ctx is NULL");
    if (const int st = flush(c)) return st;
    if (c->multi) return multi_synchronize(c);
    if (const int st = finish_aovs(c)) return st;
    (void)hipSetDevice(c->device);
    hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? JT_OK : hip_fail(e, "hipStreamSynchronize");
}

}  // extern "C"
