// jt_surface.hip — the surface at a hit and the camera's rays (include/jtrace.h: jt_eval_hits,
// jt_camera_rays, jt_gbuffer and their device-pointer variants; DESIGN.md §6f "The surface at a
// hit"): the megakernel's own scene evaluation (jt_scene_eval.h) and camera (jt_integrator.h) for
// the caller's records.
//
// surface_kernel: one record per thread on a plain grid — an evaluation's cost is near uniform,
// unlike a query's, so no persistent grid and no refill. The scene is the context's HBM copy
// (every array of JT_SCENE_ARRAYS is uploaded in both scene modes, as for the ray queries), the
// feature mask the general one. A record is checked against the scene's ranges before anything it
// names is loaded: the instance id against the instance count, the element against the element
// count of that instance's shape (jt_ctx::inst_nelem), u and v for finiteness. Whatever a
// device-pointer caller passes, the loads stay inside the scene's arrays; a record that fails is a
// miss record. A lane writes its 24 words as six 16-byte stores.
// camera_kernel: one pixel per thread; start_path's own prologue (camera_sample) for a sample
// index, eval_camera at the pixel centre for -1.
// jt_gbuffer is the three launches camera_kernel, query_kernel (jt_intersect.hip),
// surface_kernel in stream order: a lane's query ends at its own time, so an evaluation inlined in
// the query loop's epilogue would run with a few lanes active, hundreds of times per wave, and add
// its registers to that kernel's.
// From jt_intersect.hip (jt_context.h): the argument checks (ray_call_check), the launch tail
// (launch_finish), the staging buffers and copies (query_stage, query_grow, copy_in, copy_out) and
// the first call's uploads (query_setup).
#include <hip/hip_runtime.h>

#include "jt_context.h"
#include "jt_integrator.h"
#include "jt_intersect.h"

namespace jtk {

struct DSurf {
    const float* rays;  // n x (o, d): the direction is read
    const int* hits;    // n jt_hit records, 6 words each
    float4* out;        // n jt_surface records, 6 float4 each
    const int* to_dev;  // the caller's instance id -> the device's
    const int* nelem;   // the caller's instance id -> the elements of its shape
    int n, ninst;
};

__device__ __forceinline__ float4 bits4(int a, int b, float c, int d) {
    return make_float4(__int_as_float(a), __int_as_float(b), c, __int_as_float(d));
}

__global__ __launch_bounds__(BLOCK) void surface_kernel(DScene S, DSurf Q) {
    constexpr int F = FT_ALL;
    stage_tex_lut(S);  // eval_texture decodes 8-bit texels through the LUTs in LDS
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // n <= 2^30 (QUERY_MAX_RAYS)
    if (i >= Q.n) return;
    const int2* const h = reinterpret_cast<const int2*>(Q.hits + (size_t)i * 6);
    const int2 h0 = h[0], h1 = h[1], h2 = h[2];  // instance element | u v | t hit
    float4* const y = Q.out + (size_t)i * 6;
    const int inst = h0.x, elem = h0.y;
    const v2 uv = V2(__int_as_float(h1.x), __int_as_float(h1.y));
    // the range checks, each before the load it guards (&& evaluates left to right)
    const bool ok = h2.y != 0 && inst >= 0 && inst < Q.ninst && elem >= 0 && elem < Q.nelem[inst] &&
                    __builtin_isfinite(uv.x) && __builtin_isfinite(uv.y);
    if (!ok) {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = 0; k < 6; k++) y[k] = z;
        return;
    }
    const int di = Q.to_dev[inst];
    const float* const r = Q.rays + (size_t)i * 6;
    const v3 d = V3(r[3], r[4], r[5]);
    Shading sh;
    eval_shading<F>(S, di, elem, uv, -d, sh);
    const v3 gn = eval_element_normal<F>(S, di, elem);
    const DInstShade& is = S.inst_shade[di];
    const DShape shp = S.shapes[is.shape];
    const v2 tc = eval_texcoord(S, shp, S.elems[shp.idx_base + elem], uv);
    const MatPoint& m = sh.mat;
    y[0] = make_float4(sh.position.x, sh.position.y, sh.position.z, sh.normal.x);
    y[1] = make_float4(sh.normal.y, sh.normal.z, gn.x, gn.y);
    y[2] = make_float4(gn.z, tc.x, tc.y, m.opacity);
    y[3] = make_float4(m.color.x, m.color.y, m.color.z, m.roughness);
    y[4] = make_float4(m.emission.x, m.emission.y, m.emission.z, m.metallic);
    y[5] = bits4(is.material, m.type, m.ior, 1);
}

__global__ __launch_bounds__(BLOCK) void camera_kernel(DParams P, int sample, float2* rays) {
    const int pixel = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (pixel >= P.width * P.height) return;
    const int i = pixel % P.width, j = pixel / P.width;
    v3 o, d;
    if (sample >= 0) {  // start_path's ray of (pixel, sample)
        Rng rng = rng_init(P.seed, pixel, sample);
        camera_sample(P, i, j, rng, o, d);
    } else {  // through the pixel centre, from the lens centre
        eval_camera(P.cam, V2(((float)i + 0.5f) / (float)P.width, ((float)j + 0.5f) / (float)P.height), V2(0.0f, 0.0f), o, d);
    }
    float2* const y = rays + (size_t)pixel * 3;
    y[0] = make_float2(o.x, o.y);
    y[1] = make_float2(o.z, d.x);
    y[2] = make_float2(d.y, d.z);
}

}  // namespace jtk

// ---- the context's half (jt_context.h)
using namespace jtc;

namespace {

constexpr int BLOCK = jtk::BLOCK;

static_assert(sizeof(jt_surface) == 96, "surface_kernel writes a jt_surface as six 16-byte rows");
static_assert(sizeof(jt_hit) == 24, "surface_kernel reads a jt_hit as three 8-byte rows");

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

constexpr const char* SURFACE_MULTI =
    "surface evaluation and camera rays are not available on a multi-device context (jt_create_multi): use one "
    "context per device";

// jt_eval_hits' argument checks (device: the pointers are the device variant's, whose alignment the
// kernel relies on); *done: n == 0, nothing to do
int eval_check(const jt_ctx* c, int64_t n, const void* rays, const char* rays_name, const void* hits, const char* hits_name,
               const void* out, const char* out_name, bool device, bool* done) {
    const bool ok = !device || (aligned(rays, 4) && aligned(hits, 8) && aligned(out, 16));
    return ray_call_check(c, {{rays, rays_name}, {hits, hits_name}, {out, out_name}},
                          jtq::query_count_error(n, "n must be at most 2^30 records"),
                          ok ? nullptr : "d_rays, d_hits and d_out must be aligned to 4, 8 and 16 bytes", SURFACE_MULTI, n == 0, done);
}

// jt_camera_rays' and jt_gbuffer's; misaligned: nullptr, or what the device variant's pointers fail
int camera_check(const jt_ctx* c, int32_t sample, const void* out, const char* out_name, const char* misaligned = nullptr) {
    return ray_call_check(c, {{out, out_name}}, sample < -1 ? "sample must be at least -1 (-1: the pixel centres)" : nullptr, misaligned,
                          SURFACE_MULTI);
}

// the first surface call's upload: the element count of every instance's shape
int surface_setup(jt_ctx* c) {
    int st = query_setup(c);
    if (st != JT_OK || c->s_nelem) return st;
    const size_t ni = c->inst_nelem.size();
    void* a = nullptr;
    if ((st = device_alloc(c, (ni ? ni : 1) * sizeof(int), "surface element counts", &a))) return st;
    const hipError_t e = ni ? hipMemcpy(a, c->inst_nelem.data(), ni * sizeof(int), hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy surface element counts");
    c->s_nelem = (int*)a;
    return JT_OK;
}

// n >= 1 records from device pointers, on the context's stream; returns once the stream is idle
int surface_run(jt_ctx* c, int64_t n, const void* d_rays, const void* d_hits, void* d_out) {
    (void)hipSetDevice(c->device);
    if (const int st = surface_setup(c)) return st;
    jtk::DSurf Q{};
    Q.rays = (const float*)d_rays;
    Q.hits = (const int*)d_hits;
    Q.out = (float4*)d_out;
    Q.to_dev = c->q_to_dev;
    Q.nelem = c->s_nelem;
    Q.n = (int)n;
    Q.ninst = (int)c->inst_new.size();
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(jtk::surface_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, c->S, Q);
    return launch_finish(c, "surface kernel");
}

int camera_run(jt_ctx* c, int32_t sample, void* d_rays) {
    (void)hipSetDevice(c->device);
    const unsigned grid = (unsigned)(((int64_t)c->width * c->height + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(jtk::camera_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, c->P, (int)sample, (float2*)d_rays);
    return launch_finish(c, "camera kernel");
}

// the staging of n jt_surface records
int surface_stage(jt_ctx* c, int64_t n) {
    if (n <= c->q_stage_surf) return JT_OK;
    const int64_t cap = jtq::query_stage_rays(c->q_stage_surf, n);
    c->q_stage_surf = 0;
    if (const int st = query_grow(c, jt_ctx::Q_SURF, (size_t)cap * sizeof(jt_surface), "surface records")) return st;
    c->q_stage_surf = cap;
    return JT_OK;
}

}  // namespace

extern "C" {

int jt_eval_hits_device(jt_ctx* c, int64_t n, const void* d_rays, const void* d_hits, void* d_out) {
    bool done;
    if (const int st = eval_check(c, n, d_rays, "d_rays", d_hits, "d_hits", d_out, "d_out", true, &done)) return st;
    if (done) return JT_OK;
    return surface_run(c, n, d_rays, d_hits, d_out);
}

int jt_camera_rays_device(jt_ctx* c, int32_t sample, void* d_rays) {
    if (const int st = camera_check(c, sample, d_rays, "d_rays", aligned(d_rays, 8) ? nullptr : "d_rays must be aligned to 8 bytes"))
        return st;
    return camera_run(c, sample, d_rays);
}

int jt_gbuffer_device(jt_ctx* c, int32_t sample, void* d_rays, void* d_hits, void* d_surfaces) {
    // every alignment before any launch: a NULL d_rays or d_hits is aligned, the context's buffer stands in
    const bool ok = aligned(d_rays, 8) && aligned(d_hits, 8) && aligned(d_surfaces, 16);
    if (const int st = camera_check(c, sample, d_surfaces, "d_surfaces",
                                    ok ? nullptr : "d_rays, d_hits and d_surfaces must be aligned to 8, 8 and 16 bytes"))
        return st;
    (void)hipSetDevice(c->device);
    const int64_t n = (int64_t)c->width * c->height;
    if (!d_rays || !d_hits) {  // the context's own buffers stand in
        if (const int st = query_stage(c, n)) return st;
        if (!d_rays) d_rays = c->q_grow[jt_ctx::Q_RAYS];
        if (!d_hits) d_hits = c->q_grow[jt_ctx::Q_OUT];
    }
    int st;
    if ((st = jt_camera_rays_device(c, sample, d_rays)) || (st = jt_intersect_device(c, n, d_rays, nullptr, d_hits))) return st;
    return jt_eval_hits_device(c, n, d_rays, d_hits, d_surfaces);
}

int jt_eval_hits(jt_ctx* c, int64_t n, const float* rays, const jt_hit* hits, jt_surface* out) {
    bool done;
    if (const int st = eval_check(c, n, rays, "rays", hits, "hits", out, "out", false, &done)) return st;
    if (done) return JT_OK;
    (void)hipSetDevice(c->device);
    int st;
    if ((st = query_stage(c, n)) || (st = surface_stage(c, n))) return st;
    void* const d_rays = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_hits = c->q_grow[jt_ctx::Q_OUT];
    void* const d_out = c->q_grow[jt_ctx::Q_SURF];
    const size_t N = (size_t)n;
    if ((st = copy_in(d_rays, rays, N * 6 * sizeof(float), "hipMemcpy surface rays and hits")) ||
        (st = copy_in(d_hits, hits, N * sizeof(jt_hit), "hipMemcpy surface rays and hits")) ||
        (st = surface_run(c, n, d_rays, d_hits, d_out)))
        return st;
    return copy_out(out, d_out, N * sizeof(jt_surface), "hipMemcpy surface records");
}

int jt_camera_rays(jt_ctx* c, int32_t sample, float* rays) {
    if (const int st = camera_check(c, sample, rays, "rays")) return st;
    (void)hipSetDevice(c->device);
    const int64_t n = (int64_t)c->width * c->height;
    int st;
    if ((st = query_stage(c, n)) || (st = camera_run(c, sample, c->q_grow[jt_ctx::Q_RAYS]))) return st;
    return copy_out(rays, c->q_grow[jt_ctx::Q_RAYS], (size_t)n * 6 * sizeof(float), "hipMemcpy camera rays");
}

int jt_gbuffer(jt_ctx* c, int32_t sample, float* rays, jt_hit* hits, jt_surface* surfaces) {
    if (const int st = camera_check(c, sample, surfaces, "surfaces")) return st;
    (void)hipSetDevice(c->device);
    const int64_t n = (int64_t)c->width * c->height;
    int st;
    if ((st = query_stage(c, n)) || (st = surface_stage(c, n))) return st;
    void* const d_rays = c->q_grow[jt_ctx::Q_RAYS];
    void* const d_hits = c->q_grow[jt_ctx::Q_OUT];
    void* const d_out = c->q_grow[jt_ctx::Q_SURF];
    if ((st = jt_gbuffer_device(c, sample, d_rays, d_hits, d_out))) return st;
    if (rays && (st = copy_out(rays, d_rays, (size_t)n * 6 * sizeof(float), "hipMemcpy camera rays"))) return st;
    if (hits && (st = copy_out(hits, d_hits, (size_t)n * sizeof(jt_hit), "hipMemcpy query results"))) return st;
    return copy_out(surfaces, d_out, (size_t)n * sizeof(jt_surface), "hipMemcpy surface records");
}

}  // extern "C"
