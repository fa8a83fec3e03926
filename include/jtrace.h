/*
 * jtrace.h — C-ABI drop-in boundary for the MI355X path-tracing hot path.
 *
 * The reference (Princic-1837592/julia-raytracer, pure Julia 1.8.3) has no FFI.
 * Its natural seam is the per-batch call made by Jtrace.main:
 *
 *     trace_samples(state, scene, bvh, lights, params,
 *                   bvh_stacks, bvh_sub_stacks, volume_stacks)   src/trace.jl:215-274
 *
 * This header exports exactly what a Julia `ccall` shim (julia-raytracer_amd/julia/
 * JtraceHip.jl) or the Python `ctypes` harness binds to replace that call:
 *
 *   jt_create          ~ make_trace_state (src/trace.jl:189) + device upload of SceneData,
 *                        SceneBvh and TraceLights (src/scene.jl:337, src/bvh.jl:59, src/trace.jl:111)
 *   jt_trace_samples   == trace_samples for one batch (src/trace.jl:215)
 *   jt_trace_range     == trace_samples over an explicit global sample range (multi-GPU shards)
 *   jt_get_image       == get_image (src/trace.jl:676) — the running-mean RGBA buffer
 *   jt_get_aovs        == TraceState.albedo / normal / hits (src/trace.jl:87-100)
 *   jt_denoise         (the build's own: the reference's --denoise is forced off, src/jtrace.jl:35-46)
 *                      an a-trous filter over those means; jt_get_denoised reads its result
 *   jt_get_variance    (the build's own) the per-pixel variance of the image, from the spread of
 *                      the sample streams' means; jt_get_noise its image-level relative RMS error
 *   jt_denoise_guided  (the build's own) the a-trous filter with that variance as its colour tolerance
 *   jt_adapt           (the build's own) adaptive sampling: 8x8 tiles whose variance meets a noise
 *                      target take no more samples; jt_get_sample_counts the samples per pixel
 *   jt_intersect       ~ intersect_scene_bvh / intersect_instance_bvh (src/bvh.jl:306-520) for the
 *                      caller's own rays on the context's scene; jt_occluded its find_any form;
 *                      jt_intersect_bounded, jt_occluded_bounded the same of Ray3f(o, d, ray_eps, tmax),
 *                      jt_visible of a segment; jt_ambient_occlusion the share of a point's
 *                      hemisphere draws that meet nothing within a radius;
 *                      jt_intersect_multi the k nearest hits of that bounded query in one traversal,
 *                      jt_count_hits how many there are
 *   jt_eval_hits       ~ eval_shading_position / eval_shading_normal / eval_material (src/scene.jl:416-673)
 *                      at the caller's hit records; jt_camera_rays ~ sample_camera (src/trace.jl:651-674);
 *                      jt_gbuffer the two around jt_intersect: the surface under every pixel
 *   jt_radiance        ~ trace_sample (src/trace.jl:584-649) without its camera: the integrator's running
 *                      mean of radiance along the caller's own rays
 *   jt_destroy / jt_last_error — lifetime and error reporting (the reference throws Julia exceptions)
 *
 * Host helpers (run on the CPU, no device needed) that restate the reference's host code
 * for callers without their own:
 *   jt_build_scene_bvh ~ make_scene_bvh (src/bvh.jl:66), split_middle / split_sah exact
 *   jt_make_lights     ~ make_trace_lights (src/trace.jl:117)
 *
 * Conventions
 *   - every function returns JT_OK (0) or a negative jt_status; nothing throws across the ABI;
 *     jt_last_error() returns a thread-local message for the last failure on this thread.
 *   - all indices are 0-based int32 (the reference uses 1-based Int64; the shim subtracts 1).
 *     "none" ids (Julia invalid_id = -1, src/scene.jl:45) are -1 here too.
 *   - frames are 12 floats, column-major x, y, z, o (Frame3f, src/math.jl:46-60).
 *   - the caller owns every host array; jt_create deep-copies to the device, so host
 *     arrays may be released after it returns (Julia: GC.@preserve around the ccall).
 *   - a context is used by one host thread at a time; every call is synchronous.
 */
#ifndef JTRACE_H
#define JTRACE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JT_ABI_VERSION 5  /* 2: jt_params.traversal; 3: jt_set_option; 4: sample streams, jt_get_streams;
                            5: deferred jt_trace_range (same signatures) */

typedef enum jt_status {
    JT_OK = 0,
    JT_ERR_INVALID = -1,      /* malformed input (bad id, size, NULL pointer) */
    JT_ERR_UNSUPPORTED = -2,  /* input the reference cannot render either (see jt_create) */
    JT_ERR_DEVICE = -3,       /* HIP runtime failure / no device */
    JT_ERR_NOMEM = -4,        /* host or device allocation failed */
    JT_ERR_STACK = -5,        /* BVH deeper than params.bvhstacksize (reference: BoundsError) */
    JT_ERR_STATE = -6         /* call out of order (e.g. range outside [0, samples)) */
} jt_status;

/* MaterialType, in the order of the reference enum (src/scene.jl:191-200). */
typedef enum jt_material_type {
    JT_MATTE = 0,
    JT_GLOSSY = 1,
    JT_REFLECTIVE = 2,
    JT_TRANSPARENT = 3,
    JT_REFRACTIVE = 4,
    JT_SUBSURFACE = 5,
    JT_VOLUMETRIC = 6,
    JT_GLTFPBR = 7
} jt_material_type;

/* Samplers, index into SAMPLER_TYPES = ["path", "naive"] (src/cli.jl:88). */
typedef enum jt_sampler { JT_SAMPLER_PATH = 1, JT_SAMPLER_NAIVE = 2 } jt_sampler;

/* BVH child visit order (extension, jt_params.traversal).
 * JT_TRAVERSAL_REFERENCE: the reference's (src/bvh.jl:331-341, 396-407): for d[axis] >= 0 push
 *   start then start+1, so the upper child (start+1, higher split-axis coordinates: split_middle /
 *   split_sah partition lower centers to `start`, src/bvh.jl:171-176, 281-304) is visited first —
 *   the far child for a closest-hit query.
 * JT_TRAVERSAL_NEAR: the opposite push order, the near child by the split axis first. Fewer nodes
 *   are visited (tmax shrinks sooner). Among hits at exactly equal t the reference's later-tested
 *   one wins (src/geometry.jl:226, t > tmax rejects), which depends on the order: a near-first
 *   query that accepts a hit at exactly its current tmax is run again in the reference's child
 *   order and reports that hit (an intersect_instance_bvh of a one-leaf shape BVH has no child
 *   order and is never re-run). The closest hit then differs from the reference's only where the
 *   slab test's rounding lets one order find a hit the other culls (measured: 2e-6 of bathroom1's
 *   paths, none on cornellbox, features2, ecosys).
 * JT_TRAVERSAL_WIDE: the reference's binary tree collapsed to 4-wide records (each internal node
 *   holds its grandchildren: same leaves, same primitive order) with conservative 8-bit quantised
 *   child boxes, visited near child first in the binary DFS order (a tie's re-run: far child
 *   first, the reference's leaf sequence). A box can only pass where the exact one would, or more
 *   often, so again only boxes the exact slab test culls by rounding can resolve differently; one
 *   64-B record replaces about three 32-B node visits. */
typedef enum jt_traversal {
    JT_TRAVERSAL_REFERENCE = 0,
    JT_TRAVERSAL_NEAR = 1,
    JT_TRAVERSAL_WIDE = 2,
    JT_TRAVERSAL_AUTO = 3  /* wide for a scene that runs from HBM with a deep BVH (stack bound
                              above 32), near otherwise (LDS-mode and shallow scenes); jt_describe
                              reports the order taken ("traversal=near|wide") */
} jt_traversal;

/* CameraData (src/scene.jl:48-86), after the lookat conversion done by the loader. */
typedef struct jt_camera {
    float frame[12];
    int32_t orthographic;
    float lens, film, aspect, focus, aperture;
} jt_camera;

/* InstanceData (src/scene.jl:88-115). */
typedef struct jt_instance {
    float frame[12];
    int32_t shape;     /* 0-based shape id */
    int32_t material;  /* 0-based material id */
} jt_instance;

/* EnvironmentData (src/scene.jl:117-144). */
typedef struct jt_environment {
    float frame[12];
    float emission[3];
    int32_t emission_tex; /* -1 = none */
} jt_environment;

/* MaterialData (src/scene.jl:213-264). Texture ids are 0-based, -1 = none. */
typedef struct jt_material {
    int32_t type; /* jt_material_type */
    float emission[3];
    float color[3];
    float roughness, metallic, ior;
    float scattering[3];
    float scanisotropy, trdepth, opacity;
    int32_t emission_tex, color_tex, roughness_tex, scattering_tex, normal_tex;
} jt_material;

/* TextureData (src/scene.jl:146-162): RGBA, row-major, top row first.
 * Exactly one of pixelsf (linear float, HDR) / pixelsb (8-bit) is non-NULL. */
typedef struct jt_texture {
    int32_t width, height;
    int32_t linear;
    const float* pixelsf;   /* width*height*4 floats or NULL */
    const uint8_t* pixelsb; /* width*height*4 bytes or NULL */
} jt_texture;

/* ShapeData (src/shape.jl:13-48). Element arrays hold 0-based vertex ids.
 * Per-vertex arrays may be NULL with count 0 (the reference's empty vectors). */
typedef struct jt_shape {
    int32_t npoints, nlines, ntriangles, nquads;
    const int32_t* points;    /* npoints */
    const int32_t* lines;     /* nlines*2 */
    const int32_t* triangles; /* ntriangles*3 */
    const int32_t* quads;     /* nquads*4 */
    int32_t npositions;
    const float* positions;   /* npositions*3 */
    int32_t nnormals;
    const float* normals;     /* nnormals*3 */
    int32_t ntexcoords;
    const float* texcoords;   /* ntexcoords*2 (v already flipped by the loader, src/shape.jl:88) */
    int32_t ncolors;
    const float* colors;      /* ncolors*4 */
    int32_t nradius;
    const float* radius;      /* nradius */
} jt_shape;

/* SceneData (src/scene.jl:337-356). */
typedef struct jt_scene {
    int32_t ncameras;
    const jt_camera* cameras;
    int32_t ninstances;
    const jt_instance* instances;
    int32_t nenvironments;
    const jt_environment* environments;
    int32_t nshapes;
    const jt_shape* shapes;
    int32_t ntextures;
    const jt_texture* textures;
    int32_t nmaterials;
    const jt_material* materials;
} jt_scene;

/* BvhNode (src/bvh.jl:34-44), 0-based: `start` is the first child node (internal) or the
 * first slot of `primitives` (leaf); axis is 0..2. 32 bytes, C-compatible. */
typedef struct jt_bvh_node {
    float bmin[3];
    float bmax[3];
    int32_t start;
    int16_t num;
    int8_t axis;
    int8_t internal;
} jt_bvh_node;

/* BvhTree (src/bvh.jl:46-51). primitives[] are 0-based element (BLAS) or instance (TLAS) ids. */
typedef struct jt_bvh_tree {
    int32_t nnodes;
    jt_bvh_node* nodes;
    int32_t nprimitives;
    int32_t* primitives;
} jt_bvh_tree;

/* SceneBvh (src/bvh.jl:59-64): the instance TLAS plus one BLAS per shape. */
typedef struct jt_scene_bvh {
    jt_bvh_tree tlas;
    int32_t nshapes;
    jt_bvh_tree* blas;
} jt_scene_bvh;

/* TraceLight (src/trace.jl:102-109): exactly one of instance / environment is >= 0. */
typedef struct jt_light {
    int32_t instance;
    int32_t environment;
    int32_t ncdf;
    float* cdf;
} jt_light;

/* TraceLights (src/trace.jl:111-115). */
typedef struct jt_lights {
    int32_t nlights;
    jt_light* lights;
} jt_lights;

/* Params (src/cli.jl:90-138) restricted to the fields the hot path reads, plus the
 * build's extensions (seed, width/height override, device). */
typedef struct jt_params {
    int32_t camera;      /* 0-based camera id (find_camera result - 1) */
    int32_t resolution;  /* --resolution; W,H derived from camera aspect as make_trace_state */
    int32_t width;       /* extension: > 0 overrides W (with height) — aspect := W/H */
    int32_t height;
    int32_t samples;     /* --samples */
    int32_t bounces;     /* --bounces */
    int32_t sampler;     /* jt_sampler */
    int32_t clamp;       /* --clamp, stored as Int by the reference (src/cli.jl:105) */
    int32_t envhidden;
    int32_t tentfilter;
    int32_t nocaustics;
    int32_t batch;       /* --batch */
    int32_t bvhstacksize;
    int32_t device;      /* HIP device ordinal for this context */
    uint64_t seed;       /* extension: RNG seed; stream keyed by (seed, pixel, global sample) */
    int32_t traversal;   /* extension: jt_traversal (0 = the reference's child order) */
} jt_params;

/* Device counters accumulated over every launch of a context (diagnostic, exact). */
typedef struct jt_counters {
    uint64_t paths;          /* (pixel, sample) pairs traced */
    uint64_t rays;           /* intersect_scene_bvh calls (closest-hit scene queries) */
    uint64_t light_queries;  /* intersect_instance_bvh calls from sample_lights_pdf */
    uint64_t nodes;          /* BVH node pops (TLAS + BLAS, both query kinds) */
    uint64_t instances;      /* instance visits (TLAS leaf entries + light queries) */
    uint64_t prims;          /* triangle / quad tests */
    uint64_t shades;         /* surface hits shaded */
    uint64_t launches;       /* kernel launches */
    double kernel_ms;        /* summed device time of the trace launches (HIP events) */
} jt_counters;

/* Device pointers of a context's accumulators (for an in-place RCCL reduce). */
typedef struct jt_device_buffers {
    void* image;   /* float4[W*H]  running mean RGBA */
    void* albedo;  /* float4[W*H]  running mean albedo (w unused) */
    void* normal;  /* float4[W*H]  running mean normal (w unused) */
    void* hits;    /* int64[W*H] */
    int32_t width, height;
    void* stream;  /* hipStream_t the context launches on */
} jt_device_buffers;

/* Parameters of the denoiser (jt_denoise). iterations: 1..8; the sigmas and the floor finite, > 0. */
typedef struct jt_denoise_params {
    int32_t iterations;  /* a-trous iterations I; iteration i taps at a distance of 2^i pixels */
    float sigma_color;   /* of the demodulated radiance at iteration 0; halved every iteration */
    float sigma_normal;
    float sigma_albedo;
    float albedo_floor;  /* lower bound of the albedo the radiance is divided by */
} jt_denoise_params;

/* Parameters of the variance-guided denoiser (jt_denoise_guided). iterations: 1..8; every other
 * field finite, > 0, and sigma_variance^2 * variance_floor a normal float. */
typedef struct jt_denoise_guided_params {
    int32_t iterations;    /* a-trous iterations I; iteration i taps at a distance of 2^i pixels */
    float sigma_variance;  /* colour tolerance in standard deviations of the two pixels' difference */
    float sigma_normal;
    float sigma_albedo;
    float albedo_floor;    /* lower bound of the albedo the radiance is divided by */
    float variance_floor;  /* lower bound of V(p) + V(q), of demodulated radiance */
} jt_denoise_guided_params;

typedef struct jt_ctx jt_ctx;

/* ---- library ---------------------------------------------------------------------- */
const char* jt_version(void);
int jt_abi_version(void);
const char* jt_last_error(void);
int jt_device_count(int32_t* out);

/* ---- run-time options ---------------------------------------------------------------- */
/* Process-wide switches, read by jt_create / jt_create_multi for the contexts they create
 * afterwards (a context keeps the values it was created with). The library never reads the
 * environment. name, value: NUL-terminated; value NULL removes one option, name NULL (with
 * value NULL) removes all. An unknown name fails with JT_ERR_INVALID. Unless stated, every
 * option leaves images, AOVs and counters bit-identical to the default:
 *   "env_alias" "1"          environment lights sample texels through alias tables (O(1)) instead
 *                            of upper_bound: the same distribution, so results equal the default
 *                            statistically, NOT bitwise (a variant, off by default)
 *   "features" "all"         run the general kernel instead of the scene's specialisation
 *   "lds_scene" "<bytes>"    budget of the small-scene LDS blob (0: scene arrays stay in HBM;
 *                            the stream count, hence the bits, never depend on the mode)
 *   "lds_stack" "32"         a 32-entry LDS stack ring instead of 16
 *   "light_inline" "0"       sample_lights_pdf's light queries through the traversal loop
 *   "wait_lanes", "light_lanes"  the shading gate; the light-hit step gate
 *   "multi_split" "tiles"|"samples"  jt_create_multi's split mode
 * Options that change WHAT a context traces (jt_describe reports them when set):
 *   "streams" "<k>"          sample streams per pixel (a power of two <= 64) instead of the
 *                            automatic count (jt_get_streams): the running means combine in a
 *                            different order, so images differ in the last bits
 *   "tile_share" "k,o"       trace only the 8x8 tiles o, o + k, o + 2k, ...: this process's share
 *                            of a k-way tile split when one process per GPU shards a render by
 *                            tiles (bench.py); jt_create_multi sets its own split instead
 *   "test_lds_ring" "1|2|4|8|16"  (tests only) use that many LDS ring entries, the rest overflow to
 *                            HBM: the overflow path on small scenes
 *   "test_probe_chunk" "<n>"  (tests only) jt_probe_sh's host variant stages at most n points per
 *                            chunk instead of 2^22: a chunk boundary on a small array
 *   "test_multi_chunk" "<n>"  (tests only) jt_intersect_multi's host variant stages at most n rays
 *                            per chunk instead of 2^22 / k
 *   "test_trace_chunk" "<n>"  (tests only) a one-stream context (batch <= 1) traces a range of more
 *                            than one sample in chunks of at most n samples instead of up to 64:
 *                            n a power of two in [1, 64] (jt_create fails with JT_ERR_INVALID
 *                            otherwise); 1: no chunks, one launch of the whole range. It only ever
 *                            lowers the chunk */
int jt_set_option(const char* name, const char* value);

/* ---- host helpers (CPU only) ------------------------------------------------------- */
/* make_scene_bvh (src/bvh.jl:66-88): one BLAS per shape (make_shape_bvh :90) and the
 * instance TLAS over transformed root boxes; split_middle (:185) or split_sah (:218). */
int jt_build_scene_bvh(const jt_scene* scene, int32_t high_quality, jt_scene_bvh* out);
void jt_free_scene_bvh(jt_scene_bvh* bvh);
/* make_trace_lights (src/trace.jl:117-187). */
int jt_make_lights(const jt_scene* scene, jt_lights* out);
void jt_free_lights(jt_lights* lights);
/* W,H as make_trace_state (src/trace.jl:189-197) or the width/height extension. */
int jt_image_size(const jt_scene* scene, const jt_params* params, int32_t* width, int32_t* height);

/* ---- device context ---------------------------------------------------------------- */
/* Uploads scene, BVH and lights; allocates zeroed accumulators (make_trace_state).
 * Rejects with JT_ERR_UNSUPPORTED what the reference cannot shade either: shapes with
 * points (src/scene.jl:429), lines without normals (src/scene.jl:605), gltfpbr materials
 * on instances (src/shading.jl:254-321 call undefined functions), and untextured
 * environment lights (src/trace.jl:1003). */
int jt_create(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights,
              const jt_params* params, jt_ctx** out);
/* jt_create over several GPUs of one node (SURVEY §8(b) "jt_create(..., num_devices, ...)"; the
 * reference's caller is Jtrace.main's batch loop, src/jtrace.jl:83-106). devices: ndevices
 * distinct HIP ordinals, or NULL for 0 .. ndevices-1 (params->device is ignored). Every other
 * function takes the returned context. Every batch is split across the devices in one of two
 * modes, fixed at creation:
 *   - sample split (params->batch >= ndevices): contiguous per-device shares of the batch's
 *     samples, traced concurrently, each device keeping its own running mean over its samples;
 *     jt_get_image / jt_get_aovs reduce them onto device 0 with one RCCL reduce whose op is a
 *     premultiplied sum (mean_d * n_d / N; hits summed), so the image equals the single-device
 *     one up to fp32 summation order;
 *   - tile split (params->batch < ndevices, e.g. the reference's default --batch 1): device d
 *     traces every sample of the batch on the interleaved 8x8 pixel tiles t with t mod ndevices
 *     == d; the reduce is a plain sum of the disjoint tiles, bit-identical to one device.
 * The option "multi_split" (jt_set_option: "tiles" | "samples") overrides the rule.
 * jt_get_counters sums the devices (kernel_ms: per launch the slowest device);
 * jt_get_device_buffers returns device 0's share. */
int jt_create_multi(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights,
                    const jt_params* params, const int32_t* devices, int32_t ndevices, jt_ctx** out);
/* trace_samples (src/trace.jl:215-274): samples [n, min(n+batch, samples)), n += batch
 * (jt_trace_range of that range: it may return before the samples are traced). */
int jt_trace_samples(jt_ctx* ctx);
/* Accumulate global samples [sample_begin, sample_end) into the running mean, in order.
 * Deferred: the range is queued behind the ranges queued before it and all are traced together
 * (one launch per 64 samples or so) once 64 samples are queued, the context's params.samples are
 * reached, or the context is read: jt_get_image / jt_get_aovs / jt_get_counters /
 * jt_get_device_buffers / jt_synchronize trace the queued samples first and report their errors
 * (a failed launch then marks the context failed, as an immediate one would). A context whose
 * device buffers were handed out (jt_get_device_buffers) traces every range at once. Merging
 * changes only the launch count (jt_counters.launches), never the bits (below). jt_get_samples
 * counts queued samples; jt_reset drops them.
 * Sample streams (fixed per context, jt_get_streams: k, a power of two): local sample
 * t = s - first_sample (first_sample: the first sample this context ever traced, 0 for a single
 * device) belongs to stream j = t mod k and is the c-th sample of that stream, c = t div k; every
 * stream keeps its own running mean (src/trace.jl:631-648, weight 1/(c + 1)), and after every
 * call the image / AOVs are the streams' means combined in stream order,
 *     image = sum_{j < min(k, n)} mean_j * w_j,  w_j = (float)((double)n_j / n),
 * n the local samples so far and n_j those of stream j (float multiply-adds without FMA,
 * starting from mean_0 * w_0); hits = sum_j hits_j. k = 1 is the reference's single running mean.
 * The result does not depend on how a render is split into calls. */
int jt_trace_range(jt_ctx* ctx, int32_t sample_begin, int32_t sample_end);
/* The context's sample streams per pixel k (jt_trace_range). Chosen by jt_create from the
 * pixels it traces and the batch only (never the scene or its LDS/HBM mode): 1 when
 * params->batch is 1 (the reference's default); otherwise the smallest power of two k >= 16
 * (>= 32 for a batch of at least 64) with (pixels the context traces) * k >= 2^22, reduced to
 * at most 64, the batch, and (pixels) * k <= 2^27 (at least 1) — halved further while the
 * stream means (48 B per pixel and stream) cannot be allocated; or the "streams" option.
 * k = 1 contexts trace a range of m > 1 samples as chunks of one-sample streams folded into the
 * single running mean in sample order: the bits of one launch per sample. */
int jt_get_streams(const jt_ctx* ctx, int32_t* streams);
int jt_get_samples(const jt_ctx* ctx, int32_t* samples);
int jt_get_size(const jt_ctx* ctx, int32_t* width, int32_t* height);
int jt_get_image(jt_ctx* ctx, float* rgba);                          /* W*H*4 */
int jt_get_aovs(jt_ctx* ctx, float* albedo, float* normal, int64_t* hits); /* W*H*3, W*H*3, W*H */
int jt_get_counters(jt_ctx* ctx, jt_counters* out);

/* ---- denoiser ------------------------------------------------------------------------ */
/* The edge-avoiding a-trous wavelet filter of Dammertz et al. (HPG 2010) on albedo-demodulated
 * radiance, guided by the albedo and normal means (the reference mirrors a --denoise flag and
 * switches it off, src/jtrace.jl; this is the build's own). All float32, no FMA. With c the
 * mean radiance RGBA, a the mean albedo, n the mean normal (as accumulated, not renormalised):
 *   m = max(a, albedo_floor) per channel;  d_0 = c.rgb / m;
 *   for i = 0 .. iterations-1, s = 2^i, sc_i = sigma_color / s, at every pixel p:
 *     d_{i+1}(p) = sum_q w(p,q) d_i(q) / sum_q w(p,q),  q = p + s (dx, dy), dx, dy in -2..2,
 *     taps outside the image skipped;
 *     w(p,q) = k[dy+2] k[dx+2] exp(-(|d_i(p)-d_i(q)|^2 / sc_i^2 + |n(p)-n(q)|^2 / sigma_normal^2
 *                                    + |a(p)-a(q)|^2 / sigma_albedo^2)),
 *     k = {1/16, 1/4, 3/8, 1/4, 1/16}, |.|^2 summed over the three channels (the centre tap
 *     weighs 9/64, so the denominator is never 0);
 *   out.rgb = d_I * m;  out.a = c.a.
 * jt_denoise_defaults (host only): iterations 5, sigma_color 8 / sqrtf(max(samples, 1)) (the
 * noise falls as 1 / sqrt(spp)), sigma_normal 0.3, sigma_albedo 0.1, albedo_floor 0.01. */
int jt_denoise_defaults(int32_t samples, jt_denoise_params* out);
/* Filters the context's running means into a buffer the context owns (allocated with its
 * scratch by the first call, kept across jt_reset, freed by jt_destroy). params NULL: the
 * defaults for the samples traced so far. Traces the queued samples first, as every reader
 * does; image, albedo, normal, hits and every jt_counters field stay bit for bit as they were.
 * JT_ERR_STATE when no sample has been traced or the context has failed; JT_ERR_INVALID
 * (naming the field) for iterations outside 1..8 or a sigma or floor that is not finite and
 * > 0. A multi-device context reduces image, albedo and normal as jt_get_image / jt_get_aovs do
 * and filters them on its first device. */
int jt_denoise(jt_ctx* ctx, const jt_denoise_params* params);
/* The result of the last jt_denoise or jt_denoise_guided, W*H*4. JT_ERR_STATE when none has run since the last
 * sample was traced (or queued) or since jt_reset: a stale result is never returned. */
int jt_get_denoised(jt_ctx* ctx, float* rgba);
/* The same filter on the caller's host arrays (rgba W*H*4, albedo W*H*3, normal W*H*3, row-major)
 * on HIP device `device`, into out_rgba (W*H*4): for callers who reduce the shards of a render
 * themselves (one process per GPU). Arguments are checked before any device work; params is
 * required; width, height >= 1 and within jt_create's image size limit. Non-finite pixels in
 * the arrays are the caller's responsibility (they spread to every pixel whose taps reach them);
 * the tracer's own buffers never hold any. */
int jt_denoise_image(const float* rgba, const float* albedo, const float* normal, int32_t width, int32_t height,
                     const jt_denoise_params* params, int32_t device, float* out_rgba);

/* The variance-guided filter: the same window and guides, but the colour tolerance of a tap is
 * the two pixels' own variance (the error estimate below) instead of one global sigma_color, and
 * that variance is carried through the iterations. All float32, no FMA. With c the mean radiance
 * RGBA, v the variance of the mean RGBA as jt_get_variance returns it (v.a is ignored), a the
 * mean albedo, n the mean normal (as accumulated):
 *   m = max(a, albedo_floor) per channel;  d_0 = c.rgb / m;
 *   u = v.rgb / (m * m) per channel;  V_0 = (u.x + u.y) + u.z;  sv2 = sigma_variance * sigma_variance;
 *   for i = 0 .. iterations-1, s = 2^i, at every pixel p:
 *     taps q = p + s (dx, dy), dx, dy in -2..2; taps outside the image are skipped;
 *     e(p,q) = |d_i(p)-d_i(q)|^2 / (sv2 * max(V_i(p) + V_i(q), variance_floor))
 *            + |n(p)-n(q)|^2 / sigma_normal^2 + |a(p)-a(q)|^2 / sigma_albedo^2;
 *     w(p,q) = k[dy+2] k[dx+2] exp(-e),  k = {1/16, 1/4, 3/8, 1/4, 1/16} (the centre tap weighs 9/64);
 *     d_{i+1}(p) = sum_q w d_i(q) / sum_q w;
 *     V_{i+1}(p) = sum_q (w * w) V_i(q) / (sum_q w)^2;
 *   out.rgb = d_I * m;  out.a = c.a, copied by its bits.
 * |.|^2 is summed over the three channels, as in jt_denoise. The colour tolerance is not halved
 * per iteration: the propagated variance shrinks it where the filter has already averaged. The
 * weight is symmetric (V(p) + V(q)), so a pixel whose own estimate is 0 still accepts a noisy
 * neighbour's evidence while two zero-variance pixels stay anchors; V_0 = 0 everywhere makes the
 * filter the identity up to the c / m * m round trip.
 * jt_denoise_guided_defaults (host only, independent of the sample count: the variance carries
 * it): iterations 5, sigma_variance 2.0, sigma_normal 0.3, sigma_albedo 0.1, albedo_floor 0.01,
 * variance_floor 1e-10. */
int jt_denoise_guided_defaults(jt_denoise_guided_params* out);
/* Filters the context's running means into the buffer jt_denoise uses; jt_get_denoised reads the
 * result of whichever of the two ran last, and its staleness rule is unchanged. params NULL: the
 * defaults. Traces the queued samples first and obtains the error estimate exactly as
 * jt_get_variance does: one already valid for these samples is reused, and one computed here
 * serves a later jt_get_variance / jt_get_noise. Image, albedo, normal, hits, the stream means,
 * the variance and every jt_counters field stay bit for bit as they were.
 * Errors, in this order: JT_ERR_INVALID (naming the field) for a NULL ctx, iterations outside
 * 1..8, a field that is not finite and > 0, or a sigma_variance^2 * variance_floor that
 * underflows; then every error of jt_get_variance: JT_ERR_UNSUPPORTED for a multi-device context
 * (jt_create_multi), JT_ERR_STATE for a failed context, a one-stream context, no sample, or fewer
 * than two samples. */
int jt_denoise_guided(jt_ctx* ctx, const jt_denoise_guided_params* params);
/* The same filter on the caller's host arrays, as jt_denoise_image with variance W*H*4 (alpha
 * ignored). Arguments and sizes are checked before any device work; params is required.
 * Negative or non-finite variance is the caller's responsibility. */
int jt_denoise_guided_image(const float* rgba, const float* variance, const float* albedo, const float* normal,
                            int32_t width, int32_t height, const jt_denoise_guided_params* params, int32_t device,
                            float* out_rgba);

/* ---- error estimate -------------------------------------------------------------------- */
/* The per-pixel variance of the image, from the spread of the sample streams' means. A
 * single-device context with k > 1 streams (jt_get_streams) keeps k independent running means
 * per pixel; after n >= 2 local samples ns = min(n, k) of them hold a sample, stream j n_j
 * (jt_trace_range states the rule). With m_j stream j's mean RGBA, w_j = (float)((double)n_j / n)
 * the weight it was combined with, and mu the image pixel as jt_get_image returns it, per
 * channel, float32, no FMA:
 *   acc = 0;  for j = 0 .. ns-1 in order:  d = m_j - mu;  acc = acc + (d * d) * w_j
 *   var = acc / (float)(ns - 1)
 * the between-stream estimate of Var(mu), the variance OF THE MEAN (it falls as 1 / n).
 * jt_get_variance copies var out, W*H*4; pixels a tile share (option tile_share) does not
 * trace are 0. jt_get_noise is the image's relative RMS error over the N pixels the context
 * traces: with V = sum_p ((var.x + var.y) + var.z) and M = sum_p ((mu.x + mu.y) + mu.z),
 *   noise = sqrt(3 N V) / M  ( = sqrt(mean channel variance) / mean channel value ), 0 when M == 0,
 * the sums per workgroup in float32 on the device (no atomics: deterministic), over the
 * workgroups in double on the host.
 * Both trace the queued samples first, as every reader does, and leave image, albedo, normal,
 * hits, the stream means and every jt_counters field as a flush alone would; the estimate lives
 * in buffers the context owns (allocated by the first call, kept across jt_reset, freed by
 * jt_destroy), and a result computed for the current samples serves both calls.
 * JT_ERR_INVALID (naming the argument) for a NULL ctx or output; JT_ERR_UNSUPPORTED for a
 * multi-device context (jt_create_multi); JT_ERR_STATE when the context has failed, when no
 * sample has been traced (also after jt_reset), or when fewer than two streams hold a sample:
 * a one-stream context (batch 1 without the option streams) or n < 2. */
int jt_get_variance(jt_ctx* ctx, float* var_rgba);   /* W*H*4, variance of the mean per channel */
int jt_get_noise(jt_ctx* ctx, double* noise);

/* ---- adaptive sampling ------------------------------------------------------------------ */
/* jt_adapt freezes the 8x8 tiles whose error estimate already meets the image-level noise target
 * T; from then on every jt_trace_range / jt_trace_samples of the context skips them, so the
 * samples go where the noise is. It decides only where samples go: when to stop stays the
 * caller's (jt_get_noise <= T; waiting for every tile to freeze takes far longer).
 * The rule, for a context with k > 1 streams after n local samples, n a multiple of k (every
 * stream holds n / k samples, every combine weight is exactly 1 / k): with var, N and M those of
 * jt_get_variance / jt_get_noise for these samples (a valid estimate is reused, one computed here
 * serves later calls),
 *   vmax = (float)((T * M) * (T * M) / (3.0 * N * N))           in double, rounded once
 * and for every tile t the context traces that is not frozen, lane l = 8 * row + col the pixel
 * (col, row) of the tile, float32, no FMA:
 *   v[l] = (var.x + var.y) + var.z for a pixel inside the image, 0 outside
 *   for off = 32, 16, ..., 1:  v[l] += v[l + off]  (l < off);   V_t = v[0]
 *   N_t = the tile's pixels inside the image;   the tile freezes iff V_t <= (float)N_t * vmax
 * i.e. the tile's mean channel variance is at most (T x the image's mean channel value)^2.
 * Summed over the tiles this is 3 N V <= (T M)^2: if every tile meets it at one call,
 * jt_get_noise <= T. Freezing is monotone: a frozen tile stays frozen until jt_reset, which
 * unfreezes every tile. *active_tiles (may be NULL) receives the traced tiles still active.
 * A frozen pixel's stream means are those of its freeze time. jt_get_image combines them with
 * the weights of the context's current n, as for every pixel: at any n that is a multiple of k
 * this is bit for bit the pixel's value when it froze, and the same holds for albedo, normal,
 * hits and jt_get_variance. jt_get_samples and the sample indices do not change: a pixel still
 * active at sample s gets exactly the sample s it would get without adaptation. jt_counters
 * counts what was traced. A tile_share context adapts over its own tiles. jt_describe appends
 * " adaptive=<active>/<traced tiles>" once jt_adapt has run on the context. A context that never
 * calls jt_adapt behaves exactly as before.
 * jt_adapt traces the queued samples first, as every reader does, and leaves image, albedo,
 * normal, hits, the stream means, the variance and every jt_counters field as a flush alone
 * would (its launch is not counted). Errors, in this order: JT_ERR_INVALID (naming the argument)
 * for a NULL ctx or a noise_target that is not finite and > 0, before the context is looked at;
 * every error of jt_get_variance; JT_ERR_STATE (stating n and k) when n is not a multiple of k.
 * jt_get_sample_counts (W*H int32; traces the queued samples first): for the pixels of a frozen
 * tile the n at which it froze, for an active traced tile the context's n, 0 for pixels a tile
 * share does not trace; all n on a context that never adapted. */
int jt_adapt(jt_ctx* ctx, double noise_target, int32_t* active_tiles /* may be NULL */);
int jt_get_sample_counts(jt_ctx* ctx, int32_t* counts /* W*H */);

/* ---- ray queries ------------------------------------------------------------------------- */
/* Closest-hit and any-hit queries of arbitrary rays against the context's scene: the traversal
 * the path integrator itself runs (src/bvh.jl:306-520), for callers who want what is under a
 * pixel, visibility, depth or instance-id maps, ambient occlusion or probe placement. */
typedef struct jt_hit {      /* 24 bytes */
    int32_t instance;        /* index into jt_scene.instances (the caller's numbering), -1: miss */
    int32_t element;         /* triangle / quad index within the instance's shape, -1: miss */
    float u, v;              /* element uv as the reference's intersection.uv; 0 on a miss */
    float t;                 /* distance; +inf on a miss */
    int32_t hit;             /* 1 / 0 */
} jt_hit;
/* jt_intersect: for every ray i (rays[6 i ..] = origin, direction) the closest hit of the
 * reference's intersect_scene_bvh(..., find_any = false), or, where instance is not NULL and
 * instance[i] >= 0, of intersect_instance_bvh of that instance. It runs in the traversal the
 * context was created with (reference, near or wide, JT_TRAVERSAL_AUTO as resolved), the re-run
 * of an exact-t tie included: the hit the integrator would find for that ray, bit for bit, whatever
 * the number of rays and their order. Rays are unbounded, as every query of the reference's
 * integrator is: tmax is infinite (jt_intersect_bounded below takes a bound), tmin is the
 * reference's ray_eps inside the primitive tests. The direction
 * need not be normalised; t is in units of it.
 * jt_occluded: find_any = true reduced to its flag. A ray's query ends at its first accepted hit
 * and is never re-run for a tie. Until a hit is accepted tmax is infinite, exactly as in the
 * closest-hit query, so both queries take the same steps in the same order up to that hit: the
 * any-hit query visits a prefix of the closest-hit query's steps and accepts a hit iff that
 * query accepts one. occluded[i] therefore equals jt_intersect's hit for every ray (the near-first
 * orders' tie re-run never turns a hit into a miss: it runs only after a hit was accepted, and
 * finds the same primitives), for less work.
 * Instances are numbered as in jt_scene.instances, in the argument and in the results.
 * The *_device variants take device pointers on the context's device (d_instance may be NULL),
 * run on the context's stream and return when it is idle; in them an instance id outside
 * -1 .. ninstances-1 reports a miss. The host variants stage through buffers the context owns
 * (allocated by the first call, grown when needed, kept across jt_reset, freed by jt_destroy).
 * A query reads the scene only: image, AOVs, stream means, variance, the adaptive mask and every
 * jt_counters field stay bit for bit as they were, queued samples stay queued, and query work
 * is not counted. A context that never queries behaves exactly as before.
 * Errors, in this order: JT_ERR_INVALID (naming the argument) for a NULL ctx, rays or output,
 * n < 0 or n > 2^30, before the context is looked at; n == 0 returns JT_OK with no device work;
 * JT_ERR_UNSUPPORTED for a multi-device context (jt_create_multi); JT_ERR_STATE for a failed
 * context; JT_ERR_INVALID for a host instance[i] outside -1 .. ninstances-1.
 * Non-finite ray components are the caller's responsibility: the query terminates for any input
 * (every step pops an entry of a finite tree), the result for such a ray is unspecified. */
int jt_intersect(jt_ctx* ctx, int64_t n, const float* rays /* n x (o, d), 6 floats */,
                 const int32_t* instance /* NULL, or per ray -1 / an instance id */, jt_hit* hits);
int jt_occluded(jt_ctx* ctx, int64_t n, const float* rays, uint8_t* occluded /* n */);
int jt_intersect_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_instance, void* d_hits);
int jt_occluded_device(jt_ctx* ctx, int64_t n, const void* d_rays, void* d_occluded);

/* ---- bounded ray queries ------------------------------------------------------------------ */
/* The same queries on a ray with an end: a shadow ray to a point light, line of sight between two
 * points, probe-to-probe links. The reference's Ray3f carries tmin and tmax (src/geometry.jl:36-46),
 * its box and primitive tests read ray.tmax, transform_ray keeps it and intersect_scene_bvh shrinks
 * it as hits are accepted (src/bvh.jl:363): a bounded query is the reference's own function called
 * with Ray3f(o, d, ray_eps, tmax). There is no per-ray tmin: ray_eps is a literal of every step.
 * jt_intersect_bounded: jt_intersect with ray i's query started at tmax = tmax[i] instead of +inf:
 * intersect_scene_bvh / intersect_instance_bvh of Ray3f(o, d, ray_eps, tmax[i]), in the context's
 * traversal. A hit is accepted iff ray_eps <= t <= (current tmax): a hit exactly at the bound
 * counts. The caller's bound is the current tmax for the tie rule: a near-first query (near or
 * wide) whose accepted hit lies exactly on it is an exact-t tie like any other, and is run again
 * in the reference's child order with the same bound. A miss is the unbounded miss record
 * (t = +inf, ids -1, u = v = 0). tmax NULL, or tmax[i] = +inf, gives the bits of jt_intersect. A
 * bound below ray_eps, zero or negative, yields a miss by the rule itself. A NaN bound is the
 * caller's responsibility: the result is unspecified, and the lane still ends in a bounded number
 * of steps. Everything else as jt_intersect: the instance numbering, "whatever the number of rays
 * and their order", the host instance[i] range check, t in units of the direction.
 * jt_occluded_bounded: find_any on the same bounded ray. jt_occluded's prefix argument carries
 * over unchanged: until a hit is accepted both queries hold the same tmax, namely the bound, so
 * they take the same steps in the same order up to that hit, and occluded[i] equals the hit flag
 * of jt_intersect_bounded for every ray in every traversal.
 * jt_visible: for every segment i (segments[6 i ..] = a, b) the any-hit query of the ray
 * (a, b - a), the subtraction one float32 operation per component, with the bound 1.0f - ray_eps
 * (float32); visible[i] = 1 iff nothing is hit. t is in units of the segment, so both ends get
 * the same relative epsilon: a surface through a (t < ray_eps) or through b (t > 1 - ray_eps) does
 * not hide the one from the other. By definition the result is 1 - jt_occluded_bounded of those
 * rays and that bound, bit for bit. a == b, a zero direction, is the caller's responsibility.
 * The *_device variants take device pointers on the context's device (d_tmax and d_instance may
 * be NULL), run on the context's stream and return when it is idle. The host variants stage
 * through the buffers the ray queries' host variants use, the bounds in one more of them.
 * The context is read only, as for jt_intersect: image, AOVs, stream means, variance, the adaptive
 * mask and every jt_counters field stay bit for bit, queued samples stay queued.
 * Errors: jt_intersect's, in its order and with its messages (the segments and the flags named
 * `segments` and `visible`). */
int jt_intersect_bounded(jt_ctx* ctx, int64_t n, const float* rays, const float* tmax /* n, or NULL */,
                         const int32_t* instance /* or NULL */, jt_hit* hits);
int jt_occluded_bounded(jt_ctx* ctx, int64_t n, const float* rays, const float* tmax /* n, or NULL */, uint8_t* occluded);
int jt_visible(jt_ctx* ctx, int64_t n, const float* segments /* n x (a, b), 6 floats */, uint8_t* visible);
int jt_intersect_bounded_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance, void* d_hits);
int jt_occluded_bounded_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_tmax, void* d_occluded);
int jt_visible_device(jt_ctx* ctx, int64_t n, const void* d_segments, void* d_visible);

/* ---- all hits along a ray ------------------------------------------------------------------ */
/* The hits behind the first one, in one traversal: transparency and cutout layers, thickness,
 * inside / outside by crossing parity, and the records jt_eval_hits needs for an opacity-aware
 * visibility.
 * jt_intersect_multi: ray i, its bound B (tmax[i]; +inf for tmax NULL) and instance[i] are exactly
 * jt_intersect_bounded's: the scene query, or intersect_instance_bvh of one instance, of
 * Ray3f(o, d, ray_eps, B) in the context's traversal. A *candidate* is a primitive the traversal
 * tests whose test (intersect_triangle / intersect_quad, the closest-hit query's own) accepts it at
 * the query's current tmax: ray_eps <= t <= tmax. Candidates are ordered by the key
 * (t, instance, element): t compared as float32, the instance in the caller's numbering, all three
 * ascending. The result is the k smallest keys, ascending, in hits[i k + 0 .. counts[i]); records
 * counts[i] .. k - 1 are the miss record (-1, -1, 0, 0, +inf, 0); counts[i] <= k; u, v and t are
 * the bits the primitive test produced. The current tmax is B while the list holds fewer than k
 * entries and the k-th entry's t afterwards; every box test and primitive test reads it, as in
 * the closest-hit query. A candidate that arrives at a full list is inserted iff its key is smaller
 * than the last entry's, which is then dropped.
 * There is no tie re-run: among the primitives a traversal tests the result does not depend on the
 * order in which they are tested (a primitive among the k smallest has t <= every tmax the query
 * ever holds, and the ids decide an equal t). The order can matter only where the reference's slab
 * test culls a box that holds a hit (0 * inf for an axis-parallel ray from a box plane, rounding at
 * a box edge): which boxes are asked, and at which tmax, depends on the child order and, in the
 * wide order, on the quantised planes — the caveat of jt_traversal. k = 1 shrinks tmax exactly as
 * the closest-hit query does, so its flag and t are jt_intersect_bounded's; the ids differ only at
 * an exact-t tie: the smallest id here, the last one tested there.
 * jt_count_hits: counts[i] is the number of candidates with tmax held at B throughout: no list,
 * nothing shrinks, so every test reads the same tmax whatever the child order and the reference
 * and near orders return the same count. An odd count from a point outside a closed mesh means
 * the origin is inside it.
 * The *_device variants take device pointers on the context's device (d_tmax and d_instance may be
 * NULL; d_hits aligned to 8 bytes, d_counts to 4), run on the context's stream and return when it
 * is idle; an instance id out of range gives count 0. The host variant of jt_intersect_multi runs
 * the array in chunks of at most 2^22 / k rays through a buffer the context owns; a ray's result
 * does not depend on the call's other rays, so the chunks give the bits of one call.
 * The context is read only, as for every query.
 * Errors: jt_intersect_bounded's, in its order and with its messages (outputs: hits, then counts);
 * after the NULL and n checks, k < 1, k > JT_MULTI_MAX_HITS or n * k > 2^30 is JT_ERR_INVALID
 * naming k; then the device variants' alignment; all before the context is looked at and before
 * anything is written. n == 0 returns JT_OK with no device work. A NaN bound and non-finite rays
 * are the caller's responsibility: every lane still ends in a bounded number of steps. */
#define JT_MULTI_MAX_HITS 16
int jt_intersect_multi(jt_ctx* ctx, int64_t n, const float* rays /* n x 6 */, const float* tmax /* n, or NULL */,
                       const int32_t* instance /* or NULL */, int32_t k, jt_hit* hits /* n x k */, int32_t* counts /* n */);
int jt_count_hits(jt_ctx* ctx, int64_t n, const float* rays, const float* tmax /* or NULL */,
                  const int32_t* instance /* or NULL */, int32_t* counts /* n */);
int jt_intersect_multi_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance,
                              int32_t k, void* d_hits, void* d_counts);
int jt_count_hits_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_tmax, const void* d_instance, void* d_counts);

/* ---- the surface at a hit ---------------------------------------------------------------- */
/* What the integrator evaluates at a hit (src/scene.jl eval_shading_position, eval_shading_normal,
 * eval_material) and the camera ray it starts from (src/trace.jl sample_camera), for the caller's
 * own records: the position or normal under a pixel, noise-free albedo, normal and depth guide
 * images, baking, probe placement, picking. */
typedef struct jt_surface {   /* 96 bytes, 24 words */
    float position[3];   /* eval_shading_position: the element's interpolated point, in world space */
    float normal[3];     /* eval_shading_normal with outgoing = -d: normal map / vertex normals / element
                            normal, flipped to face -d unless the material is refractive: the
                            integrator's `normal`, the normal AOV's value */
    float gnormal[3];    /* eval_element_normal, never flipped */
    float texcoord[2];   /* eval_texcoord (u, v where the shape has none) */
    float opacity;
    float color[3];      /* material.color * colour texture * vertex colour: the albedo AOV's value */
    float roughness;     /* the material point's: squared, then clamped / zeroed by type (eval_material) */
    float emission[3];
    float metallic;
    int32_t material;    /* index into jt_scene.materials */
    int32_t type;        /* jt_material_type */
    float ior;
    int32_t hit;         /* 1 / 0; on 0 every other word is 0 */
} jt_surface;
/* jt_eval_hits: for record i the surface hits[i] names, as seen along rays[i] (rays as in
 * jt_intersect, n x (o, d)). Only the ray's direction is read and it need not be normalised: it
 * enters through the sign of dot(normal, -d) alone. Instances are numbered as in
 * jt_scene.instances, as in jt_hit. The record is a miss record (all 24 words zero) when
 * hits[i].hit == 0, when the instance is outside 0 .. ninstances-1, when the element is outside
 * the shape's elements, or when u or v is not finite: the kernel checks these before it loads
 * anything the record names, so it stays inside the scene's arrays for any input. A finite uv
 * outside the element is evaluated as given. Every value has the bits the integrator computes
 * at that hit.
 * jt_camera_rays: the W*H camera rays (o, d), row-major pixels. sample >= 0: the ray the
 * integrator traces for (pixel, sample) — the sample's random stream, its four draws, the tent
 * filter if the context has it, the lens sample — bit for bit; sample is not bounded by
 * params.samples. sample == -1: the deterministic ray through the pixel centre, image uv
 * ((i + 0.5f) / W, (j + 0.5f) / H), lens uv (0, 0), no filter. A context with a tile share still
 * produces every pixel.
 * jt_gbuffer: jt_camera_rays, then jt_intersect_device of those rays (scene queries, the
 * context's traversal, the tie re-run included), then jt_eval_hits, in stream order on buffers
 * the context owns; rays and hits are copied out where not NULL. It returns the bits those three
 * calls give. It reports the first geometric hit: the integrator passes through a surface with
 * probability 1 - opacity, the G-buffer never does, so where opacity < 1 the integrator's AOVs
 * can be those of a surface behind.
 * The *_device variants take device pointers on the context's device, run on the context's
 * stream and return when it is idle; d_hits must be aligned to 8 bytes, d_out and d_surfaces to
 * 16, d_rays to 8 where rays are written (any device allocation is; JT_ERR_INVALID otherwise).
 * The host variants stage through buffers the context owns, as the ray queries do. All of this reads the scene and the parameters only: image, AOVs, stream
 * means, variance, the adaptive mask and every jt_counters field stay bit for bit as they were,
 * queued samples stay queued.
 * Errors, in this order: JT_ERR_INVALID (naming the argument) for a NULL ctx, rays, hits or
 * output, n < 0 or n > 2^30, sample < -1, a misaligned device pointer, before the context is looked
 * at and before anything is written; n == 0 returns JT_OK
 * with no device work; JT_ERR_UNSUPPORTED for a multi-device context; JT_ERR_STATE for a failed
 * context. */
int jt_eval_hits(jt_ctx* ctx, int64_t n, const float* rays /* n x 6 */, const jt_hit* hits, jt_surface* out);
int jt_camera_rays(jt_ctx* ctx, int32_t sample, float* rays /* W*H x 6, row-major pixels */);
int jt_gbuffer(jt_ctx* ctx, int32_t sample, float* rays /* W*H x 6, may be NULL */, jt_hit* hits /* W*H, may be NULL */,
               jt_surface* surfaces /* W*H */);
int jt_eval_hits_device(jt_ctx* ctx, int64_t n, const void* d_rays, const void* d_hits, void* d_out);
int jt_camera_rays_device(jt_ctx* ctx, int32_t sample, void* d_rays);
int jt_gbuffer_device(jt_ctx* ctx, int32_t sample, void* d_rays /* may be NULL */, void* d_hits /* may be NULL */,
                      void* d_surfaces);

/* ---- radiance along the caller's rays ---------------------------------------------------- */
/* The path integrator itself (trace_sample, src/trace.jl:584-649: trace_path or trace_naive, the
 * BSDFs, light sampling and MIS) on rays no camera of the context makes: a light probe, a lightmap
 * texel, a lat-long panorama, a fisheye or stereo rig, one path re-traced for debugging.
 * jt_radiance: for every ray i (rays[6 i ..] = origin, direction) the running mean of samples
 * [sample_begin, sample_end), in order. For sample s:
 *   - rng = rng_init(params.seed, stream_base + i, s), the stream the integrator gives pixel
 *     stream_base + i, and the sample prologue's four floats are drawn and discarded (the two
 *     rand2f a camera ray uses);
 *   - the path state starts as trace_sample's does, with (o, d) taken from ray i;
 *   - the context's sampler (trace_path or trace_naive) runs with the context's bounces, nocaustics,
 *     envhidden and clamp, in the traversal the context was created with;
 *   - trace_sample's epilogue: non-finite radiance becomes 0, then the clamp; the target is
 *     (radiance, 1) if a bounce-0 surface was accepted or the ray escaped to a visible environment,
 *     else (0, 0, 0, 0);
 *   - acc = acc * (1 - w) + target * w with w = 1 / (float)(c + 1), c = s - sample_begin, acc from 0,
 *     in float32 without fused multiply-adds, the weight as the integrator computes it.
 * rgba[4 i ..] = acc after the last sample.
 * The direction is used as given. The integrator's camera rays have unit length, and a caller's
 * must too for the BSDF terms to mean anything; it is neither checked nor normalised (normalising
 * would change the bits of camera rays).
 * So with rays = jt_camera_rays(ctx, s), n = W*H, stream_base = 0 and the range [s, s + 1) the
 * result is, bit for bit at every pixel, the image of a context whose first and only traced
 * sample is s. A ray's result depends on the ray, its stream and the sample range only: an array
 * split over several calls, stream_base advanced by the rays already done, gives the bits of one call.
 * The *_device variant takes device pointers on the context's device (d_rgba aligned to 16 bytes),
 * runs on the context's stream and returns when it is idle. The host variant stages through the
 * buffers the ray queries' host variants use.
 * It reads the scene and the parameters only: image, AOVs, stream means, variance, the adaptive
 * mask and every jt_counters field stay bit for bit as they were, queued samples stay queued.
 * Errors, in this order: JT_ERR_INVALID (naming the argument) for a NULL ctx, rays or output,
 * n < 0 or n > 2^30, stream_base < 0 or stream_base + n > 2^31, sample_begin < 0, sample_end <=
 * sample_begin, more than 2^24 samples, a d_rgba not aligned to 16 bytes, before the context is
 * looked at and before anything is written; n == 0 returns JT_OK with no device work;
 * JT_ERR_UNSUPPORTED for a multi-device context; JT_ERR_STATE for a failed context.
 * Non-finite ray components are the caller's responsibility: every lane ends in a bounded number
 * of steps for any input, the result for such a ray is unspecified. */
int jt_radiance(jt_ctx* ctx, int64_t n, const float* rays /* n x (o, d) */, int64_t stream_base,
                int32_t sample_begin, int32_t sample_end, float* rgba /* n x 4 */);
int jt_radiance_device(jt_ctx* ctx, int64_t n, const void* d_rays, int64_t stream_base,
                       int32_t sample_begin, int32_t sample_end, void* d_rgba);

/* ---- cosine-weighted gathers at the caller's points --------------------------------------- */
/* What a lightmap texel, an irradiance probe or an ambient-occlusion map needs: the integrator's
 * mean over the hemisphere at a point, every sample along a direction of its own. jt_radiance
 * keeps one ray for all samples of a record; here the direction is drawn per sample, in the
 * kernel, from the sample's own random stream.
 * A point record is 6 floats, position then normal: the layout of a ray record.
 * jt_irradiance: for every point i (points[6 i ..] = position, normal) the running mean of samples
 * [sample_begin, sample_end), in order. For sample s:
 *   - rng = rng_init(params.seed, stream_base + i, s), as in jt_radiance;
 *   - ruv = rand2f(rng), the first of the sample prologue's two draws (the one that picks the image
 *     position for a camera); the second rand2f is drawn and discarded, so after the prologue
 *     the stream is exactly where jt_radiance leaves it;
 *   - o = position, as given; d = sample_hemisphere_cos(normal, ruv), the matte lobe's own function
 *     (src/shading.jl:716-722): z = sqrt(ruv.y), r = sqrt(1 - z z), phi = 2 pi ruv.x, the local
 *     direction (r cos phi, r sin phi, z) in basis_fromz(normal), which normalises the normal, and
 *     the result normalised;
 *   - from there on everything is jt_radiance's: the path state, the context's sampler, bounces,
 *     nocaustics, envhidden, clamp and traversal, trace_sample's epilogue, the target (radiance, 1)
 *     or (0, 0, 0, 0), and acc = acc * (1 - w) + target * w with w = 1 / (float)(c + 1), in float32
 *     without fused multiply-adds.
 * rgba[4 i ..] = acc after the last sample.
 * jt_hemisphere_rays: rays[6 i ..] = exactly that (o, d) of point i for the one sample `sample`:
 * the position's bits and the direction jt_irradiance draws.
 * The contract: jt_irradiance(points, base, s, s + 1) is, in every bit,
 * jt_radiance(jt_hemisphere_rays(points, base, s), base, s, s + 1), and a range is the float32
 * fold above of its one-sample calls. As in jt_radiance a point's result depends on the point, its
 * stream and the sample range only: an array split over several calls, stream_base advanced by
 * the points already done, gives the bits of one call.
 * What the mean is: the directions have the pdf cos(theta) / pi, so the irradiance at the point
 * is E = pi * rgb, and a matte surface of albedo rho there sends out rho * rgb. alpha is the share
 * of gather rays that met a surface or a visible environment; in a scene without an environment,
 * or with envhidden, 1 - alpha is the cosine-weighted sky visibility: ambient occlusion at
 * unbounded distance. The gather ray is the integrator's bounce 0: an emitter it sees directly
 * counts, and max_roughness starts at 0. The origin lies on the caller's surface as given; the
 * primitive tests' ray_eps keeps the ray from hitting that surface, as it does for the
 * integrator's own bounce rays. With the six axis normals at one position the result is an
 * ambient cube.
 * A zero or non-finite normal or position is the caller's responsibility: every lane still ends
 * in a bounded number of steps, the result for such a point is unspecified.
 * Everything else as jt_radiance: the calls read the scene and the parameters only (image, AOVs,
 * stream means, variance, the adaptive mask and every jt_counters field stay bit for bit as they
 * were, queued samples stay queued); the *_device variants take device pointers on the context's
 * device (d_rgba aligned to 16 bytes, d_rays to 8), run on the context's stream and return when it
 * is idle; the host variants stage through the buffers the ray queries' host variants use.
 * Errors, in jt_radiance's order and with its messages: JT_ERR_INVALID (naming the argument) for a
 * NULL ctx, points or output, n < 0 or n > 2^30, stream_base < 0 or stream_base + n > 2^31, then
 * for jt_irradiance sample_begin < 0, sample_end <= sample_begin, more than 2^24 samples, for
 * jt_hemisphere_rays sample < 0, then a d_rgba not aligned to 16 bytes or a d_rays not aligned to
 * 8, before the context is looked at and before anything is written; n == 0 returns JT_OK with no
 * device work; JT_ERR_UNSUPPORTED for a multi-device context; JT_ERR_STATE for a failed context. */
int jt_irradiance(jt_ctx* ctx, int64_t n, const float* points /* n x (position, normal) */, int64_t stream_base,
                  int32_t sample_begin, int32_t sample_end, float* rgba /* n x 4 */);
int jt_irradiance_device(jt_ctx* ctx, int64_t n, const void* d_points, int64_t stream_base,
                         int32_t sample_begin, int32_t sample_end, void* d_rgba);
int jt_hemisphere_rays(jt_ctx* ctx, int64_t n, const float* points, int64_t stream_base, int32_t sample,
                       float* rays /* n x (o, d) */);
int jt_hemisphere_rays_device(jt_ctx* ctx, int64_t n, const void* d_points, int64_t stream_base, int32_t sample,
                              void* d_rays);

/* ---- ambient occlusion within a radius ---------------------------------------------------- */
/* jt_irradiance's 1 - alpha is ambient occlusion at unbounded distance, which in a closed interior
 * is full occlusion almost everywhere; an occlusion map wants a radius, and one bit per ray, not a
 * path. jt_ambient_occlusion: for point i (points[6 i ..] = position, normal) and every sample s of
 * [sample_begin, sample_end) the ray is exactly jt_hemisphere_rays(points, stream_base, s)'s ray i:
 * the stream (params.seed, stream_base + i, s), the same two draws, the same
 * sample_hemisphere_cos. On it runs the any-hit query bounded by `radius`
 * (jt_occluded_bounded's), in the context's traversal.
 * visibility[i] = (float)(samples whose query found nothing) / (float)(sample_end - sample_begin):
 * one float32 division of two integers that are exact in float32 (at most 2^24 samples), so the
 * value does not depend on the order in which samples finish. One sample is 0.0 or 1.0, namely
 * 1 - jt_occluded_bounded of jt_hemisphere_rays' rays with the radius as every bound, and a range
 * is the count of its one-sample calls over their number. A point's result depends on the point,
 * its stream and the sample range only: an array split over several calls, stream_base advanced by
 * the points already done, gives the bits of one call.
 * radius must be > 0; +inf is allowed and means unbounded. The directions have unit length, so the
 * radius is a distance in the scene's units.
 * The *_device variant takes device pointers on the context's device (d_visibility aligned to 4
 * bytes), runs on the context's stream and returns when it is idle; the host variant stages through
 * the buffers the ray queries' host variants use. The context is read only: image, AOVs, stream
 * means, variance, the adaptive mask and every jt_counters field stay bit for bit, queued samples
 * stay queued.
 * Errors, in jt_radiance's order and with its messages: JT_ERR_INVALID (naming the argument) for a
 * NULL ctx, points or output, n < 0 or n > 2^30, stream_base < 0 or stream_base + n > 2^31,
 * sample_begin < 0, sample_end <= sample_begin, more than 2^24 samples, then a radius that is NaN
 * or <= 0, then a misaligned d_visibility, before the context is looked at and before anything is
 * written; n == 0 returns JT_OK with no device work; JT_ERR_UNSUPPORTED for a multi-device
 * context; JT_ERR_STATE for a failed context. */
int jt_ambient_occlusion(jt_ctx* ctx, int64_t n, const float* points /* n x (position, normal) */, int64_t stream_base,
                         int32_t sample_begin, int32_t sample_end, float radius, float* visibility /* n */);
int jt_ambient_occlusion_device(jt_ctx* ctx, int64_t n, const void* d_points, int64_t stream_base,
                                int32_t sample_begin, int32_t sample_end, float radius, void* d_visibility);

/* ---- spherical-harmonic radiance probes ---------------------------------------------------- */
/* What a grid of light probes for dynamic objects needs: at a position, the incoming radiance over
 * the whole sphere projected onto the nine real spherical harmonics of bands 0..2. jt_irradiance
 * gathers over a hemisphere and returns a mean that is already cosine-convolved; here every sample
 * goes along a uniform direction over the sphere and is weighted by the basis at that direction.
 * A point record is 3 floats, the position.
 * The ray of (point i, sample s), which jt_sphere_rays writes to rays[6 i ..] and jt_probe_sh
 * starts sample s with:
 *   - rng = rng_init(params.seed, stream_base + i, s), as in jt_radiance;
 *   - ruv = rand2f(rng); the second rand2f is drawn and discarded, so after the prologue the
 *     stream is exactly where jt_radiance leaves it;
 *   - o = position, as given (its bits); d = sample_sphere(ruv), which the reference names but
 *     never defines, so the library's own: z = 2 ruv.y - 1, r = sqrt(clamp(1 - z z, 0, 1)),
 *     phi = 2 pi ruv.x, d = normalize((r cos phi, r sin phi, z)) in world axes, with the square
 *     root, sine, cosine and normalize of sample_hemisphere_cos.
 * The basis, in float32, every operation rounded, no fused multiply-adds, in this association,
 * with (x, y, z) = d:
 *   c0 = 0.282095f  c1 = 0.488603f  c2 = 1.092548f  c3 = 0.315392f  c4 = 0.546274f
 *   Y0 = c0            Y1 = c1*y            Y2 = c1*z            Y3 = c1*x
 *   Y4 = c2*(x*y)      Y5 = c2*(y*z)        Y6 = c3*(3.0f*(z*z) - 1.0f)
 *   Y7 = c2*(x*z)      Y8 = c4*(x*x - y*y)
 * jt_probe_sh: for every point i the running mean over samples [sample_begin, sample_end), in
 * order, of target * Y_k. For sample s, target is exactly jt_radiance's rgba target on the ray
 * above: the path state, the context's sampler, bounces, nocaustics, envhidden, clamp and
 * traversal, then trace_sample's epilogue, (radiance, 1) or (0, 0, 0, 0). For k = 0..8 and each of
 * the four channels c:
 *   v = target.c * Y_k;  acc_k.c = acc_k.c * (1 - w) + v * w,  w = 1 / (float)(s - sample_begin + 1)
 * with acc from 0 and the weight as the integrator computes it. sh[(9 i + k) * 4 + c] = acc_k.c
 * after the last sample: nine rgba coefficients per point, 144 bytes.
 * The first step of the fold is 0 * 0 + v * 1, so a product of -0 (zero radiance times a negative
 * Y_k) becomes +0: a one-sample call is that step, not the bare product, and no result of the
 * call holds a -0 that came from a zero target.
 * The contract: jt_probe_sh(points, base, s, s + 1) is, in every bit, that fold step applied to
 * jt_radiance(jt_sphere_rays(points, base, s), base, s, s + 1) and Y(d) of those rays, and a range
 * is the float32 fold above of its one-sample results. A point's result depends on the point, its
 * stream and the sample range only: an array split over several calls, stream_base advanced by the
 * points already done, gives the bits of one call.
 * What the coefficients are: the directions have the pdf 1 / (4 pi), so the radiance field's SH
 * coefficients are L_k = 4 pi * sh_k.rgb, and the irradiance about a unit normal n is
 * E(n) = sum_k A_l(k) L_k Y_k(n) with A = pi, 2 pi / 3, pi / 4 for bands 0, 1, 2. The alpha channel
 * is the same projection of the coverage flag: in a scene without an environment, or with
 * envhidden, c0 - sh_0.a and the higher -sh_k.a are the SH of sky visibility. Coefficient 0 over c0
 * is the plain mean over the sphere.
 * Everything else as jt_radiance: the calls read the scene and the parameters only (image, AOVs,
 * stream means, variance, the adaptive mask and every jt_counters field stay bit for bit as they
 * were, queued samples stay queued); the *_device variants take device pointers on the context's
 * device (d_sh aligned to 16 bytes, d_rays to 8), run on the context's stream and return when it
 * is idle. The host variant of jt_sphere_rays stages through the buffers the ray queries' host
 * variants use; jt_probe_sh's runs the array in chunks of at most 2^22 points through a staging
 * buffer of its own, stream_base advanced, which by the contract gives the bits of one call.
 * rays must not overlap points: the records differ in size.
 * Errors, in jt_radiance's order: JT_ERR_INVALID (naming the argument) for a NULL ctx, points or
 * output, n < 0 or n > 2^30, stream_base < 0 or stream_base + n > 2^31, then for jt_probe_sh
 * sample_begin < 0, sample_end <= sample_begin, more than 2^24 samples, for jt_sphere_rays
 * sample < 0, then a d_sh not aligned to 16 bytes or a d_rays not aligned to 8, before the context
 * is looked at and before anything is written; n == 0 returns JT_OK with no device work;
 * JT_ERR_UNSUPPORTED for a multi-device context; JT_ERR_STATE for a failed context.
 * A non-finite position is the caller's responsibility: every lane still ends in a bounded number
 * of steps, the result for such a point is unspecified. */
int jt_probe_sh(jt_ctx* ctx, int64_t n, const float* points /* n x 3 */, int64_t stream_base,
                int32_t sample_begin, int32_t sample_end, float* sh /* n x 9 x 4 */);
int jt_probe_sh_device(jt_ctx* ctx, int64_t n, const void* d_points, int64_t stream_base,
                       int32_t sample_begin, int32_t sample_end, void* d_sh);
int jt_sphere_rays(jt_ctx* ctx, int64_t n, const float* points /* n x 3 */, int64_t stream_base, int32_t sample,
                   float* rays /* n x 6 */);
int jt_sphere_rays_device(jt_ctx* ctx, int64_t n, const void* d_points, int64_t stream_base, int32_t sample,
                          void* d_rays);

/* zero accumulators (at once if their device pointers were handed out, else before they are
 * next read or overwritten), samples = 0, queued samples dropped */
int jt_reset(jt_ctx* ctx);
/* the accumulators' device pointers, current: queued samples are traced first, and from now on
 * every jt_trace_range traces at once and jt_reset zeroes at once. The image is current when
 * jt_trace_range returns; with k > 1 streams albedo, normal and hits are combined from the
 * streams' means only when read, so through these pointers they are current after
 * jt_synchronize (or jt_get_aovs) */
int jt_get_device_buffers(jt_ctx* ctx, jt_device_buffers* out);
/* Counter level of subsequent launches: 1 (default) counts every jt_counters field; 0 counts
 * paths, rays and light_queries only (the timed production kernel; the other fields are
 * deterministic given seed + BVH and are taken from a level-1 launch of the same range). */
int jt_set_counters(jt_ctx* ctx, int32_t level);
/* NUL-terminated one-line description of the launch configuration the next jt_trace_range
 * uses (kernel instance, LDS/HBM scene mode, stack depth, grid): names the kernel in
 * rocprofv3 traces. Truncated to n bytes. */
int jt_describe(const jt_ctx* ctx, char* buf, int32_t n);
int jt_synchronize(jt_ctx* ctx);
void jt_destroy(jt_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* JTRACE_H */
