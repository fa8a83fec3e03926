/*
 * jt_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference hot path (Princic-1837592/julia-raytracer, src/trace.jl,
 * src/bvh.jl, src/scene.jl, src/shading.jl, src/sampling.jl, src/geometry.jl, src/math.jl,
 * src/color.jl). Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load it, and only as the checker / the timed CPU baseline — never as the product path.
 *
 * Parity status: the reference cannot run here (no Julia), ships no
 * tests or golden vectors, and draws from an unseeded thread-local Xoshiro RNG. The oracle is
 * pinned statistically against the reference's own render images/cornellbox_path.png
 * (tests/golden/) and structurally against BVH shapes derived from src/bvh.jl.
 */
#ifndef JT_ORACLE_H
#define JT_ORACLE_H

#include "../include/jtrace.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct or_counters {
    uint64_t paths, rays, light_queries, nodes, instances, prims, shades;
} or_counters;

/* make_scene_bvh (src/bvh.jl:66-88), independent of the product's host builder. */
int or_build_scene_bvh(const jt_scene* scene, int32_t high_quality, jt_scene_bvh* out);
void or_free_scene_bvh(jt_scene_bvh* bvh);

/* make_trace_lights (src/trace.jl:117-187). */
int or_make_lights(const jt_scene* scene, jt_lights* out);
void or_free_lights(jt_lights* lights);

/* trace_samples (src/trace.jl:215-274) over global samples [s0, s1) for all W*H pixels into
 * one running mean (one sample stream), weight 1/(s - first + 1). image: W*H*4, albedo/normal:
 * W*H*3, hits: W*H. Rows are split over nthreads pthreads. Returns 0 or a negative jt_status. */
int or_trace(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights,
             const jt_params* params, int32_t width, int32_t height, int32_t first,
             int32_t s0, int32_t s1, float* image, float* albedo, float* normal,
             int64_t* hits, int32_t nthreads, or_counters* counters);

/* Row-restricted variant: pixels of rows [row0, row1) only (bounded CPU samples), with 2^lk
 * sample streams (include/jtrace.h jt_trace_range): for lk > 0 the streams' running means live
 * in part_img (k*W*H*4), part_alb / part_nrm (k*W*H*3) and part_hits (k*W*H), stream-major, and
 * the rows' image / AOVs / hits are their combination after the range. */
int or_trace_rows(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights,
                  const jt_params* params, int32_t width, int32_t height, int32_t row0,
                  int32_t row1, int32_t first, int32_t s0, int32_t s1, float* image,
                  float* albedo, float* normal, int64_t* hits, int32_t lk, float* part_img,
                  float* part_alb, float* part_nrm, int64_t* part_hits, int32_t nthreads,
                  or_counters* counters);

/* The build's env_alias option (include/jtrace.h jt_set_option "env_alias"): environment lights
 * draw their texel through Vose alias tables instead of upper_bound (jt_oracle.c, "alias
 * tables"). Applies to contexts set up after the call (or_trace*). */
void or_set_env_alias(int32_t on);
/* that alias table of one CDF: keep[i] (probability of keeping column i), other[i] (0-based) */
int or_alias_table(const float* cdf, int32_t n, float* keep, int32_t* other);

/* Single-function known-answer entry points (tests/test_oracle_kat.py). */
int or_intersect_triangle(const float* o, const float* d, float tmin, float tmax,
                          const float* p1, const float* p2, const float* p3, float* out_uvt);
int or_intersect_bbox(const float* o, const float* d, float tmin, float tmax,
                      const float* bmin, const float* bmax);
float or_fresnel_dielectric(float eta, const float* normal, const float* outgoing);
void or_rng_first(uint64_t seed, int32_t pixel, int32_t sample, int32_t n, float* out);
void or_inverse_frame(const float* frame, int32_t non_rigid, float* out);
void or_srgb_to_rgb(const uint8_t* bytes, int32_t n, float* out);
/* wide-record property check (tests): records, non-conservative children, leaves, volume ratio x 1000 */
int or_wide_check(const jt_bvh_tree* tlas, const jt_bvh_tree* blas, int32_t nblas, int64_t* out);

/* Ray queries (tests/test_queries_host.py, tests/test_gpu_queries.py). or_query: n rays (o, d: 6
 * floats each) through the traversal params->traversal selects, the tie re-run included; inst NULL
 * or per ray -1 for the scene query, >= 0 for the instance query of that instance. ids: n x
 * (instance in the reference's numbering, element, hit); uvt: n x (u, v, t); counts: n x (hits
 * accepted by the run that reports — the true count, not saturated —, nodes, instances, prims of
 * the whole query). or_query_brute: the closest hit with no BVH (every instance in id order, every
 * element in order, the same transform_ray, intersect_triangle / intersect_quad, tmin = ray_eps,
 * t <= tmax): t n minimal distances (inf: miss), nmin the number of (instance, element) pairs that
 * reach it, mins n x cap such pairs in test order. */
int or_query(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_params* params, int64_t n, const float* rays,
             const int32_t* inst, int32_t* ids, float* uvt, int64_t* counts);
int or_query_brute(const jt_scene* scene, int64_t n, const float* rays, const int32_t* inst, float* t, int32_t* nmin,
                   int32_t* mins, int32_t cap);
/* the ray (o, d: 6 floats) an instance visit traces: transform_ray by inverse(frame, true) */
void or_instance_ray(const float* frame, const float* o, const float* d, float* out);

/* Single-primitive probes: op `op` of the table below over n lanes, `in` n x nin floats, `out`
 * n x nout floats (booleans as 0.0f / 1.0f). The ops, their ids and widths are those of the device
 * probe library (tests/probe/jt_probe.hip jp_run); a CPU test compares the two tables. Returns 0,
 * or -1 for an unknown op. */
int or_probe(int op, int64_t n, const float* in, float* out);
int or_probe_count(void);
const char* or_probe_name(int op);
int or_probe_nin(int op);
int or_probe_nout(int op);
/* eval_texture of one texture (bytes or floats, 4 per texel) at n lookups q = n x (u, v, as_linear). */
int or_probe_texture(int32_t width, int32_t height, int32_t linear, const uint8_t* pixelsb, const float* pixelsf,
                     int64_t n, const float* q, float* out);

#ifdef __cplusplus
}
#endif

#endif
