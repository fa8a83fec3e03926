// jt_records.h — the device records of the MI355X path tracer: what jt_layout.cpp writes on the
// host and the kernels (jt_device.h, jt_kernels.h and its headers) read. Plain data: it compiles in a host-only
// C++ translation unit (-D__HIP_PLATFORM_AMD__) as well as in HIP.
#pragma once

#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "jt_plan.h"  // the stream-count constants (JT_MAX_STREAMS, JT_STREAM_ITEMS_MAX, ...)
#include "jt_select.h"  // the feature bits (FT_*), the launch constants and the kernel choice

// jt_trace_range defers its range until this many samples are queued (jt_ctx::pend0)
#define JT_DEFER_SAMPLES 64
#ifndef JT_EXACT_MATH
#define JT_EXACT_MATH 1
#endif

namespace jtd {

// ------------------------------------------------------------------------------ layout in HBM
// BVH node, 32 B = two 16-B loads: a = (bmin.x, bmax.x, bmin.y, bmax.y), b = (bmin.z, bmax.z,
// start bits, meta bits), each axis's slab planes side by side. meta = num | axis << 16 |
// internal << 24. TLAS nodes come first (breadth-first), then every BLAS; `start` is a global
// node index (internal), a triangle-pair / quad record slot (BLAS leaf) or, for a TLAS leaf, its
// first instance: the device numbers instances in TLAS leaf order (bvh.primitives[i] of the
// reference becomes instance i), so a leaf's instances are start .. start+num-1.
struct alignas(16) DNode {
    float4 a, b;
};
// Wide (4-ary) node record, 64 B = four 16-B loads: the traversal jt_params.traversal =
// JT_TRAVERSAL_WIDE. A record stands for an internal binary node N of the
// reference's tree (or a leaf root) and holds N's grandchildren: N's two children, each internal
// child replaced by its own two children, so one visit tests up to four boxes and a DFS visits the
// reference's leaves in the binary order. The boxes are conservative 8-bit quantisations relative
// to N's box (dequantised lo = origin + q * scale in float, never above the exact bmin; hi never
// below bmax), tested with the reference's intersect_bbox:
//   r0: origin.xyz = N's bmin, meta bits = ex | ey << 8 | ez << 16 | (a0 | a1 << 2 | a2 << 4) << 24
//       (scale of an axis = the float with biased exponent e, 2^(e - 127); a0 = N's split axis,
//       a1 / a2 the split axes of N's children L / R, 0 for a leaf child)
//   r1: bytes lo.x[4] hi.x[4] lo.y[4] hi.y[4] of slots 0..3; r2: lo.z[4] hi.z[4], 0, 0
//   r3: child words of slots [LL, LR, RL, RR] (a leaf child L / R takes slot 0 / 2 alone)
// child word: W_EMPTY; bit 31 clear: a record index; bit 31 set: a leaf, bit 30 set for a TLAS
// leaf (instances start .. start + num - 1), bits 28-29 num - 1, bits 0-27 start (first instance,
// triangle-pair record or quad record)
struct alignas(16) DWide {
    float4 r0;
    uint4 r1, r2;
    uint4 r3;
};
enum : unsigned { W_EMPTY = 0xffffffffu, W_LEAF = 0x80000000u, W_INST = 0x40000000u, W_START = 0x0fffffffu };
// Traversal record of an instance, 64 B: inverse(frame, true) as 12 floats + ids.
struct alignas(16) DInstTrav {
    float4 i0, i1, i2;  // inv x.xyz y.x | y.yz z.xy | z.z o.xyz
    int shape, blas_root, kind, prim_base;
};
// Shading record of an instance, 64 B: frame (12 floats) + material / shape ids.
struct alignas(16) DInstShade {
    float4 f0, f1, f2;
    int material, shape, mat_type;
    int rot_identity;  // frame x, y, z are exactly the unit axes: element normals from enrm_id
};
enum { KIND_TRI = 0, KIND_QUAD = 1 };
struct alignas(16) DShape {
    int kind, blas_root, prim_base, idx_base;
    int pos_base, nrm_base, tc_base, col_base;  // -1 = absent
};
struct alignas(16) DMaterial {
    int type, emission_tex, color_tex, roughness_tex;
    int scattering_tex, normal_tex, pad0, pad1;
    float emission[3], roughness;
    float color[3], metallic;
    float scattering[3], ior;
    float scanisotropy, trdepth, opacity, pad2;
};
struct alignas(16) DTexture {
    int width, height, linear, is_float;
    long long offset;  // texel index into texb (uchar4) or texf (float4)
    long long pad;
};
struct alignas(16) DEnv {
    float frame[12];
    float inv[12];  // inverse(frame) rigid (src/scene.jl:906)
    float emission[3];
    int tex;
};
// One element of an instance light, as light_hit reads it (5 float4): its object-space vertex
// positions p1 p2 p3 (p4 for a quad in row 4), the element normal light_hit transforms (enrm, or
// enrm_id already final when the instance frame has no rotation), the light's area (last of its
// CDF), the rot_identity flag and the shape kind. The same floats as the arrays they come from:
// light_hit's results are unchanged, from 4-5 loads instead of 10.
//   row 0: p1.xyz p2.x | row 1: p2.yz p3.xy | row 2: p3.z n.xyz | row 3: area rot kind 0 | row 4: p4.xyz 0
struct alignas(16) DLight {
    int instance, environment, cdf_offset, ncdf;
    // guide table of a long CDF (env lights; nguide = 0: plain binary search): thresholds
    // guide_t[k] (float) and guide_a[k] = first 0-based index i with cdf[i] > guide_t[k]
    int guide_offset, nguide;
    float guide_scale;  // nguide / last(cdf): first guess of the bucket of a limit
    // JT_ENV_ALIAS=1 (statistical variant, not the default): offset of an environment light's
    // Vose alias table in DScene::alias (ncdf entries), -1 = none
    int alias_offset;
};

struct DScene {
    const DNode* nodes;      // TLAS nodes, then every BLAS (global node indices)
    const DWide* wnodes;     // the wide traversal's records: TLAS records, then every BLAS's
    int tlas_wnodes;         // TLAS records (a record index below it is a TLAS record)
    const float4* prims;  // triangle pair: 5 float4 (p1, p2-p1, p3-p1 of two triangles interleaved,
                          // then both element ids); quad: 4 float4 (p1|elem, p2, p3, p4|p3==p4)
    const DInstTrav* inst_trav;
    const int4* inst_blas;  // per instance: blas_root, identity-transform flag, kind, shape
    const DInstShade* inst_shade;
    const DShape* shapes;
    const float4* pos;
    const float4* nrm;
    const float2* tc;
    const float4* col;
    const int4* elems;  // triangle (a,b,c,0) / quad (a,b,c,d), global vertex ids
    // per element, precomputed on the host with the device's float operations:
    // triangle_normal / quad_normal in object space, and transform_normal of it by an
    // identity-rotation frame (eval_element_normal of an instance whose frame has no rotation)
    const float4* enrm;
    const float4* enrm_id;
    const DMaterial* materials;
    const DTexture* textures;
    const uchar4* texb;
    const float4* texf;
    const DEnv* envs;
    const DLight* lights;
    // light-hit records (light_hit, src/trace.jl:1024-1044): per light (instance, first record,
    // 0, 0), and per element of an instance light's shape one 80-B record of what light_hit
    // reads, gathered on the host (DLightElem)
    const int4* light_hit;
    const float4* light_elems;
    const float* cdf;
    const float* guide_t;   // DLight guide tables (thresholds / first indices)
    const int* guide_a;
    const float2* alias;    // DLight alias tables: (keep probability, alias index bits) per texel
    const float* srgb_lut;  // srgb_to_rgb(byte_to_float(b)), 256 entries (src/color.jl:12-23)
    const float* byte_lut;  // byte_to_float(b)
    int tlas_nnodes, nenvs, nlights;
    int order_flip;  // jt_params.traversal: 0 the reference's child order, 7 the near child first
                     // (near and wide)
    float light_pick_pdf;  // sample_uniform_pdf(nlights) = Float32(1 / nlights) (src/sampling.jl:31)
    int light_inline;  // every instance light's shape BVH is one leaf: light chains run inline (jtk::light_chain)
    // Small-scene mode: every array above that the traversal and shading read per step, packed
    // in one 16-B aligned blob the workgroup copies into LDS at kernel start (offsets in 16-B
    // units; -1 = not in the blob). Texels, environments and LUTs stay in HBM.
    const uint4* blob;
    int blob_n16;
    // traversal-stack overflow (scenes deeper than the LDS ring): ovf_stride entries per pixel
    int* ovf;
    int ovf_stride;
    int ring;  // entries of the LDS ring in use (a power of two <= the kernel's RING)
    int stack_need;  // stack bound of the scene: LDS-mode kernels without overflow allocate this many
    int o_wnodes;
    int o_nodes, o_prims, o_inst_trav, o_inst_blas, o_inst_shade, o_shapes;
    int o_pos, o_nrm, o_tc, o_col, o_elems, o_materials, o_lights, o_cdf, o_enrm, o_enrm_id;
    int o_light_hit, o_light_elems;
};

struct DCamera {
    float frame[12];
    int orthographic;
    float lens, film, aspect, focus, aperture;
    float film_x, film_y;  // the film vector of eval_camera (src/scene.jl:377-378), host-computed
    int pinhole;           // aperture is +0: only the signs of sample_disk matter
};

struct DParams {
    DCamera cam;
    int width, height;
    int bounces, sampler;
    float clamp;
    int envhidden, tentfilter, nocaustics;
    int first;  // running-mean origin: local sample t = s - first
    // sample streams (DESIGN.md §2 "Sample streams"): local sample t belongs to stream
    // t & (2^lk - 1) and is the (t >> lk)-th sample of that stream's own running mean, weight
    // 1/((t >> lk) + 1); the launch ends by combining the streams' means (jt_accum.hip combine)
    int lk;
    int wait_lanes;
    int light_lanes;  // path sampler: run a light-hit step inside the traversal phase once this
                      // many lanes wait on a sample_lights_pdf query result (65: never)
    // the 8x8 tiles this launch covers: every tile_stride-th from tile_offset (a multi-device context
    // split by pixel tiles, jt_create_multi; 1 / 0 otherwise: every tile)
    int tile_stride, tile_offset;
    float tile_stride_rcp;  // 1.0f / (float)tile_stride (jtk::tile_stride_rcp), set wherever tile_stride is
    unsigned long long seed;
};

}  // namespace jtd
