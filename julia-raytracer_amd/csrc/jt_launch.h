// jt_launch.h — what the host needs of the megakernel, and nothing of its device code: the launch
// geometry and LDS sizing constants, the kernels' argument records (DAccum, KArgs, DCombine), the
// kernel-family masks with kernel_mask, and the kernel configurations (LaunchConfig) with the
// declaration of their launch function. The device context (jt_context.h) and the accumulation
// kernels (jt_accum.h) include this; the per-lane device functions are in jt_scene_eval.h,
// jt_traverse.h and jt_integrator.h, the kernel body and launch_cfg's definition in jt_kernels.h,
// which only jt_kv.hip includes.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_records.h"

namespace jtk {
using namespace jtd;

// ============================================================================ stack entries, LDS slots
// Unified per-lane stack in LDS, entry = type << 30 | snap << 24 | index (24 bits; jt_create
// checks the scene fits). snap (HBM mode): the query's hit count when a pre-tested child was
// pushed (SNAP_NONE: not pre-tested). Layout stack[k * BLOCK + lane]:
// every lane owns one bank (conflict-free ds_read/write_b32 whatever the per-lane depth).
// The LDS part is a ring of RING entries; when a scene's bound exceeds it (OVF), the oldest
// entries spill to a per-lane HBM area (slot blockIdx.x * BLOCK + threadIdx.x of the persistent
// grid: a query never outlives its lane) and come back one at a time when popped.
constexpr int BLOCK = 256;
constexpr unsigned T_TLAS = 0u, T_INST = 1u, T_BLAS = 2u;
constexpr unsigned IDX_MASK = (1u << 24) - 1;
constexpr unsigned SNAP_NONE = 63u << 24;

// Parked path state (JT_PARK): the radiance sum, the light chain's shading position and the
// nocaustics roughness bound are read only in the shading code, so they live in LDS slots of
// the lane (pk[k * BLOCK], after the running means) instead of registers kept live across the
// traversal loop — where the compiler spilled them to scratch (written back every shading phase).
#ifndef JT_PARK
#define JT_PARK 1
#endif
// pb (sample_bsdfcos_pdf of the bounce) is read once, after the bounce's whole light chain: in
// the FT_LINL mesh kernels the chain runs inline, and a register kept live across it was spilled
// and written back to scratch every shading phase (features2: 9.1 GB of WRITE per launch)
#ifndef JT_PARK_PB
#define JT_PARK_PB 1
#endif
constexpr int PARK_SLOTS = 7 + (JT_PARK_PB ? 1 : 0);  // radiance xyz, max_roughness, lq xyz, pb
// slots: [0, 3) radiance, 3 max_roughness, [4, 7) lq, 7 pb. The mesh kernels park (features2 +6 %,
// bathroom1 +14 %, ecosys +9 %: their spills fell from 12-28 to 0-7 VGPRs). The FT_NONE kernel
// (cornellbox, 2-8 spilled VGPRs either way) does not: its light-hit steps read the light-chain
// position every few traversal iterations, and parking cost 4-11 % there (profiles/r03_park/).
__host__ __device__ constexpr bool park(int F) { return JT_PARK != 0 && !ft_none(F); }
__host__ __device__ constexpr int park_slots(int F) { return park(F) ? PARK_SLOTS : 0; }

// Per-lane running means of the lane's pixel, kept in LDS for the whole launch (a lane owns
// its pixel for all its samples): acc[k * BLOCK], k = 0..3 image rgba, 4..6 albedo, 7..9
// normal, 10 hit count of this launch (int). Loaded from / stored to HBM once per launch; the
// per-sample lerps are the same float operations as a read-modify-write of the HBM buffers.
// JT_LANE_LDS: 11 the lane's current sample (int), 12 its running-mean weight 1/(n+1) — per-sample
// state parked in LDS instead of registers kept live (and spilled) across the traversal loop.
#ifndef JT_LANE_LDS
#define JT_LANE_LDS 1
#endif
// The mesh kernels gain (features2 +7 %, bathroom1 +1 %, ecosys +0.6 %). The FT_NONE kernels
// keep only the sample index (12 slots, the weight is recomputed from it): with 13 slots
// cornellbox's LDS-mode kernel no longer fit 5 workgroups per CU (-9 %); with 12 it does, and
// its spills drop from 37 to 23 VGPRs (scratch 112 -> 80 B/lane, spill write-back 36.3 -> 22.6
// GB per launch, +0.5 %; gpurun_out/ab_ll, s8).
#ifndef JT_LANE_LDS_NONE
#define JT_LANE_LDS_NONE 1
#endif
__host__ __device__ constexpr bool lane_lds(int F) { return JT_LANE_LDS && (!ft_none(F) || JT_LANE_LDS_NONE); }
constexpr int ACC_SLOTS = (JT_LANE_LDS ? 13 : 11) + (JT_PARK ? PARK_SLOTS : 0);  // the host sizes LDS for the larger layout
// Lane-LDS slots: [11] the lane's sample index, [12] its running-mean weight. The FT_NONE
// kernels (JT_LANE_LDS_NONE) recompute the weight from the sample index instead of storing it:
// with 12 slots cornellbox's LDS-mode workgroup still fits 5 per CU.
__host__ __device__ constexpr int acc_base_slots(int F) { return lane_lds(F) ? (ft_none(F) ? 12 : 13) : 11; }
// + the parked path state (JT_PARK, Path::pk = acc + acc_base_slots(F) * BLOCK)
__host__ __device__ constexpr int acc_slots(int F) { return acc_base_slots(F) + park_slots(F); }

// ============================================================================ kernel arguments
struct DAccum {
    float4* image;
    float4* albedo;
    float4* normal;
    long long* hits;
    unsigned long long* counters;  // 7 x u64: paths rays light_queries nodes instances prims shades;
                                   // [8..31]: the stamps build's per-phase clocks (JT_STAMPS)
    unsigned* work;                // unit counters of the launch, one per XCD band at work[16 b]
                                   // (zeroed before each launch)
    // sample-stream means (P.lk > 0): stream j of a pixel at [j * nslot + slot], slot = the pixel's
    // place in the launch's tiles (item_slot: launch tile u * 64 + pixel of the tile), so a tile
    // share stores only its own pixels; image RGBA, albedo xyz + the stream's hit count (int bits
    // in w), normal xyz
    float4* part_img;
    float4* part_alb;
    float4* part_nrm;
    int nslot;  // launch tiles x 64 (the allocation's slots per stream)
};

// The kernels' argument layout (trace_kernel, trace_kernel_lds: by-value arguments in this order,
// each at its natural alignment, as the AMDGPU kernarg segment lays them out).
struct KArgs {
    DScene S;
    DParams P;
    int s_begin, s_end;
    DAccum A;
};

// The launch's last step when k > 1 (combine_kernel, jt_accum.hip): each pixel's stream means
// combined in stream order, mean = sum_j mean_j * w_j over the streams with samples (w_j = n_j /
// n, host-computed in double and rounded once), hits = sum_j hits_j.
struct DCombine {
    float w[JT_MAX_STREAMS];
    int ns;  // streams with samples: min(k, n)
};
// the combine after n local samples of a context with 2^lk streams (jt_plan.h)
inline void combine_weights(long long n, int lk, DCombine& cw) {
    cw = DCombine{};
    cw.ns = combine_weights(n, lk, cw.w);
}

// number of 8x8 tiles a launch covers (DParams tile_stride / tile_offset)
__host__ __device__ __forceinline__ int launch_tiles(const DParams& P) {
    return plan_tiles(P.width, P.height, P.tile_stride, P.tile_offset);
}

// the work-unit counters of a launch (DAccum::work; the work units of jt_kernels.h): one per band
// of tile rows, a band per XCD, BAND_STRIDE words apart
constexpr int NBANDS = 8, BAND_STRIDE = 16;

// LDS-mode stack bytes per workgroup: a RING-entry ring with HBM overflow, else the scene's bound
__host__ __device__ constexpr size_t lds_stack_bytes(bool ovf, int ring, int need) {
    return (size_t)(ovf ? ring : need) * BLOCK * 4;
}

// ============================================================================ kernel families and configurations
// Feature specialisations compiled per stack configuration (besides FT_ALL): FT_NONE for small
// scenes with a 16-entry stack (cornellbox), and three masks for large HBM-mode scenes with the
// ring + HBM overflow stack — textured, attributed meshes (bathroom1), plus environments
// (ecosys), plus quads (features2). FT_NONE, FT_MESH and FT_MESH_ENV_QUAD are FT_LINL builds
// (light chains inline, no light-hit steps); a second FT_NONE build keeps the light-hit steps.
constexpr int FT_MESH = FT_TEX | FT_ATTR | FT_MAT | FT_OPAC | FT_XFORM;
constexpr int FT_MESH_ENV = FT_MESH | FT_ENV;
constexpr int FT_MESH_ENV_QUAD = FT_MESH_ENV | FT_QUAD;
// a kernel mask of one of those families, with or without the light-chain build flags
__host__ __device__ constexpr bool mesh_family(int F) { return (F & ~(FT_LINL | FT_NOIL)) == FT_MESH; }
__host__ __device__ constexpr bool mesh_env_quad_family(int F) { return (F & ~(FT_LINL | FT_NOIL)) == FT_MESH_ENV_QUAD; }
// the kernel mask a scene with feature bits `feat` runs with: the smallest compiled superset.
// `linl`: the scene's light chains can run inline (DScene::light_inline), which the FT_LINL
// builds need; FT_MESH_ENV is built for scenes without instance lights (FT_NOIL: no light
// queries at all; the chain code cost ecosys 4 spilled VGPRs). Matte scenes
// whose chains cannot run inline get the FT_NONE build with light-hit steps.
inline int kernel_mask(int feat, int need, int ring, bool lds, bool linl, bool inst_light) {
    if (need <= 16) return feat == FT_NONE ? (linl ? FT_NONE | FT_LINL : FT_NONE) : FT_ALL;
    if (ring > 16 || lds) return FT_ALL;
    for (int m : {FT_MESH | FT_LINL, FT_MESH_ENV | FT_NOIL, FT_MESH_ENV_QUAD | FT_LINL})
        if (!(feat & ~m & ~(FT_LINL | FT_NOIL)) && ((m & FT_LINL) ? linl : !inst_light)) return m;
    return FT_ALL;
}
// Light-hit steps (trace_body) run in the path-sampler FT_NONE kernel built without FT_LINL:
// matte scenes whose light chains cannot run inline (a light shape BVH of more than one leaf).
// Every other kernel either runs the chains inline (FT_LINL, or DScene::light_inline at run time)
// or, with environments, shades light results in the shading phase.
__host__ __device__ constexpr bool light_steps(int sampler, int F) {
    return sampler == 1 && !(F & FT_ENV) && !(F & FT_LINL);
}

// Kernel configurations: (stack ring, HBM overflow, feature mask, LDS-mode kernel too), each in
// the binary traversal (ID 0-7) and the wide one (ID + 8, JT_TRAVERSAL_WIDE). Each is compiled
// in its own translation unit (jt_kv.hip with JT_VARIANT = its index) for both samplers and both
// counter levels; launch_s (jt_trace.hip) dispatches among them.
constexpr int NUM_BASE_CONFIGS = 8;
template <int ID>
struct LaunchConfig;
#define JT_LAUNCH_CONFIG(ID, R, O, F, L)                            \
    template <>                                                      \
    struct LaunchConfig<ID> {                                        \
        static constexpr int ring = R;                               \
        static constexpr bool ovf = O;                               \
        static constexpr int feat = F;                               \
        static constexpr bool lds = L;                               \
        static constexpr bool wide = false;                          \
    };                                                               \
    template <>                                                      \
    struct LaunchConfig<ID + NUM_BASE_CONFIGS> : LaunchConfig<ID> {  \
        static constexpr bool wide = true;                           \
    };
JT_LAUNCH_CONFIG(0, 16, false, FT_NONE | FT_LINL, true)  // small scenes, matte triangles (cornellbox)
JT_LAUNCH_CONFIG(1, 16, false, FT_ALL, true)             // small scenes, any features
JT_LAUNCH_CONFIG(2, 16, true, FT_MESH | FT_LINL, false)  // deep BVHs: textured meshes (bathroom1)
JT_LAUNCH_CONFIG(3, 16, true, FT_MESH_ENV | FT_NOIL, false)  // + environments, no instance lights (ecosys)
JT_LAUNCH_CONFIG(4, 16, true, FT_MESH_ENV_QUAD | FT_LINL, false)  // + quads (features2)
JT_LAUNCH_CONFIG(5, 16, true, FT_ALL, true)              // deep BVHs, any features
JT_LAUNCH_CONFIG(6, 32, true, FT_ALL, true)              // a 32-entry LDS ring (JT_LDS_STACK)
JT_LAUNCH_CONFIG(7, 16, false, FT_NONE, true)            // matte triangles, light chains through the traversal
#undef JT_LAUNCH_CONFIG
constexpr int NUM_LAUNCH_CONFIGS = 2 * NUM_BASE_CONFIGS;

// defined in jt_kernels.h, instantiated by jt_kv.hip
template <int ID, int SAMPLER, int COUNT>
hipError_t launch_cfg(const DScene& S, const DParams& P, int s0, int s1, const DAccum& A, hipStream_t st, int cus);
// explicit instantiation (JT_KV_INSTANTIATE, in jt_kv.hip) or declaration (elsewhere) of one
// configuration for both samplers and both counter levels
#define JT_KV_FOR(ID, KW)                                                                                    \
    KW hipError_t launch_cfg<ID, 1, 0>(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int); \
    KW hipError_t launch_cfg<ID, 1, 1>(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int); \
    KW hipError_t launch_cfg<ID, 2, 0>(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int); \
    KW hipError_t launch_cfg<ID, 2, 1>(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int);

}  // namespace jtk
