// jt_select.h — every integer rule between a laid-out scene and a launch: the feature bits, the
// launch geometry and LDS sizing constants, the kernel families, the table of kernel
// configurations and select_kernel, the one function that answers "which configuration does this
// scene run, in which memory mode, with which stack and which gate". Plain C++ (no HIP runtime),
// shared by the kernels, the device context (jt_trace.hip) and the host check
// (tests/select_check.cpp).
#pragma once

#include <stddef.h>

#include "../../include/jtrace.h"  // JT_TRAVERSAL_*, JT_SAMPLER_*

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JT_SELECT_HD __host__ __device__ inline
#else
#define JT_SELECT_HD inline
#endif

#ifndef JT_AUTO_WIDE_MIN_STACK
#define JT_AUTO_WIDE_MIN_STACK 32  // JT_TRAVERSAL_AUTO: wide records for HBM-mode scenes deeper than this
#endif

namespace jtd {

// Scene feature bits of a kernel specialisation (chosen per scene by jt_create): a kernel built
// without a bit assumes the scene has none of it, so the branches it guards are compiled out.
// FT_ALL is the general kernel; FT_NONE serves scenes of matte triangles without textures,
// vertex attributes, environments or opacity (cornellbox); jt_create picks the smallest compiled
// mask that covers the scene (select_kernel, below). Results are bit-identical.
enum : int {
    FT_TEX = 1,    // material textures (incl. normal maps)
    FT_ATTR = 2,   // shape normals / texcoords / colors
    FT_QUAD = 4,   // quad shapes
    FT_MAT = 8,    // materials other than matte
    FT_ENV = 16,   // environments (escaped rays, environment lights)
    FT_OPAC = 32,  // opacity < 1 possible (material opacity, color-texture or vertex-color alpha)
    FT_VOL = 64,   // refractive / subsurface / volumetric materials (the volume stack)
    FT_XFORM = 128,  // instances whose inverse frame is not exactly the identity
    FT_NONE = 0,
    FT_ALL = 255,
    // kernel build flag, not a scene feature: the scene's light chains run inline
    // (DScene::light_inline; jt_integrator.h light_chain), so the kernel has no light-hit steps
    FT_LINL = 8192,
    // kernel build flag: the scene has no instance light (sample_lights_pdf never queries a BVH)
    FT_NOIL = 16384
};
// a kernel mask of no scene feature (the FT_NONE kernels, with or without the FT_LINL build flag)
JT_SELECT_HD constexpr bool ft_none(int F) { return (F & ~(FT_LINL | FT_NOIL)) == FT_NONE; }

}  // namespace jtd

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
JT_SELECT_HD constexpr bool park(int F) { return JT_PARK != 0 && !ft_none(F); }
JT_SELECT_HD constexpr int park_slots(int F) { return park(F) ? PARK_SLOTS : 0; }

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
JT_SELECT_HD constexpr bool lane_lds(int F) { return JT_LANE_LDS && (!ft_none(F) || JT_LANE_LDS_NONE); }
constexpr int ACC_SLOTS = (JT_LANE_LDS ? 13 : 11) + (JT_PARK ? PARK_SLOTS : 0);  // the host sizes LDS for the larger layout
// Lane-LDS slots: [11] the lane's sample index, [12] its running-mean weight. The FT_NONE
// kernels (JT_LANE_LDS_NONE) recompute the weight from the sample index instead of storing it:
// with 12 slots cornellbox's LDS-mode workgroup still fits 5 per CU.
JT_SELECT_HD constexpr int acc_base_slots(int F) { return lane_lds(F) ? (ft_none(F) ? 12 : 13) : 11; }
// + the parked path state (JT_PARK, Path::pk = acc + acc_base_slots(F) * BLOCK)
JT_SELECT_HD constexpr int acc_slots(int F) { return acc_base_slots(F) + park_slots(F); }

// LDS-mode stack bytes per workgroup: a RING-entry ring with HBM overflow, else the scene's bound
JT_SELECT_HD constexpr size_t lds_stack_bytes(bool ovf, int ring, int need) {
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
JT_SELECT_HD constexpr bool mesh_family(int F) { return (F & ~(FT_LINL | FT_NOIL)) == FT_MESH; }
JT_SELECT_HD constexpr bool mesh_env_quad_family(int F) { return (F & ~(FT_LINL | FT_NOIL)) == FT_MESH_ENV_QUAD; }
// Light-hit steps (trace_body) run in the path-sampler FT_NONE kernel built without FT_LINL:
// matte scenes whose light chains cannot run inline (a light shape BVH of more than one leaf).
// Every other kernel either runs the chains inline (FT_LINL, or DScene::light_inline at run time)
// or, with environments, shades light results in the shading phase.
JT_SELECT_HD constexpr bool light_steps(int sampler, int F) {
    return sampler == 1 && !(F & FT_ENV) && !(F & FT_LINL);
}

// Kernel configurations: (stack ring, HBM overflow, feature mask, LDS-mode kernel too), each in
// the binary traversal (ID 0-7) and the wide one (ID + 8, JT_TRAVERSAL_WIDE). Each is compiled
// in its own translation unit (jt_kv.hip with JT_VARIANT = its index) for both samplers and both
// counter levels; select_kernel picks one, jt_trace.hip launches it through its table of
// launch_cfg pointers.
struct ConfigRow {
    int ring;
    bool ovf;
    int feat;
    bool lds;
};
constexpr int NUM_BASE_CONFIGS = 8;
constexpr ConfigRow CONFIGS[NUM_BASE_CONFIGS] = {
    {16, false, FT_NONE | FT_LINL, true},          // 0 small scenes, matte triangles (cornellbox)
    {16, false, FT_ALL, true},                     // 1 small scenes, any features
    {16, true, FT_MESH | FT_LINL, false},          // 2 deep BVHs: textured meshes (bathroom1)
    {16, true, FT_MESH_ENV | FT_NOIL, false},      // 3 + environments, no instance lights (ecosys)
    {16, true, FT_MESH_ENV_QUAD | FT_LINL, false}, // 4 + quads (features2)
    {16, true, FT_ALL, true},                      // 5 deep BVHs, any features
    {32, true, FT_ALL, true},                      // 6 a 32-entry LDS ring (JT_LDS_STACK)
    {16, false, FT_NONE, true},                    // 7 matte triangles, light chains through the traversal
};
constexpr int NUM_LAUNCH_CONFIGS = 2 * NUM_BASE_CONFIGS;
template <int ID>
struct LaunchConfig {
    static_assert(ID >= 0 && ID < NUM_LAUNCH_CONFIGS, "no such kernel configuration");
    static constexpr int ring = CONFIGS[ID % NUM_BASE_CONFIGS].ring;
    static constexpr bool ovf = CONFIGS[ID % NUM_BASE_CONFIGS].ovf;
    static constexpr int feat = CONFIGS[ID % NUM_BASE_CONFIGS].feat;
    static constexpr bool lds = CONFIGS[ID % NUM_BASE_CONFIGS].lds;
    static constexpr bool wide = ID >= NUM_BASE_CONFIGS;
};

// ============================================================================ the kernel choice
// What select_kernel reads: the laid-out scene (jt_layout.h HostScene), jt_params, and the options
// that bear on the choice, already parsed to integers.
struct SelectIn {
    int feat = FT_ALL;          // scene feature bits
    int need = 16;              // stack bound of the scene (entries)
    size_t blob_bytes = 0;      // the packed small-scene blob
    bool inst_light = false;    // sample_lights_pdf runs instance queries
    bool light_inline = false;  // the scene's light chains can run inline (DScene::light_inline)
    int traversal = JT_TRAVERSAL_AUTO;  // jt_params.traversal
    int sampler = JT_SAMPLER_PATH;      // jt_params.sampler
    size_t lds_scene = 48 * 1024;  // option lds_scene: the blob's byte budget for LDS mode (0: off)
    int lds_stack = 16;            // option lds_stack: entries of the overflow kernels' LDS ring, 16 or 32
    int test_lds_ring = 0;         // option test_lds_ring (tests only; 0: unset): ring entries in use
    int wait_lanes = 0;            // options wait_lanes / light_lanes as given_lanes clamped them
    int light_lanes = 0;           // (0: unset)
};
// The answer, fixed at jt_create: jt_ctx keeps it, the launch, DScene's stack members, DParams'
// gates and jt_describe read it.
struct KernelChoice {
    int id = 1;                  // the configuration (LaunchConfig<id>): row id % 8 of CONFIGS, + 8 wide
    int kmask = FT_ALL;          // feature mask of the kernel specialisation the scene runs
    size_t lds_scene_bytes = 0;  // > 0: small-scene LDS mode, the bytes of the blob; 0: HBM mode
    bool wide = false;           // JT_TRAVERSAL_WIDE: the wide-record kernels (configurations 8-15)
    int traversal = 0;           // jt_params.traversal as resolved (JT_TRAVERSAL_AUTO: near or wide)
    int stack = 16;       // stack bound the kernel runs with (entries); > 16: LDS ring of `ring` + HBM overflow
    int stack_need = 16;  // the scene's own bound (DScene::stack_need, ovf_stride)
    int ring = 16;        // entries of the kernel's LDS stack ring
    int ring_used = 16;   // entries of it in use (DScene::ring)
    bool ovf = false;     // the kernel spills the stack to HBM (stack > 16)
    int wait_lanes = 40, light_lanes = 2;  // DParams
    // option test_lds_ring in effect: fewer ring entries in use than the kernel has
    bool ring_shortened() const { return ring_used < ring; }
};

// the value of the options wait_lanes (hi = 64) and light_lanes (hi = 65: never) when given
inline constexpr int given_lanes(int v, int hi) { return v < 1 ? 1 : v > hi ? hi : v; }

// The bytes of the LDS blob when the scene runs from it, 0 for HBM mode.
// LDS mode only when the blob does not cost workgroups per CU: the kernel holds at most
// 4 workgroups per CU (4 waves/SIMD), so the blob + stack + accumulators may use up to
// 160 KiB / 4, or as much as HBM mode's stack + accumulators already cost. Override
// with the option lds_scene=0 (off) or a byte budget for the blob.
inline constexpr size_t lds_mode_bytes(int feat, int need, size_t bytes, int ring, size_t budget) {
    // HBM mode's stack is the kernel's static ring (16 or 32 entries); LDS mode's, without
    // overflow, just the scene's bound
    // + the texel-decode LUTs a texture kernel keeps in LDS (trace_body)
    const size_t acc_bytes = (size_t)ACC_SLOTS * BLOCK * 4 + ((feat & FT_TEX) ? 2048 : 0);
    const size_t base_bytes = (size_t)(need <= 16 ? 16 : ring) * BLOCK * 4 + acc_bytes;
    const size_t lds_base = lds_stack_bytes(need > 16, ring, need) + acc_bytes;
    const size_t lds_cu = 160 * 1024;
    const size_t wg_hbm = lds_cu / base_bytes < 4 ? lds_cu / base_bytes : 4, wg_lds = lds_cu / (lds_base + bytes);
    return bytes <= budget && wg_lds >= wg_hbm ? bytes : 0;
}

// scene features a kernel mask covers (the build flags are none)
inline constexpr int feature_count(int F) {
    int n = 0;
    for (int b = 1; b <= FT_ALL; b <<= 1) n += (F & b) != 0;
    return n;
}

inline KernelChoice select_kernel(const SelectIn& in) {
    KernelChoice k;
    // ---- memory mode and traversal
    k.lds_scene_bytes = lds_mode_bytes(in.feat, in.need, in.blob_bytes, in.lds_stack, in.lds_scene);
    // auto: wide for a scene in HBM mode whose BVH is deep (a stack bound above 32: bathroom1 46,
    // ecosys 43: +20 %, +30 % over near); near otherwise — features2 (bound 24) runs 2737/2742
    // Mrays/s near vs 2677/2646 wide at 512 spp (gpurun_out/r04m), cornellbox runs from LDS
    k.wide = in.traversal == JT_TRAVERSAL_WIDE ||
             (in.traversal == JT_TRAVERSAL_AUTO && !k.lds_scene_bytes && in.need > JT_AUTO_WIDE_MIN_STACK);
    k.traversal = in.traversal == JT_TRAVERSAL_AUTO ? (k.wide ? JT_TRAVERSAL_WIDE : JT_TRAVERSAL_NEAR) : in.traversal;

    // ---- stack: the whole bound in a 16-entry LDS ring, or a `ring`-entry ring + HBM overflow
    // option test_lds_ring (tests only): use fewer ring entries than allocated, to exercise the
    // overflow. It forces the overflow-capable kernel of the 16-entry ring.
    const int t = in.test_lds_ring;
    const bool shortened = t >= 1 && t <= 16 && (t & (t - 1)) == 0;
    k.stack_need = in.need;
    k.stack = shortened && in.need < 17 ? 17 : in.need;
    k.ovf = k.stack > 16;
    k.ring = k.ovf && !shortened ? in.lds_stack : 16;
    k.ring_used = shortened ? t : in.lds_stack;

    // ---- the configuration: of the rows with this stack — and an LDS-mode kernel for a scene in
    // LDS mode — the smallest compiled superset of the scene's features (the first of equals).
    // The FT_LINL builds need the scene's light chains to run inline; FT_MESH_ENV is built for
    // scenes without instance lights (FT_NOIL: no light queries at all; the chain code cost ecosys
    // 4 spilled VGPRs). Matte scenes whose chains cannot run inline get the FT_NONE build with
    // light-hit steps. An FT_ALL row exists for every stack, with an LDS-mode kernel.
    int row = -1;
    for (int r = 0; r < NUM_BASE_CONFIGS; r++) {
        const ConfigRow& c = CONFIGS[r];
        if (c.ring != k.ring || c.ovf != k.ovf || (k.lds_scene_bytes && !c.lds)) continue;
        if (in.feat & ~c.feat & ~(FT_LINL | FT_NOIL)) continue;
        if (((c.feat & FT_LINL) && !in.light_inline) || ((c.feat & FT_NOIL) && in.inst_light)) continue;
        if (row < 0 || feature_count(c.feat) < feature_count(CONFIGS[row].feat)) row = r;
    }
    k.kmask = CONFIGS[row].feat;
    k.id = row + (k.wide ? NUM_BASE_CONFIGS : 0);

    // ---- the shading gate
    // measured best (cornellbox): 40 waiting lanes per shading phase; 48 with
    // light-hit steps in the traversal phase (they take the light queries out of the phases)
    // light queries leave the shading phase's waiting lanes early (light-hit steps) or never wait
    // there at all (inline chains): the gate then waits for more lanes
    const int smp = in.sampler == JT_SAMPLER_NAIVE ? 2 : 1;
    const bool lstep = in.inst_light && smp == 1 && (light_steps(smp, k.kmask) || in.light_inline);
    // deep BVHs (stack bound > 32: bathroom1, ecosys) shade sooner: their lanes finish queries far
    // apart, so waiting for many leaves the wave idle. Re-swept in round 4 (per-lane work items,
    // short chunks, auto traversal; profiles/r04_ab/wait_lanes_r04o.txt): cornellbox 56 (52
    // even, 48 / 60 -1.3 %, 64 -6 %), features2 56 (60 -2.9 %, 48 -0.5 %, 64 -9 %), bathroom1 40
    // (48 even, 24 -10 %), ecosys (no instance lights) 24 (16 -1.2 %, 32 -2.2 %, 8 -11 %)
    const bool deep = k.stack > 32;
    k.wait_lanes = in.wait_lanes ? in.wait_lanes : lstep ? (deep ? 40 : 56) : deep ? 24 : 40;
    k.light_lanes = in.light_lanes ? in.light_lanes : 2;
    return k;
}

}  // namespace jtk
