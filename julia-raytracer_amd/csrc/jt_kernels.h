// jt_kernels.h — the MI355X (gfx950) path-tracing megakernel: the kernel body, the two kernels and
// their launch. Its per-lane device functions are in jt_scene_eval.h, jt_traverse.h and
// jt_integrator.h; what the host needs of it in jt_launch.h (argument records) and jt_select.h
// (masks, configurations).
//
// Replaces trace_samples (Princic-1837592/julia-raytracer src/trace.jl:215-274) and everything
// it calls per (pixel, sample, bounce): trace_sample :584, trace_path :276 / trace_naive :471,
// intersect_scene_bvh / intersect_shape_bvh / intersect_instance_bvh (src/bvh.jl:306-520),
// scene evaluation (src/scene.jl:372-928), shading (src/shading.jl), sampling (src/sampling.jl).
//
// Design: one lane owns one pixel and loops over its samples with path
// regeneration — a lane whose path terminated starts its next sample in the same loop
// iteration in which other lanes continue bouncing, so the wave stays full. Two-level BVH
// traversal is one loop over a unified per-lane stack in LDS (TLAS nodes, instance entries,
// BLAS nodes) so that every lane does one stack pop per iteration whatever level it is at;
// the traversal order (and hence hit tie-breaking) is exactly the reference's. The running
// mean (lerp with w = 1/(s+1), src/trace.jl:631-648) is kept in LDS across samples and
// written once per work unit.
//
// Build: every kernel configuration (CONFIGS, jt_select.h) is instantiated in its own
// translation unit (jt_kv.hip, compiled once per configuration, the only file that includes this
// header) so the kernels compile in parallel, and once more with the kernels' last template
// argument ADAPT set, for the contexts that jt_adapt has touched; the host context
// (jt_trace.hip) only declares them (jt_launch.h). The records the kernels read are declared in jt_records.h (through jt_device.h)
// and written on the host by jt_layout.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "jt_integrator.h"
#include "jt_launch.h"

namespace jtk {
using namespace jtd;

#ifndef JT_STAMPS
#define JT_STAMPS 0
#endif
// pops per node iteration: the LDS-mode FT_NONE kernel (cornellbox) gains with 4 (+1.2 %),
// the HBM-mode mesh kernels lose with 4 or 2 (bathroom1 -4 %, ecosys -1.5 %; gpurun_out/ab_nr)
#ifndef JT_NODE_REPEAT_NONE
#define JT_NODE_REPEAT_NONE 4
#endif
#ifndef JT_NODE_REPEAT
#define JT_NODE_REPEAT 3
#endif
// stack pops of a new query run where it is issued, in the shading phase (most lanes take part)
// rather than in sparser traversal iterations: 2 in the FT_LINL mesh kernels since inline light
// chains (features2 +1.5 %, bathroom1 even; cornellbox -0.4 % with 2,
// profiles/r03_inline/ab_fp_nr.txt), 1 in the others (ecosys lost 7 % with 2)
#ifndef JT_FIRST_POP_NONE
#define JT_FIRST_POP_NONE 1
#endif
#ifndef JT_FIRST_POP
#define JT_FIRST_POP 2
#endif
// the first pops of a query issued in a kernel with mask F
template <int F>
constexpr int first_pops() { return !ft_none(F) && (F & FT_LINL) ? JT_FIRST_POP : JT_FIRST_POP_NONE; }
#ifndef JT_VOTE_P
#define JT_VOTE_P 3
#endif
#ifndef JT_VOTE_N
#define JT_VOTE_N 1
#endif
#ifndef JT_RAY_FROM_PATH
#define JT_RAY_FROM_PATH 1
#endif

// active lanes of a ballot, as a 32-bit scalar (keeps the comparisons of counts on the SALU)
__device__ __forceinline__ int lane_count(unsigned long long m) {
    return __builtin_popcount((unsigned)m) + __builtin_popcount((unsigned)(m >> 32));
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// JT_KARG_RELOAD: the launch's sample range and accumulator pointers are read from the kernel
// argument segment (a scalar load through the kernarg pointer, laundered so it is not hoisted)
// where they are used — at a work unit's fetch, an item's start and end — instead of being kept in
// SGPRs across the path loop, where the register allocator spilled them to VGPR lanes and reloaded
// them with v_readlane (a VALU instruction and a hazard wait each) in every shading phase.
// Measured against keeping them (two runs each, interleaved, profiles/r06_ab/karg_reload_r06karg.txt):
// cornellbox +3.1 %, bathroom1 1920x1080x64 +1.8 %, ecosys 3840x2160x8 +11 %, features2 -1.5 % (its
// kernel's VGPR spills rose from 3 to 6), so the FT_MESH_ENV_QUAD kernel keeps them in registers.
#ifndef JT_KARG_RELOAD
#define JT_KARG_RELOAD 1
#endif
template <int F>
__host__ __device__ constexpr bool karg_reload() {
    return JT_KARG_RELOAD && !mesh_env_quad_family(F);
}
template <class T>
__device__ __forceinline__ T karg(size_t off) {
    typedef __attribute__((address_space(4))) const char* kptr;
    kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const __attribute__((address_space(4))) T*)(p + off);
}
// JT_KARG_SCENE (HBM-mode kernels, whose scene is the kernel argument itself): the shading phase
// reads the scene's fields through the kernarg segment too (one scalar load per field used there,
// re-issued every phase), instead of keeping every pointer the shading code needs live in SGPRs
// across the traversal loop. Measured (two runs each, interleaved, profiles/r06_ab/
// karg_scene_r06ks.txt): features2 1920x1080x64 +3.7 %, materials2 +1.4 %, features1 +0.9 %,
// ecosys +0.8 %, cornellbox (LDS mode: not used) even; bathroom1 -2.1 %, so the FT_MESH kernel
// keeps its scene in registers.
#ifndef JT_KARG_SCENE
#define JT_KARG_SCENE 1
#endif
template <bool NCACHE, int F>
__host__ __device__ constexpr bool karg_scene() {
    return NCACHE && JT_KARG_SCENE && !mesh_family(F);
}
template <bool FROM_KARG>
__device__ __forceinline__ const DScene& shade_scene(const DScene& S) {
    if constexpr (FROM_KARG) {
        typedef __attribute__((address_space(4))) const char* kptr;
        kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return *(const DScene*)(const __attribute__((address_space(4))) DScene*)(p + offsetof(KArgs, S));
    } else {
        return S;
    }
}
// JT_KARG_PARAMS: the sample start and the shading phase read the render parameters (camera,
// bounces, clamp, flags) through the kernarg segment too (the cornellbox kernel's SGPR spills
// 36 -> 16, VGPR spills 1 -> 0). Two runs each (profiles/r06_ab/karg_params_r06kp.txt): cornellbox
// +0.7 %, ecosys +1.0 %, features2 +0.9 %, materials2 +0.2 %; config 1's naive kernel -0.8 % and
// bathroom1 -0.5 %, so the path-sampler kernels other than FT_MESH use it
#ifndef JT_KARG_PARAMS
#define JT_KARG_PARAMS 1
#endif
template <int SAMPLER, int F>
__host__ __device__ constexpr bool karg_params_on() {
    return JT_KARG_PARAMS && SAMPLER == 1 && !mesh_family(F);
}
template <bool FROM_KARG>
__device__ __forceinline__ const DParams& karg_params(const DParams& P) {
    if constexpr (FROM_KARG) {
        typedef __attribute__((address_space(4))) const char* kptr;
        kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return *(const DParams*)(const __attribute__((address_space(4))) DParams*)(p + offsetof(KArgs, P));
    } else {
        return P;
    }
}
// JT_KARG_SCENE_LDS: the same in the LDS-mode kernels, whose scene is the blob view of the kernel
// argument (blob_scene): the shading phase rebuilds the view from the kernarg segment (the
// cornellbox kernel's SGPR spills 53 -> 36; two runs each, profiles/r06_ab/karg_scene_lds_r06ksl.txt:
// cornellbox +0.35 %, its 1/8 share +0.3 %, config 1 even)
#ifndef JT_KARG_SCENE_LDS
#define JT_KARG_SCENE_LDS 1
#endif
__device__ __forceinline__ DScene blob_scene(const DScene& S, const uint4* blob);
template <bool NCACHE, int RING, bool OVF, int F>
__device__ __forceinline__ DScene shade_scene_lds(const DScene& S0) {
    if constexpr (!NCACHE && JT_KARG_SCENE_LDS) {
        extern __shared__ uint4 dyn_lds[];
        const DScene& K = shade_scene<true>(S0);
        return blob_scene(K, dyn_lds + lds_stack_bytes(OVF, RING, K.stack_need) / 16);
    } else {
        return S0;
    }
}
#define JT_A(f) (karg_reload<F>() ? karg<decltype(DAccum::f)>(offsetof(KArgs, A) + offsetof(DAccum, f)) : A.f)
#define JT_SB (karg_reload<F>() ? karg<int>(offsetof(KArgs, s_begin)) : s_begin)
#define JT_SE (karg_reload<F>() ? karg<int>(offsetof(KArgs, s_end)) : s_end)

// Work units: (8x8 pixel tile t, stream slot q), fetched by whole waves from atomic counters, so
// every wave stays busy until the launch's last units. The tiles are split into 8 bands of rows,
// one per XCD: a wave drains its own XCD's band first (neighbouring pixels share that XCD's L2),
// then helps the other bands. Within a band units are numbered tile-major: a tile's stream slots
// are consecutive units, so the waves running at one time trace the same pixels' samples (the
// first bounces share nodes and texels in the XCD's L2). Measured against stream-major numbering
// (gpurun_out/r05x, two runs each): features2 +4.5 %, ecosys +1.1 %, bathroom1 +0.6 %,
// cornellbox +0.4 %. NBANDS and BAND_STRIDE, which size the counters: jt_launch.h.

#ifndef JT_BAND_STRIP
// tile rows per strip of a band's unit order (1: row-major). Measured against row-major
// (gpurun_out/r05st, r05st2, two runs each): 16 rows cornellbox +2.0 %, features2 +1.1 %, ecosys
// +1.1 %; 8 rows cornellbox +1.3 %, features2 +1.4 %, ecosys +1.1 %, bathroom1 +0.4 %; 4 rows
// and 32 rows in between
#define JT_BAND_STRIP 16
#endif

// ============================================================================ sample streams + per-lane work items
// Sample streams: the samples of a pixel are dealt to k = 2^P.lk streams (local sample t = s -
// first goes to stream t mod k), and each stream keeps its own running mean (src/trace.jl:631-648,
// weight 1/(c + 1) for the stream's c-th sample). A (pixel, stream) item is one lane's work for
// the launch: its samples in order, then one store of the stream's means. Items are independent
// of each other — no item waits for another — so a launch has W·H·min(k, samples) concurrent
// items however few pixels it covers, and the launch ends by combining each pixel's stream means
// in stream order (combine_kernel, weights n_j / n). k = 1 is the reference's own single running
// mean (the image buffer is stream 0): one sample per launch reads and writes it here; a longer
// range runs as chunks of one-sample streams folded in sample order (chain_kernel, jt_accum.hip).
// Results depend on k (fixed per context, jt_get_streams) and not on how a render is split into
// calls or launches.
//
// Per-lane work items: the work units are (8x8 tile, stream), fetched by whole waves, but a lane
// is not tied to its wave's unit: a lane that has finished its item takes the next pixel of its
// wave's current unit at once, and the wave fetches the next unit when every pixel of the
// current one has been handed out. A wave therefore never waits for the slowest lane of a unit;
// lanes hold pixels of at most a few consecutive units, so neighbouring lanes stay spatially
// close. The wave-level hand-out is a ballot and a prefix count (mbcnt): the k-th needy lane
// takes pixel bnext + k.
// JT_ITEM_FIRST_POP: a sample's first node pops run at its start, in the hand-out, where most of
// the wave's lanes start samples together (1: every kernel, 0: none, 2: the binary-order mesh
// kernels only). Measured in round 4 (profiles/r04_ab/knobs*_r04[rs].txt, two runs each), off
// against on: cornellbox +0.4 % (10317/10318 vs 10273/10277 Mrays/s), bathroom1 and ecosys (wide)
// +1.2 % and even, features2 (near, mesh) -1.5 % (2666/2679 vs 2722/2709). 2.
#ifndef JT_ITEM_FIRST_POP
#define JT_ITEM_FIRST_POP 2
#endif
template <bool WIDE, int F>
__host__ __device__ constexpr bool item_first_pop() {
    return JT_ITEM_FIRST_POP == 1 || (JT_ITEM_FIRST_POP == 2 && !WIDE && !ft_none(F));
}
// a lane's item: its pixel's image coordinates, (j << 16) | i (item_encode, jt_plan.h; jt_create
// keeps width and height within JT_ITEM_MAX_DIM); ITEM_NONE: no pixel. The item's stream and sample
// live in the lane's LDS slot [11] (its current global sample). The hand-out has i and j in hand;
// the sample start and the item's store take them back by shifts and masks, where recovering them
// from tile * 64 + l took two divisions by the tile columns and two by the width each.
// JT_ITEM_COORDS, measured against the tile form (three runs each, interleaved,
// profiles/item_sqrt_rcp/ab_headline.txt, ab_others.txt): cornellbox +1.0 %; features2 1920x1080x64
// -1.4 % (its kernel, which keeps the launch's arguments in registers, spilled 76 SGPRs instead of
// 61), so the FT_MESH_ENV_QUAD kernels keep the tile form: the item is tile * 64 + l (jt_create
// keeps tiles below 2^20), its pixel is item_pixel's.
#ifndef JT_ITEM_COORDS
#define JT_ITEM_COORDS 1
#endif
template <int F>
__host__ __device__ constexpr bool item_coords() {
    return JT_ITEM_COORDS && !mesh_env_quad_family(F);
}
// tile form: the image index of an item's pixel (its slot holds the global tile and the pixel of the tile)
__device__ __forceinline__ int item_pixel(unsigned item, const DParams& P, int tiles_x) {
    const int t = (int)(item >> 6), l = (int)(item & 63u);
    return ((t / tiles_x) * 8 + (l >> 3)) * P.width + (t % tiles_x) * 8 + (l & 7);
}
// the item of pixel (i, j), pixel l of tile ut
template <int F>
__device__ __forceinline__ unsigned item_of(int ut, int l, int i, int j) {
    return item_coords<F>() ? item_encode(i, j) : (unsigned)(ut * 64 + l);
}
// the image index of an item's pixel
template <int F>
__device__ __forceinline__ int item_pixel_index(unsigned item, const DParams& P, int tiles_x) {
    return item_coords<F>() ? item_j(item) * P.width + item_i(item) : item_pixel(item, P, tiles_x);
}
// an item's slot among the launch's tiles (DAccum::part_*; item_slot, jt_plan.h): the inverse of
// slot_pixel, with the host's reciprocal of the tile stride (DParams::tile_stride_rcp)
template <int F>
__device__ __forceinline__ int item_slot(unsigned item, const DParams& P) {
    if constexpr (item_coords<F>()) return item_slot(item, (P.width + 7) >> 3, P.tile_offset, P.tile_stride_rcp);
    else {
        // the tile form computes the reciprocal itself, as a scalar (wave-uniform and loop-invariant:
        // hoisted out of the persistent loop it would hold a VGPR for the whole kernel): with the
        // host's, one more launch argument stayed live in this family's registers (features2 -0.7 %)
        const float inv = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(1.0f / (float)P.tile_stride)));
        return launch_tile((int)(item >> 6), P.tile_offset, inv) * 64 + (int)(item & 63u);
    }
}
// running-mean weight of global sample s within its stream
__device__ __forceinline__ float stream_weight(const DParams& P, int s) {
    return jl_rcp_weight((float)(((s - P.first) >> P.lk) + 1));
}

#if JT_STAMPS
#define JT_STAMP(x) x
#else
#define JT_STAMP(x)
#endif

// ADAPT: the twin an adapted context launches (jt_adapt, jt_adapt.hip): its hand-out skips the
// units of frozen tiles. Every other instantiation holds no trace of it.
template <int SAMPLER, int RING, bool OVF, int COUNT, int F, bool NCACHE, bool WIDE, bool ADAPT = false>
__device__ __forceinline__ void trace_body_items(const DScene& S0, const DParams& P0, int s_begin, int s_end,
                                                 const DAccum& A, int* stack) {
    const DScene& S = S0;
    const DParams& P = P0;
    static_assert(lane_lds(F), "the per-lane item body keeps the lane's sample index in LDS");
    constexpr int PB = push_bit(node_baked<OVF, NCACHE, WIDE, F>());  // the push mask's bit of a baking kernel
    constexpr bool SB = shade_baked<OVF, NCACHE, WIDE, F>();          // its matte bounces read the baked shading
    const int lane = threadIdx.x & 63;
    const int oslot = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // the lane's HBM stack-overflow area
    if constexpr ((F & (FT_TEX | FT_ENV)) != 0) {  // the texel-decode LUTs into LDS (tex_lut)
        for (int k = threadIdx.x; k < 512; k += BLOCK) tex_lut[k] = k < 256 ? S.srgb_lut[k] : S.byte_lut[k - 256];
        __syncthreads();
    }
    Counters cnt{0, 0, 0, 0};
    // Paths, scene rays and light queries are counted per wave, never in per-lane registers
    // (three VGPRs live across the traversal loop, spilled and written back every shading
    // phase: 14 GB of scratch write-back per cornellbox launch).
    // WC (mesh kernels): ballots at wave-uniform points, summed in scalar registers (bathroom1
    // +3 %, features2 +1 % over per-lane counters). The FT_NONE kernel, whose light-hit steps run
    // every few iterations, adds to three per-wave LDS words instead (ds_add, no ballot).
    constexpr bool WC = !ft_none(F);
    unsigned w_paths = 0, w_rays = 0, w_lq = 0;
    __shared__ unsigned wave_cnt[WC ? 1 : (BLOCK / 64) * 4];
    unsigned* const wcnt = wave_cnt + (WC ? 0 : (threadIdx.x >> 6) * 4);
    if (!WC && lane < 3) wcnt[lane] = 0u;
    auto lds_count = [&](int k, bool c) {
        if (c) __hip_atomic_fetch_add(wcnt + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    __shared__ float acc_lds[acc_slots(F) * BLOCK];
    float* acc = acc_lds + threadIdx.x;
    int* const acc_i = reinterpret_cast<int*>(acc);
#if JT_STAMPS
    // per-phase wave clocks, step lanes, shading-phase material coherence (scripts/stamps.py)
    unsigned long long t_trav = 0, t_shade = 0, n_trav = 0, n_shade = 0, lanes_p = 0, lanes_n = 0, steps_p = 0, steps_n = 0;
    unsigned long long t_hit = 0, t_fin = 0, t_qb = 0, n_phit = 0, n_fin = 0, idle = 0, n_mph = 0, n_mty = 0, n_mid = 0;
    unsigned long long lanes_sh = 0, lanes_hit = 0, t_start = 0, n_start = 0, lanes_start = 0;
#endif
    const int tiles_x = (P.width + 7) / 8, tiles = launch_tiles(P);
    const int kstr = 1 << P.lk;
    // stream slots of this launch: q = 0 .. nq-1 starts at global sample s_begin + q
    const int nq = s_end - s_begin < kstr ? s_end - s_begin : kstr;
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    int band_k = 0;
    int ut = 0, uq = 0, bnext = 64;  // the wave's current unit (tile, stream slot) and its next pixel to hand out
    bool drained = false;            // every band's units handed out
    unsigned item = ITEM_NONE;       // the lane's pixel (ITEM_* above)
    bool next_sample = false;        // the lane's next sample starts at the top of the iteration
    Aov aov{acc, 0.0f, P.first, P.lk};
    Path st;
    st.pk = acc + acc_base_slots(F) * BLOCK;
    Trav T;
    T.sp = -1;
    T.nprim = 0;
    T.nxt = W_EMPTY;
    for (;;) {
        JT_STAMP(const unsigned long long ts0 = __builtin_amdgcn_s_memtime());
        // ---- hand out pixels to the lanes without one (wave-uniform control); a lane taking an
        // item starts from its stream's means so far (zero for the stream's first sample)
        bool start = next_sample;
        for (;;) {
            const unsigned long long needm = __builtin_amdgcn_ballot_w64(item == ITEM_NONE);
            if (!needm || drained) break;
            if (bnext >= 64) {  // the next unit of this XCD's band, or of the next band
                const int band = (int)((xcc + (unsigned)band_k) & (NBANDS - 1));
                // JT_BAND_STRIP > 1: bands of whole tile rows, each walked in strips of that many
                // rows, column by column, so the tiles in flight on an XCD form a compact block
                // (their rays share nodes and texels in L2).
                // A tile share (tile_stride D) whose D divides the tile columns is a grid of
                // tiles_x / D columns in launch-tile numbering and is walked the same way.
                constexpr int STRIP = JT_BAND_STRIP;
                const int gx = tiles_x % P.tile_stride == 0 ? tiles_x / P.tile_stride : 0;
                const bool strips = STRIP > 1 && gx > 0;
                const int tiles_y = (P.height + 7) / 8;
                const int bt0 = strips ? band * tiles_y / NBANDS * gx : band * tiles / NBANDS;
                const int bn = strips ? (band + 1) * tiles_y / NBANDS * gx - bt0 : (band + 1) * tiles / NBANDS - bt0;
                unsigned unit = 0;
                if (lane == 0) unit = atomicAdd(JT_A(work) + band * BAND_STRIDE, 1u);
                unit = __builtin_amdgcn_readfirstlane(unit);
                if (unit >= (unsigned)bn * (unsigned)nq) {
                    if (++band_k >= NBANDS) drained = true;
                    continue;
                }
                uq = (int)(unit % (unsigned)nq);  // tile-major (NBANDS above)
                const int tu = (int)(unit / (unsigned)nq);
                int tile = bt0 + tu;
                if (strips) {
                    const int rows = bn / gx, sidx = tu / (STRIP * gx);
                    const int v = tu - sidx * STRIP * gx, h = rows - sidx * STRIP < STRIP ? rows - sidx * STRIP : STRIP;
                    tile = bt0 + (sidx * STRIP + v % h) * gx + v / h;
                }
                ut = tile * P.tile_stride + P.tile_offset;
                // a tile jt_adapt froze takes no more samples: its stream means stay as they are
                // (ut is wave-uniform: a scalar load and a scalar branch per unit)
                if constexpr (ADAPT) {
                    if (JT_A(frozen)[ut]) {
                        bnext = 64;
                        continue;
                    }
                }
                bnext = 0;
            }
            const int nneed = lane_count(needm), take = nneed < 64 - bnext ? nneed : 64 - bnext;
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(needm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)needm, 0u));
            if (item == ITEM_NONE && rank < take) {
                const int l = bnext + rank;
                const int i = (ut % tiles_x) * 8 + (l & 7), j = (ut / tiles_x) * 8 + (l >> 3);
                // a pixel outside the image (edge tiles) is skipped: the lane takes another
                if (i < P.width && j < P.height) {
                    item = item_of<F>(ut, l, i, j);
                    start = true;
                    const int s = JT_SB + uq;
                    acc_i[11 * BLOCK] = s;
                    const int pixel = j * P.width + i;
                    float4 im = make_float4(0, 0, 0, 0), al = im, nr = im;
                    int h = 0;
                    if (s - P.first >= kstr) {  // the stream has earlier samples (an earlier launch)
                        if (P.lk == 0) {
                            im = JT_A(image)[pixel];
                            al = JT_A(albedo)[pixel];
                            nr = JT_A(normal)[pixel];
                            h = (int)JT_A(hits)[pixel];
                        } else {
                            const size_t o = (size_t)((s - P.first) & (kstr - 1)) * (size_t)JT_A(nslot) +
                                             (size_t)item_slot<F>(item, P);
                            im = JT_A(part_img)[o];
                            al = JT_A(part_alb)[o];
                            nr = JT_A(part_nrm)[o];
                            h = __float_as_int(al.w);
                        }
                    }
                    acc[0] = im.x;
                    acc[BLOCK] = im.y;
                    acc[2 * BLOCK] = im.z;
                    acc[3 * BLOCK] = im.w;
                    acc[4 * BLOCK] = al.x;
                    acc[5 * BLOCK] = al.y;
                    acc[6 * BLOCK] = al.z;
                    acc[7 * BLOCK] = nr.x;
                    acc[8 * BLOCK] = nr.y;
                    acc[9 * BLOCK] = nr.z;
                    acc_i[10 * BLOCK] = h;
                }
            }
            bnext += take;
        }
        // ---- every lane starting a sample (a new item, or the next sample of its stream): the
        // camera ray (trace_sample's prologue) and its query's first pops, where many lanes share them
        next_sample = false;
        if (start) {
            const int sample = acc_i[11 * BLOCK];
            const int tpixel = item_coords<F>() ? 0 : item_pixel(item, P, tiles_x);  // tile form
            if (!ft_none(F)) acc[12 * BLOCK] = stream_weight(P, sample);
            const DParams& P = karg_params<karg_params_on<SAMPLER, F>()>(P0);
            const int i = item_coords<F>() ? item_i(item) : tpixel % P.width;
            const int j = item_coords<F>() ? item_j(item) : tpixel / P.width;
            start_path<F, SB && JT_SINCOS_UNIT >= 2>(P, i, j, item_coords<F>() ? j * P.width + i : tpixel, sample, st);
            query_start<WIDE>(S, T, st.o, st.d, -1, stack, 0, PB);
            if (!WC) lds_count(1, true);
            if constexpr (item_first_pop<WIDE, F>()) {
#pragma unroll
                for (int k = 0; k < first_pops<F>(); k++)
                    if (wants_node<WIDE>(T)) node_step_any<WIDE, RING, OVF, COUNT, NCACHE, F>(S, T, stack, oslot, cnt);
            }
        }
        if (WC) w_rays += lane_count(__builtin_amdgcn_ballot_w64(start));
#if JT_STAMPS
        const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
        t_start += ts1 - ts0;
        n_start++;
        lanes_start += lane_count(__builtin_amdgcn_ballot_w64(start));
#endif
        if (__builtin_amdgcn_ballot_w64(item != ITEM_NONE) == 0) break;  // drained, and every lane is done
        // ---- traversal phase: step every lane with a query in flight until enough lanes wait.
        // Each iteration runs ONE step kind — primitive tests or stack pops — picked by a biased
        // lane vote (a wave-uniform branch), so the SIMD executes one code path per iteration; a
        // lane's own sequence of steps is unchanged, it only waits while the other kind runs.
        // Light-hit steps (path sampler, matte scenes whose light chains cannot run inline): a
        // lane whose sample_lights_pdf query has finished does not wait for the shading phase.
        constexpr bool LSTEP = light_steps(SAMPLER, F);
        for (;;) {
            const bool wantp = T.nprim > 0;
            const bool wantn = wants_node<WIDE>(T);
            const bool waiting = query_done<WIDE>(T);
            const int np = lane_count(__builtin_amdgcn_ballot_w64(wantp));
            const int nn = lane_count(__builtin_amdgcn_ballot_w64(wantn));
            int nw = lane_count(__builtin_amdgcn_ballot_w64(waiting));
            const int nb = np + nn;
            if (LSTEP && !S.light_inline) {
                const bool wantl = waiting && st.phase == PH_LIGHT;
                const int nl = lane_count(__builtin_amdgcn_ballot_w64(wantl));
                if (nl > 0 && (nl >= P.light_lanes || nb == 0)) {
                    bool c_lq = false, c_ray = false;
                    if (wantl && rerun_tie<WIDE>(S, T, st.o, st.d, S.lights[st.li].instance, stack, PB)) {
                        // an exact-t tie: the query runs again in the reference's order
                    } else if (wantl) {
                        if (light_hit<F>(S, P, st, query_hit(T))) {
                            st.phase = PH_FINISH;
                        } else if (st.phase == PH_LIGHT) {
                            if (WC) c_lq = true;
                            else lds_count(2, true);
                            query_start<WIDE>(S, T, st.o, st.d, S.lights[st.li].instance, stack, 0, PB);
                        } else {
                            if (WC) c_ray = true;
                            else lds_count(1, true);
                            query_start<WIDE>(S, T, st.o, st.d, -1, stack, 0, PB);
                        }
                    }
                    if (WC) {
                        w_lq += lane_count(__builtin_amdgcn_ballot_w64(c_lq));
                        w_rays += lane_count(__builtin_amdgcn_ballot_w64(c_ray));
                    }
                    continue;
                }
                nw -= nl;
            }
            if (nb == 0 || nw >= (nb + nw < P.wait_lanes ? nb + nw : P.wait_lanes)) break;
#if JT_STAMPS
            n_trav++;
            idle += 64 - lane_count(__builtin_amdgcn_ballot_w64(item != ITEM_NONE));
            if (np * JT_VOTE_P >= nn * JT_VOTE_N) { steps_p++; lanes_p += np; } else { steps_n++; lanes_n += nn; }
#endif
            if (JT_RAY_FROM_PATH && !(F & FT_XFORM)) {
                // without instance transforms a query's ray is its path's (st.o, st.d), unchanged
                // while the query runs: re-reading it here keeps one copy, not two, live across
                // the loop (register renaming only, no instructions)
                T.lo = st.o;
                T.ld = st.d;
            }
            if (np * JT_VOTE_P >= nn * JT_VOTE_N) {
                if (T.nprim > 0) prim_step<COUNT, F>(S, T, cnt);
            } else {
                // JT_NODE_REPEAT pops per node iteration: a lane whose next step is again a
                // stack pop takes it at once (the same steps in the same per-lane order, less
                // per-iteration vote and loop overhead)
                constexpr int NREP = ft_none(F) ? JT_NODE_REPEAT_NONE : JT_NODE_REPEAT;
#pragma unroll
                for (int k = 0; k < NREP; k++)
                    if (wants_node<WIDE>(T)) node_step_any<WIDE, RING, OVF, COUNT, NCACHE, F>(S, T, stack, oslot, cnt);
            }
        }
#if JT_STAMPS
        const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
        t_trav += ts2 - ts1;
        n_shade++;
        lanes_sh += lane_count(__builtin_amdgcn_ballot_w64(query_done<WIDE>(T)));
        {
            int mid = -1, mt = -1;
            if (query_done<WIDE>(T) && st.phase == PH_SCENE && T.h_inst >= 0) {
                mid = S.inst_shade[T.h_inst].material;
                mt = (F & FT_MAT) ? S.materials[mid].type : (int)M_MATTE;
            }
            if (__builtin_amdgcn_ballot_w64(mt >= 0)) {
                n_mph++;
                lanes_hit += lane_count(__builtin_amdgcn_ballot_w64(mt >= 0));
                for (int ty = 0; ty <= (int)M_GLTFPBR; ty++) n_mty += __builtin_amdgcn_ballot_w64(mt == ty) ? 1u : 0u;
                bool counted = mt < 0;
                for (;;) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(!counted);
                    if (!m) break;
                    const int v = __shfl(mid, __ffsll((long long)m) - 1);
                    counted = counted || mid == v;
                    n_mid++;
                }
            }
        }
        unsigned long long ts3 = ts2, ts4 = ts2;
#endif
        // ---- shading phase: every waiting lane consumes its hit and issues its next query; a
        // near-first query that saw an exact-t tie first runs again in the reference's order
        constexpr bool LINL = (F & (FT_LINL | FT_NOIL)) != 0;
        {
            const bool tie = query_done<WIDE>(T) && (T.nh & (TIE_SEEN | REF_RERUN)) == TIE_SEEN &&
                             !(LSTEP && st.phase == PH_FINISH);
            if (S.order_flip && __builtin_amdgcn_ballot_w64(tie))
                if (tie) rerun_tie<WIDE>(S, T, st.o, st.d, SAMPLER == 1 && !LINL && st.phase == PH_LIGHT ? S.lights[st.li].instance : -1, stack, PB);
        }
        bool c_path = false, c_lq = false, c_ray = false;
        unsigned n_inl = 0;
        if (query_done<WIDE>(T)) {
            const DParams& P = karg_params<karg_params_on<SAMPLER, F>()>(P0);
            const DScene SL = shade_scene_lds<NCACHE, RING, OVF, F>(S0);
            const DScene& S = NCACHE ? shade_scene<karg_scene<NCACHE, F>()>(S0) : SL;
            bool alive = true;
            // no light query ever leaves the shading phase (FT_LINL), or none exists (FT_NOIL)
            const bool light = SAMPLER == 1 && !LINL && st.phase == PH_LIGHT;
            bool done;
            if (LSTEP && st.phase == PH_FINISH) done = true;
            else if (light) done = light_hit<F>(S, P, st, query_hit(T));
            else if (SAMPLER == 2) done = naive_hit<F, SB>(S, P, st, query_hit(T), aov, cnt.shades);
            else done = path_hit<F, SB>(S, P, st, query_hit(T), aov, cnt.shades);
            bool chained = false;  // the lane ran its bounce's light chains here (query_restart below)
            if (SAMPLER == 1 && !done && st.phase == PH_LIGHT && chains_inline(F, S)) {
                unsigned nlq = 0;
                chained = true;
                done = light_chain<WIDE, RING, OVF, COUNT, NCACHE, F>(S, P, st, T, stack, oslot, cnt, [&] {
                    if (WC) nlq++;
                    else lds_count(2, true);
                });
                if (WC) n_inl += nlq;
            }
#if JT_STAMPS
            ts3 = __builtin_amdgcn_s_memtime();
            n_phit++;
#endif
            if (done) {
                // trace_sample epilogue (src/trace.jl:625-648), into the item's stream mean
                if (WC) c_path = true;
                else lds_count(0, true);
                v3 radiance = st.radiance<F>();
                if (!all_finite(radiance)) radiance = V3(0, 0, 0);
                const float mr = max3(radiance);
                if (mr > P.clamp) radiance = radiance * (P.clamp / mr);
                const float w = aov.w<F>();
                const float omw = 1 - w;
                const bool hit = st.flag(F_HIT);
                const bool env = !hit && !P.envhidden && S.nenvs != 0;
                const v4 target = (hit || env) ? V4(radiance.x, radiance.y, radiance.z, 1) : V4(0, 0, 0, 0);
                // no bounce-0 surface was accepted: st.d is still the camera ray direction
                if (!hit) aov_update<F>(aov, env ? V3(1, 1, 1) : V3(0, 0, 0), -st.d);
                acc[0] = acc[0] * omw + target.x * w;
                acc[BLOCK] = acc[BLOCK] * omw + target.y * w;
                acc[2 * BLOCK] = acc[2 * BLOCK] * omw + target.z * w;
                acc[3 * BLOCK] = acc[3 * BLOCK] * omw + target.w * w;
                if (hit || env) acc_i[10 * BLOCK] += 1;
                alive = false;
                T.sp = -1;
                const int sample = acc_i[11 * BLOCK];
                if (sample + kstr >= JT_SE) {
                    // the item is complete: store its stream's means (plain stores: no other item
                    // of this launch reads them; the combine kernel runs after the launch)
                    const int pixel = item_pixel_index<F>(item, P, tiles_x);
                    const float4 im = make_float4(acc[0], acc[BLOCK], acc[2 * BLOCK], acc[3 * BLOCK]);
                    if (P.lk == 0) {
                        JT_A(image)[pixel] = im;
                        JT_A(albedo)[pixel] = make_float4(acc[4 * BLOCK], acc[5 * BLOCK], acc[6 * BLOCK], 0.0f);
                        JT_A(normal)[pixel] = make_float4(acc[7 * BLOCK], acc[8 * BLOCK], acc[9 * BLOCK], 0.0f);
                        JT_A(hits)[pixel] = (long long)acc_i[10 * BLOCK];
                    } else {
                        const size_t o = (size_t)((sample - P.first) & (kstr - 1)) * (size_t)JT_A(nslot) +
                                         (size_t)item_slot<F>(item, P);
                        JT_A(part_img)[o] = im;
                        JT_A(part_alb)[o] = make_float4(acc[4 * BLOCK], acc[5 * BLOCK], acc[6 * BLOCK], __int_as_float(acc_i[10 * BLOCK]));
                        JT_A(part_nrm)[o] = make_float4(acc[7 * BLOCK], acc[8 * BLOCK], acc[9 * BLOCK], 0.0f);
                    }
                    item = ITEM_NONE;
                } else {
                    acc_i[11 * BLOCK] = sample + kstr;  // started at the top of the next iteration
                    next_sample = true;
                }
            }
#if JT_STAMPS
            ts4 = __builtin_amdgcn_s_memtime();
            if (__builtin_amdgcn_ballot_w64(done)) n_fin++;
#endif
            if (alive) {
                if (SAMPLER == 1 && !LINL && st.phase == PH_LIGHT) {
                    if (WC) c_lq = true;
                    else lds_count(2, true);
                    query_start<WIDE>(S, T, st.o, st.d, S.lights[st.li].instance, stack, 0, PB);
                } else {
                    if (WC) c_ray = true;
                    else lds_count(1, true);
                    // when every lane of the wave that goes on comes from a chain (none from a delta
                    // material, none in a scene without instance lights), the wave's scene queries
                    // keep the chain's 1/d: st.d has not changed since. A wave-uniform choice, so
                    // only one of the two forms executes.
                    if (SAMPLER == 1 && chain_dinv_once<WIDE, OVF, NCACHE, F>() && __builtin_amdgcn_ballot_w64(!chained) == 0)
                        query_restart<F>(S, T, st.o, st.d, stack, PB);
                    else query_start<WIDE>(S, T, st.o, st.d, -1, stack, 0, PB);
                }
                // the query's first pop (TLAS root, or the light instance and its BLAS root) here,
                // where most of the wave's lanes take part, rather than in a sparser traversal step
#pragma unroll
                for (int k = 0; k < first_pops<F>(); k++)
                    if (wants_node<WIDE>(T)) node_step_any<WIDE, RING, OVF, COUNT, NCACHE, F>(S, T, stack, oslot, cnt);
            }
        }
#if JT_STAMPS
        const unsigned long long ts5 = __builtin_amdgcn_s_memtime();
        t_shade += ts5 - ts2;
        t_hit += ts3 - ts2;
        t_fin += ts4 - ts3;
        t_qb += ts5 - ts4;
#endif
        if (WC) {
            w_paths += lane_count(__builtin_amdgcn_ballot_w64(c_path));
            w_lq += lane_count(__builtin_amdgcn_ballot_w64(c_lq));
            w_rays += lane_count(__builtin_amdgcn_ballot_w64(c_ray));
            if (SAMPLER == 1 && chains_inline(F, S)) w_lq += __builtin_amdgcn_readfirstlane(wave_sum(n_inl));
        }
    }
#if JT_STAMPS
    if (lane == 0) {
        unsigned long long* dbg = A.counters + 8;
        const unsigned long long v[24] = {t_trav, t_shade, n_trav,  n_shade, lanes_p, lanes_n,  steps_p, steps_n,
                                          0,      t_hit,   t_fin,   t_qb,    0,       n_phit,   n_fin,   idle,
                                          n_mph,  n_mty,   n_mid,   lanes_sh, lanes_hit, t_start, n_start, lanes_start};
        for (int k = 0; k < 24; k++) atomicAdd(dbg + k, v[k]);
    }
#endif
    // one atomic per counter per wave (the wave's own LDS adds precede this read in program order)
    const unsigned wv[3] = {w_paths, w_rays, w_lq};
    unsigned v[7] = {0u, 0u, 0u, cnt.nodes, cnt.instances, cnt.prims, COUNT ? cnt.shades : 0u};
#pragma unroll
    for (int k = 0; k < 7; k++) {
        unsigned sum = k < 3 ? (WC ? wv[k] : wcnt[k]) : wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(&A.counters[k], (unsigned long long)sum);
    }
}

// Occupancy request (waves per SIMD); JT_WAVES=0 leaves it to the compiler. The LDS-mode
// FT_NONE kernel (cornellbox: 96 VGPRs, LDS for 5 workgroups per CU with the stack sized to the
// scene) asks for JT_WAVES_NONE: measured +4 % over 4 waves with its wait_lanes of 56.
#ifndef JT_WAVES
#define JT_WAVES 0
#endif
#ifndef JT_WAVES_NONE
#define JT_WAVES_NONE 5
#endif
#if JT_WAVES > 0
#define JT_WAVES_PER_EU __attribute__((amdgpu_waves_per_eu(JT_WAVES, JT_WAVES)))
#define JT_WAVES_PER_EU_F(F) \
    __attribute__((amdgpu_waves_per_eu(ft_none(F) ? JT_WAVES_NONE : JT_WAVES, ft_none(F) ? JT_WAVES_NONE : JT_WAVES)))
#else
#define JT_WAVES_PER_EU
#define JT_WAVES_PER_EU_F(F)
#endif

// the scene arrays of the LDS blob (small-scene mode; offsets from jt_create)
__device__ __forceinline__ DScene blob_scene(const DScene& S, const uint4* blob) {
    DScene L = S;
    L.nodes = reinterpret_cast<const DNode*>(blob + S.o_nodes);
    L.wnodes = reinterpret_cast<const DWide*>(blob + S.o_wnodes);
    L.prims = reinterpret_cast<const float4*>(blob + S.o_prims);
    L.inst_trav = reinterpret_cast<const DInstTrav*>(blob + S.o_inst_trav);
    L.inst_blas = reinterpret_cast<const int4*>(blob + S.o_inst_blas);
    L.inst_shade = reinterpret_cast<const DInstShade*>(blob + S.o_inst_shade);
    L.shapes = reinterpret_cast<const DShape*>(blob + S.o_shapes);
    L.pos = reinterpret_cast<const float4*>(blob + S.o_pos);
    L.nrm = reinterpret_cast<const float4*>(blob + S.o_nrm);
    L.tc = reinterpret_cast<const float2*>(blob + S.o_tc);
    L.col = reinterpret_cast<const float4*>(blob + S.o_col);
    L.elems = reinterpret_cast<const int4*>(blob + S.o_elems);
    L.enrm = reinterpret_cast<const float4*>(blob + S.o_enrm);
    L.enrm_id = reinterpret_cast<const float4*>(blob + S.o_enrm_id);
    L.materials = reinterpret_cast<const DMaterial*>(blob + S.o_materials);
    L.lights = reinterpret_cast<const DLight*>(blob + S.o_lights);
    L.light_hit = reinterpret_cast<const int4*>(blob + S.o_light_hit);
    L.light_elems = reinterpret_cast<const float4*>(blob + S.o_light_elems);
    L.cdf = reinterpret_cast<const float*>(blob + S.o_cdf);
    return L;
}

// The bake pass of the LDS-mode kernels whose node step runs on the baked form (node_baked,
// jt_traverse.h; jt_push.h): every node of the workgroup's LDS copy gets its two words rewritten,
// once per launch, between two barriers. The host's bytes (hs.nodes, the blob in HBM) are not
// touched. The nodes are the blob's first array, the wide records follow (JT_SCENE_ARRAYS): their
// count is the gap, two 16-B units per node (an empty array keeps one unit: no node). The TLAS
// nodes come first (layout_scene), so the index gives the level.
// Instance roots (JT_INST_ROOTS, jt_push.h): a TLAS leaf's baked entries name root rows, and the same
// pass writes the rows: row i, node iroot0 + i of the LDS node array, is the baked BLAS root of
// instance i, over the LDS copy of inst_trav (4 units per instance up to inst_blas; an empty array
// keeps one unit: no row). A row's sources are the blob in HBM, which nobody writes, so a row never
// sees another thread's half-baked node; its destination is read by nothing before the barrier.
// (That is one instance record and one root node re-read from HBM per instance, per workgroup and
// launch: a few loads from L2 against a persistent launch of tens of milliseconds.)
__device__ __forceinline__ void bake_nodes(const DScene& S, uint4* blob) {
    uint4* const nodes = blob + S.o_nodes;
    const int nnodes = (S.o_wnodes - S.o_nodes) >> 1;
    const int iroot0 = JT_INST_ROOTS ? instance_root_base(S.o_nodes, S.o_inst_trav) : 0;
    for (int k = threadIdx.x; k < nnodes; k += BLOCK) {
        uint4& b = nodes[2 * k + 1];  // DNode::b: z the start word, w the meta word
        const BakedNode bn = bake_node(b.w, (int)b.z, k < S.tlas_nnodes ? T_TLAS : T_BLAS, iroot0);
        b.z = bn.e0;
        b.w = bn.meta;
    }
    if (JT_INST_ROOTS) {
        const int ninst = (S.o_inst_blas - S.o_inst_trav) >> 2;
        for (int i = threadIdx.x; i < ninst; i += BLOCK) {
            const uint4* const root = S.blob + S.o_nodes + 2 * (int)S.blob[S.o_inst_blas + i].x;
            uint4 b = root[1];
            const BakedNode bn = bake_node(b.w, (int)b.z, T_BLAS);
            b.z = bn.e0;
            b.w = bn.meta;
            nodes[2 * (iroot0 + i)] = root[0];
            nodes[2 * (iroot0 + i) + 1] = b;
        }
    }
}

// Baked shading (shade_baked, jt_traverse.h; BakedBasis, jt_bsdf.h), in the same pass: per element g
// of the LDS copy basis_fromz of its normal enrm_id[g], per material color / pif, written with the
// device functions the matte bounce would call, into bytes of the copy that a kernel without scene
// features never reads:
//   enrm[g] (Z, X.x)       element_normal reads enrm only for an instance that is not rot_identity;
//                          without FT_XFORM a scene has none (layout_scene), and eval_shading<F, true>
//                          reads enrm_id without looking
//   enrm_id[g].w (Y.x)     xyz() of the row is the normal; nothing reads w
//   elems[g].w (Y.y)       the fourth vertex of a quad: read under FT_QUAD only
//   DMaterial::scattering  MatPoint::scattering feeds the volume stack: FT_VOL only
// The arrays lie in JT_SCENE_ARRAYS' order, one 16-B unit per element in elems, enrm and enrm_id
// alike (an empty array keeps one unit in each: a harmless write), six units per material up to the
// lights. A thread reads and writes rows of its own element or material only, and nothing reads
// them before the barrier. The host's bytes (hs.*, the blob in HBM) are not touched.
__device__ __forceinline__ void bake_shading(const DScene& S, uint4* blob) {
    static_assert(sizeof(DMaterial) == 6 * 16, "six 16-B units per material");
    const int nelem = S.o_enrm_id - S.o_enrm;
    for (int g = threadIdx.x; g < nelem; g += BLOCK) {
        float4& ni = reinterpret_cast<float4*>(blob + S.o_enrm_id)[g];
        const m3 b = basis_fromz(xyz(ni));
        reinterpret_cast<float4*>(blob + S.o_enrm)[g] = make_float4(b.c3.x, b.c3.y, b.c3.z, b.c1.x);
        ni.w = b.c2.x;
        blob[S.o_elems + g].w = __float_as_uint(b.c2.y);
    }
    const int nmat = (S.o_lights - S.o_materials) / 6;
    for (int k = threadIdx.x; k < nmat; k += BLOCK) {
        DMaterial& m = reinterpret_cast<DMaterial*>(blob + S.o_materials)[k];
        const v3 c = V3(m.color[0], m.color[1], m.color[2]) / pif;
        m.scattering[0] = c.x;
        m.scattering[1] = c.y;
        m.scattering[2] = c.z;
    }
}

// HBM mode: the scene is read from global memory (L2/MALL-resident); stack in static LDS.
// ADAPT (both kernels): the instance an adapted context launches (A.frozen is set), passed on to
// trace_body_items. A template parameter here leaves every instance's ISA as it is; moving a
// kernel's text into a shared device function does not.
template <int SAMPLER, int RING, bool OVF, int COUNT, int F, bool WIDE, bool ADAPT>
__global__ __launch_bounds__(BLOCK) JT_WAVES_PER_EU void trace_kernel(DScene S, DParams P, int s_begin, int s_end, DAccum A) {
    __shared__ int lds_stack[RING * BLOCK];
    trace_body_items<SAMPLER, RING, OVF, COUNT, F, true, WIDE, ADAPT>(S, P, s_begin, s_end, A, lds_stack + threadIdx.x);
}

// LDS mode (small scenes): the workgroup stages the scene blob into LDS once; every node,
// instance, primitive and shading record is then a ds_read instead of a vector-memory load
// through the TA/TD path (the measured limiter of the HBM-mode kernel).
template <int SAMPLER, int RING, bool OVF, int COUNT, int F, bool WIDE, bool ADAPT>
__global__ __launch_bounds__(BLOCK) JT_WAVES_PER_EU_F(F) void trace_kernel_lds(DScene S, DParams P, int s_begin, int s_end, DAccum A) {
    extern __shared__ uint4 dyn_lds[];
    // the stack takes the first bytes (lds_stack_bytes), the blob follows
    uint4* blob = dyn_lds + lds_stack_bytes(OVF, RING, S.stack_need) / 16;
    for (int k = threadIdx.x; k < S.blob_n16; k += BLOCK) blob[k] = S.blob[k];
    __syncthreads();
    if constexpr (node_baked<OVF, false, WIDE, F>()) {
        bake_nodes(S, blob);
        if constexpr (shade_baked<OVF, false, WIDE, F>()) bake_shading(S, blob);
        __syncthreads();
    }
    const DScene L = blob_scene(S, blob);
    trace_body_items<SAMPLER, RING, OVF, COUNT, F, false, WIDE, ADAPT>(L, P, s_begin, s_end, A, reinterpret_cast<int*>(dyn_lds) + threadIdx.x);
}

// Persistent launch: as many workgroups as the device holds at once (capped by the number of
// tiles), each wave then pulls work units until the launch's units are exhausted.
// LDSK: the specialisation also has an LDS-mode kernel (the large-scene masks run in HBM mode).
template <int SAMPLER, int RING, bool OVF, int COUNT, int F, bool LDSK, bool WIDE, bool ADAPT>
hipError_t launch_t(const DScene& S, const DParams& P, int s0, int s1, const DAccum& A, hipStream_t st, int cus) {
    // one wave per work unit (tile, stream slot) at most
    const long long units = (long long)launch_tiles(P) * std::min(s1 - s0, 1 << P.lk);
    const int want = (int)std::min<long long>((units + BLOCK / 64 - 1) / (BLOCK / 64), 1 << 30);
    if (want == 0) return hipSuccess;  // a multi-device share without tiles (tiny image)
    int per_cu = 0;
    hipError_t e;
    if constexpr (LDSK) {
        if (S.blob_n16 > 0) {
        const size_t lds = lds_stack_bytes(OVF, RING, S.stack_need) + (size_t)S.blob_n16 * 16;
        constexpr auto kl = &trace_kernel_lds<SAMPLER, RING, OVF, COUNT, F, WIDE, ADAPT>;
        const void* k = (const void*)kl;
        if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        const int nwg = std::min(want, std::min(per_cu, 8) * cus);  // <= 8 per CU: the overflow area's bound
        hipLaunchKernelGGL(kl, dim3(nwg), dim3(BLOCK), lds, st, S, P, s0, s1, A);
        return hipGetLastError();
        }
    }
    constexpr auto kh = &trace_kernel<SAMPLER, RING, OVF, COUNT, F, WIDE, ADAPT>;
    const void* k = (const void*)kh;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    const int nwg = std::min(want, std::min(per_cu, 8) * cus);
    hipLaunchKernelGGL(kh, dim3(nwg), dim3(BLOCK), 0, st, S, P, s0, s1, A);
    return hipGetLastError();
}

template <int ID, int SAMPLER, int COUNT, bool ADAPT>
hipError_t launch_cfg(const DScene& S, const DParams& P, int s0, int s1, const DAccum& A, hipStream_t st, int cus) {
    using C = LaunchConfig<ID>;
    return launch_t<SAMPLER, C::ring, C::ovf, COUNT, C::feat, C::lds, C::wide, ADAPT>(S, P, s0, s1, A, st, cus);
}

}  // namespace jtk
