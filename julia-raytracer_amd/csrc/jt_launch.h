// jt_launch.h — what the host needs to launch the megakernel, and nothing of its device code: the
// kernels' argument records (DAccum, KArgs, DCombine), launch_tiles, the band constants of the
// work-unit counters and the declaration of the configurations' launch function. The integer
// rules that pick a configuration, with the launch geometry and LDS sizing constants, are in
// jt_select.h (through jt_records.h). The device context (jt_context.h) and the accumulation
// kernels (jt_accum.h) include this; the per-lane device functions are in jt_scene_eval.h,
// jt_traverse.h and jt_integrator.h, the kernel body and launch_cfg's definition in jt_kernels.h,
// which only jt_kv.hip includes.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_records.h"

namespace jtk {
using namespace jtd;

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
    // adaptive sampling (jt_adapt, jt_adapt.hip): per image tile the local sample count at which
    // it froze, 0: active. nullptr until the context's first jt_adapt, and always in multi-device
    // sub-contexts and one-stream chunks; once set, the context launches the configuration's
    // ADAPT instances (launch_cfg<..., true>), whose hand-out skips the units of a frozen tile.
    // The production instances never read it
    const unsigned* frozen;
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

// One configuration (LaunchConfig<ID>, jt_select.h): defined in jt_kernels.h, instantiated by
// jt_kv.hip. Every other unit sees this declaration only, so naming a specialisation there (the
// launch table of jt_trace.hip) refers to jt_kv's symbol and instantiates nothing.
// ADAPT: the configuration's kernels with the frozen-tile skip in the hand-out, for an adapted
// context (DAccum::frozen); jt_kv.hip instantiates them in translation units of their own.
template <int ID, int SAMPLER, int COUNT, bool ADAPT>
hipError_t launch_cfg(const DScene& S, const DParams& P, int s0, int s1, const DAccum& A, hipStream_t st, int cus);
// explicit instantiation (in jt_kv.hip) of one configuration for both samplers and both counter levels
#define JT_KV_INSTANCE(ID, SAMPLER, COUNT, ADAPT) \
    template hipError_t launch_cfg<ID, SAMPLER, COUNT, ADAPT>(const DScene&, const DParams&, int, int, const DAccum&, hipStream_t, int);
#define JT_KV_INSTANTIATE(ID, ADAPT) \
    JT_KV_INSTANCE(ID, 1, 0, ADAPT) JT_KV_INSTANCE(ID, 1, 1, ADAPT) JT_KV_INSTANCE(ID, 2, 0, ADAPT) JT_KV_INSTANCE(ID, 2, 1, ADAPT)

}  // namespace jtk
