// jt_adapt.h — adaptive sampling's freeze rule: its launch and threshold; the kernel and the
// context's half (jt_adapt, jt_get_sample_counts) are in jt_adapt.hip. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_records.h"

namespace jt {

constexpr int ADAPT_BLOCK = 256;  // threads per workgroup: four 8x8 tiles, one per wave, as error_kernel's

// One launch over the slots of a context's tiles: thread g is launch slot g (slot_pixel,
// jt_plan.h), wave g >> 6 is launch tile g >> 6. The launch's share of the tiles is carried here,
// as in DError.
struct DAdapt {
    const float4* var;    // float4[width * height]: the error estimate's variance (jt_ctx::err_var)
    unsigned* frozen_at;  // per image tile: the local sample count at which it froze, 0: active
    unsigned* active;     // one word per workgroup: its tiles still active after the launch
    float vmax;           // adapt_vmax: the tile freezes iff V_t <= (float)N_t * vmax
    unsigned n;           // the context's local samples, written for a tile that newly freezes
    int width, height;
    int tiles;            // launch tiles (launch_tiles)
    int tile_stride, tile_offset;
};

// workgroups of the launch: every slot of the launch's tiles
inline int adapt_blocks(int tiles) { return (int)(((long long)tiles * 64 + ADAPT_BLOCK - 1) / ADAPT_BLOCK); }

// The per-pixel channel-variance sum a tile may hold per pixel: the image-level target T handed
// down to tiles. With M the sum of (mu.x + mu.y) + mu.z and N the traced pixels, V_t <= N_t * vmax
// for every tile sums to 3 N V <= (T M)^2, which is jt_get_noise <= T. In double, rounded once.
inline float adapt_vmax(double noise_target, double M, long long N) {
    return (float)((noise_target * M) * (noise_target * M) / (3.0 * (double)N * (double)N));
}

// Enqueues the kernel on `stream`; nothing waits, the caller synchronises.
hipError_t adapt_launch(hipStream_t stream, const DAdapt& D);

}  // namespace jt
