// jt_plan.h — the launch plan of a context as integer functions: which 8x8 tiles a launch covers,
// which pixel a launch slot is, how many sample streams a context keeps, the stream weights of a
// combine, the chunk size and chunk schedule of a one-stream context and a device's share of a batch. Plain C++ (no
// HIP runtime), shared by the kernels, the device context and the host check (tests/plan_check.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JT_PLAN_HD __host__ __device__ inline
#else
#define JT_PLAN_HD inline
#endif

// automatic stream count (stream_log2): at least JT_STREAMS_MIN streams — JT_STREAMS_WIDE for a
// batch of at least two samples per such stream — and JT_STREAM_ITEMS (pixel, stream) items, at
// most JT_STREAM_ITEMS_MAX items
#define JT_STREAMS_MIN 16
#define JT_STREAMS_WIDE 32
#define JT_STREAM_ITEMS (1LL << 22)
#define JT_STREAM_ITEMS_MAX (1LL << 27)
#ifndef JT_MAX_STREAMS
#define JT_MAX_STREAMS 64  // sample streams per pixel (a power of two, jt_ctx::lk)
#endif

namespace jtk {

// number of 8x8 tiles a launch covers: tiles offset, offset + stride, ... of the image's
// (DParams tile_stride / tile_offset)
JT_PLAN_HD int plan_tiles(int width, int height, int stride, int offset) {
    const int all = ((width + 7) / 8) * ((height + 7) / 8);
    return all > offset ? (all - offset + stride - 1) / stride : 0;
}

// Launch slot g (< plan_tiles * 64) is lane g & 63 of launch tile g >> 6: pixel (i, j) of image
// tile t = (g >> 6) * tile_stride + tile_offset, row-major within the tile. inside: false for the pixels of
// an edge tile past the image's width or height.
struct SlotPixel {
    int i, j;
    bool inside;
};
JT_PLAN_HD SlotPixel slot_pixel(int g, int width, int height, int tile_stride, int tile_offset) {
    const int tiles_x = (width + 7) / 8;
    const int t = (g >> 6) * tile_stride + tile_offset, l = g & 63;
    const int i = (t % tiles_x) * 8 + (l & 7), j = (t / tiles_x) * 8 + (l >> 3);
    return SlotPixel{i, j, i < width && j < height};
}

// A lane's work item in the trace kernels: its pixel's image coordinates, (j << 16) | i, so a
// sample start and an item's store take i, j and the pixel index by shifts, masks and multiply-adds
// (no division by the runtime tile columns). Width and height stay at or below JT_ITEM_MAX_DIM
// (jt_create rejects more), so no item equals ITEM_NONE: no pixel.
#define JT_ITEM_MAX_DIM 32768
constexpr unsigned ITEM_NONE = 0xffffffffu;
JT_PLAN_HD unsigned item_encode(int i, int j) { return ((unsigned)j << 16) | (unsigned)i; }
JT_PLAN_HD int item_i(unsigned item) { return (int)(item & 0xffffu); }
JT_PLAN_HD int item_j(unsigned item) { return (int)(item >> 16); }
// 1 / tile_stride as the float the slot rule below multiplies by: computed once on the host
// (DParams::tile_stride_rcp), the IEEE quotient
JT_PLAN_HD float tile_stride_rcp(int tile_stride) { return 1.0f / (float)tile_stride; }
// The launch tile of image tile t of the share, (t - offset) / stride. The quotient is exact in
// integers; t < 2^20 (jt_create) keeps the float product within 2^-3 of it, so adding a half and
// truncating gives it. Against the integer division in the kernel: cornellbox +0.5 %, its 1/8 share
// +0.9 % (two runs each, profiles/r06_ab/slot_float_vs_div_r06d.txt; the division's code raised the
// kernels' spills from 1-2 to 4-6 VGPRs)
JT_PLAN_HD int launch_tile(int t, int tile_offset, float stride_rcp) {
    return (int)((float)(t - tile_offset) * stride_rcp + 0.5f);
}
// An item's launch slot, the inverse of slot_pixel: image tile (j >> 3) * tiles_x + (i >> 3), the
// pixel of the tile (j & 7) * 8 + (i & 7)
JT_PLAN_HD int item_slot(unsigned item, int tiles_x, int tile_offset, float stride_rcp) {
    const int i = item_i(item), j = item_j(item);
    return launch_tile((j >> 3) * tiles_x + (i >> 3), tile_offset, stride_rcp) * 64 + (j & 7) * 8 + (i & 7);
}

// the launch slots inside the image: every pixel the launch traces (edge tiles are clipped)
JT_PLAN_HD long long traced_pixels(int width, int height, int stride, int offset) {
    const int tiles = plan_tiles(width, height, stride, offset);
    long long n = 0;
    for (int u = 0; u < tiles; u++) {
        const SlotPixel p = slot_pixel(u * 64, width, height, stride, offset);  // the tile's first pixel
        const int w = width - p.i, h = height - p.j;
        n += (long long)(w < 8 ? w : 8) * (h < 8 ? h : 8);
    }
    return n;
}

// Sample streams per pixel (DESIGN.md §2 "Sample streams"), fixed at jt_create from the pixels
// the context traces and the batch only (never from the scene's memory mode, so every option
// that picks LDS or HBM mode keeps the image bits): 1 for the reference's default one-sample
// batches (its single running mean); otherwise at least 16 — 32 from a batch of 64 (two samples
// per stream) — and enough for 2^22 (pixel, stream) items (a context tracing few pixels — a tile
// share, a small image — still fills the GPU), at most 64, the batch, and 2^27 items of stream
// means (6.4 GB).
// Measured (gpurun_out/r05i, r05j): bathroom1 1024 spp 8 -> 16 streams +0.8 %, features2 512 spp
// +2 %, ecosys 64 spp 2 -> 16 +2.6 %, its 1/8 share (512 spp) +3.7 %; a 1/8 tile share of the
// headline 32 streams 9265, 64 streams 9794 Mrays/s. A context whose scene runs from HBM starts
// from 32 streams when the batch gives each at least two samples (gpurun_out/r05sk, r05sk2:
// features2 +0.6 %, bathroom1 +0.5 %; cornellbox +1.0 %, round 5, when 32 streams were the
// HBM-mode rule only). The option "streams" overrides.
JT_PLAN_HD int stream_log2(long long pixels, int batch) {
    if (batch <= 1) return 0;
    long long want = batch >= 2 * JT_STREAMS_WIDE ? JT_STREAMS_WIDE : JT_STREAMS_MIN;
    while (pixels * want < JT_STREAM_ITEMS) want *= 2;
    int lk = 0;
    while (lk < 6 && (2LL << lk) <= want && (2 << lk) <= batch && (2 << lk) <= JT_MAX_STREAMS &&
           pixels * (2LL << lk) <= JT_STREAM_ITEMS_MAX)
        lk++;
    return lk;
}

// weights n_j / n of the k = 2^lk streams after n local samples: stream j holds those t < n with
// t mod k == j (include/jtrace.h jt_get_streams restates the rule), computed in double and rounded
// once. Fills w[0 .. ns) and returns ns = min(n, k), the streams that hold a sample.
JT_PLAN_HD int combine_weights(long long n, int lk, float* w) {
    const long long k = 1LL << lk;
    const int ns = (int)(n < k ? n : k);
    for (int j = 0; j < ns; j++) w[j] = (float)((double)((n - 1 - j) / k + 1) / (double)n);
    return ns;
}

// the chunk size of a one-stream context whose launches cover nslot slots: as many one-sample
// streams as two sets of stream-mean buffers hold, at most 64 (JT_MAX_STREAMS) and 2^27 (stream,
// slot) records in all (6.4 GB). 1: none possible.
JT_PLAN_HD int chunk_samples(long long nslot) {
    int m = JT_MAX_STREAMS;
    while (m > 1 && 2 * nslot * m > JT_STREAM_ITEMS_MAX) m >>= 1;
    return m;
}

// the option test_trace_chunk (tests only) as a cap on that chunk size: n itself when it is a power
// of two in [1, 64], 0 (jt_create rejects the option) otherwise. The cap only ever lowers the chunk.
JT_PLAN_HD int chunk_cap(long long n) { return n >= 1 && n <= JT_MAX_STREAMS && (n & (n - 1)) == 0 ? (int)n : 0; }

// The chunk schedule of a one-stream range [s0, s1) at chunk size `chunk` > 1 (trace_launch,
// jt_trace.hip): chunk i of chunk_count traces samples [x, y) as one-sample streams of a launch with
// DParams::first = x and DParams::lk = lk into buffer set `set`, and chain_kernel folds its y - x
// records into the running mean.
// Every chunk goes through the chunk buffers, a one-sample tail included: lk >= 1 always, since a
// launch with lk == 0 stores into the running mean itself, which the previous chunk's chain is
// still writing on the second stream, and leaves the chunk's buffer set unwritten for its own chain.
// So lk is the smallest value >= 1 with 2^lk >= y - x; a tail of one sample is stream 0 of a
// two-stream launch (the launch's stream slots are min(y - x, 2^lk) = 1), folded with m = 1 like any
// other chunk: one code path and one launch shape, where a plain lk == 0 launch of the tail would
// need a wait of its own on the last chain and no chain launch.
struct ChunkPlan {
    int x, y;  // the chunk's global samples [x, y)
    int lk;    // log2 of its launch's streams
    int set;   // its buffer set, i & 1
};
JT_PLAN_HD int chunk_lk(int len) {
    int lk = 1;
    while ((1 << lk) < len) lk++;
    return lk;
}
JT_PLAN_HD int chunk_count(int s0, int s1, int chunk) { return (int)(((long long)s1 - s0 + chunk - 1) / chunk); }
JT_PLAN_HD ChunkPlan chunk_plan(int s0, int s1, int chunk, int i) {
    const long long x = (long long)s0 + (long long)i * chunk;
    const long long y = x + chunk < s1 ? x + chunk : s1;
    return ChunkPlan{(int)x, (int)y, chunk_lk((int)(y - x)), i & 1};
}

// the contiguous share [*a, *b) of device d of D of the batch [s0, s1) under the sample split
JT_PLAN_HD void sample_share(int s0, int s1, int d, int D, int* a, int* b) {
    const long long L = s1 - s0;
    *a = s0 + (int)(L * d / D);
    *b = s0 + (int)(L * (d + 1) / D);
}

}  // namespace jtk
