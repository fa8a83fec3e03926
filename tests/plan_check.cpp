// plan_check.cpp — the launch plan's integer rules (csrc/jt_plan.h) enumerated on the host.
// tests/test_plan.py builds it with the host compiler under -fsanitize=address,undefined and runs
// it. No Python, no HIP runtime, no GPU.
//
//   - slot_pixel is a bijection between the launch slots inside the image and the pixels of the
//     launch's tiles (t = offset mod stride), over odd sizes and tile shares down to one tile and
//     none; plan_tiles counts those tiles and traced_pixels those pixels;
//   - stream_log2 against the pinned rows of tests/test_gpu_parity.py's stream-count table;
//   - combine_weights: ns = min(n, k), the streams' counts sum to n, every weight is
//     (float)((double)n_j / n), and two rows pinned from tests/error_ref.py stream_weights;
//   - sample_share: contiguous, disjoint shares that cover the batch;
//   - chunk_samples: a power of two in [1, 64], the largest whose two buffer sets stay within
//     2^27 records; chunk_cap (option test_trace_chunk): a power of two in [1, 64] or rejected;
//   - the chunk schedule of a one-stream range (chunk_count, chunk_plan, chunk_lk), for every chunk
//     size 2 .. 64 and every range of 2 .. 200 samples from the starts 0, 1 and 7:
//       (a) the chunks tile [s0, s1) once and in order, ceil(n / chunk) of them, none empty and
//           only the last shorter than the chunk size;
//       (b) every chunk has lk >= 1 and 2^lk >= y - x;
//       (c) lk is the smallest such value >= 1 (a tail of one sample has lk = 1, not the 0 that
//           2^lk >= 1 alone would give);
//       (d) set == i & 1.
//     trace_launch (csrc/jt_trace.hip) relies on (a) for which samples are traced, and on (b) for
//     the fix of the one-sample tail: a launch with lk == 0 stores into the running mean, not into
//     its buffer set, while the previous chunk's chain_kernel writes that mean on the second
//     stream, and the chunk's own chain then folds a set this launch never wrote. With lk >= 1
//     every chunk's records land in its set (2^lk >= y - x: no two samples share a stream, so each
//     record is one sample's value) and chain_kernel folds y - x of them. (d) is what the
//     chain_done wait of chunk i >= 2 assumes: the set was last read by chain i - 2.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_plan.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "plan_check: %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

void check_slots(int w, int h, int stride, int offset) {
    const int tiles_x = (w + 7) / 8, all = tiles_x * ((h + 7) / 8);
    int mine = 0;  // image tiles of the share
    for (int t = 0; t < all; t++) mine += t % stride == offset;
    const int tiles = jtk::plan_tiles(w, h, stride, offset);
    check(tiles == mine, "plan_tiles", w, h, stride, offset);
    std::vector<int> hit((size_t)w * h, 0);
    long long inside = 0;
    for (int g = 0; g < tiles * 64; g++) {
        const jtk::SlotPixel p = jtk::slot_pixel(g, w, h, stride, offset);
        const bool in_image = p.i >= 0 && p.i < w && p.j >= 0 && p.j < h;
        if (p.inside != in_image) check(false, "inside flag", w, h, stride, g);
        if (!in_image) continue;
        const int t = (p.j / 8) * tiles_x + p.i / 8;
        if (t % stride != offset) check(false, "a slot outside the share's tiles", w, h, stride, g);
        hit[(size_t)p.j * w + p.i]++;
        inside++;
    }
    long wrong = 0;  // every pixel of the share's tiles exactly once, no other pixel
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) wrong += hit[(size_t)j * w + i] != (((j / 8) * tiles_x + i / 8) % stride == offset ? 1 : 0);
    check(wrong == 0, "pixels not hit exactly once", w, h, stride, offset);
    check(jtk::traced_pixels(w, h, stride, offset) == inside, "traced_pixels", w, h, stride, offset);
}

// (width, height, batch, tile share, HBM mode) -> streams: the `expect` rows of
// tests/test_gpu_parity.py test_stream_count_rule (the memory mode never enters the rule)
const int STREAM_ROWS[][6] = {
    {1280, 720, 256, 1, 0, 32},   {1280, 720, 256, 1, 1, 32}, {1280, 720, 32, 1, 1, 16},    {1280, 720, 1, 1, 0, 1},
    {256, 256, 16, 1, 0, 16},     {1920, 1080, 1024, 1, 1, 32}, {1920, 1080, 1024, 1, 0, 32}, {3840, 2160, 4096, 1, 1, 16},
    {1280, 720, 256, 8, 0, 64},   {1280, 720, 256, 8, 1, 64}, {64, 64, 5, 1, 0, 4},         {7680, 4320, 64, 1, 1, 4},
};

// tests/error_ref.py stream_weights(6, 4) and (32, 16)
const float W_6_4[4] = {0x1.555556p-2f, 0x1.555556p-2f, 0x1.555556p-3f, 0x1.555556p-3f};
const float W_32_16 = 0x1p-4f;  // all sixteen

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check_weights() {
    for (int lk : {1, 2, 4, 6}) {
        const long long k = 1LL << lk;
        for (long long n = 1; n <= 3 * k; n++) {
            float w[JT_MAX_STREAMS + 1];
            for (float& x : w) x = -1.0f;
            const int ns = jtk::combine_weights(n, lk, w);
            check(ns == (n < k ? n : k), "combine_weights ns", n, k, ns);
            long long sum = 0;
            bool exact = true;
            for (int j = 0; j < ns; j++) {
                const long long nj = (n - 1 - j) / k + 1;
                sum += nj;
                exact = exact && same_bits(w[j], (float)((double)nj / (double)n));
            }
            check(sum == n, "stream counts do not sum to n", n, k, sum);
            check(exact, "a weight is not (float)((double)n_j / n)", n, k);
            check(w[ns] == -1.0f, "combine_weights wrote past ns", n, k, ns);
        }
    }
    float w[JT_MAX_STREAMS];
    bool ok = jtk::combine_weights(6, 2, w) == 4;
    for (int j = 0; ok && j < 4; j++) ok = same_bits(w[j], W_6_4[j]);
    check(ok, "combine_weights(6, k = 4) against the pinned row");
    ok = jtk::combine_weights(32, 4, w) == 16;
    for (int j = 0; ok && j < 16; j++) ok = same_bits(w[j], W_32_16);
    check(ok, "combine_weights(32, k = 16) against the pinned row");
}

void check_chunks() {
    for (long long n = -2; n <= 130; n++) {
        const bool pow2 = n >= 1 && n <= 64 && (n & (n - 1)) == 0;
        check(jtk::chunk_cap(n) == (pow2 ? n : 0), "chunk_cap", n);
    }
    check(jtk::chunk_cap(1LL << 40) == 0 && jtk::chunk_cap(-64) == 0, "chunk_cap: far values");
    for (int chunk = 2; chunk <= 64; chunk *= 2)
        for (int s0 : {0, 1, 7})
            for (int n = 2; n <= 200; n++) {
                const int s1 = s0 + n, count = jtk::chunk_count(s0, s1, chunk);
                check(count == (n + chunk - 1) / chunk, "chunk_count", chunk, s0, n, count);
                int end = s0;  // (a): the chunks follow each other from s0 to s1
                bool tiled = true, through = true, smallest = true, sets = true;
                for (int i = 0; i < count; i++) {
                    const jtk::ChunkPlan p = jtk::chunk_plan(s0, s1, chunk, i);
                    const int len = p.y - p.x;
                    tiled = tiled && p.x == end && len >= 1 && len <= chunk && (len == chunk || i == count - 1);
                    end = p.y;
                    through = through && p.lk >= 1 && (1 << p.lk) >= len;                   // (b)
                    smallest = smallest && (p.lk == 1 || (1 << (p.lk - 1)) < len);          // (c)
                    sets = sets && p.set == (i & 1);                                        // (d)
                    check(p.lk == jtk::chunk_lk(len), "chunk_plan: lk is not chunk_lk of its length", chunk, s0, n, i);
                }
                check(tiled && end == s1, "chunk_plan: the chunks do not tile the range in order", chunk, s0, n);
                check(through, "chunk_plan: a chunk misses the chunk buffers (lk < 1 or 2^lk < y - x)", chunk, s0, n);
                check(smallest, "chunk_plan: lk is not the smallest", chunk, s0, n);
                check(sets, "chunk_plan: set != i & 1", chunk, s0, n);
            }
    // the tails the schedule used to get wrong, and the natural chunk's: 64 + 1, 32 + 1, 8 + 1
    const int tails[][2] = {{64, 65}, {32, 33}, {8, 9}, {4, 9}, {2, 3}};  // chunk size, samples
    for (const auto& r : tails) {
        const jtk::ChunkPlan p = jtk::chunk_plan(0, r[1], r[0], jtk::chunk_count(0, r[1], r[0]) - 1);
        check(p.x == r[1] - 1 && p.y == r[1] && p.lk == 1, "a tail of one sample", r[0], r[1], p.lk);
    }
    check(jtk::chunk_lk(1) == 1 && jtk::chunk_lk(2) == 1 && jtk::chunk_lk(3) == 2 && jtk::chunk_lk(64) == 6, "chunk_lk pins");
    // a range that ends at the last sample index: no overflow past s1
    const int top = 0x7fffffff;
    const jtk::ChunkPlan last = jtk::chunk_plan(top - 65, top, 64, 1);
    check(jtk::chunk_count(top - 65, top, 64) == 2 && last.x == top - 1 && last.y == top && last.lk == 1, "the last sample index");
}

}  // namespace

int main() {
    const int sizes[][2] = {{13, 7}, {44, 36}, {200, 72}, {8, 8}, {1, 1}};
    // of the 30 tiles (0 .. 29) of 44 x 36, (30, 29) leaves one, the clipped corner tile; (31, 30) and
    // (40, 39) start past the last tile and leave none
    const int shares[][2] = {{1, 0}, {2, 1}, {3, 1}, {4, 3}, {5, 1}, {8, 7}, {30, 29}, {31, 30}, {40, 39}};
    for (const auto& s : sizes)
        for (const auto& sh : shares) check_slots(s[0], s[1], sh[0], sh[1]);
    check(jtk::plan_tiles(44, 36, 30, 29) == 1 && jtk::traced_pixels(44, 36, 30, 29) == 16, "the one-tile share");
    check(jtk::plan_tiles(44, 36, 31, 30) == 0 && jtk::plan_tiles(44, 36, 40, 39) == 0, "the no-tile shares");

    for (const auto& r : STREAM_ROWS) {
        const long long px = r[3] == 1 ? (long long)r[0] * r[1] : ((long long)r[0] * r[1] + r[3] - 1) / r[3];
        check((1 << jtk::stream_log2(px, r[2])) == r[5], "stream_log2", r[0], r[1], r[2], r[3]);
    }

    check_weights();

    for (int D : {2, 3, 4, 8})
        for (int L = 0; L <= 20; L++)
            for (int s0 : {0, 7, 1000003}) {
                int end = s0;  // the shares follow each other from s0 to s0 + L
                bool ok = true;
                for (int d = 0; d < D; d++) {
                    int a = -1, b = -1;
                    jtk::sample_share(s0, s0 + L, d, D, &a, &b);
                    ok = ok && a == end && b >= a;
                    end = b;
                }
                check(ok && end == s0 + L, "sample_share", D, L, s0);
            }

    const long long tile_counts[] = {0, 1, 2, 30, 14400, 16383, 16384, 16385, 32768, 65536, 100000, 262144, 524288, (1 << 20) - 1};
    for (long long tiles : tile_counts) {
        const long long nslot = tiles * 64;
        const int m = jtk::chunk_samples(nslot);
        check(m >= 1 && m <= 64 && (m & (m - 1)) == 0, "chunk_samples: not a power of two in [1, 64]", tiles, m);
        check(m == 1 || 2 * nslot * m <= (1LL << 27), "chunk_samples: above 2^27 records", tiles, m);
        check(m == 64 || 2 * nslot * (2 * m) > (1LL << 27), "chunk_samples: not the largest", tiles, m);
    }

    check_chunks();

    std::printf("plan_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
