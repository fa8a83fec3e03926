// item_coords_check.cpp — the trace kernels' per-lane work item (csrc/jt_plan.h: item_encode, item_i,
// item_j, item_slot) enumerated on the host against slot_pixel, the map that the combine, chain,
// error and adapt kernels read the stream means by. tests/test_item_coords_host.py builds it with the
// host compiler under -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
// For every width and height of {1, 7, 8, 9, 13, 64, 70} and the tile shares (stride, offset) of
// {(1, 0), (2, 1), (3, 2)}:
//   - every pixel (i, j) of the image encodes to an item that is not ITEM_NONE and decodes to (i, j),
//     so the pixel index the kernel forms, j * width + i, is the pixel's;
//   - for the pixels of the share's tiles, slot_pixel(item_slot(item)) is (i, j), inside the image;
//   - those slots are distinct, lie below plan_tiles * 64, and are all of slot_pixel's inside slots:
//     a bijection between the share's pixels and the launch's slots inside the image.
// The reciprocal of the stride is tile_stride_rcp's, as jt_create passes it to the kernels.
#include <cstdio>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_plan.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "item_coords_check: %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

void check_image(int w, int h, int stride, int offset) {
    const int tiles_x = (w + 7) / 8;
    const int tiles = jtk::plan_tiles(w, h, stride, offset);
    const float rcp = jtk::tile_stride_rcp(stride);
    std::vector<int> used((size_t)tiles * 64, 0);
    long mine = 0;
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            const unsigned item = jtk::item_encode(i, j);
            check(item != jtk::ITEM_NONE, "an item equals ITEM_NONE", w, h, i, j);
            check(jtk::item_i(item) == i && jtk::item_j(item) == j, "item does not decode to its pixel", w, h, i, j);
            check(jtk::item_j(item) * w + jtk::item_i(item) == j * w + i, "pixel index", w, h, i, j);
            const int t = (j / 8) * tiles_x + i / 8;
            if (t % stride != offset) continue;  // another share's tile: never handed out
            mine++;
            const int g = jtk::item_slot(item, tiles_x, offset, rcp);
            if (g < 0 || g >= tiles * 64) {
                check(false, "slot outside the launch's slots", w, h, stride, g);
                continue;
            }
            const jtk::SlotPixel p = jtk::slot_pixel(g, w, h, stride, offset);
            check(p.inside && p.i == i && p.j == j, "slot_pixel(item_slot) is another pixel", w, h, i, j);
            check(used[(size_t)g]++ == 0, "two pixels share a slot", w, h, stride, g);
        }
    long inside = 0, unused = 0;  // onto: every inside slot of the launch was reached
    for (int g = 0; g < tiles * 64; g++) {
        const bool in = jtk::slot_pixel(g, w, h, stride, offset).inside;
        inside += in;
        unused += in && !used[(size_t)g];
        check(in || !used[(size_t)g], "a slot outside the image was reached", w, h, stride, g);
    }
    check(unused == 0 && inside == mine, "slots are not a bijection onto the launch's inside slots", w, h, stride, offset);
    check(jtk::traced_pixels(w, h, stride, offset) == mine, "traced_pixels", w, h, stride, offset);
}

}  // namespace

int main() {
    const int dims[] = {1, 7, 8, 9, 13, 64, 70};
    const int shares[][2] = {{1, 0}, {2, 1}, {3, 2}};
    for (int w : dims)
        for (int h : dims)
            for (const auto& s : shares) check_image(w, h, s[0], s[1]);
    // the limits jt_create keeps: the largest coordinates still differ from ITEM_NONE and decode
    const unsigned top = jtk::item_encode(JT_ITEM_MAX_DIM - 1, JT_ITEM_MAX_DIM - 1);
    check(top != jtk::ITEM_NONE && jtk::item_i(top) == JT_ITEM_MAX_DIM - 1 && jtk::item_j(top) == JT_ITEM_MAX_DIM - 1,
          "the largest item");
    // the largest tile count (2^20 - 1 tiles): the float quotient still gives the integer one
    for (int stride : {1, 2, 3, 7, 8, 64}) {
        const int tx = 4096, t = (1 << 20) - 1 - ((1 << 20) - 1) % stride;  // a tile of share (stride, 0)
        const unsigned item = jtk::item_encode((t % tx) * 8 + 7, (t / tx) * 8 + 7);
        check(jtk::item_slot(item, tx, 0, jtk::tile_stride_rcp(stride)) == (t / stride) * 64 + 63, "slot of the last tile", stride, t);
    }
    std::printf("item_coords_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
