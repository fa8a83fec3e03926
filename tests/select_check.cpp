// select_check.cpp — the choice of a scene's kernel configuration (csrc/jt_select.h: select_kernel
// over the CONFIGS table) enumerated on the host. tests/test_select.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU.
//
//   - the old form: the rules as jt_trace.hip and jt_launch.h spelt them in five places before
//     they became select_kernel (kernel_mask, the launch_s ladder, lds_mode_bytes, the auto-wide
//     rule, the test_lds_ring rewrite, the wait_lanes / light_lanes rule, jt_describe's ovf, ring
//     and kernel name), transcribed below; select_kernel is compared with them field by field
//     over every combination of the domain in main;
//   - properties of the table over the same domain: the chosen row has the choice's ring, overflow
//     and mask; LDS mode only with a row that has an LDS kernel; wide <=> id >= 8; overflow <=>
//     stack > 16; the mask covers the scene's features; FT_LINL only with inline light chains,
//     FT_NOIL only without instance lights; every id 0..15 is chosen by some input;
//   - pinned rows, literal, derived by hand from the old form: the configurations the GPU tests
//     assert through jt_describe (test_gpu_node_bake.py, test_gpu_node_push.py,
//     test_gpu_light_chain.py), and configuration 6.
#include <algorithm>
#include <cstdio>
#include <initializer_list>

#include "../julia-raytracer_amd/csrc/jt_select.h"

namespace {
using namespace jtk;

long cases = 0, bad = 0;
void check(bool ok, const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "select_check: %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

// ---------------------------------------------------------------------------- the old form
int old_kernel_mask(int feat, int need, int ring, bool lds, bool linl, bool inst_light) {
    if (need <= 16) return feat == FT_NONE ? (linl ? FT_NONE | FT_LINL : FT_NONE) : FT_ALL;
    if (ring > 16 || lds) return FT_ALL;
    for (int m : {FT_MESH | FT_LINL, FT_MESH_ENV | FT_NOIL, FT_MESH_ENV_QUAD | FT_LINL})
        if (!(feat & ~m & ~(FT_LINL | FT_NOIL)) && ((m & FT_LINL) ? linl : !inst_light)) return m;
    return FT_ALL;
}
// launch_tw<ID>: configuration ID of the binary traversal, or its wide twin
int old_launch_tw(int id, bool wide) { return wide ? id + NUM_BASE_CONFIGS : id; }
// launch_s: the configuration launched for (need, ring, kmask, wide)
int old_launch_s(int need, int ring, int kmask, bool wide) {
    if (need <= 16) {
        if (kmask == (FT_NONE | FT_LINL)) return old_launch_tw(0, wide);
        if (kmask == FT_NONE) return old_launch_tw(7, wide);
        return old_launch_tw(1, wide);
    }
    if (ring <= 16) {
        switch (kmask) {
            case FT_MESH | FT_LINL: return old_launch_tw(2, wide);
            case FT_MESH_ENV | FT_NOIL: return old_launch_tw(3, wide);
            case FT_MESH_ENV_QUAD | FT_LINL: return old_launch_tw(4, wide);
            default: return old_launch_tw(5, wide);
        }
    }
    return old_launch_tw(6, wide);
}
size_t old_lds_mode_bytes(int feat, int need, size_t blob_bytes, int ring, size_t budget) {
    const size_t acc_bytes = (size_t)ACC_SLOTS * BLOCK * 4 + ((feat & FT_TEX) ? 2048 : 0);
    const size_t base_bytes = (size_t)(need <= 16 ? 16 : ring) * BLOCK * 4 + acc_bytes;
    const size_t lds_base = lds_stack_bytes(need > 16, ring, need) + acc_bytes;
    const size_t bytes = blob_bytes;
    const size_t lds_cu = 160 * 1024;
    const size_t wg_hbm = std::min<size_t>(4, lds_cu / base_bytes), wg_lds = lds_cu / (lds_base + bytes);
    return bytes <= budget && wg_lds >= wg_hbm ? bytes : 0;
}
// the context fields and device-scene members the old jt_create ended with, and jt_describe's view
struct Old {
    int stack, ring, kmask, traversal, id;
    bool wide;
    size_t lds_scene_bytes;
    int S_ring, S_stack_need, ovf_stride;  // DScene
    int wait_lanes, light_lanes;           // DParams
    bool d_ovf, d_filt;                    // jt_describe: ovf, and "ring_used=" printed for the ring
    int d_ring;
    bool d_kernel_lds;  // the kernel named is trace_kernel_lds, not trace_kernel
};
// has_wl / has_ll: the options wait_lanes / light_lanes are set, to the text of the integer wl / ll
Old old_create(const SelectIn& in, bool has_wl, int wl, bool has_ll, int ll) {
    Old c{};
    // prepare_scene
    c.ring = in.lds_stack;
    c.lds_scene_bytes = old_lds_mode_bytes(in.feat, in.need, in.blob_bytes, c.ring, in.lds_scene);
    c.wide = in.traversal == JT_TRAVERSAL_WIDE;  // layout_scene builds the wide records
    if (in.traversal == JT_TRAVERSAL_AUTO && !c.lds_scene_bytes && in.need > JT_AUTO_WIDE_MIN_STACK) c.wide = true;  // make_wide
    c.traversal = in.traversal == JT_TRAVERSAL_AUTO ? (c.wide ? JT_TRAVERSAL_WIDE : JT_TRAVERSAL_NEAR) : in.traversal;
    // jt_create
    c.stack = in.need;
    // alloc_stack_overflow
    const int need = c.stack;
    c.ovf_stride = 0;
    c.S_ring = c.ring;
    c.S_stack_need = c.stack;
    if (in.test_lds_ring != 0) {  // the option is set
        int v = in.test_lds_ring;
        if (v >= 1 && v <= 16 && (v & (v - 1)) == 0) {
            c.S_ring = v;
            c.stack = std::max(c.stack, 17);
            c.ring = 16;
        }
    }
    if (c.stack > 16) c.ovf_stride = need;
    // make_params
    c.kmask = old_kernel_mask(in.feat, c.stack, c.ring, c.lds_scene_bytes > 0, in.light_inline, in.inst_light);
    const int smp = in.sampler == JT_SAMPLER_NAIVE ? 2 : 1;
    const bool lstep = in.inst_light && smp == 1 && (light_steps(smp, c.kmask) || in.light_inline);
    const bool deep = c.stack > 32;
    c.wait_lanes = lstep ? (deep ? 40 : 56) : deep ? 24 : 40;
    if (has_wl) c.wait_lanes = std::max(1, std::min(64, wl));
    c.light_lanes = 2;
    if (has_ll) c.light_lanes = std::max(1, std::min(65, ll));
    // launch_range
    c.id = old_launch_s(c.stack, c.ring, c.kmask, c.wide);
    // jt_describe
    c.d_ovf = c.stack > 16;
    c.d_ring = c.d_ovf ? c.ring : 16;
    c.d_filt = c.S_ring != c.ring;
    c.d_kernel_lds = c.lds_scene_bytes ? true : false;  // "trace_kernel_lds" : "trace_kernel"
    return c;
}

// the kernel launch_t runs for a choice: the LDS-mode one when the configuration has it and the
// blob was uploaded (DScene::blob_n16 > 0, set from lds_scene_bytes)
bool launched_kernel_lds(const KernelChoice& k) { return CONFIGS[k.id % NUM_BASE_CONFIGS].lds && k.lds_scene_bytes > 0; }

bool chosen[NUM_LAUNCH_CONFIGS];

// one input of the domain: a case is good when every comparison and property below holds; a bad one
// names each that does not
void check_case(const SelectIn& in, bool has_wl, int wl) {
    const KernelChoice k = select_kernel(in);
    const Old o = old_create(in, has_wl, wl, false, 0);
    const long a = in.feat, b = in.need, c = (long)in.blob_bytes, d = in.traversal;
    if (k.id < 0 || k.id >= NUM_LAUNCH_CONFIGS) return check(false, "id out of range", a, b, c, d);
    chosen[k.id] = true;
    const ConfigRow& row = CONFIGS[k.id % NUM_BASE_CONFIGS];
    const bool ok[] = {
        // ---- against the old form
        k.id == o.id && k.kmask == o.kmask && k.lds_scene_bytes == o.lds_scene_bytes && k.wide == o.wide && k.traversal == o.traversal,
        k.stack == o.stack && k.stack_need == o.S_stack_need && (k.ovf ? k.stack_need : 0) == o.ovf_stride && k.ring_used == o.S_ring &&
            k.ovf == o.d_ovf && k.ring == o.d_ring && k.ring_shortened() == o.d_filt,
        k.wait_lanes == o.wait_lanes && k.light_lanes == o.light_lanes,
        launched_kernel_lds(k) == o.d_kernel_lds,
        // ---- the table
        row.ring == k.ring && row.ovf == k.ovf && row.feat == k.kmask,
        !k.lds_scene_bytes || row.lds,
        k.wide == (k.id >= NUM_BASE_CONFIGS),
        k.ovf == (k.stack > 16),
        !(in.feat & ~k.kmask),
        !(k.kmask & FT_LINL) || in.light_inline,
        !(k.kmask & FT_NOIL) || !in.inst_light,
    };
    static const char* const what[] = {
        "id / kmask / lds_scene_bytes / wide / traversal differ from the old form",
        "stack / stack_need / ring / ring_used / ovf differ from the old form",
        "wait_lanes / light_lanes differ from the old form",
        "the kernel launched is not the one jt_describe names",
        "the id's row is not the choice's",
        "LDS mode with a row that has no LDS kernel",
        "wide <=> id >= 8",
        "ovf <=> stack > 16",
        "the mask does not cover the scene's features",
        "an FT_LINL mask without inline light chains",
        "an FT_NOIL mask with instance lights",
    };
    static_assert(sizeof ok / sizeof ok[0] == sizeof what / sizeof what[0], "one text per condition");
    bool all = true;
    for (bool x : ok) all = all && x;
    if (all) return check(true, "");
    for (size_t i = 0; i < sizeof ok / sizeof ok[0]; i++)
        if (!ok[i]) check(false, what[i], a, b, c, d);
}

// ---------------------------------------------------------------------------- pinned rows
SelectIn scene(int feat, int need, size_t blob_bytes, bool light_inline, bool inst_light) {
    SelectIn in;
    in.feat = feat;
    in.need = need;
    in.blob_bytes = blob_bytes;
    in.light_inline = light_inline;
    in.inst_light = inst_light;
    return in;  // traversal auto, the path sampler, no option
}

void check_pinned() {
    const size_t MiB = 1 << 20;
    // cornellbox-like: matte triangles, bound 10, a blob that just fits 4 workgroups per CU
    SelectIn in = scene(FT_NONE, 10, 9216, true, true);
    KernelChoice k = select_kernel(in);
    check(k.lds_scene_bytes == 9216 && k.kmask == 8192 && k.id == 0, "pinned: FT_NONE in LDS mode", k.id, k.kmask, (long)k.lds_scene_bytes);
    in.blob_bytes = 9232;
    check(select_kernel(in).lds_scene_bytes == 0, "pinned: one 16-B unit more is HBM mode");
    in = scene(FT_NONE, 10, 9216, false, true);
    k = select_kernel(in);
    check(k.kmask == 0 && k.id == 7, "pinned: FT_NONE with light-hit steps", k.id, k.kmask);
    in = scene(FT_TEX, 10, 9216, true, true);
    k = select_kernel(in);
    check(k.kmask == 255 && k.id == 1, "pinned: a small scene with features", k.id, k.kmask);
    in = scene(FT_NONE, 10, 9216, true, true);
    in.test_lds_ring = 2;
    k = select_kernel(in);
    check(k.lds_scene_bytes == 9216 && k.stack == 17 && k.kmask == 255 && k.id == 5, "pinned: test_lds_ring 2, the kernel", k.id, k.kmask, k.stack);
    check(k.stack_need == 10 && k.ovf && k.ring_used == 2 && k.ring == 16 && k.ring_shortened(), "pinned: test_lds_ring 2, the stack",
          k.stack_need, k.ring_used, k.ring);
    // bathroom1-like
    in = scene(FT_TEX | FT_XFORM, 46, MiB, true, true);
    k = select_kernel(in);
    check(k.lds_scene_bytes == 0 && k.traversal == JT_TRAVERSAL_WIDE && k.wide && k.kmask == 8363 && k.id == 10 && k.wait_lanes == 40,
          "pinned: a deep textured mesh scene", k.id, k.kmask, k.wait_lanes);
    in.sampler = JT_SAMPLER_NAIVE;
    check(select_kernel(in).wait_lanes == 24, "pinned: the same with the naive sampler");
    // ecosys-like
    in = scene(FT_TEX | FT_ENV, 43, MiB, false, false);
    k = select_kernel(in);
    check(k.kmask == 16571 && k.id == 11 && k.wait_lanes == 24, "pinned: environments, no instance light", k.id, k.kmask, k.wait_lanes);
    // features2-like
    in = scene(FT_QUAD | FT_MAT, 24, MiB, true, true);
    k = select_kernel(in);
    check(k.traversal == JT_TRAVERSAL_NEAR && !k.wide && k.kmask == 8383 && k.id == 4 && k.wait_lanes == 56, "pinned: quads, bound 24",
          k.id, k.kmask, k.wait_lanes);
    in.light_inline = false;
    k = select_kernel(in);
    check(k.kmask == 255 && k.id == 5 && k.wait_lanes == 40, "pinned: the same without inline light chains", k.id, k.kmask, k.wait_lanes);
    // configuration 6: the 32-entry ring, whatever the features
    for (int need : {17, 24, 32, 33, 46, 64})
        for (int feat : {(int)FT_NONE, (int)FT_TEX, FT_MESH, (int)FT_ALL})
            for (size_t blob : {(size_t)16, MiB})
                for (int traversal : {JT_TRAVERSAL_REFERENCE, JT_TRAVERSAL_NEAR, JT_TRAVERSAL_WIDE}) {
                    in = scene(feat, need, blob, true, false);
                    in.lds_stack = 32;
                    in.traversal = traversal;
                    k = select_kernel(in);
                    check(k.kmask == 255 && k.id == (traversal == JT_TRAVERSAL_WIDE ? 14 : 6) && k.ring == 32 && k.ring_used == 32,
                          "pinned: lds_stack 32 on a deep scene", need, feat, k.id, k.ring);
                }
    // the options' clamps, and light_lanes (not part of the enumerated domain)
    check(given_lanes(0, 64) == 1 && given_lanes(-3, 64) == 1 && given_lanes(70, 64) == 64 && given_lanes(65, 65) == 65 && given_lanes(48, 64) == 48,
          "given_lanes");
    in = scene(FT_NONE, 10, 9216, true, true);
    in.light_lanes = given_lanes(70, 65);
    k = select_kernel(in);
    const Old o = old_create(in, false, 0, true, 70);
    check(k.light_lanes == 65 && o.light_lanes == 65 && select_kernel(scene(FT_NONE, 10, 9216, true, true)).light_lanes == 2, "light_lanes");
}

// LaunchConfig is the table: the kernels' template arguments come from these
static_assert(LaunchConfig<0>::feat == (FT_NONE | FT_LINL) && LaunchConfig<0>::lds && !LaunchConfig<0>::ovf && !LaunchConfig<0>::wide, "");
static_assert(LaunchConfig<14>::ring == 32 && LaunchConfig<14>::ovf && LaunchConfig<14>::wide && LaunchConfig<14>::feat == FT_ALL, "");
static_assert(LaunchConfig<11>::feat == (FT_MESH_ENV | FT_NOIL) && !LaunchConfig<11>::lds && LaunchConfig<11>::wide, "");

}  // namespace

int main() {
    const size_t blobs[] = {0, 16, 9216, 9232, 48 * 1024, 48 * 1024 + 16, (size_t)1 << 20};
    const size_t budgets[] = {SelectIn{}.lds_scene, 0};
    // the option wait_lanes: unset, "0" (clamped to 1), "70" (clamped to 64)
    const struct { bool has; int text; } waits[] = {{false, 0}, {true, 0}, {true, 70}};
    for (int feat = 0; feat <= 255; feat++)
        for (int need : {1, 10, 16, 17, 24, 32, 33, 46, 64})
            for (int lds_stack : {16, 32})
                for (size_t blob : blobs)
                    for (size_t budget : budgets)
                        for (int linl = 0; linl < 2; linl++)
                            for (int il = 0; il < 2; il++)
                                for (int traversal : {JT_TRAVERSAL_REFERENCE, JT_TRAVERSAL_NEAR, JT_TRAVERSAL_WIDE, JT_TRAVERSAL_AUTO})
                                    for (int sampler : {JT_SAMPLER_PATH, JT_SAMPLER_NAIVE})
                                        for (int test_ring : {0, 2, 16, 3})
                                            for (const auto& w : waits) {
                                                SelectIn in;
                                                in.feat = feat;
                                                in.need = need;
                                                in.blob_bytes = blob;
                                                in.inst_light = il != 0;
                                                in.light_inline = linl != 0;
                                                in.traversal = traversal;
                                                in.sampler = sampler;
                                                in.lds_scene = budget;
                                                in.lds_stack = lds_stack;
                                                in.test_lds_ring = test_ring;
                                                in.wait_lanes = w.has ? given_lanes(w.text, 64) : 0;
                                                check_case(in, w.has, w.text);
                                            }
    for (int id = 0; id < NUM_LAUNCH_CONFIGS; id++) check(chosen[id], "a configuration no input chooses", id);
    check_pinned();
    std::printf("select_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
