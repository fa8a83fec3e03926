// jt_layout.cpp — validation and host-side layout of a scene (jt_layout.h): instance renumbering,
// the stack bound, and the flattening into the device records of jt_records.h, the wide records and
// the small-scene LDS blob included. Pure host arithmetic, no HIP runtime. This is where the
// bit-exactness contract with the kernels lives: record order, padding records, quantised boxes, and
// element normals computed with the device's float operations (-ffp-contract=off, as jt_host.cpp).
#include "jt_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace jtd;

namespace jt {
namespace {

inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
template <class I>
inline float as_f(I v) {  // the bits of a 32-bit integer as a float
    static_assert(sizeof(I) == 4, "32-bit integers only");
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}

// Vose's alias table of the pmf a light CDF holds (p_i = cdf[i] - cdf[i-1], src/sampling.jl:39-40),
// appended to `out`: entry i = (probability of keeping column i, the other index of the column).
// Built in double; the JT_ENV_ALIAS variant's sample_lights reads it.
void build_alias_table(const float* cdf, int n, std::vector<float2>& out) {
    std::vector<double> q(n);
    double total = 0;
    for (int i = 0; i < n; i++) {
        q[i] = std::max(0.0, (double)cdf[i] - (i ? (double)cdf[i - 1] : 0.0));
        total += q[i];
    }
    const size_t base = out.size();
    out.resize(base + n);
    std::vector<int> small, large;
    for (int i = 0; i < n; i++) {
        q[i] = total > 0 ? q[i] * n / total : 1.0;
        (q[i] < 1.0 ? small : large).push_back(i);
    }
    while (!small.empty() && !large.empty()) {
        const int s = small.back(), l = large.back();
        small.pop_back();
        out[base + s] = make_float2((float)q[s], as_f(l));
        q[l] -= 1.0 - q[s];
        if (q[l] < 1.0) {
            large.pop_back();
            small.push_back(l);
        }
    }
    for (int i : large) out[base + i] = make_float2(1.0f, as_f(i));
    for (int i : small) out[base + i] = make_float2(1.0f, as_f(i));  // rounding leftovers
}

int tree_depth(const jt_bvh_tree& t) {
    if (t.nnodes == 0) return 0;
    std::vector<std::pair<int, int>> st{{0, 0}};
    int depth = 0;
    while (!st.empty()) {
        auto [n, d] = st.back();
        st.pop_back();
        depth = std::max(depth, d);
        const jt_bvh_node& nd = t.nodes[n];
        if (nd.internal) {
            st.push_back({nd.start, d + 1});
            st.push_back({nd.start + 1, d + 1});
        }
    }
    return depth;
}

// the frame's x, y, z columns are bitwise the unit axes (+0 entries: a -0 could flip the sign
// of a zero normal component in transform_normal)
bool rot_identity(const float* fv) {
    const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    return std::memcmp(fv, id, sizeof id) == 0;
}
DNode pack_node(const jt_bvh_node& n, int start) {
    unsigned meta = (unsigned)(uint16_t)n.num | ((unsigned)(uint8_t)n.axis << 16) | ((unsigned)(n.internal ? 1 : 0) << 24);
    return DNode{f4(n.bmin[0], n.bmax[0], n.bmin[1], n.bmax[1]), f4(n.bmin[2], n.bmax[2], as_f(start), as_f(meta))};
}

// ------------------------------------------------------------- wide records (JT_TRAVERSAL_WIDE)
// Conservative 8-bit quantisation of a child's slab [cmin, cmax] on one axis, relative to the
// record's origin o with scale s (a power of two): the largest lo with o + lo * s <= cmin and the
// smallest hi with o + hi * s >= cmax, evaluated in the device's float operations (wide_box,
// jt_traverse.h; -ffp-contract=off on both sides). false: no byte fits at this scale.
bool quantize_axis(float o, float s, float cmin, float cmax, unsigned& lo, unsigned& hi) {
    auto deq = [&](int q) { return o + (float)q * s; };
    int q = (int)std::max(0.0, std::min(255.0, std::floor(((double)cmin - (double)o) / (double)s)));
    while (q > 0 && deq(q) > cmin) q--;
    while (q < 255 && deq(q + 1) <= cmin) q++;
    if (!(deq(q) <= cmin)) return false;
    lo = (unsigned)q;
    q = (int)std::max(0.0, std::min(255.0, std::ceil(((double)cmax - (double)o) / (double)s)));
    while (q < 255 && deq(q) < cmax) q++;
    while (q > 0 && deq(q - 1) >= cmax) q--;
    if (!(deq(q) >= cmax)) return false;
    hi = (unsigned)q;
    return true;
}
float exp_scale(int e) {  // 2^(e - 127), e = a normal float's biased exponent
    return as_f((unsigned)e << 23);
}
// The wide records of a binary tree: one per internal node N (or the root leaf), holding N's
// grandchildren in slots [LL, LR, RL, RR] (a leaf child takes the pair's first slot alone).
void wide_slots(const jt_bvh_tree& t, int n, int slot[4]) {
    slot[0] = slot[1] = slot[2] = slot[3] = -1;
    const jt_bvh_node& N = t.nodes[n];
    if (!N.internal) {
        slot[0] = n;
        return;
    }
    const int L = N.start, R = N.start + 1;
    if (t.nodes[L].internal) slot[0] = t.nodes[L].start, slot[1] = t.nodes[L].start + 1;
    else slot[0] = L;
    if (t.nodes[R].internal) slot[2] = t.nodes[R].start, slot[3] = t.nodes[R].start + 1;
    else slot[2] = R;
}
// Storage order of the wide records (the binary node each record stands for). JT_WIDE_ORDER 0:
// breadth-first. 1: sibling groups depth-first — a record's internal children are stored
// together, then each child's subtree in slot order, so a subtree is one contiguous run of
// records (a ray descending it stays in a few pages and L2 sets). Storage only: the traversal
// visits the same records in the same order. Measured against breadth-first (two runs each,
// profiles/r06_ab/wide_order_dfs_vs_bfs_r06d.txt): bathroom1 1920x1080x64 +0.1 %, ecosys
// 3840x2160x8 +0.2 %: within noise, so breadth-first stays the default.
#ifndef JT_WIDE_ORDER
#define JT_WIDE_ORDER 0
#endif
std::vector<int> wide_record_order(const jt_bvh_tree& t) {
    std::vector<int> seq;
    if (t.nnodes <= 0) return seq;
    seq.push_back(0);
    if (JT_WIDE_ORDER == 0) {
        for (size_t h = 0; h < seq.size(); h++) {
            if (!t.nodes[seq[h]].internal) continue;
            int slot[4];
            wide_slots(t, seq[h], slot);
            for (int c = 0; c < 4; c++)
                if (slot[c] >= 0 && t.nodes[slot[c]].internal) seq.push_back(slot[c]);
        }
        return seq;
    }
    // depth-first over sibling groups, iterative: a stack of the records whose children are still
    // to be appended (their subtrees then follow in slot order)
    std::vector<int> st{0};
    while (!st.empty()) {
        const int n = st.back();
        st.pop_back();
        if (!t.nodes[n].internal) continue;
        int slot[4];
        wide_slots(t, n, slot);
        int kids[4], nk = 0;
        for (int c = 0; c < 4; c++)
            if (slot[c] >= 0 && t.nodes[slot[c]].internal) kids[nk++] = slot[c];
        for (int c = 0; c < nk; c++) seq.push_back(kids[c]);
        for (int c = nk - 1; c >= 0; c--) st.push_back(kids[c]);
    }
    return seq;
}
// The binary leaves of a tree in the order the wide records list them: records in storage order
// (wide_record_order), within a record its leaf children in slot order. The device lays out
// primitive records and numbers instances in this order, so a record's leaf children are
// consecutive runs (a record could address them from one start) and every binary leaf is
// still one run (the binary traversal addresses a leaf by its start). Measured against node-index
// order: bathroom1 even, ecosys even (profiles/r05_ab/wide48_vs_wide64_r05f.txt "base"); it is
// what a record addressing its leaf children from one start needs (the 48-B record experiment,
// DESIGN.md §2).
std::vector<int> wide_leaf_order(const jt_bvh_tree& t) {
    std::vector<int> order;
    if (t.nnodes <= 0) return order;
    if (!t.nodes[0].internal) {
        order.push_back(0);
        return order;
    }
    for (int n : wide_record_order(t)) {
        int slot[4];
        wide_slots(t, n, slot);
        for (int c = 0; c < 4; c++)
            if (slot[c] >= 0 && !t.nodes[slot[c]].internal) order.push_back(slot[c]);
    }
    return order;
}

// The wide records of one binary tree, appended to `out` in wide_record_order (global indices =
// positions in `out`), their boxes quantised relative to N's box per axis at the smallest scale
// 2^(e-127) >= extent / 255 (and the next larger ones until every child fits). leaf_word(k): the
// child word of binary leaf k. Returns the root record's index, or -1 with the error set.
int build_wide(const jt_bvh_tree& t, const std::function<unsigned(int)>& leaf_word, std::vector<DWide>& out) {
    if (t.nnodes <= 0 || (!t.nodes[0].internal && t.nodes[0].num <= 0)) {
        // an empty tree (make_bvh of no boxes is one leaf without primitives, src/bvh.jl:138-183):
        // one record without children, so a query visits it and finds nothing
        DWide w{};
        w.r3 = make_uint4(W_EMPTY, W_EMPTY, W_EMPTY, W_EMPTY);
        out.push_back(w);
        return (int)out.size() - 1;
    }
    const std::vector<int> seq = wide_record_order(t);
    const size_t base = out.size();
    if (base + seq.size() > (size_t)IDX_MASK) return jt::fail(JT_ERR_UNSUPPORTED, "scene exceeds 2^24 wide records"), -1;
    std::vector<int> rec_of(t.nnodes, -1);  // binary internal node -> its record
    for (size_t h = 0; h < seq.size(); h++) rec_of[seq[h]] = (int)(base + h);
    out.resize(base + seq.size());
    for (size_t h = 0; h < seq.size(); h++) {
        const jt_bvh_node& N = t.nodes[seq[h]];
        int slot[4], a1 = 0, a2 = 0;
        wide_slots(t, seq[h], slot);
        if (N.internal) {
            if (t.nodes[N.start].internal) a1 = t.nodes[N.start].axis;
            if (t.nodes[N.start + 1].internal) a2 = t.nodes[N.start + 1].axis;
        }
        unsigned word[4] = {W_EMPTY, W_EMPTY, W_EMPTY, W_EMPTY};
        for (int c = 0; c < 4; c++) {
            if (slot[c] < 0) continue;
            const jt_bvh_node& C = t.nodes[slot[c]];
            if (C.internal) {
                word[c] = (unsigned)rec_of[slot[c]];
            } else {
                if (C.num < 1 || C.num > 4) return jt::fail(JT_ERR_UNSUPPORTED, "wide traversal: a BVH leaf outside 1..4 primitives"), -1;
                word[c] = leaf_word(slot[c]);
                if (word[c] == W_EMPTY) return -1;
            }
        }
        // quantisation per axis
        unsigned e3[3], lo[3][4] = {}, hi[3][4] = {};
        for (int ax = 0; ax < 3; ax++) {
            const float o = N.bmin[ax];
            bool finite = std::isfinite(N.bmin[ax]) && std::isfinite(N.bmax[ax]);
            for (int c = 0; c < 4; c++)
                if (slot[c] >= 0)
                    finite = finite && std::isfinite(t.nodes[slot[c]].bmin[ax]) && std::isfinite(t.nodes[slot[c]].bmax[ax]);
            if (!finite) return jt::fail(JT_ERR_UNSUPPORTED, "wide traversal: a non-finite BVH box"), -1;
            const double ext = (double)N.bmax[ax] - (double)N.bmin[ax];
            int e = 1;  // smallest biased exponent with 255 * 2^(e - 127) >= ext
            while (e < 254 && 255.0 * std::ldexp(1.0, e - 127) < ext) e++;
            for (;; e++) {
                if (e > 254) return jt::fail(JT_ERR_UNSUPPORTED, "wide traversal: a box cannot be quantised"), -1;
                const float sc = exp_scale(e);
                bool ok = std::isfinite(o + 255.0f * sc);
                for (int c = 0; c < 4 && ok; c++)
                    if (slot[c] >= 0)
                        ok = quantize_axis(o, sc, t.nodes[slot[c]].bmin[ax], t.nodes[slot[c]].bmax[ax], lo[ax][c], hi[ax][c]);
                if (ok) break;
            }
            e3[ax] = (unsigned)e;
        }
        auto bytes = [](const unsigned* v) { return v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24; };
        DWide& W = out[base + h];
        const unsigned meta = e3[0] | e3[1] << 8 | e3[2] << 16 |
                              ((unsigned)(N.internal ? N.axis : 0) | (unsigned)a1 << 2 | (unsigned)a2 << 4) << 24;
        W.r0 = make_float4(N.bmin[0], N.bmin[1], N.bmin[2], as_f(meta));
        W.r1 = make_uint4(bytes(lo[0]), bytes(hi[0]), bytes(lo[1]), bytes(hi[1]));
        W.r2 = make_uint4(bytes(lo[2]), bytes(hi[2]), 0u, 0u);
        W.r3 = make_uint4(word[0], word[1], word[2], word[3]);
    }
    return (int)base;
}

int check_tree(const jt_bvh_tree& t, int nprims_expected, const char* what) {
    if (t.nprimitives != nprims_expected) return jt::fail(JT_ERR_INVALID, std::string(what) + ": primitive count mismatch");
    for (int k = 0; k < t.nnodes; k++) {
        const jt_bvh_node& n = t.nodes[k];
        if (n.internal) {
            if (n.start < 0 || n.start + 1 >= t.nnodes) return jt::fail(JT_ERR_INVALID, std::string(what) + ": bad child index");
        } else if (n.start < 0 || n.num < 0 || n.start + n.num > t.nprimitives) {
            return jt::fail(JT_ERR_INVALID, std::string(what) + ": bad leaf range");
        } else if (n.num > 4) {  // make_bvh's leaves hold at most BVH_MAX_PRIMS (src/bvh.jl:32,166)
            return jt::fail(JT_ERR_INVALID, std::string(what) + ": a leaf above BVH_MAX_PRIMS (4) primitives");
        }
    }
    for (int k = 0; k < t.nprimitives; k++)
        if (t.primitives[k] < 0 || t.primitives[k] >= nprims_expected)
            return jt::fail(JT_ERR_INVALID, std::string(what) + ": bad primitive id");
    return JT_OK;
}

// srgb_to_rgb(byte_to_float(b)) (src/color.jl:12-23), the power evaluated in double
void build_luts(std::vector<float>& srgb, std::vector<float>& bytes) {
    srgb.resize(256);
    bytes.resize(256);
    for (int b = 0; b < 256; b++) {
        float c = (float)b / 255.0f;
        bytes[b] = c;
        srgb[b] = c <= 0.04045f ? c / 12.92f : (float)std::pow((double)((c + 0.055f) / 1.055f), (double)2.4f);
    }
}


// ---------------------------------------------------------------------------------- validation
// what the reference can shade, and every id the flattening follows
int validate(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params) {
    if (params->camera < 0 || params->camera >= scene->ncameras) return jt::fail(JT_ERR_INVALID, "camera id out of range");
    if (params->sampler != JT_SAMPLER_PATH && params->sampler != JT_SAMPLER_NAIVE)
        return jt::fail(JT_ERR_INVALID, "sampler must be 1 (path) or 2 (naive)");
    if (params->samples < 0 || params->bounces < 0 || params->batch < 1)
        return jt::fail(JT_ERR_INVALID, "samples/bounces must be >= 0 and batch >= 1");
    if (params->bounces > 32766)  // the kernel keeps bounce in 15 bits of the path's control word
        return jt::fail(JT_ERR_UNSUPPORTED, "bounces above 32766 are not supported");
    if (bvh->nshapes != scene->nshapes) return jt::fail(JT_ERR_INVALID, "bvh.nshapes != scene.nshapes");
    // ------------------------------------------------------------- validate what the reference can shade
    for (int s = 0; s < scene->nshapes; s++) {
        const jt_shape& sh = scene->shapes[s];
        if (sh.npoints > 0 || (sh.nlines > 0 && sh.ntriangles == 0 && sh.nquads == 0))
            return jt::fail(JT_ERR_UNSUPPORTED, "shape " + std::to_string(s) +
                                                    ": points/lines are not shaded by the reference (src/scene.jl:429,605)");
        if (sh.ntriangles == 0 && sh.nquads == 0)
            return jt::fail(JT_ERR_UNSUPPORTED, "shape " + std::to_string(s) + " has no triangles or quads");
        if (sh.nnormals != 0 && sh.nnormals != sh.npositions)
            return jt::fail(JT_ERR_INVALID, "shape " + std::to_string(s) + ": normals/positions length mismatch");
        if (sh.ntexcoords != 0 && sh.ntexcoords != sh.npositions)
            return jt::fail(JT_ERR_INVALID, "shape " + std::to_string(s) + ": texcoords/positions length mismatch");
        if (sh.ncolors != 0 && sh.ncolors != sh.npositions)
            return jt::fail(JT_ERR_INVALID, "shape " + std::to_string(s) + ": colors/positions length mismatch");
        // (jt_host.cpp validate_scene checks the same ids for the BVH build and the lights, with
        // its own messages)
        const int32_t* idx = sh.ntriangles ? sh.triangles : sh.quads;
        long n = sh.ntriangles ? 3L * sh.ntriangles : 4L * sh.nquads;
        for (long k = 0; k < n; k++)
            if (idx[k] < 0 || idx[k] >= sh.npositions)
                return jt::fail(JT_ERR_INVALID, "shape " + std::to_string(s) + ": vertex id out of range");
    }
    for (int k = 0; k < scene->ninstances; k++) {
        const jt_instance& in = scene->instances[k];
        if (in.shape < 0 || in.shape >= scene->nshapes || in.material < 0 || in.material >= scene->nmaterials)
            return jt::fail(JT_ERR_INVALID, "instance " + std::to_string(k) + ": invalid shape/material id");
        if (scene->materials[in.material].type == JT_GLTFPBR)
            return jt::fail(JT_ERR_UNSUPPORTED, "instance " + std::to_string(k) +
                                                    ": gltfpbr calls undefined functions in the reference (src/shading.jl:254-321)");
    }
    auto tex_ok = [&](int t) { return t >= -1 && t < scene->ntextures; };
    for (int k = 0; k < scene->nmaterials; k++) {
        const jt_material& m = scene->materials[k];
        if (m.type < 0 || m.type > JT_GLTFPBR) return jt::fail(JT_ERR_INVALID, "material type out of range");
        if (!tex_ok(m.emission_tex) || !tex_ok(m.color_tex) || !tex_ok(m.roughness_tex) || !tex_ok(m.scattering_tex) ||
            !tex_ok(m.normal_tex))
            return jt::fail(JT_ERR_INVALID, "material " + std::to_string(k) + ": texture id out of range");
    }
    for (int k = 0; k < scene->nenvironments; k++)
        if (!tex_ok(scene->environments[k].emission_tex)) return jt::fail(JT_ERR_INVALID, "environment texture id out of range");
    for (int k = 0; k < lights->nlights; k++) {
        const jt_light& l = lights->lights[k];
        if ((l.instance >= 0) == (l.environment >= 0) || l.ncdf <= 0 || !l.cdf)
            return jt::fail(JT_ERR_INVALID, "light " + std::to_string(k) + ": malformed");
        if (l.instance >= scene->ninstances || l.environment >= scene->nenvironments)
            return jt::fail(JT_ERR_INVALID, "light " + std::to_string(k) + ": id out of range");
        if (l.environment >= 0 && scene->environments[l.environment].emission_tex < 0)
            return jt::fail(JT_ERR_UNSUPPORTED, "untextured environment light: sample_sphere is undefined (src/trace.jl:1003)");
    }
    return JT_OK;
}

// -------------------------------------------------------- instance renumbering and the stack bound
int renumber_instances(const jt_scene* scene, const jt_scene_bvh* bvh, HostScene& hs) {
    const int st = check_tree(bvh->tlas, scene->ninstances, "tlas");
    if (st != JT_OK) return st;
    // the device numbers instances by TLAS leaf, leaves in wide-record order (wide_leaf_order), a
    // leaf's instances in its own order: a leaf's instances are then the id range start ..
    // start+num-1 (no per-instance index load) and a wide record's leaf children one range. The
    // TLAS must list each instance once.
    hs.inst_new.assign(scene->ninstances, -1);                  // reference instance id -> device id
    hs.tleaf_start.assign(std::max(0, bvh->tlas.nnodes), 0);  // binary TLAS leaf -> first device id
    int next = 0;
    for (int k : wide_leaf_order(bvh->tlas)) {
        const jt_bvh_node& n = bvh->tlas.nodes[k];
        hs.tleaf_start[k] = next;
        for (int q = 0; q < n.num; q++) {
            int& slot = hs.inst_new[bvh->tlas.primitives[n.start + q]];
            if (slot >= 0) return jt::fail(JT_ERR_INVALID, "tlas: an instance is listed twice");
            slot = next++;
        }
    }
    for (int& v : hs.inst_new)  // instances no TLAS leaf lists are never visited
        if (v < 0) v = next++;
    return JT_OK;
}

int stack_bound(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_params* params, HostScene& hs) {
    int max_blas_depth = 0;
    for (int s = 0; s < scene->nshapes; s++) {
        const jt_shape& sh = scene->shapes[s];
        const int st = check_tree(bvh->blas[s], sh.ntriangles ? sh.ntriangles : sh.nquads, "blas");
        if (st != JT_OK) return st;
        max_blas_depth = std::max(max_blas_depth, tree_depth(bvh->blas[s]));
    }
    const int tlas_depth = tree_depth(bvh->tlas);
    // the reference's stacks hold bvhstacksize entries each; a DFS needs depth + 1
    if (std::max(tlas_depth, max_blas_depth) + 1 > params->bvhstacksize)
        return jt::fail(JT_ERR_STACK, "BVH deeper than --bvhstacksize (the reference throws BoundsError)");
    hs.need = tlas_depth + max_blas_depth + 6;  // unified stack bound
    return JT_OK;
}

// scene feature bits (jt_records.h): scenes with none of them run the FT_NONE kernel
int scene_features(const jt_scene* scene, const Options& opts) {
    int f = scene->nenvironments > 0 ? FT_ENV : 0;
    for (int k = 0; k < scene->nmaterials; k++) {
        const jt_material& m = scene->materials[k];
        if (m.type != JT_MATTE) f |= FT_MAT;
        if (m.type == JT_REFRACTIVE || m.type == JT_VOLUMETRIC || m.type == JT_SUBSURFACE) f |= FT_VOL;
        if (m.emission_tex >= 0 || m.color_tex >= 0 || m.roughness_tex >= 0 || m.scattering_tex >= 0 ||
            m.normal_tex >= 0)
            f |= FT_TEX;
        // opacity = m.opacity * color_tex.w * color_shp.w (src/scene.jl:649): a bilinear or
        // barycentric alpha of 1s need not round to exactly 1, so any color texture counts
        if (m.opacity < 1 || m.color_tex >= 0) f |= FT_OPAC;
    }
    for (int k = 0; k < scene->nshapes; k++) {
        const jt_shape& sh = scene->shapes[k];
        if (sh.nquads > 0) f |= FT_QUAD;
        if (sh.nnormals > 0 || sh.ntexcoords > 0 || sh.ncolors > 0) f |= FT_ATTR;
        if (sh.ncolors > 0) f |= FT_OPAC;
    }
    const char* fe = opt(opts, "features");
    return (fe && std::strcmp(fe, "all") == 0) ? FT_ALL : f;
}

// ------------------------------------------------------------------- flatten to the HBM layout
// The TLAS is stored breadth-first (sibling pairs stay adjacent, the root stays node 0), so its
// top levels share cache lines. Storage order only: the traversal still visits the
// reference's nodes in the reference's order.
void flatten_tlas(const jt_bvh_tree& tlas, HostScene& hs) {
    const int tn = std::max(0, tlas.nnodes);
    std::vector<int> order, newidx(tn, -1);
    if (tn > 0) order.push_back(0);
    for (size_t q = 0; q < order.size(); q++) {
        const jt_bvh_node& n = tlas.nodes[order[q]];
        if (n.internal) {
            order.push_back(n.start);
            order.push_back(n.start + 1);
        }
    }
    for (size_t q = 0; q < order.size(); q++) newidx[order[q]] = (int)q;
    hs.nodes.resize(order.size());
    for (size_t q = 0; q < order.size(); q++) {
        const jt_bvh_node& n = tlas.nodes[order[q]];
        hs.nodes[q] = pack_node(n, n.internal ? newidx[n.start] : hs.tleaf_start[order[q]]);
    }
    hs.S.tlas_nnodes = (int)hs.nodes.size();
}

inline jt::f3 vertex(const jt_shape& sh, int vi) {
    return jt::mk3(sh.positions[3 * vi], sh.positions[3 * vi + 1], sh.positions[3 * vi + 2]);
}

// a shape's vertex arrays, elements and element normals; its DShape bases
void flatten_shape(const jt_shape& sh, HostScene& hs, DShape& d) {
    d.kind = sh.ntriangles ? KIND_TRI : KIND_QUAD;
    const int stride = d.kind == KIND_TRI ? 5 : 4;
    d.blas_root = (int)hs.nodes.size();  // global index: TLAS nodes come first, then every BLAS so far
    // records are triangle pairs of 5 float4s or quads of 4: align the shape's first record to
    // its stride so prim_base * stride addresses it exactly when shape kinds are mixed
    while (hs.prims.size() % stride) hs.prims.push_back(f4(0, 0, 0, 0));
    d.prim_base = (int)(hs.prims.size() / stride);  // in records
    d.idx_base = (int)hs.elems.size();
    d.pos_base = (int)hs.pos.size();
    for (int v = 0; v < sh.npositions; v++) hs.pos.push_back(f4(sh.positions[3 * v], sh.positions[3 * v + 1], sh.positions[3 * v + 2], 0));
    d.nrm_base = -1;
    d.tc_base = -1;
    d.col_base = -1;
    // per-vertex attribute arrays are padded to the positions' base so one vertex id serves all
    if (sh.nnormals) {
        while ((int)hs.nrm.size() < d.pos_base) hs.nrm.push_back(f4(0, 0, 0, 0));
        d.nrm_base = (int)hs.nrm.size();
        for (int v = 0; v < sh.nnormals; v++) hs.nrm.push_back(f4(sh.normals[3 * v], sh.normals[3 * v + 1], sh.normals[3 * v + 2], 0));
    }
    if (sh.ntexcoords) {
        while ((int)hs.tc.size() < d.pos_base) hs.tc.push_back(make_float2(0, 0));
        d.tc_base = (int)hs.tc.size();
        for (int v = 0; v < sh.ntexcoords; v++) hs.tc.push_back(make_float2(sh.texcoords[2 * v], sh.texcoords[2 * v + 1]));
    }
    if (sh.ncolors) {
        while ((int)hs.col.size() < d.pos_base) hs.col.push_back(f4(0, 0, 0, 0));
        d.col_base = (int)hs.col.size();
        for (int v = 0; v < sh.ncolors; v++)
            hs.col.push_back(f4(sh.colors[4 * v], sh.colors[4 * v + 1], sh.colors[4 * v + 2], sh.colors[4 * v + 3]));
    }
    const int nel = d.kind == KIND_TRI ? sh.ntriangles : sh.nquads;
    // element normals (triangle_normal / quad_normal, src/geometry.jl:260-271) and their
    // transform_normal by an unrotated frame: host float ops identical to the device's
    for (int k = 0; k < nel; k++) {
        const int* v = d.kind == KIND_TRI ? &sh.triangles[3 * k] : &sh.quads[4 * k];
        auto P3 = [&](int vi) { return vertex(sh, vi); };
        auto tri_n = [](jt::f3 a, jt::f3 b, jt::f3 cc) { return jt::normalize(jt::cross(b - a, cc - a)); };
        jt::f3 n = d.kind == KIND_TRI ? tri_n(P3(v[0]), P3(v[1]), P3(v[2]))
                                      : jt::normalize(tri_n(P3(v[0]), P3(v[1]), P3(v[3])) + tri_n(P3(v[2]), P3(v[3]), P3(v[1])));
        const jt::frame3 I{jt::mk3(1, 0, 0), jt::mk3(0, 1, 0), jt::mk3(0, 0, 1), jt::mk3(0, 0, 0)};
        const jt::f3 ni = jt::normalize(jt::transform_vector(I, n));
        hs.enrm.push_back(f4(n.x, n.y, n.z, 0));
        hs.enrm_id.push_back(f4(ni.x, ni.y, ni.z, 0));
    }
    for (int k = 0; k < nel; k++) {
        if (d.kind == KIND_TRI)
            hs.elems.push_back(make_int4(d.pos_base + sh.triangles[3 * k], d.pos_base + sh.triangles[3 * k + 1],
                                         d.pos_base + sh.triangles[3 * k + 2], 0));
        else
            hs.elems.push_back(make_int4(d.pos_base + sh.quads[4 * k], d.pos_base + sh.quads[4 * k + 1],
                                         d.pos_base + sh.quads[4 * k + 2], d.pos_base + sh.quads[4 * k + 3]));
    }
}

// a shape's BLAS nodes and primitive records; leaf_rec: the record (pair / quad) where each binary
// BLAS leaf's primitives start: the wide records' leaf words (JT_TRAVERSAL_WIDE)
void flatten_blas(const jt_shape& sh, const jt_bvh_tree& t, const DShape& d, HostScene& hs, std::vector<int>& leaf_rec) {
    leaf_rec.assign(t.nnodes, -1);
    // records leaf by leaf, the leaves in wide-record order (wide_leaf_order: a wide record's
    // leaf children are consecutive runs); a leaf's records are its primitives in the
    // reference's order (bvh.primitives[start .. start+num-1]), pre-gathered
    const std::vector<int> lorder = wide_leaf_order(t);
    {
        int at = 0;
        for (int k : lorder) {
            leaf_rec[k] = d.prim_base + at;
            at += d.kind == KIND_TRI ? (t.nodes[k].num + 1) / 2 : t.nodes[k].num;
        }
    }
    for (int k = 0; k < t.nnodes; k++) {
        const jt_bvh_node& n = t.nodes[k];
        hs.nodes.push_back(pack_node(n, n.internal ? d.blas_root + n.start : std::max(0, leaf_rec[k])));
    }
    std::vector<float4>& prims = hs.prims;
    for (int k : lorder) {
        const jt_bvh_node& n = t.nodes[k];
        if (d.kind == KIND_TRI) {
            // Triangle-pair records (a leaf starts a record; an odd leaf's last record has a
            // zero second triangle, never accepted: the leaf count masks it). The two
            // triangles' components are interleaved so the pair test runs on packed FP32:
            //   (p1x p1x' p1y p1y') (p1z p1z' e1x e1x') (e1y e1y' e1z e1z') (e2x e2x' e2y e2y')
            //   (e2z e2z' el el'), edge1 = p2 - p1, edge2 = p3 - p1 (src/geometry.jl:208-209).
            for (int q = 0; q < n.num; q += 2) {
                float4 p[2], e1[2], e2[2];
                int el[2] = {-1, -1};
                for (int h = 0; h < 2; h++) {
                    p[h] = e1[h] = e2[h] = f4(0, 0, 0, 0);
                    if (q + h >= n.num) continue;
                    el[h] = t.primitives[n.start + q + h];
                    const int* v = &sh.triangles[3 * el[h]];
                    const jt::f3 a = vertex(sh, v[0]), b = vertex(sh, v[1]), cc = vertex(sh, v[2]);
                    p[h] = f4(a.x, a.y, a.z, 0);
                    e1[h] = f4(b.x - a.x, b.y - a.y, b.z - a.z, 0);
                    e2[h] = f4(cc.x - a.x, cc.y - a.y, cc.z - a.z, 0);
                }
                prims.push_back(f4(p[0].x, p[1].x, p[0].y, p[1].y));
                prims.push_back(f4(p[0].z, p[1].z, e1[0].x, e1[1].x));
                prims.push_back(f4(e1[0].y, e1[1].y, e1[0].z, e1[1].z));
                prims.push_back(f4(e2[0].x, e2[1].x, e2[0].y, e2[1].y));
                prims.push_back(f4(e2[0].z, e2[1].z, as_f(el[0]), as_f(el[1])));
            }
        } else {
            // quad records (the reference reads positions through bvh.primitives[i])
            for (int q = 0; q < n.num; q++) {
                const int el = t.primitives[n.start + q];
                const int* v = &sh.quads[4 * el];
                const jt::f3 a = vertex(sh, v[0]), b = vertex(sh, v[1]), cc = vertex(sh, v[2]), dd = vertex(sh, v[3]);
                const bool degenerate = cc.x == dd.x && cc.y == dd.y && cc.z == dd.z;  // p3 == p4
                prims.push_back(f4(a.x, a.y, a.z, as_f(el)));
                prims.push_back(f4(b.x, b.y, b.z, 0));
                prims.push_back(f4(cc.x, cc.y, cc.z, 0));
                prims.push_back(f4(dd.x, dd.y, dd.z, degenerate ? 1.0f : 0.0f));
            }
        }
    }
}

void flatten_instances(const jt_scene* scene, const jt_scene_bvh* bvh, HostScene& hs) {
    hs.inst_trav.resize(scene->ninstances);
    hs.inst_blas.resize(scene->ninstances);
    hs.inst_shade.resize(scene->ninstances);
    for (int k0 = 0; k0 < scene->ninstances; k0++) {  // k0: the reference's id, k: the device's
        const int k = hs.inst_new[k0];
        const jt_instance& in = scene->instances[k0];
        jt::frame3 f = jt::load_frame(in.frame);
        jt::frame3 inv = jt::inverse_frame(f, true);
        float iv[12], fv[12];
        jt::store_frame(inv, iv);
        jt::store_frame(f, fv);
        const DShape& d = hs.shapes[in.shape];
        hs.inst_trav[k] = DInstTrav{f4(iv[0], iv[1], iv[2], iv[3]), f4(iv[4], iv[5], iv[6], iv[7]), f4(iv[8], iv[9], iv[10], iv[11]),
                                    in.shape, d.blas_root, d.kind, d.prim_base};
        // identity inverse (exact 1/0 entries, zero offset): transform_ray is the identity on
        // floats, so the traversal reuses the world ray (bit-identical)
        const float idm[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        bool ident = true;
        for (int q = 0; q < 12; q++) ident = ident && iv[q] == idm[q];
        // jtk::node_step reads x, y (z); the wide traversal's x is the BLAS's root record; y the
        // identity inverse; w the shape, with bit 30 (jtk::INST_LEAF_ROOT) set for a one-leaf BLAS:
        // its intersect_instance_bvh tests the leaf's primitives in order whatever the child order,
        // so an exact-t tie there needs no re-run in the reference's order (jtk::rerun_tie)
        const jt_bvh_tree& bt = bvh->blas[in.shape];
        const bool leaf_root = bt.nnodes > 0 && !bt.nodes[0].internal;
        hs.inst_blas[k] = make_int4(hs.wide ? hs.wroot[in.shape] : d.blas_root, ident ? 1 : 0, d.kind, in.shape | (leaf_root ? 1 << 30 : 0));
        // a frame of -0 entries has an identity inverse under == and is not rot_identity: its element
        // normals come from enrm through transform_normal (zero components may change sign), which
        // the kernels without FT_XFORM do not keep (baked shading, jt_kernels.h bake_shading)
        if (!ident || !rot_identity(fv)) hs.feat |= FT_XFORM;
        hs.inst_shade[k] = DInstShade{f4(fv[0], fv[1], fv[2], fv[3]), f4(fv[4], fv[5], fv[6], fv[7]), f4(fv[8], fv[9], fv[10], fv[11]),
                                      in.material, in.shape, scene->materials[in.material].type,
                                      rot_identity(fv) ? 1 : 0};
    }
}

// material, texture (with the texel arrays) and environment records
int flatten_materials(const jt_scene* scene, HostScene& hs) {
    hs.materials.resize(scene->nmaterials);
    for (int k = 0; k < scene->nmaterials; k++) {
        const jt_material& m = scene->materials[k];
        DMaterial& d = hs.materials[k];
        std::memset(&d, 0, sizeof(d));
        d.type = m.type;
        d.emission_tex = m.emission_tex;
        d.color_tex = m.color_tex;
        d.roughness_tex = m.roughness_tex;
        d.scattering_tex = m.scattering_tex;
        d.normal_tex = m.normal_tex;
        for (int q = 0; q < 3; q++) {
            d.emission[q] = m.emission[q];
            d.color[q] = m.color[q];
            d.scattering[q] = m.scattering[q];
        }
        d.roughness = m.roughness;
        d.metallic = m.metallic;
        d.ior = m.ior;
        d.scanisotropy = m.scanisotropy;
        d.trdepth = m.trdepth;
        d.opacity = m.opacity;
    }
    hs.textures.resize(scene->ntextures);
    for (int k = 0; k < scene->ntextures; k++) {
        const jt_texture& t = scene->textures[k];
        DTexture& d = hs.textures[k];
        std::memset(&d, 0, sizeof(d));
        d.width = t.width;
        d.height = t.height;
        d.linear = t.linear;
        d.is_float = t.pixelsf != nullptr;
        const size_t n = (size_t)t.width * (size_t)t.height;
        if (d.is_float) {
            d.offset = (long long)hs.texf.size();
            for (size_t q = 0; q < n; q++)
                hs.texf.push_back(f4(t.pixelsf[4 * q], t.pixelsf[4 * q + 1], t.pixelsf[4 * q + 2], t.pixelsf[4 * q + 3]));
        } else {
            if (!t.pixelsb && n) return jt::fail(JT_ERR_INVALID, "texture without pixels");
            d.offset = (long long)hs.texb.size();
            for (size_t q = 0; q < n; q++)
                hs.texb.push_back(make_uchar4(t.pixelsb[4 * q], t.pixelsb[4 * q + 1], t.pixelsb[4 * q + 2], t.pixelsb[4 * q + 3]));
        }
    }
    // one padding texel: eval_texture loads texels (i, j) and (i + 1, j) as one 8-B pair, which
    // past a texture's last texel reads one texel beyond it (and ignores it)
    hs.texb.push_back(make_uchar4(0, 0, 0, 0));
    hs.envs.resize(scene->nenvironments);
    for (int k = 0; k < scene->nenvironments; k++) {
        const jt_environment& en = scene->environments[k];
        DEnv& d = hs.envs[k];
        std::memset(&d, 0, sizeof(d));
        jt::frame3 f = jt::load_frame(en.frame);
        jt::store_frame(f, d.frame);
        jt::store_frame(jt::inverse_frame(f, false), d.inv);
        for (int q = 0; q < 3; q++) d.emission[q] = en.emission[q];
        d.tex = en.emission_tex;
    }
    return JT_OK;
}

// light records with their CDFs, guide and alias tables, and the light-hit records
void flatten_lights(const jt_scene* scene, const jt_lights* lights, HostScene& hs) {
    std::vector<DLight>& dl = hs.lights;
    dl.resize(lights->nlights);
    for (int k = 0; k < lights->nlights; k++) {
        const jt_light& l = lights->lights[k];
        dl[k] = DLight{l.instance >= 0 ? hs.inst_new[l.instance] : -1, l.environment, (int)hs.cdf.size(), l.ncdf, 0, 0, 0.0f, -1};
        hs.inst_light |= l.instance >= 0;
        hs.cdf.insert(hs.cdf.end(), l.cdf, l.cdf + l.ncdf);
        const float last = l.ncdf > 0 ? l.cdf[l.ncdf - 1] : 0.0f;
        bool monotone = true;
        for (int i = 1; i < l.ncdf && monotone; i++) monotone = l.cdf[i] >= l.cdf[i - 1];
        if (l.ncdf >= 1024 && monotone && last > 0 && std::isfinite(last)) {
            // K buckets of the value range; K + 1 thresholds, the last one = last(cdf)
            const int K = std::min(65536, l.ncdf / 16);
            dl[k].guide_offset = (int)hs.guide_t.size();
            dl[k].nguide = K;
            dl[k].guide_scale = (float)K / last;
            for (int b = 0; b <= K; b++) {
                const float t = b == K ? last : (float)((double)last * b / K);
                // first index with cdf[i] > t (n if none)
                const int a = (int)(std::upper_bound(l.cdf, l.cdf + l.ncdf, t) - l.cdf);
                hs.guide_t.push_back(t);
                hs.guide_a.push_back(a);
            }
            if (hs.env_alias && l.environment >= 0) {
                dl[k].alias_offset = (int)hs.alias.size();
                build_alias_table(l.cdf, l.ncdf, hs.alias);
            }
        }
    }
    // light-hit records (DLightElem, jt_records.h): per instance light, one per element of its shape
    hs.light_hit.assign(std::max(1, lights->nlights), make_int4(-1, 0, 0, 0));
    std::vector<float4>& lelems = hs.light_elems;
    for (int k = 0; k < lights->nlights; k++) {
        const int inst = dl[k].instance;
        if (inst < 0) continue;
        const DInstShade& is = hs.inst_shade[inst];
        const DShape& d = hs.shapes[is.shape];
        const jt_shape& sh = scene->shapes[is.shape];
        const int nel = d.kind == KIND_TRI ? sh.ntriangles : sh.nquads;
        const float area = lights->lights[k].ncdf > 0 ? lights->lights[k].cdf[lights->lights[k].ncdf - 1] : 0.0f;
        hs.light_hit[k] = make_int4(inst, (int)(lelems.size() / 5), 0, 0);
        for (int e = 0; e < nel; e++) {
            const int g = d.idx_base + e;
            const int4 v = hs.elems[g];
            const float4 p1 = hs.pos[v.x], p2 = hs.pos[v.y], p3 = hs.pos[v.z];
            const float4 p4 = d.kind == KIND_TRI ? f4(0, 0, 0, 0) : hs.pos[v.w];
            const float4 n = is.rot_identity ? hs.enrm_id[g] : hs.enrm[g];
            lelems.push_back(f4(p1.x, p1.y, p1.z, p2.x));
            lelems.push_back(f4(p2.y, p2.z, p3.x, p3.y));
            lelems.push_back(f4(p3.z, n.x, n.y, n.z));
            lelems.push_back(f4(area, as_f(is.rot_identity ? 1 : 0), as_f(d.kind), 0));
            lelems.push_back(f4(p4.x, p4.y, p4.z, 0));
        }
    }
    if (lelems.empty()) lelems.assign(5, f4(0, 0, 0, 0));
}

// Inline light queries: when every instance light's shape BVH is one leaf (cornellbox's and
// bathroom1's two-triangle lights, features2's quads), each intersect_instance_bvh of
// sample_lights_pdf is an instance visit, one box test and at most four primitive tests, so the
// lane runs its whole light chain where the chain starts (jtk::light_chain) instead of through
// the traversal loop. Option light_inline=0 turns it off (A/B runs); results are identical.
int light_inline(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const Options& opts) {
    bool inl = true;
    for (int k = 0; k < lights->nlights; k++) {
        const int i0 = lights->lights[k].instance;
        if (i0 < 0) continue;
        const jt_bvh_tree& t = bvh->blas[scene->instances[i0].shape];
        inl = inl && t.nnodes > 0 && !t.nodes[0].internal;
    }
    const char* li = opt(opts, "light_inline");
    if (li && std::atoi(li) == 0) inl = false;
    return inl ? 1 : 0;
}

// ------------------------------------------------------------- small-scene LDS blob
void pack_blob(HostScene& hs) {
    std::vector<uint4>& blob = hs.blob;
    auto add = [&](const void* data, size_t bytes) {
        const int off = (int)blob.size();
        const size_t n16 = (bytes + 15) / 16;
        blob.resize(blob.size() + std::max<size_t>(1, n16));
        if (bytes) std::memcpy(blob.data() + off, data, bytes);
        return off;
    };
#define JT_PACK(T, name) hs.S.o_##name = add(hs.name.data(), hs.name.size() * sizeof(T));
#define JT_SKIP(T, name)
    JT_SCENE_ARRAYS(JT_PACK, JT_SKIP)
#undef JT_PACK
#undef JT_SKIP
}

}  // namespace

int make_wide(HostScene& hs, const jt_scene* scene, const jt_scene_bvh* bvh) {
    hs.wroot.assign(scene->nshapes, 0);
    const int r = build_wide(bvh->tlas, [&](int k) -> unsigned {
        const jt_bvh_node& n = bvh->tlas.nodes[k];
        return W_LEAF | W_INST | (unsigned)(n.num - 1) << 28 | (unsigned)hs.tleaf_start[k];
    }, hs.wnodes);
    if (r < 0) return JT_ERR_UNSUPPORTED;
    hs.S.tlas_wnodes = (int)hs.wnodes.size();
    for (int s = 0; s < scene->nshapes; s++) {
        const jt_bvh_tree& t = bvh->blas[s];
        hs.wroot[s] = build_wide(t, [&](int k) -> unsigned {
            const int st0 = hs.leaf_rec[s][k];
            if (st0 < 0 || st0 > (int)IDX_MASK) return jt::fail(JT_ERR_UNSUPPORTED, "wide traversal: too many primitive records"), (unsigned)W_EMPTY;
            return W_LEAF | (unsigned)(t.nodes[k].num - 1) << 28 | (unsigned)st0;
        }, hs.wnodes);
        if (hs.wroot[s] < 0) return JT_ERR_UNSUPPORTED;
    }
    // the instances' BLAS roots become root records (none yet when layout_scene builds the records)
    for (size_t k0 = 0; k0 < hs.inst_blas.size(); k0++) hs.inst_blas[hs.inst_new[k0]].x = hs.wroot[scene->instances[k0].shape];
    hs.wide = true;
    return JT_OK;
}

int layout_scene(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                 const Options& opts, HostScene& hs) {
    if (!scene || !bvh || !lights || !params) return jt::fail(JT_ERR_INVALID, "NULL argument");
    hs = HostScene{};
    int st;
    if ((st = validate(scene, bvh, lights, params)) || (st = renumber_instances(scene, bvh, hs)) ||
        (st = stack_bound(scene, bvh, params, hs)))
        return st;
    int32_t W = 0, H = 0;
    if ((st = jt_image_size(scene, params, &W, &H)) != JT_OK) return st;
    hs.width = W;
    hs.height = H;
    hs.feat = scene_features(scene, opts);

    flatten_tlas(bvh->tlas, hs);
    hs.shapes.resize(scene->nshapes);
    hs.leaf_rec.resize(scene->nshapes);
    for (int s = 0; s < scene->nshapes; s++) {
        flatten_shape(scene->shapes[s], hs, hs.shapes[s]);
        flatten_blas(scene->shapes[s], bvh->blas[s], hs.shapes[s], hs, hs.leaf_rec[s]);
    }
    // wide records (JT_TRAVERSAL_WIDE): the TLAS's, then every BLAS's; the binary node array is
    // then not uploaded. JT_TRAVERSAL_AUTO resolves to near for a small scene that runs from LDS
    // or a shallow one, and to wide otherwise (decided with the LDS blob, jt_trace.hip
    // prepare_scene; the records are built then).
    if (params->traversal < JT_TRAVERSAL_REFERENCE || params->traversal > JT_TRAVERSAL_AUTO)
        return jt::fail(JT_ERR_INVALID, "traversal must be 0 (reference), 1 (near), 2 (wide) or 3 (auto)");
    hs.wroot.assign(scene->nshapes, 0);
    if (params->traversal == JT_TRAVERSAL_WIDE && (st = make_wide(hs, scene, bvh)) != JT_OK) return st;
    flatten_instances(scene, bvh, hs);
    if ((st = flatten_materials(scene, hs)) != JT_OK) return st;
    const char* ea = opt(opts, "env_alias");
    hs.env_alias = ea && std::atoi(ea) != 0;
    flatten_lights(scene, lights, hs);
    build_luts(hs.srgb_lut, hs.byte_lut);

    // one zero record past the last primitive: prim_step reads the record after a leaf's last
    for (int q = 0; q < 4; q++) hs.prims.push_back(f4(0, 0, 0, 0));
    if (hs.wide) hs.nodes.clear();
    // traversal stack entries carry a 24-bit node / instance index (IDX_MASK)
    if (hs.nodes.size() > IDX_MASK || (size_t)scene->ninstances > IDX_MASK)
        return jt::fail(JT_ERR_UNSUPPORTED, "scene exceeds 2^24 BVH nodes or instances");
    DScene& S = hs.S;
    S.order_flip = params->traversal == JT_TRAVERSAL_REFERENCE ? 0 : 7;  // near and wide: near child first
    S.nenvs = scene->nenvironments;
    S.nlights = lights->nlights;
    S.light_pick_pdf = lights->nlights > 0 ? (float)(1.0 / (double)lights->nlights) : 0.0f;
    S.light_inline = light_inline(scene, bvh, lights, opts);
    pack_blob(hs);
    return JT_OK;
}

}  // namespace jt
