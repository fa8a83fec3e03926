// jt_layout.h — the host-side layout of a scene: validation, instance renumbering and the flattening
// of jt_scene / jt_scene_bvh / jt_lights into the device records of jt_records.h (jt_layout.cpp).
// No HIP runtime: it runs, and is tested, on a machine without a GPU. jt_trace.hip uploads the result.
#pragma once

#include <map>
#include <string>
#include <vector>

#include "jt_internal.h"
#include "jt_records.h"

// Every device array of a scene, named once: BLOB(type, name) arrays are also packed into the
// small-scene LDS blob, in this order, at DScene::o_<name>; HBM(type, name) arrays stay in HBM.
// `name` is the HostScene vector and the DScene pointer member. The upload (jt_trace.hip), the blob
// packing (jt_layout.cpp) and the layout digest (jt_debug_layout_digest) all walk this list.
#define JT_SCENE_ARRAYS(BLOB, HBM)                                                                      \
    BLOB(jtd::DNode, nodes) BLOB(jtd::DWide, wnodes) BLOB(float4, prims) BLOB(jtd::DInstTrav, inst_trav) \
    BLOB(int4, inst_blas) BLOB(jtd::DInstShade, inst_shade) BLOB(jtd::DShape, shapes) BLOB(float4, pos)  \
    BLOB(float4, nrm) BLOB(float2, tc) BLOB(float4, col) BLOB(int4, elems) BLOB(float4, enrm)            \
    BLOB(float4, enrm_id) BLOB(jtd::DMaterial, materials) HBM(jtd::DTexture, textures) HBM(uchar4, texb) \
    HBM(float4, texf) HBM(jtd::DEnv, envs) BLOB(jtd::DLight, lights) BLOB(float, cdf)                    \
    BLOB(int4, light_hit) BLOB(float4, light_elems) HBM(float, guide_t) HBM(int, guide_a)                \
    HBM(float2, alias) HBM(float, srgb_lut) HBM(float, byte_lut)

namespace jt {

using Options = std::map<std::string, std::string>;  // options_snapshot()
inline const char* opt(const Options& opts, const char* k) {  // an option's value, or nullptr
    const auto it = opts.find(k);
    return it == opts.end() ? nullptr : it->second.c_str();
}

// traversal stack entries and wide child words carry a 24-bit node / record / instance index
// (jt_select.h)
using jtk::IDX_MASK;

struct HostScene {
#define JT_ARRAY_VECTOR(T, name) std::vector<T> name;
    JT_SCENE_ARRAYS(JT_ARRAY_VECTOR, JT_ARRAY_VECTOR)
#undef JT_ARRAY_VECTOR
    // the small-scene LDS blob: every BLOB array, 16-B aligned, at S.o_<name> (16-B units). Always
    // packed; jt_trace.hip decides whether the scene runs from it (LDS mode)
    std::vector<uint4> blob;
    // the scalars of the device scene (tlas_nnodes, tlas_wnodes, order_flip, nenvs, nlights,
    // light_pick_pdf, light_inline, o_*); the pointers, the blob and the stack members are set at upload
    jtd::DScene S{};
    int need = 0;             // unified stack bound of the scene (entries)
    int feat = jtd::FT_ALL;   // scene feature bits (jt_records.h), or FT_ALL by the option features=all
    int width = 0, height = 0;  // jt_image_size
    bool wide = false;        // the wide records are built and inst_blas[].x are root records
    bool env_alias = false;   // option env_alias: environment lights carry alias tables
    bool inst_light = false;  // sample_lights_pdf runs instance queries (light-hit steps can run)
    // what make_wide needs of the renumbering: reference instance id -> device id, binary TLAS leaf
    // -> first device id, per shape the record (pair / quad) where each binary BLAS leaf's
    // primitives start, and (its result) per shape the root record
    std::vector<int> inst_new, tleaf_start, wroot;
    std::vector<std::vector<int>> leaf_rec;
};

// Validates scene, BVH, lights and params, renumbers the instances, derives the stack bound and
// flattens everything into `hs`, the blob included. Wide records only for JT_TRAVERSAL_WIDE
// (JT_TRAVERSAL_AUTO is resolved by the caller: make_wide). JT_OK or the error (jt_last_error).
int layout_scene(const jt_scene* scene, const jt_scene_bvh* bvh, const jt_lights* lights, const jt_params* params,
                 const Options& opts, HostScene& hs);
// The wide records of a laid-out scene (the TLAS's, then every BLAS's); the instances' BLAS roots
// (inst_blas[].x) become root records. The blob is not repacked: a scene that runs from it stays binary.
int make_wide(HostScene& hs, const jt_scene* scene, const jt_scene_bvh* bvh);

}  // namespace jt
