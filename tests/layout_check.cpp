// layout_check.cpp — a stand-alone pass over the host layout (csrc/jt_layout.cpp) for the sanitizers:
// `make -C julia-raytracer_amd layout-check` builds it with jt_layout.cpp and jt_host.cpp under
// -fsanitize=address,undefined and runs it. No Python, no HIP runtime, no GPU. A manual target for
// a CPU build machine: not a pytest test and not part of `all`.
//
// The scene is synthetic and small, chosen for the layout's edge cases: a triangle shape of 9
// triangles (odd leaves: a pair record with a zero second triangle), a quad shape of 5 quads with
// texcoords, one of them degenerate (p3 == p4), three instances (one rotated, one emissive: an
// instance light), and a second scene without instances (an empty TLAS: one leaf without primitives).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_layout.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "layout_check:%d: %s\n", __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)
#define OK(call)                                                                                  \
    do {                                                                                          \
        if ((call) != JT_OK) {                                                                    \
            std::fprintf(stderr, "layout_check:%d: %s: %s\n", __LINE__, #call, jt_last_error()); \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

static jt_instance instance(int shape, int material, float angle, float tx, float ty, float tz) {
    jt_instance in{};
    const float c = std::cos(angle), s = std::sin(angle);
    const float f[12] = {c, s, 0, -s, c, 0, 0, 0, 1, tx, ty, tz};  // rotation about z, then the offset
    std::memcpy(in.frame, f, sizeof f);
    in.shape = shape;
    in.material = material;
    return in;
}

static int check_layout(const jt_scene& scene, bool expect_light) {
    jt_scene_bvh bvh{};
    jt_lights lights{};
    OK(jt_build_scene_bvh(&scene, 0, &bvh));
    OK(jt_make_lights(&scene, &lights));
    CHECK((lights.nlights > 0) == expect_light);
    jt_params params{};
    params.resolution = 64;
    params.samples = 1;
    params.bounces = 4;
    params.sampler = JT_SAMPLER_PATH;
    params.clamp = 10;
    params.batch = 1;
    params.bvhstacksize = 128;
    for (int traversal = JT_TRAVERSAL_REFERENCE; traversal <= JT_TRAVERSAL_AUTO; traversal++) {
        params.traversal = traversal;
        for (const char* alias : {"0", "1"}) {
            jt::HostScene hs;
            OK(jt::layout_scene(&scene, &bvh, &lights, &params, jt::Options{{"env_alias", alias}}, hs));
            CHECK(hs.wide == (traversal == JT_TRAVERSAL_WIDE));
            CHECK(hs.nodes.empty() == hs.wide && hs.wnodes.empty() == !hs.wide);
            CHECK((int)hs.inst_blas.size() == scene.ninstances && hs.inst_light == expect_light);
            CHECK(hs.prims.size() >= 4 && !hs.blob.empty() && hs.need >= 6);
            if (!hs.wide) OK(jt::make_wide(hs, &scene, &bvh));  // the auto -> wide step
            CHECK(hs.wide && hs.S.tlas_wnodes >= 1 && hs.wnodes.size() >= (size_t)hs.S.tlas_wnodes);
            for (const int4& b : hs.inst_blas) CHECK(b.x >= hs.S.tlas_wnodes && (size_t)b.x < hs.wnodes.size());
        }
    }
    jt_free_lights(&lights);
    jt_free_scene_bvh(&bvh);
    return 0;
}

int main() {
    // 9 triangles: a strip over 11 vertices
    std::vector<float> tpos;
    std::vector<int32_t> tris;
    for (int i = 0; i < 11; i++) tpos.insert(tpos.end(), {0.5f * i, (float)(i & 1), 0.1f * i});
    for (int i = 0; i < 9; i++) tris.insert(tris.end(), {i, i + 1, i + 2});
    // 5 quads: a band between two rows of 6 vertices; the last one ends in a repeated vertex
    std::vector<float> qpos, qtc;
    std::vector<int32_t> quads;
    for (int r = 0; r < 2; r++)
        for (int i = 0; i < 6; i++) {
            qpos.insert(qpos.end(), {(float)i, (float)r, 0.25f * (i % 3)});
            qtc.insert(qtc.end(), {i / 5.0f, (float)r});
        }
    for (int i = 0; i < 5; i++) quads.insert(quads.end(), {i, i + 1, i + 7, i == 4 ? i + 7 : i + 6});

    jt_shape shapes[2] = {};
    shapes[0].ntriangles = 9;
    shapes[0].triangles = tris.data();
    shapes[0].npositions = 11;
    shapes[0].positions = tpos.data();
    shapes[1].nquads = 5;
    shapes[1].quads = quads.data();
    shapes[1].npositions = 12;
    shapes[1].positions = qpos.data();
    shapes[1].ntexcoords = 12;
    shapes[1].texcoords = qtc.data();

    jt_material mats[2] = {};
    for (jt_material& m : mats) {
        m.type = JT_MATTE;
        m.color[0] = m.color[1] = m.color[2] = 0.8f;
        m.ior = 1.5f;
        m.trdepth = 0.01f;
        m.opacity = 1;
        m.emission_tex = m.color_tex = m.roughness_tex = m.scattering_tex = m.normal_tex = -1;
    }
    mats[1].emission[0] = mats[1].emission[1] = mats[1].emission[2] = 5;

    const jt_instance insts[3] = {instance(0, 0, 0, 0, 0, 0), instance(1, 0, 0.5f, 1, 2, 3), instance(0, 1, 0, 0, 4, 0)};
    jt_camera cam{};
    const float camf[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 1, 10};
    std::memcpy(cam.frame, camf, sizeof camf);
    cam.lens = 0.05f, cam.film = 0.036f, cam.aspect = 1.5f, cam.focus = 10000, cam.aperture = 0;

    jt_scene scene{};
    scene.ncameras = 1;
    scene.cameras = &cam;
    scene.ninstances = 3;
    scene.instances = insts;
    scene.nshapes = 2;
    scene.shapes = shapes;
    scene.nmaterials = 2;
    scene.materials = mats;
    if (check_layout(scene, true)) return 1;
    scene.ninstances = 0;  // an empty TLAS
    if (check_layout(scene, false)) return 1;
    std::puts("layout_check: ok");
    return 0;
}
