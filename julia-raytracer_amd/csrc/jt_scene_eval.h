// jt_scene_eval.h — scene evaluation of the megakernel (src/scene.jl:372-928): positions, normals,
// texture coordinates, textures, the material point at a hit, environments. Per-lane device
// functions, included by jt_integrator.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_bsdf.h"
#include "jt_device.h"

namespace jtk {
using namespace jtd;

// ============================================================================ scene evaluation
// One 16-B row of a record, loaded whole for every lane that reaches it. Without the pin the
// compiler narrows a record load to the fields each path reads, and fields read on different
// paths (or at non-adjacent offsets) become several smaller loads. On gfx950 a gather costs one
// vector-memory wave-instruction whatever its width up to 16 B and whatever the number of active
// lanes (scripts/td_width_bench.hip, scripts/td_lanes_bench.hip), and the HBM-mode kernels are
// bound by exactly those instructions. Only the kernels with scene features pin (!ft_none(F)):
// cornellbox's LDS-mode kernel reads these records from LDS.
template <int F>
__device__ __forceinline__ int4 row16(const void* p) {
    int4 v = *reinterpret_cast<const int4*>(p);
    if (!ft_none(F)) __asm__("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
}
// row 3 of DInstShade: material, shape, mat_type, rot_identity
template <int F>
__device__ __forceinline__ int4 inst_ids(const DScene& S, int inst) {
    return row16<F>(reinterpret_cast<const char*>(S.inst_shade + inst) + 48);
}
__device__ __forceinline__ fr3 inst_frame(const DScene& S, int inst) {
    const DInstShade& r = S.inst_shade[inst];
    return frame_from(r.f0, r.f1, r.f2);
}

// eval_position (src/scene.jl:435-476)
template <int F>
__device__ __forceinline__ v3 eval_position(const DScene& S, int inst, int elem, v2 uv) {
    const DInstShade& is = S.inst_shade[inst];
    const int4 sh = row16<F>(S.shapes + inst_ids<F>(S, inst).y);  // DShape row 0: kind, .., idx_base
    const int4 e = S.elems[sh.w + elem];
    const fr3 f = frame_from(is.f0, is.f1, is.f2);
    v3 p1 = xyz(S.pos[e.x]), p2 = xyz(S.pos[e.y]), p3 = xyz(S.pos[e.z]);
    if (!(F & FT_QUAD) || sh.x == KIND_TRI) return transform_point(f, interp_tri(p1, p2, p3, uv));
    return transform_point(f, interp_quad(p1, p2, p3, xyz(S.pos[e.w]), uv));
}
// eval_element_normal (src/scene.jl:578-612): transform_normal(frame, triangle/quad normal),
// with the element normal (and, for an unrotated frame, the whole result) precomputed
// (one load from either array, selected per lane: lanes of both kinds share the instruction)
__device__ __forceinline__ v3 element_normal(const DScene& S, int rot_identity, const fr3& f, int g) {
    const v3 n = xyz((rot_identity ? S.enrm_id : S.enrm)[g]);
    return rot_identity ? n : transform_normal(f, n);
}
template <int F>
__device__ __forceinline__ v3 eval_element_normal(const DScene& S, int inst, int elem) {
    const DInstShade& is = S.inst_shade[inst];
    const int4 ids = inst_ids<F>(S, inst);
    const int4 sh = row16<F>(S.shapes + ids.y);
    return element_normal(S, ids.w, frame_from(is.f0, is.f1, is.f2), sh.w + elem);
}
// eval_normal (src/scene.jl:525-576)
__device__ __forceinline__ v3 eval_normal(const DScene& S, const DShape& sh, const int4& e, const fr3& f, v2 uv) {
    if (sh.nrm_base < 0) {
        v3 p1 = xyz(S.pos[e.x]), p2 = xyz(S.pos[e.y]), p3 = xyz(S.pos[e.z]);
        if (sh.kind == KIND_TRI) return transform_normal(f, triangle_normal(p1, p2, p3));
        return transform_normal(f, quad_normal(p1, p2, p3, xyz(S.pos[e.w])));
    }
    const int b = sh.nrm_base - sh.pos_base;  // normals share vertex ids with positions
    v3 n1 = xyz(S.nrm[e.x + b]), n2 = xyz(S.nrm[e.y + b]), n3 = xyz(S.nrm[e.z + b]);
    if (sh.kind == KIND_TRI) return transform_normal(f, normalize(interp_tri(n1, n2, n3, uv)));
    return transform_normal(f, normalize(interp_quad(n1, n2, n3, xyz(S.nrm[e.w + b]), uv)));
}
// eval_texcoord (src/scene.jl:753-788)
__device__ __forceinline__ v2 eval_texcoord(const DScene& S, const DShape& sh, const int4& e, v2 uv) {
    if (sh.tc_base < 0) return uv;
    const int b = sh.tc_base - sh.pos_base;
    float2 t1 = S.tc[e.x + b], t2 = S.tc[e.y + b], t3 = S.tc[e.z + b];
    if (sh.kind == KIND_TRI) return interp_tri(V2(t1.x, t1.y), V2(t2.x, t2.y), V2(t3.x, t3.y), uv);
    float2 t4 = S.tc[e.w + b];
    return interp_quad(V2(t1.x, t1.y), V2(t2.x, t2.y), V2(t3.x, t3.y), V2(t4.x, t4.y), uv);
}
// eval_color (src/scene.jl:690-720)
__device__ __forceinline__ v4 eval_color(const DScene& S, const DShape& sh, const int4& e, v2 uv) {
    if (sh.col_base < 0) return V4(1, 1, 1, 1);
    const int b = sh.col_base - sh.pos_base;
    float4 c1 = S.col[e.x + b], c2 = S.col[e.y + b], c3 = S.col[e.z + b];
    v4 a = V4(c1.x, c1.y, c1.z, c1.w), bb = V4(c2.x, c2.y, c2.z, c2.w), c = V4(c3.x, c3.y, c3.z, c3.w);
    if (sh.kind == KIND_TRI) return interp_tri(a, bb, c, uv);
    float4 c4 = S.col[e.w + b];
    return interp_quad(a, bb, c, V4(c4.x, c4.y, c4.z, c4.w), uv);
}
// lookup_texture (src/scene.jl:836-849): 8-bit texels decode through exact host-built LUTs
__device__ __forceinline__ v4 lookup_texture(const DScene& S, const DTexture& t, int i, int j, bool as_linear) {
    long long k = t.offset + (long long)j * t.width + i;
    if (t.is_float) {
        float4 c = S.texf[k];
        return V4(c.x, c.y, c.z, c.w);
    }
    uchar4 b = S.texb[k];
    const float* lut = (as_linear && !t.linear) ? S.srgb_lut : S.byte_lut;
    return V4(lut[b.x], lut[b.y], lut[b.z], S.byte_lut[b.w]);
}
// mod1(x, 1.0f0) (Julia base: mod via rem, then 0 -> 1)
__device__ __forceinline__ float jl_mod1(float x) {
    float r = __builtin_fmodf(x, 1.0f);
    float m = r == 0 ? __builtin_copysignf(r, 1.0f) : (r < 0 ? r + 1.0f : r);
    return m == 0 ? 1.0f : m;
}
// two horizontally adjacent 8-bit texels (i, j) and (i + 1, j) in one 8-B load (one vector-memory
// instruction instead of two; texb carries a padding texel past its end)
struct __attribute__((aligned(4))) TexelPair {
    uchar4 a, b;
};
// The two 256-entry texel-decode LUTs (srgb_lut, then byte_lut) in LDS, filled at kernel start
// by the kernels that evaluate textures: a texel's four channel decodes are then LDS reads, not
// four more vector-memory gathers per texel.
static __shared__ float tex_lut[512];
// fills them: every thread of the workgroup, once, before the first eval_texture. The megakernel
// (trace_body_items, jt_kernels.h) keeps the loop written out: through this function two of its
// ADAPT instances spill two and four more SGPRs
__device__ __forceinline__ void stage_tex_lut(const DScene& S) {
    for (int k = threadIdx.x; k < 512; k += BLOCK) tex_lut[k] = k < 256 ? S.srgb_lut[k] : S.byte_lut[k - 256];
    __syncthreads();
}
__device__ __forceinline__ v4 decode_texel(uchar4 b, const float* lut) {
    return V4(lut[b.x], lut[b.y], lut[b.z], tex_lut[256 + b.w]);
}
// eval_texture (src/scene.jl:790-834): bilinear, wrap
__device__ __forceinline__ v4 eval_texture(const DScene& S, int tex, v2 uv, bool as_linear) {
    if (tex < 0) return V4(1, 1, 1, 1);
    const DTexture t = S.textures[tex];
    if (t.width == 0 || t.height == 0) return V4(0, 0, 0, 0);
    float s = jl_mod1(uv.x) * (float)t.width;
    if (s < 0) s += (float)t.width;
    float tt = jl_mod1(uv.y) * (float)t.height;
    if (tt < 0) tt += (float)t.height;
    int i = jl_clampi((int)__builtin_truncf(s), 0, t.width - 1);
    int j = jl_clampi((int)__builtin_truncf(tt), 0, t.height - 1);
    int ii = (i + 1) % t.width, jj = (j + 1) % t.height;
    float u = s - (float)i, v = tt - (float)j;
    v4 ta, tb, tc, td;  // texels (i, j), (i, jj), (ii, j), (ii, jj)
    if (t.is_float) {
        ta = lookup_texture(S, t, i, j, as_linear);
        tb = lookup_texture(S, t, i, jj, as_linear);
        tc = lookup_texture(S, t, ii, j, as_linear);
        td = lookup_texture(S, t, ii, jj, as_linear);
    } else {
        const TexelPair r0 = *reinterpret_cast<const TexelPair*>(S.texb + t.offset + (long long)j * t.width + i);
        const TexelPair r1 = *reinterpret_cast<const TexelPair*>(S.texb + t.offset + (long long)jj * t.width + i);
        uchar4 c0 = r0.b, c1 = r1.b;
        if (ii == 0) {  // right edge: the neighbour wraps to column 0
            c0 = S.texb[t.offset + (long long)j * t.width];
            c1 = S.texb[t.offset + (long long)jj * t.width];
        }
        const float* lut = tex_lut + ((as_linear && !t.linear) ? 0 : 256);
        ta = decode_texel(r0.a, lut);
        tb = decode_texel(r1.a, lut);
        tc = decode_texel(c0, lut);
        td = decode_texel(c1, lut);
    }
    v4 a = (ta * (1 - u)) * (1 - v);
    v4 b = (tb * (1 - u)) * v;
    v4 c = (tc * u) * (1 - v);
    v4 d = (td * u) * v;
    return ((a + b) + c) + d;
}
// eval_normalmap (src/scene.jl:722-751) with eval_element_tangents (:851-891)
__device__ __forceinline__ v3 eval_normalmap(const DScene& S, const DShape& sh, const int4& e, const fr3& f,
                                          const DMaterial& m, v2 uv) {
    v3 normal = eval_normal(S, sh, e, f, uv);
    v2 texcoord = eval_texcoord(S, sh, e, uv);
    v4 t4 = eval_texture(S, m.normal_tex, texcoord, false);
    v3 nm = V3(t4.x * 2 - 1, t4.y * 2 - 1, t4.z * 2 - 1);
    v3 tu = V3(0, 0, 0), tv = V3(0, 0, 0);
    if (sh.tc_base >= 0) {
        const int b = sh.tc_base - sh.pos_base;
        float2 a1 = S.tc[e.x + b], a2 = S.tc[e.y + b];
        if (sh.kind == KIND_TRI) {
            float2 a3 = S.tc[e.z + b];
            triangle_tangents_fromuv(xyz(S.pos[e.x]), xyz(S.pos[e.y]), xyz(S.pos[e.z]), V2(a1.x, a1.y),
                                     V2(a2.x, a2.y), V2(a3.x, a3.y), tu, tv);
        } else {  // quad_tangents_fromuv at current_uv = (0, 0): triangle (p1, p2, p4)
            float2 a4 = S.tc[e.w + b];
            triangle_tangents_fromuv(xyz(S.pos[e.x]), xyz(S.pos[e.y]), xyz(S.pos[e.w]), V2(a1.x, a1.y),
                                     V2(a2.x, a2.y), V2(a4.x, a4.y), tu, tv);
        }
        tu = transform_direction(f, tu);
        tv = transform_direction(f, tv);
    }
    v3 f1 = normalize(tu - normal * dot(tu, normal));  // orthonormalize(frame[1], frame[3])
    v3 f2 = normalize(cross(normal, tu));
    bool flip_v = dot(f2, tv) < 0;
    nm = V3(nm.x, nm.y * (flip_v ? 1.0f : -1.0f), nm.z);
    fr3 fr{f1, f2, normal, V3(0, 0, 0)};
    return transform_normal(fr, nm);
}

struct Shading {
    v3 position, normal;
    MatPoint mat;
};
// Where the baked shading of a hit lies in the workgroup's LDS copy (bake_shading, jt_kernels.h,
// names the bytes): kept as two indices and read at the use, not as nine floats across the bounce
struct BakedShade {
    int elem, material;  // global element, material
};
__device__ __forceinline__ BakedBasis baked_basis(const DScene& S, int g) {
    const float4 bz = S.enrm[g], ni = S.enrm_id[g];
    return BakedBasis{xyz(ni), bz.w, ni.w, __int_as_float(S.elems[g].w), xyz(bz)};
}
__device__ __forceinline__ v3 baked_color_pi(const DScene& S, int material) {
    const DMaterial& m = S.materials[material];
    return V3(m.scattering[0], m.scattering[1], m.scattering[2]);
}

// eval_shading_position + eval_shading_normal + eval_material (src/scene.jl:416-673)
// SB (the baking LDS-mode kernels, shade_baked: S is the workgroup's baked copy): the element's and
// the material's baked shading are read where the bounce uses them (bk says where).
template <int F, bool SB = false>
__device__ __forceinline__ void eval_shading(const DScene& S, int inst, int elem, v2 uv, v3 outgoing, Shading& out,
                                             BakedShade* bk = nullptr) {
    static_assert(!SB || ft_none(F), "baked shading: the FT_NONE kernels only");
    const DInstShade is = S.inst_shade[inst];
    const DShape sh = S.shapes[is.shape];
    const int4 e = S.elems[sh.idx_base + elem];
    const fr3 f = frame_from(is.f0, is.f1, is.f2);
    const DMaterial& m = S.materials[is.material];
    v3 p1 = xyz(S.pos[e.x]), p2 = xyz(S.pos[e.y]), p3 = xyz(S.pos[e.z]);
    const bool tri = !(F & FT_QUAD) || sh.kind == KIND_TRI;
    v3 p4 = !tri ? xyz(S.pos[e.w]) : p3;
    // position
    out.position = tri ? transform_point(f, interp_tri(p1, p2, p3, uv))
                       : transform_point(f, interp_quad(p1, p2, p3, p4, uv));
    // shading normal
    const int mtype = (F & FT_MAT) ? m.type : (int)M_MATTE;
    v3 normal;
    if ((F & FT_TEX) && m.normal_tex >= 0) {
        normal = eval_normalmap(S, sh, e, f, m, uv);
    } else if constexpr (SB) {
        // a scene without FT_XFORM has only instances of rot_identity (layout_scene), so the element
        // normal is enrm_id's; the bake pass (bake_shading) left the basis in the bytes around it
        normal = xyz(S.enrm_id[sh.idx_base + elem]);
        bk->elem = sh.idx_base + elem;
        bk->material = is.material;
    } else if (!(F & FT_ATTR) || sh.nrm_base < 0) {
        normal = element_normal(S, is.rot_identity, f, sh.idx_base + elem);
    } else {
        normal = eval_normal(S, sh, e, f, uv);
    }
    if (mtype != M_REFRACTIVE) normal = dot(normal, outgoing) >= 0 ? normal : -normal;
    out.normal = normal;
    // material point
    MatPoint& p = out.mat;
    const v4 one = V4(1, 1, 1, 1);
    v2 texcoord = (F & FT_ATTR) ? eval_texcoord(S, sh, e, uv) : uv;
    v4 emission_tex = (F & FT_TEX) ? eval_texture(S, m.emission_tex, texcoord, true) : one;
    v4 color_shp = (F & FT_ATTR) ? eval_color(S, sh, e, uv) : one;
    v4 color_tex = (F & FT_TEX) ? eval_texture(S, m.color_tex, texcoord, true) : one;
    v4 roughness_tex = (F & FT_TEX) ? eval_texture(S, m.roughness_tex, texcoord, false) : one;
    v4 scattering_tex = (F & FT_TEX) ? eval_texture(S, m.scattering_tex, texcoord, true) : one;
    p.type = mtype;
    p.emission = V3(m.emission[0], m.emission[1], m.emission[2]) * xyz(emission_tex);
    p.color = (V3(m.color[0], m.color[1], m.color[2]) * xyz(color_tex)) * xyz(color_shp);
    p.opacity = m.opacity * color_tex.w * color_shp.w;
    p.metallic = m.metallic * roughness_tex.z;
    float roughness = m.roughness * roughness_tex.y;
    roughness = roughness * roughness;
    p.ior = m.ior;
    // (baked shading keeps color / pif in DMaterial::scattering: read by kernels with FT_VOL only)
    p.scattering = SB ? V3(0, 0, 0) : V3(m.scattering[0], m.scattering[1], m.scattering[2]) * xyz(scattering_tex);
    p.scanisotropy = m.scanisotropy;
    p.trdepth = m.trdepth;
    if ((F & FT_VOL) && (mtype == M_REFRACTIVE || mtype == M_VOLUMETRIC || mtype == M_SUBSURFACE)) {
        p.density = V3(-jl_log(jl_clamp(p.color.x, 0.0001f, 1.0f)) / p.trdepth,
                       -jl_log(jl_clamp(p.color.y, 0.0001f, 1.0f)) / p.trdepth,
                       -jl_log(jl_clamp(p.color.z, 0.0001f, 1.0f)) / p.trdepth);
    } else {
        p.density = V3(0, 0, 0);
    }
    if (mtype == M_MATTE || mtype == M_GLTFPBR || mtype == M_GLOSSY) roughness = jl_clamp(roughness, min_roughness, 1.0f);
    else if (mtype == M_VOLUMETRIC) roughness = 0.0f;
    else if (roughness < min_roughness) roughness = 0.0f;
    p.roughness = roughness;
}

// eval_environment (src/scene.jl:893-914)
template <int F>
__device__ __forceinline__ v3 eval_environment(const DScene& S, v3 direction) {
    v3 emission = V3(0, 0, 0);
    if (!(F & FT_ENV)) return emission;  // no environments: the sum is empty
    for (int k = 0; k < S.nenvs; k++) {
        const DEnv& env = S.envs[k];
        v3 wl = transform_direction(frame_from(env.inv), direction);
        v2 tc = V2(jl_atan2(wl.z, wl.x) / (2.0f * pif), jl_acos(jl_clamp(wl.y, -1.0f, 1.0f)) / pif);
        if (tc.x < 0.0f) tc.x = tc.x + 1.0f;
        v4 t = eval_texture(S, env.tex, tc, false);
        emission = emission + V3(env.emission[0], env.emission[1], env.emission[2]) * xyz(t);
    }
    return emission;
}

}  // namespace jtk
