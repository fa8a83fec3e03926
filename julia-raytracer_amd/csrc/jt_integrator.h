// jt_integrator.h — the integrator of the megakernel (src/trace.jl): light sampling, the per-lane
// path state (Path), the bounce helpers, sample_lights_pdf's light chain (through the traversal or
// inline), the AOV means, trace_path's and trace_naive's bounce bodies, the camera and the sample
// start. Per-lane device functions, included by jt_kernels.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_bsdf.h"
#include "jt_device.h"
#include "jt_launch.h"
#include "jt_scene_eval.h"
#include "jt_traverse.h"

// eval_bsdfcos + sample_bsdfcos_pdf in one branch per material type (jt_bsdf.h eval_bsdfcos_pdf)
#ifndef JT_FUSED_BSDF
#define JT_FUSED_BSDF 1
#endif

namespace jtk {
using namespace jtd;

// ============================================================================ lights (src/trace.jl)
// sample_lights (src/trace.jl:968-1008)
template <int F>
__device__ __forceinline__ v3 sample_lights(const DScene& S, v3 position, float rl, float rel, v2 ruv) {
    const int light_id = sample_uniform(S.nlights, rl);
    const DLight l = S.lights[light_id - 1];
    const float* cdf = S.cdf + l.cdf_offset;
    if (l.instance >= 0) {
        const int element = l.nguide ? sample_discrete_guided(cdf, l.ncdf, rel, S.guide_t + l.guide_offset,
                                                              S.guide_a + l.guide_offset, l.nguide, l.guide_scale)
                                     : sample_discrete(cdf, l.ncdf, rel);
        const DShape sh = S.shapes[S.inst_shade[l.instance].shape];
        v2 uv = (!(F & FT_QUAD) || sh.kind == KIND_TRI) ? sample_triangle(ruv) : ruv;
        v3 lposition = eval_position<F>(S, l.instance, element - 1, uv);
        return normalize(lposition - position);
    }
    if ((F & FT_ENV) && l.environment >= 0) {
        const DEnv& env = S.envs[l.environment];
        const DTexture t = S.textures[env.tex];
        int idx;  // 1-based, used as-is (:990-993)
        if (l.alias_offset >= 0) {
            // alias-table variant (JT_ENV_ALIAS=1): O(1) — column from rel,
            // keep-or-alias coin from ruv.x (an environment sample does not use ruv). It samples
            // the pmf the CDF holds, so env_light_pdf is unchanged, but it maps random numbers to
            // texels differently from upper_bound: statistically equal, not bit-exact.
            const int col = jl_clampi((int)(rel * (float)l.ncdf), 0, l.ncdf - 1);
            const float2 a = S.alias[l.alias_offset + col];
            idx = (ruv.x < a.x ? col : __float_as_int(a.y)) + 1;
        } else {
            idx = l.nguide ? sample_discrete_guided(cdf, l.ncdf, rel, S.guide_t + l.guide_offset,
                                                    S.guide_a + l.guide_offset, l.nguide, l.guide_scale)
                           : sample_discrete(cdf, l.ncdf, rel);
        }
        float u = ((float)(idx % t.width) + 0.5f) / (float)t.width;
        float v = (float)((((double)idx / (double)t.width) + 0.5) / (double)t.height);
        float su, cu, sv, cv;
        jl_sincos(u * 2 * pif, &su, &cu);
        jl_sincos(v * pif, &sv, &cv);
        return transform_direction(frame_from(env.frame), V3(cu * sv, cv, su * sv));
    }
    return V3(0, 0, 0);
}
// env-light term of sample_lights_pdf (src/trace.jl:1045-1079)
__device__ __forceinline__ float env_light_pdf(const DScene& S, const DLight l, v3 direction) {
    const float* cdf = S.cdf + l.cdf_offset;
    const DEnv& env = S.envs[l.environment];
    const DTexture t = S.textures[env.tex];
    v3 wl = transform_direction(frame_from(env.inv), direction);
    v2 tc = V2(jl_atan2(wl.z, wl.x) / (2 * pif), jl_acos(jl_clamp(wl.y, -1.0f, 1.0f)) / pif);
    if (tc.x < 0) tc.x = tc.x + 1;
    int i = jl_clampi((int)__builtin_truncf(tc.x * (float)t.width), 0, t.width - 1);
    int j = jl_clampi((int)__builtin_truncf(tc.y * (float)t.height), 0, t.height - 1);
    float prob = sample_discrete_pdf(cdf, j * t.width + i + 1) / cdf[l.ncdf - 1];
    float angle = (2 * pif / (float)t.width) * (pif / (float)t.height) *
                  jl_sin(pif * ((float)j + 0.5f) / (float)t.height);
    return prob / angle;
}

// ============================================================================ integrator
// trace_path / trace_naive restated as a per-lane state machine. Every iteration of the
// kernel's shading phase issues exactly one BVH query per waiting lane — a closest-hit scene
// query (PH_SCENE) or one intersect_instance_bvh query of sample_lights_pdf (PH_LIGHT) —
// which the traversal phase then advances (node_step / prim_step). Float operations and RNG draws happen
// in exactly the reference's order; only where the lane waits between them changes.
// PH_FINISH: path done (in a light-hit step), sample not yet accumulated
enum : int { PH_SCENE = 0, PH_LIGHT = 1, PH_FINISH = 2 };
// light_steps(sampler, F), the kernels with light-hit steps: jt_select.h
// the scene's light chains run inline: known at compile time (FT_LINL) or checked at run time
__device__ __forceinline__ bool chains_inline(int F, const DScene& S) { return !(F & FT_NOIL) && ((F & FT_LINL) || S.light_inline); }
enum : int { F_HIT = 1, F_VOLUME = 2 };

// The path's small counters share one register (they are read only in the shading code, and as
// separate registers they were spilled and written back every shading phase):
//   bits 0-14 bounce (jt_create rejects bounces > 32766), 15-22 opbounce (<= 129),
//   23-24 flags (F_HIT, F_VOLUME), 25-31 lcount (the light-query chain, < 100).
constexpr unsigned CTL_BOUNCE = 0x7fffu, CTL_OPB = 15, CTL_FLAGS = 23, CTL_LC = 25;
struct Path {
    v3 o, d;                    // pending ray (during PH_LIGHT the light query's: origin / incoming)
    v3 radiance_, weight_;  // during PH_LIGHT weight already holds weight .* f (src/trace.jl:386)
    Rng rng;
    unsigned ctl;  // bounce | opbounce | flags | lcount (CTL_*)
    int phase;
    float max_roughness_;
    float* pk;  // the lane's parked slots (park(F))
    // sample_lights_pdf in flight (src/trace.jl:1010-1084)
    int li;
    template <int F>
    __device__ __forceinline__ v3 radiance() const {
        return park(F) ? V3(pk[0], pk[BLOCK], pk[2 * BLOCK]) : radiance_;
    }
    template <int F>
    __device__ __forceinline__ void set_radiance(v3 v) {
        if (park(F)) {
            pk[0] = v.x;
            pk[BLOCK] = v.y;
            pk[2 * BLOCK] = v.z;
        } else {
            radiance_ = v;
        }
    }
    template <int F>
    __device__ __forceinline__ v3 lq() const { return park(F) ? V3(pk[4 * BLOCK], pk[5 * BLOCK], pk[6 * BLOCK]) : lq_; }
    template <int F>
    __device__ __forceinline__ void set_lq(v3 v) {
        if (park(F)) {
            pk[4 * BLOCK] = v.x;
            pk[5 * BLOCK] = v.y;
            pk[6 * BLOCK] = v.z;
        } else {
            lq_ = v;
        }
    }
    template <int F>
    __device__ __forceinline__ float max_roughness() const { return park(F) ? pk[3 * BLOCK] : max_roughness_; }
    template <int F>
    __device__ __forceinline__ void set_max_roughness(float v) {
        if (park(F)) pk[3 * BLOCK] = v;
        else max_roughness_ = v;
    }
    template <int F>
    __device__ __forceinline__ float pb() const { return park(F) && JT_PARK_PB ? pk[7 * BLOCK] : pb_; }
    template <int F>
    __device__ __forceinline__ void set_pb(float v) {
        if (park(F) && JT_PARK_PB) pk[7 * BLOCK] = v;
        else pb_ = v;
    }
    // the path weight stays in registers (parked in three more LDS slots it cost the texture
    // kernels a workgroup per CU: DESIGN.md §2 Experiments)
    template <int F>
    __device__ __forceinline__ v3 weight() const { return weight_; }
    template <int F>
    __device__ __forceinline__ void set_weight(v3 v) { weight_ = v; }
    __device__ __forceinline__ int bounce() const { return (int)(ctl & CTL_BOUNCE); }
    __device__ __forceinline__ int opbounce() const { return (int)((ctl >> CTL_OPB) & 0xffu); }
    __device__ __forceinline__ bool flag(int f) const { return (ctl >> CTL_FLAGS) & (unsigned)f; }
    __device__ __forceinline__ void set_flag(int f) { ctl |= (unsigned)f << CTL_FLAGS; }
    __device__ __forceinline__ void clear_flag(int f) { ctl &= ~((unsigned)f << CTL_FLAGS); }
    __device__ __forceinline__ int lcount() const { return (int)(ctl >> CTL_LC); }
    v3 lq_;      // during PH_LIGHT: the shading position (st.o holds the light query's origin,
                 // next_position of src/trace.jl:1039, so every query's ray is (st.o, st.d))
    float pb_;   // sample_bsdfcos_pdf / sample_scattering_pdf (pb<F>(): parked in the mesh kernels)
    float pdf, lpdf;
    Volume vol;  // volume_stack[1] (the stack never holds more than one entry)
};

// while bounce < params.bounces: bounce += 1 (src/trace.jl:295-297, 487-489)
__device__ __forceinline__ bool next_bounce(const DParams& P, Path& st) {
    if (st.bounce() >= P.bounces) return true;
    st.ctl += 1u;  // bounce += 1
    st.phase = PH_SCENE;
    return false;
}
// the opacity retry (src/trace.jl:334-339): bounce -= 1, then the loop's bounce += 1, i.e. the
// loop condition tested with bounce - 1 and bounce unchanged
__device__ __forceinline__ bool next_bounce_retry(const DParams& P, Path& st) {
    if (st.bounce() - 1 >= P.bounces) return true;
    st.phase = PH_SCENE;
    return false;
}
// end of a bounce: weight checks and Russian roulette (src/trace.jl:455-465, 557-567)
template <int F>
__device__ __forceinline__ bool after_weight(const DParams& P, Path& st) {
    if (is_zero(st.weight<F>()) || !all_finite(st.weight<F>())) return true;
    if (st.bounce() > 3) {
        float rr_prob = jl_min(0.99f, max3(st.weight<F>()));
        if (rand1f(st.rng) >= rr_prob) return true;
        st.set_weight<F>(st.weight<F>() * jl_rcp_weight(rr_prob));
    }
    return next_bounce(P, st);
}
// walk the light list: environment terms are added in place, an instance light starts its
// query chain; after the last light the one-sample MIS weight is applied (src/trace.jl:386-397)
template <int F>
__device__ __forceinline__ bool light_advance(const DScene& S, const DParams& P, Path& st) {
    for (;;) {
        st.li += 1;
        if (st.li >= S.nlights) {
            st.o = st.lq<F>();  // the next bounce's ray starts at the shading position
            const float pdf = st.pdf * S.light_pick_pdf;  // sample_uniform_pdf(nlights), host-computed
            st.set_weight<F>(st.weight<F>() / (0.5f * st.pb<F>() + 0.5f * pdf));  // (weight .* f) / (...)
            return after_weight<F>(P, st);
        }
        const DLight l = S.lights[st.li];
        if (!(F & FT_NOIL) && l.instance >= 0) {
            st.lpdf = 0.0f;
            st.ctl &= (1u << CTL_LC) - 1u;  // lcount = 0
            st.o = st.lq<F>();  // the first query starts at the shading position
            st.phase = PH_LIGHT;
            return false;
        }
        if ((F & FT_ENV) && l.environment >= 0) st.pdf += env_light_pdf(S, l, st.d);
    }
}
template <int F>
__device__ __forceinline__ bool begin_light_pdf(const DScene& S, const DParams& P, Path& st) {
    st.pdf = 0.0f;
    st.li = -1;
    st.set_lq<F>(st.o);
    return light_advance<F>(S, P, st);
}
// one intersect_instance_bvh result of the instance-light loop (src/trace.jl:1024-1044), in two
// parts. A hit (light_hit_add) adds the element's pdf term and moves the query origin behind it;
// it returns whether the chain goes on (lcount < 100). A miss, or the 100th hit, ends the chain:
// light_chain_end adds the chain's sum and walks on through the light list.
template <int F>
__device__ __forceinline__ bool light_hit_add(const DScene& S, Path& st, const Hit& h) {
    // the light's element record (DLightElem): eval_position + eval_element_normal + the area
    const int4 lh = row16<F>(S.light_hit + st.li);  // instance, first record
    const DInstShade& is = S.inst_shade[lh.x];
    const fr3 f = frame_from(is.f0, is.f1, is.f2);
    const float4* r = S.light_elems + 5 * (lh.y + h.elem);
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const v3 p1 = V3(r0.x, r0.y, r0.z), p2 = V3(r0.w, r1.x, r1.y), p3 = V3(r1.z, r1.w, r2.x);
    const v2 uv = V2(h.u, h.v);
    v3 lposition;
    if (!(F & FT_QUAD) || __float_as_int(r3.z) == KIND_TRI) {
        lposition = transform_point(f, interp_tri(p1, p2, p3, uv));
    } else {
        const float4 r4 = r[4];
        lposition = transform_point(f, interp_quad(p1, p2, p3, V3(r4.x, r4.y, r4.z), uv));
    }
    const v3 en = V3(r2.y, r2.z, r2.w);
    v3 lnormal = __float_as_int(r3.y) ? en : transform_normal(f, en);
    const float area = r3.x;
    v3 dd = lposition - st.lq<F>();
    st.lpdf += dot(dd, dd) / (__builtin_fabsf(dot(lnormal, st.d)) * area);
    st.o = lposition + st.d * 0.001f;
    st.ctl += 1u << CTL_LC;  // lcount += 1 (< 100: fits its 7 bits)
    return st.lcount() < 100;
}
template <int F>
__device__ __forceinline__ bool light_chain_end(const DScene& S, const DParams& P, Path& st) {
    st.pdf += st.lpdf;
    return light_advance<F>(S, P, st);
}
template <int F>
__device__ __forceinline__ bool light_hit(const DScene& S, const DParams& P, Path& st, const Hit& h) {
    if (h.hit && light_hit_add<F>(S, st, h)) return false;
    return light_chain_end<F>(S, P, st);
}

// The light chain of sample_lights_pdf run inline (DScene::light_inline: every instance light's
// shape BVH is one leaf): each intersect_instance_bvh (src/bvh.jl:493-520) is the instance visit
// with its root box test (node_step) and the leaf's primitives (prim_step), then light_hit, until
// the chain leaves its instance lights. The same functions and the same per-lane order as through
// the traversal loop, so results and counters are unchanged; only where the lane runs them moves:
// here, where most of the wave's lanes run their chains side by side, instead of one-prim-step
// queries and light-hit steps of a few lanes inside the traversal phase. Returns light_hit's
// "path done"; otherwise st.phase is PH_SCENE (the next bounce's scene query).
#ifndef JT_LIGHT_LEAF_STEP
#define JT_LIGHT_LEAF_STEP 1  // 0: every inline light query goes through query_start + node_step (A/B runs)
#endif
// JT_CHAIN_TAIL: a wave runs the end of a light's chain (light_chain_end: the MIS weight, Russian
// roulette, the next bounce) once, after all its lanes have left the query loop, instead of in
// every iteration in which some lane misses. In the kernels whose chains run through
// inst_leaf_query, 1/d and the push mask are computed by the first query of a bounce's chains
// only, and the scene query that follows keeps them too (query_restart). Each lane's own sequence
// of operations is unchanged. 0: the previous loops; 1: the chain's end once, 1/d per query as
// before (A/B runs).
// Adopted per kernel family where measured not slower (EXPERIMENTS.md): not in the wide kernels
// (not measured), not in FT_MESH's (bathroom1: -0.6 %, its chains keep the re-run loop); the light-steps kernel
// (FT_NONE without FT_LINL) never runs a chain inline (select_kernel) and keeps its compiled form.
#ifndef JT_CHAIN_TAIL
#define JT_CHAIN_TAIL 2
#endif
// the FT_MESH kernel (bathroom1's), with or without FT_LINL. mesh_family strips FT_NOIL too: no
// compiled configuration has FT_MESH | FT_NOIL, so the value is the same for every instantiated kernel
__host__ __device__ constexpr bool ft_mesh_kernel(int F) { return mesh_family(F); }
template <bool WIDE, int F>
__host__ __device__ constexpr bool chain_tail() {
    return JT_CHAIN_TAIL && !WIDE && !(F & FT_NOIL) && F != FT_NONE && !ft_mesh_kernel(F);
}
// the chains run through inst_leaf_query: the binary fixed-stack LDS kernels (not FT_MESH's)
template <bool WIDE, bool OVF, bool NCACHE, int F>
__host__ __device__ constexpr bool chain_leaf_step() {
    return JT_LIGHT_LEAF_STEP && !WIDE && !OVF && !NCACHE && !ft_mesh_kernel(F);
}
// 1/d and the push mask once per bounce, in the query state (light_chain, query_restart)
template <bool WIDE, bool OVF, bool NCACHE, int F>
__host__ __device__ constexpr bool chain_dinv_once() {
    return JT_CHAIN_TAIL >= 2 && chain_tail<WIDE, F>() && chain_leaf_step<WIDE, OVF, NCACHE, F>();
}

template <bool WIDE, int RING, bool OVF, int COUNT, bool NCACHE, int F, class CountLq>
__device__ __forceinline__ bool light_chain(const DScene& S, const DParams& P, Path& st, Trav& T, int* stack, int pixel,
                                            Counters& cnt, CountLq count_lq) {
    // No tie re-run is needed here: a one-leaf BLAS has no child order (INST_LEAF_ROOT). The
    // FT_MESH kernel (bathroom1) keeps the re-run loop anyway, never taken: its compiled
    // layout is 4 % faster with it, features2's kernel 1.5 % slower (gpurun_out/r05v)
    constexpr bool RERUN_LOOP = ft_mesh_kernel(F);
    constexpr bool LEAF = chain_leaf_step<WIDE, OVF, NCACHE, F>(), TAIL = chain_tail<WIDE, F>();
    // st.d does not change while the bounce's chains run (light_hit_add moves st.o only): with
    // DINV_ONCE the first query's 1/d and push mask stay in the query state for the later ones
    // (with instance transforms a query may leave its instance's mask in T.negmask: not that one)
    constexpr bool DINV_ONCE = chain_dinv_once<WIDE, OVF, NCACHE, F>();
    constexpr int PB = push_bit(node_baked<OVF, NCACHE, WIDE, F>());
    const auto dinv = [&] { T.wdinv = V3(jl_rcp(st.d.x), jl_rcp(st.d.y), jl_rcp(st.d.z)); };  // ray_dinv (src/bvh.jl:322), no guard
    // one intersect_instance_bvh of the current light
    const auto query = [&] {
        count_lq();
        const int inst = S.lights[st.li].instance;
        if (LEAF) {
            if (!DINV_ONCE) dinv();
            const int negmask = DINV_ONCE && !(F & FT_XFORM) ? T.negmask : neg_mask(st.d, S.order_flip | PB);
            inst_leaf_query<COUNT, F>(S, T, st.o, st.d, T.wdinv, negmask, inst, cnt);
            while (T.nprim > 0) prim_step<COUNT, F>(S, T, cnt);
        } else {
            query_start<WIDE>(S, T, st.o, st.d, inst, stack, 0, PB);
            do {
                node_step_any<WIDE, RING, OVF, COUNT, NCACHE, F>(S, T, stack, pixel, cnt);  // instance + its one-leaf root
                while (T.nprim > 0) prim_step<COUNT, F>(S, T, cnt);
            } while (RERUN_LOOP && rerun_tie<WIDE>(S, T, st.o, st.d, inst, stack, PB));
        }
    };
    if (TAIL) {
        if (DINV_ONCE) {
            dinv();
            if (!(F & FT_XFORM)) T.negmask = neg_mask(st.d, S.order_flip | PB);
        }
        for (;;) {
            // one light's chain: a lane stays while its query hits; then the chain's end, once for
            // the wave's chain lanes together
            do query();
            while (T.h_inst >= 0 && light_hit_add<F>(S, st, query_hit(T)));
            if (light_chain_end<F>(S, P, st)) return true;
            if (st.phase != PH_LIGHT) return false;
        }
    }
    do {
        query();
        if (light_hit<F>(S, P, st, query_hit(T))) return true;
    } while (st.phase == PH_LIGHT);
    return false;
}

// trace_path's bounce body after the closest-hit query (src/trace.jl:298-453)
// The albedo/normal running means (src/trace.jl:635-636) are updated as soon as the bounce-0
// surface is accepted — their targets are final at that point — so they are not path state.
struct Aov {
    float* acc;
    float w_;    // !lane_lds(F)
    int first_;  // params.first (the weight's sample offset)
    int lk_;     // params.lk (log2 of the sample streams)
    // the running-mean weight of the lane's current sample within its stream (stream_weight)
    template <int F>
    __device__ __forceinline__ float w() const {
        if (!lane_lds(F)) return w_;
        if (ft_none(F)) return jl_rcp_weight((float)(((reinterpret_cast<const int*>(acc)[11 * BLOCK] - first_) >> lk_) + 1));
        return acc[12 * BLOCK];
    }
};
template <int F>
__device__ __forceinline__ void aov_update(const Aov& a, v3 ta, v3 tn) {
    const float aw = a.w<F>();
    const float omw = 1 - aw;
    float* p = a.acc;
    p[4 * BLOCK] = p[4 * BLOCK] * omw + ta.x * aw;
    p[5 * BLOCK] = p[5 * BLOCK] * omw + ta.y * aw;
    p[6 * BLOCK] = p[6 * BLOCK] * omw + ta.z * aw;
    p[7 * BLOCK] = p[7 * BLOCK] * omw + tn.x * aw;
    p[8 * BLOCK] = p[8 * BLOCK] * omw + tn.y * aw;
    p[9 * BLOCK] = p[9 * BLOCK] * omw + tn.z * aw;
}
// the sink of a driver that keeps no AOV means (jt_radiance.hip: a caller's ray has no pixel)
struct NoAov {};
template <int F>
__device__ __forceinline__ void aov_update(const NoAov&, v3, v3) {}

// SB: the kernel shades from its baked copy (shade_baked, jt_traverse.h; BakedShade, jt_scene_eval.h)
template <int F, bool SB = false, class AovT>
__device__ __forceinline__ bool path_hit(const DScene& S, const DParams& P, Path& st, Hit isec, const AovT& aov,
                                         unsigned& shades) {
    if (!isec.hit) {
        if (st.bounce() > 0 || !P.envhidden)
            st.set_radiance<F>(st.radiance<F>() + st.weight<F>() * eval_environment<F>(S, st.d));
        return true;
    }
    bool in_volume = false;
    if ((F & FT_VOL) && st.flag(F_VOLUME)) {  // :307-326 (volumes need a volume material)
        float rl = rand1f(st.rng), rd = rand1f(st.rng);
        float distance = sample_transmittance(st.vol.density, isec.t, rl, rd);
        v3 tr = eval_transmittance(st.vol.density, distance);
        float tp = sample_transmittance_pdf(st.vol.density, distance, isec.t);
        st.set_weight<F>((st.weight<F>() * tr) / tp);
        in_volume = distance < isec.t;
        isec.t = distance;
    }
    if (!in_volume) {  // surface (:328-423)
        v3 outgoing = -st.d;
        Shading sh;
        BakedShade bk;
        eval_shading<F, SB>(S, isec.inst, isec.elem, V2(isec.u, isec.v), outgoing, sh, &bk);
        shades++;
        if (P.nocaustics) {
            st.set_max_roughness<F>(jl_max(sh.mat.roughness, st.max_roughness<F>()));
            sh.mat.roughness = st.max_roughness<F>();
        }
        if ((F & FT_OPAC) && sh.mat.opacity < 1 && rand1f(st.rng) >= sh.mat.opacity) {
            if (st.opbounce() > 128) return true;
            st.ctl += 1u << CTL_OPB;  // opbounce += 1 (<= 129)
            st.o = sh.position + st.d * 0.01f;
            return next_bounce_retry(P, st);  // bounce -= 1, then the loop's bounce += 1
        }
        if (st.bounce() == 0) {
            st.set_flag(F_HIT);
            aov_update<F>(aov, sh.mat.color, sh.normal);
        }
        st.set_radiance<F>(st.radiance<F>() + st.weight<F>() * (dot(sh.normal, outgoing) >= 0 ? sh.mat.emission : V3(0, 0, 0)));
        v3 incoming;
        const bool delta = is_delta(sh.mat);
        if (!delta) {
            if (rand1f(st.rng) < 0.5f) {
                float rnl = rand1f(st.rng);
                v2 rn = rand2f(st.rng);
                if constexpr (SB) incoming = sample_matte_baked([&] { return baked_basis(S, bk.elem); }, sh.mat.roughness, outgoing, rn);
                else incoming = sample_bsdfcos<F>(sh.mat, sh.normal, outgoing, rnl, rn);
            } else {
                float rl = rand1f(st.rng), rel = rand1f(st.rng);
                v2 ruv = rand2f(st.rng);
                incoming = sample_lights<F>(S, sh.position, rl, rel, ruv);
            }
            if (is_zero(incoming)) return true;
#if JT_FUSED_BSDF
            v3 fb;
            float pbv;
            if constexpr (SB) eval_matte_pdf_baked(baked_color_pi(S, bk.material), sh.mat.roughness, sh.normal, outgoing, incoming, fb, pbv);
            else eval_bsdfcos_pdf<F>(sh.mat, sh.normal, outgoing, incoming, fb, pbv);
            st.set_weight<F>(st.weight<F>() * fb);
            st.set_pb<F>(pbv);
#else
            st.set_weight<F>(st.weight<F>() * eval_bsdfcos<F>(sh.mat, sh.normal, outgoing, incoming));
            st.set_pb<F>(sample_bsdfcos_pdf<F>(sh.mat, sh.normal, outgoing, incoming));
#endif
        } else {
            float rnl = rand1f(st.rng);
            incoming = sample_delta<F>(sh.mat, sh.normal, outgoing, rnl);
            v3 f = eval_delta<F>(sh.mat, sh.normal, outgoing, incoming);
            float pd = sample_delta_pdf<F>(sh.mat, sh.normal, outgoing, incoming);
            st.set_weight<F>((st.weight<F>() * f) / pd);
        }
        // volume stack push/pop (:405-421); independent of the weight update it follows
        const int mtype = sh.mat.type;
        if ((F & FT_VOL) && (mtype == M_REFRACTIVE || mtype == M_VOLUMETRIC || mtype == M_SUBSURFACE) &&
            dot(sh.normal, outgoing) * dot(sh.normal, incoming) < 0) {
            if (!st.flag(F_VOLUME)) {
                st.set_flag(F_VOLUME);  // eval_material again: only the volume fields are kept
                st.vol.density = sh.mat.density;
                st.vol.scattering = sh.mat.scattering;
                st.vol.scanisotropy = sh.mat.scanisotropy;
            } else {
                st.clear_flag(F_VOLUME);
            }
        }
        st.o = sh.position;
        st.d = incoming;
        return delta ? after_weight<F>(P, st) : begin_light_pdf<F>(S, P, st);
    }
    // volume scattering (:424-453)
    v3 outgoing = -st.d;
    v3 position = st.o + st.d * isec.t;
    v3 incoming;
    if (rand1f(st.rng) < 0.5f) {
        (void)rand1f(st.rng);  // rnl: drawn, unused by sample_scattering
        v2 rn = rand2f(st.rng);
        incoming = sample_scattering(st.vol, outgoing, rn);
    } else {
        float rl = rand1f(st.rng), rel = rand1f(st.rng);
        v2 ruv = rand2f(st.rng);
        incoming = sample_lights<F>(S, position, rl, rel, ruv);
    }
    if (is_zero(incoming)) return true;
    st.set_weight<F>(st.weight<F>() * eval_scattering(st.vol, outgoing, incoming));
    st.set_pb<F>(sample_scattering_pdf(st.vol, outgoing, incoming));
    st.o = position;
    st.d = incoming;
    return begin_light_pdf<F>(S, P, st);
}

// trace_naive's bounce body after the closest-hit query (src/trace.jl:490-569)
template <int F, bool SB = false, class AovT>
__device__ __forceinline__ bool naive_hit(const DScene& S, const DParams& P, Path& st, Hit isec, const AovT& aov,
                                          unsigned& shades) {
    if (!isec.hit) {
        if (st.bounce() > 0 || !P.envhidden)
            st.set_radiance<F>(st.radiance<F>() + st.weight<F>() * eval_environment<F>(S, st.d));
        return true;
    }
    v3 outgoing = -st.d;
    Shading sh;
    BakedShade bk;
    eval_shading<F, SB>(S, isec.inst, isec.elem, V2(isec.u, isec.v), outgoing, sh, &bk);
    shades++;
    if ((F & FT_OPAC) && sh.mat.opacity < 1 && rand1f(st.rng) >= sh.mat.opacity) {
        if (st.opbounce() > 128) return true;
        st.ctl += 1u << CTL_OPB;  // opbounce += 1 (<= 129)
        st.o = sh.position + st.d * 0.01f;
        return next_bounce_retry(P, st);  // bounce -= 1, then the loop's bounce += 1
    }
    if (st.bounce() == 0) {
        st.set_flag(F_HIT);
        aov_update<F>(aov, sh.mat.color, sh.normal);
    }
    st.set_radiance<F>(st.radiance<F>() + st.weight<F>() * (dot(sh.normal, outgoing) >= 0 ? sh.mat.emission : V3(0, 0, 0)));
    v3 incoming, f;
    float p;
    if (sh.mat.roughness != 0) {
        float rnl = rand1f(st.rng);
        v2 rn = rand2f(st.rng);
        if constexpr (SB) incoming = sample_matte_baked([&] { return baked_basis(S, bk.elem); }, sh.mat.roughness, outgoing, rn);
        else incoming = sample_bsdfcos<F>(sh.mat, sh.normal, outgoing, rnl, rn);
        if (is_zero(incoming)) return true;
#if JT_FUSED_BSDF
        if constexpr (SB) eval_matte_pdf_baked(baked_color_pi(S, bk.material), sh.mat.roughness, sh.normal, outgoing, incoming, f, p);
        else eval_bsdfcos_pdf<F>(sh.mat, sh.normal, outgoing, incoming, f, p);
#else
        f = eval_bsdfcos<F>(sh.mat, sh.normal, outgoing, incoming);
        p = sample_bsdfcos_pdf<F>(sh.mat, sh.normal, outgoing, incoming);
#endif
    } else {
        float rnl = rand1f(st.rng);
        incoming = sample_delta<F>(sh.mat, sh.normal, outgoing, rnl);
        if (is_zero(incoming)) return true;
        f = eval_delta<F>(sh.mat, sh.normal, outgoing, incoming);
        p = sample_delta_pdf<F>(sh.mat, sh.normal, outgoing, incoming);
    }
    st.set_weight<F>((st.weight<F>() * f) / p);
    st.o = sh.position;
    st.d = incoming;
    return after_weight<F>(P, st);
}

// eval_camera (src/scene.jl:372-411)
__device__ __forceinline__ void eval_camera(const DCamera& cam, v2 image_uv, v2 lens_uv, v3& ro, v3& rd) {
    const fr3 frame = frame_from(cam.frame);
    const v2 film = V2(cam.film_x, cam.film_y);
    if (!cam.orthographic) {
        v3 q = V3(film.x * (0.5f - image_uv.x), film.y * (image_uv.y - 0.5f), cam.lens);
        v3 dc = -normalize(q);
        v3 e = V3(lens_uv.x * cam.aperture / 2, lens_uv.y * cam.aperture / 2, 0);
        v3 p = (dc * cam.focus) / __builtin_fabsf(dc.z);
        v3 d = normalize(p - e);
        ro = transform_point(frame, e);
        rd = transform_direction(frame, d);
    } else {
        float scale = 1 / cam.lens;
        v3 q = V3(film.x * (0.5f - image_uv.x) * scale, film.y * (image_uv.y - 0.5f) * scale, cam.lens);
        v3 e = V3(-q.x, -q.y, 0) + V3(lens_uv.x * cam.aperture / 2, lens_uv.y * cam.aperture / 2, 0);
        v3 p = V3(-q.x, -q.y, -cam.focus);
        v3 d = normalize(p - e);
        ro = transform_point(frame, e);
        rd = transform_direction(frame, d);
    }
}

// sample_camera (src/trace.jl:651-674) after the prologue's 4 draws (:597-608): the camera ray of
// pixel (i, j) from an rng at the start of the sample's stream (also camera_kernel, jt_surface.hip).
// UNIT (the baking kernels with JT_SINCOS_UNIT=2): the lens sample's azimuth through sincos_unit, the
// same floats; luv.x is a rand1f value
template <bool UNIT = false>
__device__ __forceinline__ void camera_sample(const DParams& P, int i, int j, Rng& rng, v3& o, v3& d) {
    v2 puv = rand2f(rng);
    v2 luv = rand2f(rng);
    v2 uv;
    if (!P.tentfilter) {
        uv = V2(((float)i + puv.x) / (float)P.width, ((float)j + puv.y) / (float)P.height);
    } else {
        const float width = 2.0f, offset = 0.5f;
        v2 fuv = V2(width * (puv.x < 0.5f ? __builtin_sqrtf(2 * puv.x) - 1 : 1 - __builtin_sqrtf(2 - 2 * puv.x)) + offset,
                    width * (puv.y < 0.5f ? __builtin_sqrtf(2 * puv.y) - 1 : 1 - __builtin_sqrtf(2 - 2 * puv.y)) + offset);
        uv = V2(((float)i + fuv.x) / (float)P.width, ((float)j + fuv.y) / (float)P.height);
    }
    eval_camera(P.cam, uv, P.cam.pinhole ? sample_disk_signs(luv) : (UNIT ? sample_disk_unit(luv) : sample_disk(luv)), o, d);
}

// trace_sample prologue (src/trace.jl:597-608): 4 draws, camera ray
template <int F, bool UNIT = false>
__device__ __forceinline__ void start_path(const DParams& P, int i, int j, int pixel, int sample, Path& st) {
    st.rng = rng_init(P.seed, pixel, sample);
    camera_sample<UNIT>(P, i, j, st.rng, st.o, st.d);
    st.set_radiance<F>(V3(0, 0, 0));
    st.set_weight<F>(V3(1, 1, 1));
    st.set_max_roughness<F>(0.0f);
    st.ctl = 0u;  // bounce 0 (the first loop iteration: -1 + 1; bounces >= 0 always enters), no flags
    st.phase = PH_SCENE;
}

}  // namespace jtk
