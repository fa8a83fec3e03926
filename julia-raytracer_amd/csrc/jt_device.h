// jt_device.h — per-lane math of the MI355X path tracer; the device-side data layout it works on
// is jt_records.h (plain data, shared with the host layout in jt_layout.cpp).
//
// Everything here runs per lane inside the trace megakernel (jt_kernels.h and the headers it is made of). Each function
// cites the reference (Princic-1837592/julia-raytracer) source it computes. Float contract
// (DESIGN.md §Numerics): compiled with -ffp-contract=off (no FMA contraction, Julia's
// evaluation order), Julia's NaN-propagating min/max, and — in the parity build
// (JT_EXACT_MATH=1, the default) — transcendentals evaluated in double and rounded once,
// which is how Julia's Float32 kernels compute them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jt_records.h"

namespace jtd {

// ------------------------------------------------------------------------------ math (src/math.jl)
static constexpr float pif = 3.14159265358979323846f;  // Float32(pi)
static constexpr float ray_eps = 0.0001f;               // src/geometry.jl:34
static constexpr float min_roughness = 0.03f * 0.03f;   // src/scene.jl:46

struct v2 {
    float x, y;
};
struct v3 {
    float x, y, z;
};
struct v4 {
    float x, y, z, w;
};

__device__ __forceinline__ v2 V2(float x, float y) { return v2{x, y}; }
__device__ __forceinline__ v3 V3(float x, float y, float z) { return v3{x, y, z}; }
__device__ __forceinline__ v4 V4(float x, float y, float z, float w) { return v4{x, y, z, w}; }
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 operator*(v3 a, v3 b) { return V3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return V3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ v3 operator/(v3 a, float s) { return V3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ v3 operator-(v3 a) { return V3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ v4 operator+(v4 a, v4 b) { return V4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ v4 operator*(v4 a, float s) { return V4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ bool is_zero(v3 a) { return a.x == 0 && a.y == 0 && a.z == 0; }
__device__ __forceinline__ bool all_finite(v3 a) {
    return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z);
}
__device__ __forceinline__ v3 xyz(float4 a) { return V3(a.x, a.y, a.z); }
__device__ __forceinline__ v3 xyz(v4 a) { return V3(a.x, a.y, a.z); }

// dot = sum(a .* b), left fold (src/math.jl:69)
__device__ __forceinline__ float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ v3 cross(v3 a, v3 b) {  // src/math.jl:112
    return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// sqrtf(x), correctly rounded like the compiler's expansion it replaces (16 VALU instructions a
// site: a pre-scale for tiny inputs, v_sqrt_f32, both 1-ulp neighbours tested with an FMA residual,
// a post-scale, the zero/inf class), as a shorter sequence for x in [2^-95, inf): the bits of such
// an x lie in [JL_SQRT_LO, JL_SQRT_HI). Zeros, denormals, smaller normals (whose residual would
// leave the normal range), inf, NaN and negatives take __builtin_sqrtf. sqrt_fast<FORM> are the
// candidate sequences; scripts/exhaustive/sqrt_check.hip compares each of them and jl_sqrt itself
// with __builtin_sqrtf over all 2^32 bit patterns on gfx950, and only a form with no mismatch in
// the domain is used (JT_SQRT_FORM; 0: __builtin_sqrtf everywhere). All four passed; 1 is the shortest
// (profiles/item_sqrt_rcp/sqrt_check.log, EXPERIMENTS.md).
// Used by normalize, length, sample_disk and sample_triangle. The hemisphere sample and the lobe
// terms of jt_bsdf.h keep __builtin_sqrtf: with jl_sqrt in sample_hemisphere_cos the cornellbox
// kernel's counting twin spilled 10 VGPRs, not 5 (with these four sites: 2).
#ifndef JT_SQRT_FORM
#define JT_SQRT_FORM 1
#endif
constexpr unsigned JL_SQRT_LO = 0x10000000u;  // 2^-95
constexpr unsigned JL_SQRT_HI = 0x7f800000u;  // +inf
template <int FORM>
__device__ __forceinline__ float sqrt_fast(float x) {
    if constexpr (FORM == 1) {
        // v_rsq_f32 and one coupled Newton step on the root
        const float y = __builtin_amdgcn_rsqf(x);
        const float s = x * y, h = 0.5f * y;
        return __builtin_fmaf(__builtin_fmaf(-s, s, x), h, s);
    } else if constexpr (FORM == 2) {
        // v_sqrt_f32 and one FMA-residual correction, half the reciprocal root from v_rsq_f32
        const float s = __builtin_amdgcn_sqrtf(x), h = 0.5f * __builtin_amdgcn_rsqf(x);
        return __builtin_fmaf(__builtin_fmaf(-s, s, x), h, s);
    } else if constexpr (FORM == 3) {
        // the compiler's correction without its scaling and class handling: v_sqrt_f32 is within
        // 1 ulp, so the root is it or a neighbour; the residuals' signs say which
        const float s = __builtin_amdgcn_sqrtf(x);
        const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
        const float rd = __builtin_fmaf(-dn, s, x), ru = __builtin_fmaf(-up, s, x);
        const float t = rd <= 0.0f ? dn : s;
        return ru > 0.0f ? up : t;
    } else {
        // v_rsq_f32, one Goldschmidt step on root and half reciprocal root, one residual correction
        const float y = __builtin_amdgcn_rsqf(x);
        float g = x * y, h = 0.5f * y;
        const float e = __builtin_fmaf(-h, g, 0.5f);
        h = __builtin_fmaf(h, e, h);
        g = __builtin_fmaf(g, e, g);
        return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
    }
}
__device__ __forceinline__ float jl_sqrt(float x) {
#if JT_SQRT_FORM
    if (__builtin_expect(__float_as_uint(x) - JL_SQRT_LO < JL_SQRT_HI - JL_SQRT_LO, 1)) return sqrt_fast<JT_SQRT_FORM>(x);
#endif
    return __builtin_sqrtf(x);
}
// jl_sqrt without the domain test, for a caller that proves its x in [2^-95, inf) itself
__device__ __forceinline__ float sqrt_in_domain(float x) {
#if JT_SQRT_FORM
    return sqrt_fast<JT_SQRT_FORM>(x);
#else
    return __builtin_sqrtf(x);
#endif
}
__device__ __forceinline__ v3 normalize(v3 a) {  // src/math.jl:71-78
    float l = jl_sqrt(dot(a, a));
    return l != 0 ? a / l : a;
}
__device__ __forceinline__ float length(v3 a) { return jl_sqrt(dot(a, a)); }

// Julia min/max for floats (base/math.jl): NaN-propagating, -0 < +0 — IEEE 754-2019
// minimum/maximum, which gfx950 has as v_minimum3_f32 / v_maximum3_f32 (JT_NAN_PROP, one
// instruction; the compare-and-select form otherwise). A NaN result may carry another payload than
// Julia's (x's or y's): no decision and no stored value depends on a NaN's payload.
#ifndef JT_NAN_PROP
#if defined(__gfx950__)
#define JT_NAN_PROP 1
#else
#define JT_NAN_PROP 0  // other targets (ARCH=gfx942) and the host pass: compare and select
#endif
#endif
__device__ __forceinline__ float jl_min3(float a, float b, float c) {
    float r;
    asm("v_minimum3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float jl_max3(float a, float b, float c) {
    float r;
    asm("v_maximum3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float jl_min(float x, float y) {
    if (JT_NAN_PROP) return jl_min3(x, y, y);
    bool c = (y < x) || (__builtin_signbit(y) && !__builtin_signbit(x));
    return c ? (__builtin_isnan(x) ? x : y) : (__builtin_isnan(y) ? y : x);
}
__device__ __forceinline__ float jl_max(float x, float y) {
    if (JT_NAN_PROP) return jl_max3(x, y, y);
    bool c = (y > x) || (!__builtin_signbit(y) && __builtin_signbit(x));
    return c ? (__builtin_isnan(x) ? x : y) : (__builtin_isnan(y) ? y : x);
}
__device__ __forceinline__ float jl_clamp(float x, float lo, float hi) { return x > hi ? hi : (x < lo ? lo : x); }
// 1.0f / x, correctly rounded like the IEEE division it replaces: v_rcp_f32 plus one FMA Newton
// step equals it for every x with a normal exponent below 2^126 (so the reciprocal is normal
// too) — verified over all 2^32 inputs by scripts/exhaustive/rcp_check.hip on gfx950. Zeros,
// denormals, |x| >= 2^126, inf and NaN take the division.
__device__ __forceinline__ float jl_rcp(float x) {
    const unsigned e = (__float_as_uint(x) >> 23) & 0xffu;
    if (__builtin_expect(e - 1u < 252u, 1)) {
        const float r = __builtin_amdgcn_rcpf(x);
        return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
    }
    return 1.0f / x;
}
// JT_RCP_WEIGHTS: the running-mean weights 1 / (c + 1) (Aov::w, stream_weight) and the Russian
// roulette's 1 / rr_prob through jl_rcp instead of the division's full sequence; the same bits
#ifndef JT_RCP_WEIGHTS
#define JT_RCP_WEIGHTS 1
#endif
__device__ __forceinline__ float jl_rcp_weight(float x) { return JT_RCP_WEIGHTS ? jl_rcp(x) : 1.0f / x; }
__device__ __forceinline__ int jl_clampi(int x, int lo, int hi) { return x > hi ? hi : (x < lo ? lo : x); }
__device__ __forceinline__ float max3(v3 a) { return JT_NAN_PROP ? jl_max3(a.x, a.y, a.z) : jl_max(jl_max(a.x, a.y), a.z); }

#if JT_EXACT_MATH
// Double-evaluated, once-rounded transcendentals (the float contract). The hot-path arguments
// of sin/cos (2*pi*u, atan(...), v*pi, u*2*pi) lie in [0, 2*pi]; for |x| < 2^19 a Cody-Waite
// reduction by pi/2 with a 33-bit leading constant is exact in double and the fdlibm kernels
// give < 1 ulp in double, so rounding to float reproduces the correctly rounded float except
// within ~2^-52 of a rounding midpoint. Larger arguments fall back to ocml's double sincos.
__device__ __forceinline__ void dsincos_small(double x, double& s, double& c) {
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11;
    const double n = __builtin_rint(x * invpio2);
    const double r = (x - n * pio2_1) - n * pio2_1t;
    const double z = r * r;
    // __kernel_sin / __kernel_cos (fdlibm k_sin.c / k_cos.c), tail y = 0
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double sr = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = r + (z * r) * (S1 + z * sr);
    const double cr = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double kc = w + (((1.0 - w) - hz) + z * cr);
    const int q = (int)n & 3;
    s = q == 0 ? ks : (q == 1 ? kc : (q == 2 ? -ks : -kc));
    c = q == 0 ? kc : (q == 1 ? -ks : (q == 2 ? -kc : ks));
}
__device__ __noinline__ void dsincos_large(double x, double* s, double* c) { sincos(x, s, c); }
__device__ __forceinline__ void jl_sincos(float x, float* s, float* c) {
    double sd, cd;
    if (__builtin_fabsf(x) < 524288.0f) {
        dsincos_small((double)x, sd, cd);
    } else {
        dsincos_large((double)x, &sd, &cd);
    }
    *s = (float)sd;
    *c = (float)cd;
}
__device__ __forceinline__ float jl_sin(float x) {
    float s, c;
    jl_sincos(x, &s, &c);
    return s;
}
__device__ __forceinline__ float jl_cos(float x) {
    float s, c;
    jl_sincos(x, &s, &c);
    return c;
}
// jl_sincos(2 * pif * u) for u = k * 2^-24, k = 0 .. 2^24 - 1 (every rand1f value), the same floats
// in half the FP64 instructions, with no large-argument call and no branch: dsincos_small's
// reduction and kernels with every multiply-add fused. The fused doubles differ from the unfused
// ones in their last bits only, and no phi of the set lies within 4 double-ulps of a float rounding
// midpoint (tests/test_primitives_host.py), so both round to the same float: "evaluated in double,
// rounded once" (DESIGN.md §3). The quadrant rint(phi * invpio2) is (k + 2^21) >> 22 for every k;
// the swap and the negation act on the rounded floats (round to nearest is sign-symmetric), as
// 32-bit selects and XORs. tests/sincos_unit_check.cpp enumerates all 2^24 k on the host, and
// tests/test_gpu_sincos_unit.py on the device. Only for such u: any other argument takes jl_sincos.
// JT_SINCOS_UNIT: 0 no caller (A/B runs), 1 the baked matte sample (sample_matte_baked, jt_bsdf.h),
// 2 the baking kernels' camera sample too (sample_disk_unit).
#ifndef JT_SINCOS_UNIT
#define JT_SINCOS_UNIT 2
#endif
// A constant of sincos_unit in a scalar register pair, made where it is used. Left to the compiler, the
// fourteen doubles of the straight-line form are hoisted out of the sample loop into vector registers
// (the headline kernel: 20 spilled VGPRs, reloaded every bounce); jl_sincos's are scalar moves
// inside its branch.
__device__ __forceinline__ double scalar_const(double c) {
    __asm__ volatile("" : "+s"(c));
    return c;
}
__device__ __forceinline__ void sincos_unit(float u, float* s, float* c) {
#define JT_K(x) scalar_const(x)  // each where it is used: the barriers keep their order, so two or three pairs live at a time
    const unsigned k = (unsigned)(u * 16777216.0f);
    const unsigned nq = (k + (1u << 21)) >> 22;  // 0 .. 4
    const double x = (double)(2 * pif * u), n = (double)nq;
    double r = __builtin_fma(-n, JT_K(1.57079632673412561417e+00), x);  // pio2_1
    r = __builtin_fma(-n, JT_K(6.07710050650619224932e-11), r);         // pio2_1t
    const double z = r * r;
    double sr = __builtin_fma(z, JT_K(1.58969099521155010221e-10), JT_K(-2.50507602534068634195e-08));  // S6, S5
    sr = __builtin_fma(z, sr, JT_K(2.75573137070700676789e-06));                                         // S4
    sr = __builtin_fma(z, sr, JT_K(-1.98412698298579493134e-04));                                        // S3
    sr = __builtin_fma(z, sr, JT_K(8.33333333332248946124e-03));                                         // S2
    const double ks = __builtin_fma(z * r, __builtin_fma(z, sr, JT_K(-1.66666666666666324348e-01)), r);  // S1
    double cr = __builtin_fma(z, JT_K(-1.13596475577881948265e-11), JT_K(2.08757232129817482790e-09));  // C6, C5
    cr = __builtin_fma(z, cr, JT_K(-2.75573143513906633035e-07));                                        // C4
    cr = __builtin_fma(z, cr, JT_K(2.48015872894767294178e-05));                                         // C3
    cr = __builtin_fma(z, cr, JT_K(-1.38888888888741095749e-03));                                        // C2
    cr = z * __builtin_fma(z, cr, JT_K(4.16666666666666019037e-02));                                     // C1
    const double kc = __builtin_fma(z, cr, __builtin_fma(-0.5, z, 1.0));
#undef JT_K
    const float sf = (float)ks, cf = (float)kc;
    const bool odd = (nq & 1u) != 0;
    *s = __uint_as_float(__float_as_uint(odd ? cf : sf) ^ ((nq & 2u) << 30));
    *c = __uint_as_float(__float_as_uint(odd ? sf : cf) ^ (((nq + 1u) & 2u) << 30));
}
// atan in double (fdlibm s_atan.c), used by sample_microfacet on every rough specular sample
__device__ __forceinline__ float jl_atan(float xf) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
                              1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
                              6.12323399573676603587e-17};
    const double a0 = 3.33333333333329318027e-01, a1 = -1.99999999998764832476e-01, a2 = 1.42857142725034663711e-01,
                 a3 = -1.11111104054623557880e-01, a4 = 9.09088713343650656196e-02, a5 = -7.69187620504482999495e-02,
                 a6 = 6.66107313738753120669e-02, a7 = -5.83357013379057348645e-02, a8 = 4.97687799461593236017e-02,
                 a9 = -3.65315727442169155270e-02, a10 = 1.62858201153657823623e-02;
    if (__builtin_isnan(xf)) return xf;
    const double x0 = (double)xf;
    double x = __builtin_fabs(x0);
    int id;
    if (x < 0.4375) {
        if (x < 1.0e-29) return xf;
        id = -1;
    } else if (x < 1.1875) {
        if (x < 0.6875) {
            id = 0;
            x = (2.0 * x - 1.0) / (2.0 + x);
        } else {
            id = 1;
            x = (x - 1.0) / (x + 1.0);
        }
    } else if (x < 2.4375) {
        id = 2;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else if (x < 1.0e17) {
        id = 3;
        x = -1.0 / x;
    } else {
        return (float)__builtin_copysign(atanhi[3] + atanlo[3], x0);
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
    const double s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
    double r;
    if (id < 0) r = x - x * (s1 + s2);
    else r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return (float)__builtin_copysign(r, x0);
}
// rare-path transcendentals (environment, volumes): ocml double, kept out of line
__device__ __noinline__ float jl_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __noinline__ float jl_acos(float x) { return (float)acos((double)x); }
__device__ __noinline__ float jl_log(float x) { return (float)log((double)x); }
__device__ __noinline__ float jl_exp(float x) { return (float)exp((double)x); }
#else
__device__ __forceinline__ float jl_sin(float x) { return sinf(x); }
__device__ __forceinline__ float jl_cos(float x) { return cosf(x); }
__device__ __forceinline__ void jl_sincos(float x, float* s, float* c) { sincosf(x, s, c); }
#ifndef JT_SINCOS_UNIT
#define JT_SINCOS_UNIT 0
#endif
__device__ __forceinline__ void sincos_unit(float u, float* s, float* c) { sincosf(2 * pif * u, s, c); }
__device__ __forceinline__ float jl_atan(float x) { return atanf(x); }
__device__ __forceinline__ float jl_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ float jl_acos(float x) { return acosf(x); }
__device__ __forceinline__ float jl_log(float x) { return logf(x); }
__device__ __forceinline__ float jl_exp(float x) { return expf(x); }
#endif

// Frame3f columns x, y, z, o packed in 12 floats
struct fr3 {
    v3 x, y, z, o;
};
__device__ __forceinline__ fr3 frame_from(const float* a) {
    return fr3{V3(a[0], a[1], a[2]), V3(a[3], a[4], a[5]), V3(a[6], a[7], a[8]), V3(a[9], a[10], a[11])};
}
__device__ __forceinline__ fr3 frame_from(float4 a, float4 b, float4 c) {
    return fr3{V3(a.x, a.y, a.z), V3(a.w, b.x, b.y), V3(b.z, b.w, c.x), V3(c.y, c.z, c.w)};
}
// transform_point / transform_vector / transform_direction / transform_normal (src/math.jl:80-129)
__device__ __forceinline__ v3 transform_point(const fr3& f, v3 p) { return ((f.x * p.x + f.y * p.y) + f.z * p.z) + f.o; }
__device__ __forceinline__ v3 transform_vector(const fr3& f, v3 b) { return (f.x * b.x + f.y * b.y) + f.z * b.z; }
__device__ __forceinline__ v3 transform_direction(const fr3& f, v3 b) { return normalize(transform_vector(f, b)); }
__device__ __forceinline__ v3 transform_normal(const fr3& f, v3 b) { return normalize(transform_vector(f, b)); }
// Mat3f (3 columns) * Vec3f (src/math.jl:105)
struct m3 {
    v3 c1, c2, c3;
};
__device__ __forceinline__ v3 mul(const m3& m, v3 f) { return (m.c1 * f.x + m.c2 * f.y) + m.c3 * f.z; }
// reflect / refract (src/math.jl:131-142)
__device__ __forceinline__ v3 reflect(v3 w, v3 n) { return -w + n * (2 * dot(n, w)); }
__device__ __forceinline__ v3 refract(v3 w, v3 n, float inv_eta) {
    float cosine = dot(n, w);
    float k = 1 + inv_eta * inv_eta * (cosine * cosine - 1);
    if (k < 0) return V3(0, 0, 0);
    return (-w) * inv_eta + n * (inv_eta * cosine - __builtin_sqrtf(k));
}

// ------------------------------------------------------------------------------ RNG (build)
// PCG32 stream keyed by (seed, pixel, global sample); rand1f = 24-bit float in [0,1) like
// Julia's rand(Float32). Stated in DESIGN.md §RNG and restated by oracle/jt_oracle.c.
struct Rng {
    unsigned long long state, inc;
};
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ Rng rng_init(unsigned long long seed, int pixel, int sample) {
    unsigned long long key = mix64(seed ^ mix64(((unsigned long long)(unsigned)pixel << 32) |
                                                 (unsigned long long)(unsigned)sample));
    Rng r;
    r.inc = (mix64(key ^ 0xda3e39cb94b95bdbULL) << 1) | 1ULL;
    r.state = (r.inc + key) * 6364136223846793005ULL + r.inc;
    return r;
}
__device__ __forceinline__ unsigned rng_next(Rng& r) {
    unsigned long long old = r.state;
    r.state = old * 6364136223846793005ULL + r.inc;
    unsigned xs = (unsigned)(((old >> 18) ^ old) >> 27);
    unsigned rot = (unsigned)(old >> 59);
    return (xs >> rot) | (xs << ((32u - rot) & 31u));
}
__device__ __forceinline__ float rand1f(Rng& r) { return (float)(rng_next(r) >> 8) * 0x1.0p-24f; }
__device__ __forceinline__ v2 rand2f(Rng& r) {
    float a = rand1f(r);
    float b = rand1f(r);
    return V2(a, b);
}

// ------------------------------------------------------------------------------ sampling.jl
__device__ __forceinline__ v2 sample_disk(v2 ruv) {  // src/sampling.jl:12-16
    float r = jl_sqrt(ruv.y);
    float phi = 2 * pif * ruv.x;
    float s, c;
    jl_sincos(phi, &s, &c);
    return V2(c * r, s * r);
}
// sample_disk for a ruv.x of rand1f's set (the baking kernels' camera sample): the same floats
__device__ __forceinline__ v2 sample_disk_unit(v2 ruv) {
    float r = jl_sqrt(ruv.y);
    float s, c;
    sincos_unit(ruv.x, &s, &c);
    return V2(c * r, s * r);
}
// With aperture == +0, eval_camera reads sample_disk's result only through lens_uv * 0, i.e.
// through the signs of c * r and s * r (r >= +0): those of cos(phi) and sin(phi). The float phi
// is compared in double against the doubles nearest pi/2, pi, 3pi/2, 2pi; no float lies
// between any of them and the true value, and cos/sin of a float are never zero except
// sin(+0), so the signs are exactly those of the rounded jl_sincos results.
__device__ __forceinline__ v2 sample_disk_signs(v2 ruv) {
    const double phi = (double)(2 * pif * ruv.x);
    const bool cneg = phi > 1.5707963267948966 && phi < 4.7123889803846897;
    const bool sneg = phi > 3.1415926535897931 && phi < 6.2831853071795862;
    return V2(cneg ? -0.0f : 0.0f, sneg ? -0.0f : 0.0f);
}
__device__ __forceinline__ float sample_hemisphere_cos_pdf(v3 normal, v3 direction) {  // :24-27
    float cosw = dot(normal, direction);
    return cosw <= 0 ? 0 : cosw / pif;
}
__device__ __forceinline__ int sample_uniform(int size, float r) {  // :29, 1-based
    return jl_clampi((int)__builtin_truncf(r * (float)size) + 1, 1, size);
}
__device__ __forceinline__ float sample_uniform_pdf(int size) { return (float)(1.0 / (double)size); }  // :31
__device__ __forceinline__ int upper_bound(const float* cdf, int n, float limit) {  // :42-56, 1-based
    int idx = 0, l = 1, r = n;
    while (l <= r) {
        int m = (l + r) / 2;
        if (cdf[m - 1] > limit) {
            idx = m;
            r = m - 1;
        } else {
            l = m + 1;
        }
    }
    return idx;
}
__device__ __forceinline__ int sample_discrete(const float* cdf, int n, float r) {  // :33-37, 1-based
    float last = cdf[n - 1];
    r = jl_clamp(r * last, 0.0f, last - 0.00001f);
    return jl_clampi(upper_bound(cdf, n, r), 1, n);
}
// upper_bound through a guide table: the same first index (cdf is nondecreasing, so the answer
// for a limit in [t_k, t_k+1) lies in [a_k, a_k+1]); a few loads instead of log2(n) dependent ones
__device__ __forceinline__ int upper_bound_guided(const float* cdf, int n, float limit, const float* gt, const int* ga,
                                                  int K, float scale) {
    int k = (int)(limit * scale);
    k = k < 0 ? 0 : (k > K - 1 ? K - 1 : k);
    while (k > 0 && limit < gt[k]) k--;
    while (k < K - 1 && limit >= gt[k + 1]) k++;
    int lo = ga[k], hi = ga[k + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > limit) hi = mid;
        else lo = mid + 1;
    }
    return lo >= n ? 0 : lo + 1;
}
__device__ __forceinline__ int sample_discrete_guided(const float* cdf, int n, float r, const float* gt, const int* ga,
                                                      int K, float scale) {
    float last = cdf[n - 1];
    r = jl_clamp(r * last, 0.0f, last - 0.00001f);
    return jl_clampi(upper_bound_guided(cdf, n, r, gt, ga, K, scale), 1, n);
}
__device__ __forceinline__ float sample_discrete_pdf(const float* cdf, int idx1) {  // :39-40
    return idx1 == 1 ? cdf[0] : cdf[idx1 - 1] - cdf[idx1 - 2];
}
__device__ __forceinline__ v2 sample_triangle(v2 ruv) {  // :58
    const float r = jl_sqrt(ruv.x);
    return V2(1 - r, ruv.y * r);
}

// ------------------------------------------------------------------------------ geometry.jl
// Raw VALU min/max. Only for operands known not to be NaN: the compiler's fminf/fmaxf
// canonicalize both inputs first (IEEE mode), which costs an extra VALU op per operand.
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The slab test's final compare, `t1 *= 1.00000024; t0 <= t1` (src/geometry.jl:102-103): the
// Float32 t1 is promoted, so the product and the compare are Float64. (An exact float decision
// with a double fallback — checked exhaustively, scripts/exhaustive/slab_check.hip — measured
// slower on gfx950, whose wave64 FP64 multiply issues at the FP32 rate)
__device__ __forceinline__ bool slab_pass(float t0, float t1) { return (double)t0 <= (double)t1 * 1.00000024; }

// intersect_bbox (src/geometry.jl:96-105): Julia min/max; `t1 *= 1.00000024` is Float64.
// Any NaN slab value makes Julia's t0 or t1 NaN and culls the box; that case is tested
// separately, so the min/max chains below only ever see non-NaN values, where IEEE min/max
// agree with Julia's (signed zeros cannot change `t0 <= t1`) and the order of the chain does
// not matter.
// a = (bmin.x, bmax.x, bmin.y, bmax.y), b = (bmin.z, bmax.z, ..) (DNode). Scalar on purpose:
// packed-FP32 (v_pk_add/v_pk_mul_f32) forms of these products measured 1.5 % slower on gfx950
// (the broadcast ray operands then occupy register pairs).
// JT_NAN_PROP (jl_min above): with Julia's min/max as single NaN-propagating instructions a NaN
// slab value makes t0 or t1 NaN and the Float64 compare false, with no separate NaN test (three
// v_cmp_o and their mask combines per box): the same decision as the form below for every input.
// Measured against it (two runs each, interleaved, gpurun_out/r06nan2): cornellbox +1.5 %,
// bathroom1 +1.6 %, ecosys +1.0 %, features2 +1.3 %.
__device__ __forceinline__ bool intersect_bbox(v3 o, v3 dinv, float tmin, float tmax, const float4& a,
                                               const float4& b) {
    const float mx = (a.x - o.x) * dinv.x, Mx = (a.y - o.x) * dinv.x;
    const float my = (a.z - o.y) * dinv.y, My = (a.w - o.y) * dinv.y;
    const float mz = (b.x - o.z) * dinv.z, Mz = (b.y - o.z) * dinv.z;
    if (JT_NAN_PROP) {
        // t0 = max(min(mx, Mx), min(my, My), max(min(mz, Mz), tmin)), t1 likewise (the order of a
        // max chain does not change its value; a NaN anywhere makes it NaN)
        const float t0 = jl_max3(jl_min3(mx, Mx, Mx), jl_min3(my, My, My), jl_max3(jl_min3(mz, Mz, Mz), tmin, tmin));
        const float t1 = jl_min3(jl_max3(mx, Mx, Mx), jl_max3(my, My, My), jl_min3(jl_max3(mz, Mz, Mz), tmax, tmax));
        return slab_pass(t0, t1);
    }
    bool nan = __builtin_isnan(mx) | __builtin_isnan(my) | __builtin_isnan(mz) | __builtin_isnan(Mx) |
               __builtin_isnan(My) | __builtin_isnan(Mz);
    float t0 = vmax3(vmin(mx, Mx), vmin(my, My), vmax(vmin(mz, Mz), tmin));
    float t1 = vmin3(vmax(mx, Mx), vmax(my, My), vmin(vmax(mz, Mz), tmax));
    return !nan && slab_pass(t0, t1);
}

struct PrimHit {
    float u, v, t;
    bool hit;
};
// intersect_triangle (src/geometry.jl:206-236), branchless: every quantity is computed and the
// reference's early-out tests are combined into one predicate (the same comparisons, so NaN
// behaves as in the reference: a NaN u, v or t fails none of them). A miss is (0, 0, inf).
__device__ __forceinline__ PrimHit intersect_triangle_e(v3 o, v3 d, float tmin, float tmax, v3 p1, v3 edge1, v3 edge2) {
    v3 pvec = cross(d, edge2);
    float det = dot(edge1, pvec);
    float inv_det = jl_rcp(det);
    v3 tvec = o - p1;
    float u = dot(tvec, pvec) * inv_det;
    v3 qvec = cross(tvec, edge1);
    float v = dot(d, qvec) * inv_det;
    float t = dot(edge2, qvec) * inv_det;
    const bool miss = (det == 0) | (u < 0 || u > 1) | (v < 0 || u + v > 1) | (t < tmin || t > tmax);
    PrimHit r;
    r.u = miss ? 0.0f : u;
    r.v = miss ? 0.0f : v;
    r.t = miss ? __builtin_inff() : t;
    r.hit = !miss;
    return r;
}
// The triangle test without its `t > tmax` rejection (the only use of tmax): hit = every other
// test passed. tri_hit_before(p, tmax) completes it, so two consecutive primitives can be
// computed side by side and then accepted in order, each against the tmax the previous one left.
__device__ __forceinline__ PrimHit intersect_triangle_pre(v3 o, v3 d, float tmin, v3 p1, v3 edge1, v3 edge2) {
    v3 pvec = cross(d, edge2);
    float det = dot(edge1, pvec);
    float inv_det = jl_rcp(det);
    v3 tvec = o - p1;
    float u = dot(tvec, pvec) * inv_det;
    v3 qvec = cross(tvec, edge1);
    float v = dot(d, qvec) * inv_det;
    float t = dot(edge2, qvec) * inv_det;
    PrimHit r;
    r.u = u;
    r.v = v;
    r.t = t;
    r.hit = !((det == 0) | (u < 0 || u > 1) | (v < 0 || u + v > 1) | (t < tmin));
    return r;
}
__device__ __forceinline__ bool tri_hit_before(const PrimHit& p, float tmax) { return p.hit && !(p.t > tmax); }
// triangle records carry the edges p2 - p1, p3 - p1, precomputed on the host (the same floats)
__device__ __forceinline__ PrimHit intersect_triangle(v3 o, v3 d, float tmin, float tmax, v3 p1, v3 p2, v3 p3) {
    return intersect_triangle_e(o, d, tmin, tmax, p1, p2 - p1, p3 - p1);
}
// intersect_quad (src/geometry.jl:238-258); `degenerate` = (p3 == p4), precomputed on the host
__device__ __forceinline__ PrimHit intersect_quad(v3 o, v3 d, float tmin, float tmax, v3 p1, v3 p2, v3 p3, v3 p4,
                                                  bool degenerate) {
    PrimHit i1 = intersect_triangle(o, d, tmin, tmax, p1, p2, p4);
    PrimHit i2 = intersect_triangle(o, d, tmin, tmax, p3, p4, p2);
    if (i2.hit) {
        i2.u = 1 - i2.u;
        i2.v = 1 - i2.v;
    }
    const bool first = degenerate || i1.t < i2.t;
    PrimHit r;
    r.u = first ? i1.u : i2.u;
    r.v = first ? i1.v : i2.v;
    r.t = first ? i1.t : i2.t;
    r.hit = first ? i1.hit : i2.hit;
    return r;
}
__device__ __forceinline__ v3 triangle_normal(v3 p1, v3 p2, v3 p3) { return normalize(cross(p2 - p1, p3 - p1)); }
__device__ __forceinline__ v3 quad_normal(v3 p1, v3 p2, v3 p3, v3 p4) {
    return normalize(triangle_normal(p1, p2, p4) + triangle_normal(p3, p4, p2));
}
// interpolate_triangle / interpolate_quad (src/geometry.jl:275-283)
__device__ __forceinline__ v3 interp_tri(v3 p1, v3 p2, v3 p3, v2 uv) {
    float w = (1 - uv.x) - uv.y;
    return (p1 * w + p2 * uv.x) + p3 * uv.y;
}
__device__ __forceinline__ v2 interp_tri(v2 p1, v2 p2, v2 p3, v2 uv) {
    float w = (1 - uv.x) - uv.y;
    return V2((p1.x * w + p2.x * uv.x) + p3.x * uv.y, (p1.y * w + p2.y * uv.x) + p3.y * uv.y);
}
__device__ __forceinline__ v4 interp_tri(v4 p1, v4 p2, v4 p3, v2 uv) {
    float w = (1 - uv.x) - uv.y;
    return (p1 * w + p2 * uv.x) + p3 * uv.y;
}
template <class T>
__device__ __forceinline__ T interp_quad(T p1, T p2, T p3, T p4, v2 uv) {
    if (uv.x + uv.y <= 1) return interp_tri(p1, p2, p4, uv);
    return interp_tri(p3, p4, p2, V2(1 - uv.x, 1 - uv.y));
}
// triangle_tangents_fromuv (src/geometry.jl:285-316)
__device__ __forceinline__ void triangle_tangents_fromuv(v3 p1, v3 p2, v3 p3, v2 uv1, v2 uv2, v2 uv3, v3& tu, v3& tv) {
    v3 p = p2 - p1, q = p3 - p1;
    v2 s = V2(uv2.x - uv1.x, uv3.x - uv1.x);
    v2 t = V2(uv2.y - uv1.y, uv3.y - uv1.y);
    float div = s.x * t.y - s.y * t.x;
    if (div != 0) {
        tu = V3(t.y * p.x - t.x * q.x, t.y * p.y - t.x * q.y, t.y * p.z - t.x * q.z) / div;
        tv = V3(s.x * q.x - s.y * p.x, s.x * q.y - s.y * p.y, s.x * q.z - s.y * p.z) / div;
    } else {
        tu = V3(1, 0, 0);
        tv = V3(0, 1, 0);
    }
}

}  // namespace jtd
