// sincos_unit_check.cpp — the baked matte sample's azimuth and square roots (csrc/jt_device.h
// sincos_unit, csrc/jt_bsdf.h sample_matte_baked) over their whole input set, on the host.
// tests/test_sincos_unit.py builds it with the host compiler (-ffp-contract=off, so every fused
// operation below is an explicit fma()) under -fsanitize=address,undefined and runs it once. No
// Python, no HIP runtime, no GPU. Every comparison is of bits.
//
// The set: u = k * 2^-24, k = 0 .. 2^24 - 1, every value rand1f returns. For each k:
//   (a) sincos_unit's doubles — the Cody-Waite reduction and the fdlibm kernels of dsincos_small with
//       every multiply-add fused, the quadrant from k, the swap and the sign applied to the rounded
//       floats — round to the floats jl_sincos's unfused doubles round to, sine and cosine;
//   (b) the quadrant identity: rint(phi * invpio2) == (k + 2^21) >> 22, and (unsigned)(u * 2^24) == k;
//   (c) with z = sqrtf(u), 1 - z * z lies in [2^-23, 1]: inside sqrt_fast's proven domain
//       [2^-95, inf) with no test at all;
//   (d) u is 0 or at least 2^-24: the first root needs only the zero handled.
// Prints "sincos_unit_check: <n> inputs, <bad> bad"; the test requires 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {

const float pif = 3.14159265358979323846f;  // Float32(pi), csrc/jt_device.h
const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
             pio2_1t = 6.07710050650619224932e-11;
const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
             S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
             C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// jl_sincos's small-argument path (dsincos_small), no fused operation
void sincos_unfused(float xf, float* s, float* c, double* n_out) {
    const double x = (double)xf;
    const double n = std::rint(x * invpio2);
    const double r = (x - n * pio2_1) - n * pio2_1t;
    const double z = r * r;
    const double sr = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = r + (z * r) * (S1 + z * sr);
    const double cr = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double kc = w + (((1.0 - w) - hz) + z * cr);
    const int q = (int)n & 3;
    *s = (float)(q == 0 ? ks : (q == 1 ? kc : (q == 2 ? -ks : -kc)));
    *c = (float)(q == 0 ? kc : (q == 1 ? -ks : (q == 2 ? -kc : ks)));
    *n_out = n;
}

// sincos_unit (csrc/jt_device.h), line for line with fma() for __builtin_fma
void sincos_unit(float u, float* s, float* c, unsigned* nq_out, unsigned* k_out) {
    const unsigned k = (unsigned)(u * 16777216.0f);
    const unsigned nq = (k + (1u << 21)) >> 22;
    const double x = (double)(2 * pif * u), n = (double)nq;
    const double r = std::fma(-n, pio2_1t, std::fma(-n, pio2_1, x));
    const double z = r * r;
    const double sr = std::fma(z, std::fma(z, std::fma(z, std::fma(z, S6, S5), S4), S3), S2);
    const double ks = std::fma(z * r, std::fma(z, sr, S1), r);
    const double cr = z * std::fma(z, std::fma(z, std::fma(z, std::fma(z, std::fma(z, C6, C5), C4), C3), C2), C1);
    const double kc = std::fma(z, cr, std::fma(-0.5, z, 1.0));
    const float sf = (float)ks, cf = (float)kc;
    float s0 = (nq & 1u) ? cf : sf, c0 = (nq & 1u) ? sf : cf;
    uint32_t sb = bits(s0) ^ ((nq & 2u) << 30), cb = bits(c0) ^ (((nq + 1u) & 2u) << 30);
    std::memcpy(s, &sb, 4);
    std::memcpy(c, &cb, 4);
    *nq_out = nq;
    *k_out = k;
}

}  // namespace

int main() {
    long bad = 0, bad_sin = 0, bad_cos = 0, bad_quadrant = 0, bad_range = 0, bad_input = 0;
    float lo = 2.0f, hi = -1.0f;
    const uint32_t N = 1u << 24;
    for (uint32_t k = 0; k < N; k++) {
        const float u = (float)k * 0x1.0p-24f;  // rand1f
        const float phi = 2 * pif * u;
        float s0, c0, s1, c1;
        double n;
        unsigned nq, kk;
        sincos_unfused(phi, &s0, &c0, &n);
        sincos_unit(u, &s1, &c1, &nq, &kk);
        const bool es = bits(s0) != bits(s1), ec = bits(c0) != bits(c1);
        const bool eq = n != (double)nq || kk != k;
        bad_sin += es, bad_cos += ec, bad_quadrant += eq;
        const float z = std::sqrt(u), t = 1 - z * z;
        const bool er = !(t >= 0x1.0p-23f && t <= 1.0f);
        const bool ei = !(u == 0.0f || (u >= 0x1.0p-24f && u < 1.0f));
        bad_range += er, bad_input += ei;
        lo = t < lo ? t : lo, hi = t > hi ? t : hi;
        if ((es || ec || eq || er || ei) && bad++ < 10)
            std::fprintf(stderr, "sincos_unit_check: k = %u: sin %a / %a, cos %a / %a, n %g / %u, 1 - z z = %a\n", k, s0, s1,
                         c0, c1, n, nq, t);
    }
    std::printf("sincos_unit_check: sine %ld, cosine %ld, quadrant %ld, root range %ld, input %ld; 1 - z z in [%a, %a]\n",
                bad_sin, bad_cos, bad_quadrant, bad_range, bad_input, lo, hi);
    std::printf("sincos_unit_check: %u inputs, %ld bad\n", N, bad_sin + bad_cos + bad_quadrant + bad_range + bad_input);
    return bad_sin + bad_cos + bad_quadrant + bad_range + bad_input ? 1 : 0;
}
