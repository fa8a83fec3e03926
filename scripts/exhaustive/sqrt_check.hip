// Exhaustive check over all 2^32 float bit patterns that jl_sqrt (julia-raytracer_amd/csrc/
// jt_device.h: a short sequence for x in [2^-95, inf), __builtin_sqrtf elsewhere) equals the
// compiler's correctly rounded __builtin_sqrtf, bit for bit (NaNs compare equal). Also reports each
// candidate sequence sqrt_fast<1..4> on its own: its mismatches inside jl_sqrt's domain (a form with
// even one is not used) and the biased exponents (bits >> 23) at which it mismatches anywhere,
// which are the inputs jl_sqrt must route to __builtin_sqrtf.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I../../julia-raytracer_amd/csrc -o sqrt_check sqrt_check.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "jt_device.h"

constexpr int NFORM = 4;
// bad[0]: jl_sqrt; bad[f]: sqrt_fast<f> inside the domain; hist[f * 512 + e]: sqrt_fast<f> at
// exponent word e = bits >> 23 (sign included), anywhere
struct Result {
    unsigned long long bad[NFORM + 1];
    unsigned long long hist[(NFORM + 1) * 512];
    unsigned first[(NFORM + 1) * 8];
};

__device__ __forceinline__ bool same(float a, float b) {
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}
template <int FORM>
__device__ __forceinline__ void check_form(unsigned bits, float x, float ref, bool in_domain, Result* r) {
    if (same(jtd::sqrt_fast<FORM>(x), ref)) return;
    atomicAdd(&r->hist[FORM * 512 + (bits >> 23)], 1ull);
    if (!in_domain) return;
    const unsigned long long n = atomicAdd(&r->bad[FORM], 1ull);
    if (n < 8) r->first[FORM * 8 + n] = bits;
}
__global__ void check(unsigned long long base, Result* r) {
    const unsigned bits = (unsigned)(base + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x);
    const float x = __uint_as_float(bits);
    const float ref = __builtin_sqrtf(x);
    const bool in_domain = bits - jtd::JL_SQRT_LO < jtd::JL_SQRT_HI - jtd::JL_SQRT_LO;
    if (!same(jtd::jl_sqrt(x), ref)) {
        const unsigned long long n = atomicAdd(&r->bad[0], 1ull);
        if (n < 8) r->first[n] = bits;
    }
    check_form<1>(bits, x, ref, in_domain, r);
    check_form<2>(bits, x, ref, in_domain, r);
    check_form<3>(bits, x, ref, in_domain, r);
    check_form<4>(bits, x, ref, in_domain, r);
}
int main() {
    Result* d;
    static Result h;
    if (hipMalloc(&d, sizeof(Result)) != hipSuccess) return 2;
    (void)hipMemset(d, 0, sizeof(Result));
    const unsigned long long chunk = 1ull << 28;
    for (unsigned long long b = 0; b < (1ull << 32); b += chunk)
        hipLaunchKernelGGL(check, dim3(chunk / 256), dim3(256), 0, 0, b, d);
    if (hipMemcpy(&h, d, sizeof(Result), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("jl_sqrt (JT_SQRT_FORM=%d, domain bits [%08x, %08x)) mismatches over 2^32 inputs: %llu\n", JT_SQRT_FORM,
           jtd::JL_SQRT_LO, jtd::JL_SQRT_HI, h.bad[0]);
    for (int k = 0; k < 8 && k < (int)h.bad[0]; k++) printf("  jl_sqrt bad x=%08x\n", h.first[k]);
    for (int f = 1; f <= NFORM; f++) {
        unsigned long long all = 0;
        for (int e = 0; e < 512; e++) all += h.hist[f * 512 + e];
        printf("sqrt_fast<%d>: %llu mismatches in the domain, %llu over all inputs\n", f, h.bad[f], all);
        for (int k = 0; k < 8 && k < (int)h.bad[f]; k++) printf("  in-domain bad x=%08x\n", h.first[f * 8 + k]);
        // runs of exponent words with a mismatch
        for (int e = 0; e < 512;) {
            if (!h.hist[f * 512 + e]) {
                e++;
                continue;
            }
            int e1 = e;
            unsigned long long n = 0;
            while (e1 < 512 && h.hist[f * 512 + e1]) n += h.hist[f * 512 + e1++];
            printf("  exponent words %d..%d: %llu\n", e, e1 - 1, n);
            e = e1;
        }
    }
    return h.bad[0] == 0 ? 0 : 1;
}
