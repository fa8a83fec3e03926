// TEST INFRASTRUCTURE ONLY — jl_sqrt (csrc/jt_device.h) against the compiler's __builtin_sqrtf, bit
// for bit, on the device. A stand-alone program (its own main), compiled by tests/test_gpu_sqrt.py's
// fixture with the product's flags; not part of any library.
//
//   jt_sqrt_probe <first> <stride> <count> <in.bin> <out.bin>
//
// 1. the bit patterns first + k * stride (k < count, modulo 2^32) are compared on the device; the
//    number of mismatches and the first few patterns are printed ("sweep: ...");
// 2. in.bin holds uint32 bit patterns; out.bin receives, for each, jl_sqrt's bits and then
//    __builtin_sqrtf's bits (two uint32 per input), for the test to compare and to hold against the
//    host's correctly rounded square root.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jt_device.h"

namespace {

constexpr int NFIRST = 16;
struct Sweep {
    unsigned long long bad;
    unsigned first[NFIRST];
};

__device__ __forceinline__ bool same(float a, float b) {
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}
__global__ void sweep_kernel(unsigned first, unsigned stride, unsigned count, Sweep* out) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const unsigned bits = first + k * stride;
    const float x = __uint_as_float(bits);
    if (!same(jtd::jl_sqrt(x), __builtin_sqrtf(x))) {
        const unsigned long long n = atomicAdd(&out->bad, 1ull);
        if (n < NFIRST) out->first[n] = bits;
    }
}
__global__ void list_kernel(const unsigned* in, unsigned n, unsigned* out) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float x = __uint_as_float(in[k]);
    out[2 * k] = __float_as_uint(jtd::jl_sqrt(x));
    out[2 * k + 1] = __float_as_uint(__builtin_sqrtf(x));
}

bool ok(hipError_t e, const char* what) {
    if (e != hipSuccess) std::fprintf(stderr, "jt_sqrt_probe: %s: %s\n", what, hipGetErrorString(e));
    return e == hipSuccess;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: jt_sqrt_probe <first> <stride> <count> <in.bin> <out.bin>\n");
        return 2;
    }
    const unsigned first = (unsigned)std::strtoul(argv[1], nullptr, 0), stride = (unsigned)std::strtoul(argv[2], nullptr, 0);
    const unsigned count = (unsigned)std::strtoul(argv[3], nullptr, 0);
    if (count == 0 || count > (1u << 28)) return 2;

    Sweep* ds = nullptr;
    Sweep hs{};
    if (!ok(hipMalloc(&ds, sizeof(Sweep)), "hipMalloc") || !ok(hipMemset(ds, 0, sizeof(Sweep)), "hipMemset")) return 3;
    hipLaunchKernelGGL(sweep_kernel, dim3((count + 255) / 256), dim3(256), 0, 0, first, stride, count, ds);
    if (!ok(hipGetLastError(), "sweep launch") || !ok(hipMemcpy(&hs, ds, sizeof(Sweep), hipMemcpyDeviceToHost), "sweep copy")) return 3;
    std::printf("sweep: form %d, %u inputs from 0x%08x by %u, %llu mismatches\n", JT_SQRT_FORM, count, first, stride, hs.bad);
    for (unsigned long long k = 0; k < hs.bad && k < NFIRST; k++) std::printf("  bad x=%08x\n", hs.first[k]);

    std::vector<unsigned> in;
    if (FILE* f = std::fopen(argv[4], "rb")) {
        unsigned v;
        while (std::fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "jt_sqrt_probe: cannot read %s\n", argv[4]);
        return 2;
    }
    const unsigned n = (unsigned)in.size();
    if (n == 0 || n > (1u << 24)) return 2;
    std::vector<unsigned> out((size_t)n * 2);
    unsigned *di = nullptr, *dout = nullptr;
    if (!ok(hipMalloc(&di, (size_t)n * 4), "hipMalloc") || !ok(hipMalloc(&dout, (size_t)n * 8), "hipMalloc") ||
        !ok(hipMemcpy(di, in.data(), (size_t)n * 4, hipMemcpyHostToDevice), "copy in"))
        return 3;
    hipLaunchKernelGGL(list_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, di, n, dout);
    if (!ok(hipGetLastError(), "list launch") || !ok(hipMemcpy(out.data(), dout, (size_t)n * 8, hipMemcpyDeviceToHost), "copy out")) return 3;
    FILE* f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    std::printf("list: %u inputs\n", n);
    return 0;
}
