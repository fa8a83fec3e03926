// jt_unit_probe.hip — TEST INFRASTRUCTURE ONLY: libjt_unit_probe.so, the baked matte sample's parts
// (csrc/jt_device.h sincos_unit, csrc/jt_bsdf.h matte_local) behind kernels of their own, for
// tests/test_gpu_sincos_unit.py. The product's headers are included as they are and compiled with
// the product's flags (tests/probe/unit_probe.mk, which takes them from tests/probe/Makefile); nothing
// here is linked into libjtrace_hip.so.
//
//   ju_sincos(n, u, out)             out[2 i] = sin, out[2 i + 1] = cos of sincos_unit(u[i])
//   ju_local(n, rn, out)             rn[2 i], rn[2 i + 1] -> out[6 i ..]: matte_local<false>, then <true>
//   ju_local_sweep(axis, fixed, res) every k = 0 .. 2^24 - 1 on one axis of rn (0: rn.x = k 2^-24 with
//                                    rn.y = fixed, 1: rn.y = k 2^-24 with rn.x = fixed), both forms
//                                    compared on the device bit for bit (a NaN only has to be a NaN).
//                                    res[0] = lanes evaluated, res[1] = lanes that differ, res[2..9] =
//                                    the first differing k (in no particular order)
// Each returns the first HIP error, 0 on success, -1 for arguments out of range.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "jt_bsdf.h"

using namespace jtd;

namespace {

constexpr unsigned BLOCK = 256;
constexpr unsigned SWEEP = 1u << 24;

__global__ void ju_sincos_kernel(size_t n, const float* __restrict__ u, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincos_unit(u[i], &out[2 * i], &out[2 * i + 1]);
}

__global__ void ju_local_kernel(size_t n, const float* __restrict__ rn, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const v2 r = V2(rn[2 * i], rn[2 * i + 1]);
        const v3 a = matte_local<false>(r), b = matte_local<true>(r);
        float* y = out + 6 * i;
        y[0] = a.x, y[1] = a.y, y[2] = a.z, y[3] = b.x, y[4] = b.y, y[5] = b.z;
    }
}

__device__ __forceinline__ bool same(float a, float b) {
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

// res: 10 words, zeroed by the caller
__global__ void ju_sweep_kernel(int axis, float fixed, unsigned* __restrict__ res) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= SWEEP) return;
    const float t = (float)k * 0x1.0p-24f;  // rand1f
    const v2 r = axis == 0 ? V2(t, fixed) : V2(fixed, t);
    const v3 a = matte_local<false>(r), b = matte_local<true>(r);
    atomicAdd(&res[0], 1u);
    if (!(same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z))) {
        const unsigned slot = atomicAdd(&res[1], 1u);
        if (slot < 8u) res[2 + slot] = k;
    }
}

template <class Launch>
int run(size_t n, const float* in, size_t nin, float* out, size_t nout, Launch launch) {
    float *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, n * nin * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, n * nout * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(din, in, n * nin * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, n * nout * sizeof(float), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

}  // namespace

extern "C" {

int ju_sincos_unit_level(void) { return JT_SINCOS_UNIT; }

int ju_sincos(int64_t n, const float* u, float* out) {
    if (n < 1 || n > ((int64_t)1 << 26)) return -1;
    const size_t N = (size_t)n;
    return run(N, u, 1, out, 2, [&](const float* din, float* dout) {
        ju_sincos_kernel<<<dim3((unsigned)((N + BLOCK - 1) / BLOCK)), dim3(BLOCK)>>>(N, din, dout);
    });
}

int ju_local(int64_t n, const float* rn, float* out) {
    if (n < 1 || n > ((int64_t)1 << 24)) return -1;
    const size_t N = (size_t)n;
    return run(N, rn, 2, out, 6, [&](const float* din, float* dout) {
        ju_local_kernel<<<dim3((unsigned)((N + BLOCK - 1) / BLOCK)), dim3(BLOCK)>>>(N, din, dout);
    });
}

int ju_local_sweep(int axis, float fixed, uint32_t* res) {
    if (axis < 0 || axis > 1 || !(fixed >= 0.0f && fixed < 1.0f)) return -1;
    unsigned* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, 10 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(d, 0, 10 * sizeof(unsigned));
    if (e == hipSuccess) {
        ju_sweep_kernel<<<dim3(SWEEP / BLOCK), dim3(BLOCK)>>>(axis, fixed, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(res, d, 10 * sizeof(unsigned), hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);
    return (int)e;
}

}  // extern "C"
