// jt_accum.hip — from stream means to the running means: combine_kernel (k > 1 streams) and
// chain_kernel (the chunks of a one-stream context), one thread per launch slot (jt_plan.h
// slot_pixel), and their launches (jt_accum.h).
#include <hip/hip_runtime.h>

#include "jt_accum.h"

using namespace jtd;

namespace jtk {
// the combine of every pixel's stream means (DCombine, jt_launch.h), one thread per pixel of
// the launch's tiles (slot g); stream j's records of neighbouring pixels are contiguous (coalesced).
// Two kernels over the same streams: the image after every launch (16 B per pixel and stream),
// the AOVs and hits (32 B per pixel and stream) only when they are read (jt_ctx::aov_pending):
// the stream means stay in place until the next launch appends to them, so the deferred AOV
// combine reads exactly what an eager one would have
template <bool AOV>
__global__ __launch_bounds__(256) void combine_kernel(DParams P, DAccum A, DCombine Cw) {
    const int tiles = launch_tiles(P);
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= tiles * 64) return;
    const SlotPixel px = slot_pixel(g, P.width, P.height, P.tile_stride, P.tile_offset);
    if (!px.inside) return;
    const size_t pixel = (size_t)px.j * P.width + px.i, ns = (size_t)A.nslot;
    const float w0 = Cw.w[0];
    if constexpr (!AOV) {
        float4 im = A.part_img[g];
        im = make_float4(im.x * w0, im.y * w0, im.z * w0, im.w * w0);
        // unrolled: eight streams' loads in flight per thread (the sums stay in stream order)
#pragma unroll 8
        for (int s = 1; s < Cw.ns; s++) {
            const float w = Cw.w[s];
            const float4 a = A.part_img[s * ns + g];
            im = make_float4(im.x + a.x * w, im.y + a.y * w, im.z + a.z * w, im.w + a.w * w);
        }
        A.image[pixel] = im;
    } else {
        float4 al = A.part_alb[g], nr = A.part_nrm[g];
        long long h = __float_as_int(al.w);
        al = make_float4(al.x * w0, al.y * w0, al.z * w0, 0.0f);
        nr = make_float4(nr.x * w0, nr.y * w0, nr.z * w0, 0.0f);
#pragma unroll 4
        for (int s = 1; s < Cw.ns; s++) {
            const float w = Cw.w[s];
            const float4 b = A.part_alb[s * ns + g], c = A.part_nrm[s * ns + g];
            al = make_float4(al.x + b.x * w, al.y + b.y * w, al.z + b.z * w, 0.0f);
            nr = make_float4(nr.x + c.x * w, nr.y + c.y * w, nr.z + c.z * w, 0.0f);
            h += __float_as_int(b.w);
        }
        A.albedo[pixel] = al;
        A.normal[pixel] = nr;
        A.hits[pixel] = h;
    }
}

// A chunk of a one-stream context (k = 1, the reference's single running mean): the chunk's
// samples x .. x+m-1 were traced as m one-sample streams (each record = that sample's value:
// 0 * 0 + value * 1), and are folded into the running mean here one by one, in sample order, with
// the epilogue's own operations (mean * (1 - w) + value * w, w = 1 / (n0 + j + 1): src/trace.jl:
// 631-648, src/math.jl:89-93) — bit for bit the image of tracing the samples one launch each.
// n0: the context's samples before the chunk (0: the mean starts from zero, as after jt_reset).
// At most 32 VGPRs: the trace kernel of the next chunk (5 waves/SIMD of 96 VGPRs in LDS mode)
// leaves 32 per SIMD free, so chain waves run on the same CUs beside it (stream2).
__global__ __launch_bounds__(256) void chain_kernel(DParams P, DAccum A, int n0, int m) {
    const int tiles = launch_tiles(P);
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= tiles * 64) return;
    const SlotPixel px = slot_pixel(g, P.width, P.height, P.tile_stride, P.tile_offset);
    if (!px.inside) return;
    const unsigned pixel = (unsigned)px.j * (unsigned)P.width + (unsigned)px.i;  // jt_create: < 2^26 pixels
    float ix = 0, iy = 0, iz = 0, iw = 0, ax = 0, ay = 0, az = 0, nx = 0, ny = 0, nz = 0;
    int h = 0;  // the chunk's hits (< 2^31 samples)
    if (n0 > 0) {
        const float4 a = A.image[pixel], b = A.albedo[pixel], c = A.normal[pixel];
        ix = a.x, iy = a.y, iz = a.z, iw = a.w, ax = b.x, ay = b.y, az = b.z, nx = c.x, ny = c.y, nz = c.z;
    }
    // few live registers (byte offsets below 4 GiB: 2^27 records of 16 B at most per buffer set
    // and array, jt_ctx::chunk), so the waves fit beside the next chunk's trace kernel
    const char* pi = reinterpret_cast<const char*>(A.part_img);
    const char* pa = reinterpret_cast<const char*>(A.part_alb);
    const char* pn = reinterpret_cast<const char*>(A.part_nrm);
    const unsigned step = (unsigned)A.nslot * 16u;
    unsigned off = (unsigned)g * 16u;
#pragma unroll 1
    for (int s = 0; s < m; s++, off += step) {
        const float w = 1.0f / (float)(n0 + s + 1), omw = 1 - w;
        const float4 a = *reinterpret_cast<const float4*>(pi + off);
        ix = ix * omw + a.x * w, iy = iy * omw + a.y * w, iz = iz * omw + a.z * w, iw = iw * omw + a.w * w;
        const float4 b = *reinterpret_cast<const float4*>(pa + off);
        ax = ax * omw + b.x * w, ay = ay * omw + b.y * w, az = az * omw + b.z * w;
        h += __float_as_int(b.w);
        const float4 c = *reinterpret_cast<const float4*>(pn + off);
        nx = nx * omw + c.x * w, ny = ny * omw + c.y * w, nz = nz * omw + c.z * w;
    }
    A.image[pixel] = make_float4(ix, iy, iz, iw);
    A.albedo[pixel] = make_float4(ax, ay, az, 0.0f);
    A.normal[pixel] = make_float4(nx, ny, nz, 0.0f);
    A.hits[pixel] = (n0 > 0 ? A.hits[pixel] : 0LL) + h;
}

}  // namespace jtk

namespace jt {

// workgroups of 256 threads over every slot of the launch's tiles
static int accum_blocks(const DParams& P) { return (int)(((long long)jtk::launch_tiles(P) * 64 + 255) / 256); }

hipError_t combine_launch(hipStream_t stream, const DParams& P, const jtk::DAccum& A, const jtk::DCombine& cw, bool aov) {
    const int nblk = accum_blocks(P);
    if (nblk > 0 && aov) hipLaunchKernelGGL(jtk::combine_kernel<true>, dim3(nblk), dim3(256), 0, stream, P, A, cw);
    if (nblk > 0 && !aov) hipLaunchKernelGGL(jtk::combine_kernel<false>, dim3(nblk), dim3(256), 0, stream, P, A, cw);
    return hipGetLastError();
}

hipError_t chain_launch(hipStream_t stream, const DParams& P, const jtk::DAccum& A, int n0, int m) {
    const int nblk = accum_blocks(P);
    if (nblk > 0) hipLaunchKernelGGL(jtk::chain_kernel, dim3(nblk), dim3(256), 0, stream, P, A, n0, m);
    return hipGetLastError();
}

}  // namespace jt
