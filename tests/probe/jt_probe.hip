// jt_probe.hip — TEST INFRASTRUCTURE ONLY: libjt_probe.so, one kernel per device primitive.
//
// The product's per-lane headers (csrc/jt_device.h, jt_bsdf.h, jt_scene_eval.h) are included as they are and
// compiled with the product's flags (tests/probe/Makefile); nothing here is linked into
// libjtrace_hip.so. An op reads `nin` floats per lane and writes `nout` floats per lane (booleans
// as 0.0f / 1.0f, integers as their float value); tests/test_gpu_primitives.py compares the output
// bits with the oracle's or_probe (oracle/jt_oracle.c), which runs the same ops under the same ids,
// and with the float64 references of tests/primitives_ref.py.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "jt_scene_eval.h"

using namespace jtd;
using namespace jtk;  // jt_scene_eval.h

enum {
    JP_SINCOS = 0,
    JP_DISK,
    JP_ATAN,
    JP_ATAN2,
    JP_ACOS,
    JP_LOG,
    JP_EXP,
    JP_MINMAX,
    JP_RCP,
    JP_BBOX,
    JP_TRIANGLE,
    JP_QUAD,
    JP_BSDF,
    JP_PARTS,
    JP_VOLUME,
    JP_NOPS
};
struct JpOp {
    const char* name;
    int nin, nout;
};
// the table tests/test_primitives_host.py compares with the oracle's
static const JpOp jp_ops[JP_NOPS] = {
    {"sincos", 1, 6},     // x -> sin, cos, then the doubles they were rounded from (lo, hi words each)
    {"disk", 1, 4},       // u -> sample_disk((u, 1)).xy, sample_disk_signs((u, 1)).xy
    {"atan", 1, 7},       // x -> t = atan(x), sincos(t), then the doubles of that sincos
    {"atan2", 2, 1},      // y, x
    {"acos", 1, 1},
    {"log", 1, 1},
    {"exp", 1, 1},
    {"minmax", 3, 6},     // a, b, c -> min(a,b), max(a,b), min3, max3, max3(v3), clamp(a, b, c)
    {"rcp", 1, 1},
    {"bbox", 14, 1},      // o, dinv, tmin, tmax, bmin, bmax -> hit
    {"triangle", 17, 12}, // o, d, tmin, tmax, p1, p2, p3 -> (u, v, t, hit) of intersect_triangle, _e, _pre + tri_hit_before
    {"quad", 20, 4},      // o, d, tmin, tmax, p1..p4 -> u, v, t, hit
    {"bsdf", 18, 18},     // type, color, ior, roughness, n, o, i, rnl, rn -> the <FT_ALL> dispatchers
    {"parts", 18, 24},    // the same record -> Fresnel terms, basis, hemisphere, microfacet, refract, D, G
    {"volume", 19, 12},   // density, scattering, anisotropy, o, i, rn, distance, max_distance, rl, rd
};

__device__ __forceinline__ v3 ld3(const float* x) { return V3(x[0], x[1], x[2]); }
__device__ __forceinline__ void st3(float* y, v3 a) {
    y[0] = a.x;
    y[1] = a.y;
    y[2] = a.z;
}
__device__ __forceinline__ void st_hit(float* y, const PrimHit& h) {
    y[0] = h.u;
    y[1] = h.v;
    y[2] = h.t;
    y[3] = h.hit ? 1.0f : 0.0f;
}
__device__ __forceinline__ MatPoint ld_mat(const float* x) {
    MatPoint m = {};
    m.type = (int)x[0];
    m.color = ld3(x + 1);
    m.ior = x[4];
    m.roughness = x[5];
    return m;
}

// The doubles jl_sincos rounds, as two 32-bit words each in float slots (moved, never computed
// with): the small-argument path's, zeros for the large path and for a build without JT_EXACT_MATH.
// With them a test pins the double evaluation itself, which the rounded floats alone cannot (an FMA
// contracted into the reduction moves the double's last bits and almost never the float).
__device__ __forceinline__ void st_sincos_doubles(float x, float* y) {
    double s = 0.0, c = 0.0;
#if JT_EXACT_MATH
    if (__builtin_fabsf(x) < 524288.0f) dsincos_small((double)x, s, c);
#endif
    const unsigned long long sb = (unsigned long long)__double_as_longlong(s), cb = (unsigned long long)__double_as_longlong(c);
    y[0] = __uint_as_float((unsigned)sb);
    y[1] = __uint_as_float((unsigned)(sb >> 32));
    y[2] = __uint_as_float((unsigned)cb);
    y[3] = __uint_as_float((unsigned)(cb >> 32));
}

template <int OP>
__device__ __forceinline__ void jp_eval(const float* x, float* y) {
    if constexpr (OP == JP_SINCOS) {
        jl_sincos(x[0], &y[0], &y[1]);
        st_sincos_doubles(x[0], y + 2);
    } else if constexpr (OP == JP_DISK) {
        const v2 d = sample_disk(V2(x[0], 1.0f)), s = sample_disk_signs(V2(x[0], 1.0f));
        y[0] = d.x, y[1] = d.y, y[2] = s.x, y[3] = s.y;
    } else if constexpr (OP == JP_ATAN) {
        y[0] = jl_atan(x[0]);
        jl_sincos(y[0], &y[1], &y[2]);
        st_sincos_doubles(y[0], y + 3);
    } else if constexpr (OP == JP_ATAN2) {
        y[0] = jl_atan2(x[0], x[1]);
    } else if constexpr (OP == JP_ACOS) {
        y[0] = jl_acos(x[0]);
    } else if constexpr (OP == JP_LOG) {
        y[0] = jl_log(x[0]);
    } else if constexpr (OP == JP_EXP) {
        y[0] = jl_exp(x[0]);
    } else if constexpr (OP == JP_MINMAX) {
        y[0] = jl_min(x[0], x[1]);
        y[1] = jl_max(x[0], x[1]);
        y[2] = jl_min3(x[0], x[1], x[2]);
        y[3] = jl_max3(x[0], x[1], x[2]);
        y[4] = max3(ld3(x));
        y[5] = jl_clamp(x[0], x[1], x[2]);
    } else if constexpr (OP == JP_RCP) {
        y[0] = jl_rcp(x[0]);
    } else if constexpr (OP == JP_BBOX) {
        const float4 a = make_float4(x[8], x[11], x[9], x[12]), b = make_float4(x[10], x[13], 0.0f, 0.0f);
        y[0] = intersect_bbox(ld3(x), ld3(x + 3), x[6], x[7], a, b) ? 1.0f : 0.0f;
    } else if constexpr (OP == JP_TRIANGLE) {
        const v3 o = ld3(x), d = ld3(x + 3), p1 = ld3(x + 8), p2 = ld3(x + 11), p3 = ld3(x + 14);
        st_hit(y, intersect_triangle(o, d, x[6], x[7], p1, p2, p3));
        st_hit(y + 4, intersect_triangle_e(o, d, x[6], x[7], p1, p2 - p1, p3 - p1));
        // the two-step form as its callers complete it: a rejected primitive is the miss (0, 0, inf)
        PrimHit p = intersect_triangle_pre(o, d, x[6], p1, p2 - p1, p3 - p1);
        if (!tri_hit_before(p, x[7])) p = PrimHit{0.0f, 0.0f, __builtin_inff(), false};
        st_hit(y + 8, p);
    } else if constexpr (OP == JP_QUAD) {
        const v3 p3 = ld3(x + 14), p4 = ld3(x + 17);
        const bool degenerate = p3.x == p4.x && p3.y == p4.y && p3.z == p4.z;  // the host layout's rule
        st_hit(y, intersect_quad(ld3(x), ld3(x + 3), x[6], x[7], ld3(x + 8), ld3(x + 11), p3, p4, degenerate));
    } else if constexpr (OP == JP_BSDF) {
        const MatPoint m = ld_mat(x);
        const v3 n = ld3(x + 6), o = ld3(x + 9), i = ld3(x + 12);
        const float rnl = x[15];
        const v2 rn = V2(x[16], x[17]);
        st3(y, eval_bsdfcos<FT_ALL>(m, n, o, i));
        st3(y + 3, sample_bsdfcos<FT_ALL>(m, n, o, rnl, rn));
        y[6] = sample_bsdfcos_pdf<FT_ALL>(m, n, o, i);
        st3(y + 7, eval_delta<FT_ALL>(m, n, o, i));
        st3(y + 10, sample_delta<FT_ALL>(m, n, o, rnl));
        y[13] = sample_delta_pdf<FT_ALL>(m, n, o, i);
        v3 f;
        float pdf;
        eval_bsdfcos_pdf<FT_ALL>(m, n, o, i, f, pdf);
        st3(y + 14, f);
        y[17] = pdf;
    } else if constexpr (OP == JP_PARTS) {
        const MatPoint m = ld_mat(x);
        const v3 n = ld3(x + 6), o = ld3(x + 9), i = ld3(x + 12);
        const v2 rn = V2(x[16], x[17]);
        y[0] = fresnel_dielectric(m.ior, n, o);
        st3(y + 1, fresnel_conductor(reflectivity_to_eta(m.color), n, o));
        const m3 b = basis_fromz(n);
        st3(y + 4, b.c1);
        st3(y + 7, b.c2);
        st3(y + 10, b.c3);
        st3(y + 13, sample_hemisphere_cos(n, rn));
        st3(y + 16, sample_microfacet(m.roughness, n, rn));
        st3(y + 19, refract(o, n, m.ior));
        const v3 h = normalize(i + o);
        y[22] = microfacet_distribution(m.roughness, n, h);
        y[23] = microfacet_shadowing(m.roughness, n, h, o, i);
    } else if constexpr (OP == JP_VOLUME) {
        Volume vol;
        vol.density = ld3(x);
        vol.scattering = ld3(x + 3);
        vol.scanisotropy = x[6];
        const v3 o = ld3(x + 7), i = ld3(x + 10);
        st3(y, eval_transmittance(vol.density, x[15]));
        y[3] = sample_transmittance(vol.density, x[16], x[17], x[18]);
        y[4] = sample_transmittance_pdf(vol.density, x[15], x[16]);
        st3(y + 5, eval_scattering(vol, o, i));
        st3(y + 8, sample_scattering(vol, o, V2(x[13], x[14])));
        y[11] = sample_scattering_pdf(vol, o, i);
    }
}

template <int OP, int NIN, int NOUT>
__global__ void jp_kernel(size_t n, const float* __restrict__ in, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float x[NIN], y[NOUT];
        for (int k = 0; k < NIN; k++) x[k] = in[i * NIN + k];
        jp_eval<OP>(x, y);
        for (int k = 0; k < NOUT; k++) out[i * NOUT + k] = y[k];
    }
}

template <int OP, int NIN, int NOUT>
static void jp_launch(size_t n, const float* in, float* out) {
    const unsigned block = 256;
    jp_kernel<OP, NIN, NOUT><<<dim3((unsigned)((n + block - 1) / block)), dim3(block)>>>(n, in, out);
}

// eval_texture over a scene that holds textures only. Lane i reads (texture, u, v, as_linear) and
// writes the four channels. The texel-decode LUTs go to LDS first, as the trace kernels stage them.
__global__ void jp_texture_kernel(DScene S, size_t n, const float* __restrict__ q, float* __restrict__ out) {
    for (int k = threadIdx.x; k < 512; k += blockDim.x) tex_lut[k] = k < 256 ? S.srgb_lut[k] : S.byte_lut[k - 256];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const v4 r = eval_texture(S, (int)q[4 * i], V2(q[4 * i + 1], q[4 * i + 2]), q[4 * i + 3] != 0.0f);
        out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
    }
}

extern "C" {

int jp_op_count(void) { return JP_NOPS; }
const char* jp_op_name(int op) { return op >= 0 && op < JP_NOPS ? jp_ops[op].name : nullptr; }
int jp_op_nin(int op) { return op >= 0 && op < JP_NOPS ? jp_ops[op].nin : -1; }
int jp_op_nout(int op) { return op >= 0 && op < JP_NOPS ? jp_ops[op].nout : -1; }

// Runs op over n lanes: in is n x nin floats, out n x nout floats (host memory, row per lane).
// Allocates, copies, launches, synchronises; returns the first HIP error, 0 on success, -1 for an
// unknown op or a lane count the launch grid cannot hold.
int jp_run(int op, int64_t n, const float* in, float* out) {
    if (op < 0 || op >= JP_NOPS || n < 0 || n > ((int64_t)1 << 30)) return -1;
    if (n == 0) return 0;
    const size_t nin = (size_t)jp_ops[op].nin, nout = (size_t)jp_ops[op].nout, N = (size_t)n;
    float *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, N * nin * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, N * nout * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(din, in, N * nin * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        switch (op) {
#define JP_CASE(OP, NIN, NOUT) \
    case OP: jp_launch<OP, NIN, NOUT>(N, din, dout); break;
            JP_CASE(JP_SINCOS, 1, 6)
            JP_CASE(JP_DISK, 1, 4)
            JP_CASE(JP_ATAN, 1, 7)
            JP_CASE(JP_ATAN2, 2, 1)
            JP_CASE(JP_ACOS, 1, 1)
            JP_CASE(JP_LOG, 1, 1)
            JP_CASE(JP_EXP, 1, 1)
            JP_CASE(JP_MINMAX, 3, 6)
            JP_CASE(JP_RCP, 1, 1)
            JP_CASE(JP_BBOX, 14, 1)
            JP_CASE(JP_TRIANGLE, 17, 12)
            JP_CASE(JP_QUAD, 20, 4)
            JP_CASE(JP_BSDF, 18, 18)
            JP_CASE(JP_PARTS, 18, 24)
            JP_CASE(JP_VOLUME, 19, 12)
#undef JP_CASE
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, N * nout * sizeof(float), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

// eval_texture on a hand-built DScene of ntex textures. desc: ntex x (width, height, linear,
// is_float); texb / texf: the byte (4 per texel) and float (4 per texel) textures' texels, each kind
// concatenated in texture order, nb / nf texels in all. Storage follows the host layout
// (jt_layout.cpp): a texture's offset is the texel count of its kind before it, and texb ends in one
// padding texel. q: n x (texture, u, v, as_linear), out: n x 4. Every texture index of q must lie
// in [0, ntex) and the texel counts must add up, or -1 is returned and nothing runs.
int jp_run_texture(int ntex, const int32_t* desc, const uint8_t* texb, int64_t nb, const float* texf, int64_t nf,
                   const float* srgb_lut, const float* byte_lut, int64_t n, const float* q, float* out) {
    if (ntex < 1 || ntex > 4096 || n < 1 || n > ((int64_t)1 << 24) || nb < 0 || nf < 0) return -1;
    DTexture* tex = new DTexture[ntex];
    long long ob = 0, of = 0;
    bool ok = true;
    for (int k = 0; k < ntex; k++) {
        const int32_t* d = desc + 4 * k;
        ok = ok && d[0] >= 0 && d[1] >= 0 && d[0] <= 4096 && d[1] <= 4096;
        tex[k] = DTexture{d[0], d[1], d[2], d[3] != 0, d[3] ? of : ob, 0};
        (d[3] ? of : ob) += (long long)d[0] * d[1];
    }
    ok = ok && ob == nb && of == nf;
    for (int64_t i = 0; ok && i < n; i++) ok = q[4 * i] >= 0 && q[4 * i] < (float)ntex && q[4 * i] == (float)(int)q[4 * i];
    if (!ok) {
        delete[] tex;
        return -1;
    }
    uchar4* hb = new uchar4[nb + 1];
    for (int64_t k = 0; k < nb; k++) hb[k] = make_uchar4(texb[4 * k], texb[4 * k + 1], texb[4 * k + 2], texb[4 * k + 3]);
    hb[nb] = make_uchar4(0, 0, 0, 0);  // the padding texel
    DTexture* dtex = nullptr;
    uchar4* db = nullptr;
    float4* df = nullptr;
    float *dl = nullptr, *dq = nullptr, *dout = nullptr;
    const size_t N = (size_t)n;
    hipError_t e = hipMalloc((void**)&dtex, ntex * sizeof(DTexture));
    if (e == hipSuccess) e = hipMalloc((void**)&db, (size_t)(nb + 1) * sizeof(uchar4));
    if (e == hipSuccess) e = hipMalloc((void**)&df, (size_t)(nf + 1) * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void**)&dl, 512 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dq, N * 4 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, N * 4 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dtex, tex, ntex * sizeof(DTexture), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, hb, (size_t)(nb + 1) * sizeof(uchar4), hipMemcpyHostToDevice);
    if (e == hipSuccess && nf) e = hipMemcpy(df, texf, (size_t)nf * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dl, srgb_lut, 256 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dl + 256, byte_lut, 256 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dq, q, N * 4 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        DScene S = {};
        S.textures = dtex;
        S.texb = db;
        S.texf = df;
        S.srgb_lut = dl;
        S.byte_lut = dl + 256;
        const unsigned block = 256;
        jp_texture_kernel<<<dim3((unsigned)((N + block - 1) / block)), dim3(block)>>>(S, N, dq, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, N * 4 * sizeof(float), hipMemcpyDeviceToHost);
    void* all[] = {dtex, db, df, dl, dq, dout};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete[] tex;
    delete[] hb;
    return (int)e;
}

}  // extern "C"
