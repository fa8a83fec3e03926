// denoise_bench.hip — device time of the denoiser's launches (jt::denoise_launch and
// jt::denoise_guided_launch, julia-raytracer_amd/csrc/jt_denoise.hip) at a frame size a user
// renders, HIP events around the launches, the two filters and the iteration counts 1..I
// interleaved round by round in one process. The time of iteration i is read as
// T(i + 1 iterations) - T(i iterations). Data are seeded noise over piecewise constant guides, the
// variance that of a 30 % relative standard error: the filters' work per pixel does not depend
// on the values.
//
//   make -C julia-raytracer_amd denoise-bench && julia-raytracer_amd/build/denoise_bench [W H rounds]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_denoise.h"

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// the device time of one launch() on st, in ms
template <class Launch>
hipError_t timed(hipStream_t st, hipEvent_t e0, hipEvent_t e1, Launch launch, float* ms) {
    hipError_t e;
    if ((e = hipEventRecord(e0, st)) != hipSuccess || (e = launch()) != hipSuccess ||
        (e = hipEventRecord(e1, st)) != hipSuccess || (e = hipEventSynchronize(e1)) != hipSuccess)
        return e;
    return hipEventElapsedTime(ms, e0, e1);
}

// one line per iteration count; returns the median of the I iterations
double report(const char* filter, std::vector<std::vector<float>>& ms, int I, size_t np) {
    const double compulsory = 64.0 * (double)np;  // d, albedo, normal read, d written: 64 B per pixel
    double prev = 0;
    for (int it = 1; it <= I; it++) {
        std::sort(ms[it].begin(), ms[it].end());
        const double med = ms[it][ms[it].size() / 2], mn = ms[it].front();
        const double dt = med - prev;
        std::printf("%siterations=%d  median %.4f ms  min %.4f ms  | step %2d (+demodulate at 1): %.4f ms, "
                    "compulsory %.1f MB = %.2f TB/s\n",
                    filter, it, med, mn, 1 << (it - 1), dt, compulsory / 1e6, compulsory / (dt * 1e-3) / 1e12);
        prev = med;
    }
    return prev;
}

int main(int argc, char** argv) {
    const int W = argc > 1 ? std::atoi(argv[1]) : 1280, H = argc > 2 ? std::atoi(argv[2]) : 720;
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 50;
    if (jt::denoise_check_size(W, H) != JT_OK || rounds < 1) {
        std::fprintf(stderr, "usage: denoise_bench [W H rounds]\n");
        return 2;
    }
    jt_denoise_params p;
    jt_denoise_defaults(16, &p);
    const int I = p.iterations;
    const size_t np = (size_t)W * H;
    jt_denoise_guided_params g;
    jt_denoise_guided_defaults(&g);
    std::vector<float4> host(np * 4);
    unsigned s = 12345u;
    auto rnd = [&] { return (float)((s = s * 1664525u + 1013904223u) >> 8) * (1.0f / 16777216.0f); };
    for (size_t k = 0; k < np; k++) {
        const int x = (int)(k % W), y = (int)(k / W), region = (x * 3 < W) ? 0 : ((x + y) * 2 < W + H ? 1 : 2);
        const float a = 0.2f + 0.3f * region;
        host[np + k] = make_float4(a, 0.5f * a, 1.0f - a, 0.0f);
        host[2 * np + k] = make_float4(region == 0, region == 1, region == 2, 0.0f);
        host[k] = make_float4(a * (0.5f + rnd()), 0.5f * a * (0.5f + rnd()), (1.0f - a) * (0.5f + rnd()), 1.0f);
        const float4 c = host[k];
        host[3 * np + k] = make_float4(0.09f * c.x * c.x, 0.09f * c.y * c.y, 0.09f * c.z * c.z, 0.0f);
    }
    float4* d = nullptr;
    // image, albedo, normal, variance, ping, pong, out
    CHECK(hipMalloc((void**)&d, np * 16 * 7));
    CHECK(hipMemcpy(d, host.data(), np * 64, hipMemcpyHostToDevice));
    hipStream_t st;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<std::vector<float>> ms(I + 1), gms(I + 1);
    for (int r = -3; r < rounds; r++) {  // three warm-up rounds
        for (int it = 1; it <= I; it++) {
            jt_denoise_params q = p;
            jt_denoise_guided_params gq = g;
            q.iterations = gq.iterations = it;
            float t = 0;
            CHECK(timed(st, e0, e1, [&] {
                return jt::denoise_launch(st, d, d + np, d + 2 * np, W, H, q, d + 4 * np, d + 5 * np, d + 6 * np);
            }, &t));
            if (r >= 0) ms[it].push_back(t);
            CHECK(timed(st, e0, e1, [&] {
                return jt::denoise_guided_launch(st, d, d + 3 * np, d + np, d + 2 * np, W, H, gq, d + 4 * np, d + 5 * np,
                                                 d + 6 * np);
            }, &t));
            if (r >= 0) gms[it].push_back(t);
        }
    }
    std::printf("denoise %dx%d, defaults for 16 spp, %d rounds, filters and iteration counts interleaved\n", W, H, rounds);
    const double plain = report("", ms, I, np);
    std::printf("one default denoise (%d iterations): median %.4f ms\n", I, plain);
    const double guided = report("guided ", gms, I, np);
    std::printf("one default guided denoise (%d iterations): median %.4f ms, %.3f x the plain filter\n", I, guided,
                guided / plain);
    return 0;
}
