// bounded_rules_check.cpp — the argument rules the bounded ray queries and jt_ambient_occlusion add
// (csrc/jt_intersect.h, csrc/jt_radiance.h), enumerated on the host. tests/test_bounded_host.py builds
// it with the host compiler under -fsanitize=address,undefined and runs it. No Python, no HIP
// runtime, no GPU.
//
//   - SEGMENT_TMAX: jt_visible's bound is the float32 value of 1 - ray_eps, below 1 and above
//     1 - 2 ray_eps, so a hit at the far end's surface (t within ray_eps of 1) is not accepted;
//   - occlusion_radius_error: nullptr exactly for radius > 0, +inf included; a message naming
//     `radius` for NaN, +-0, negatives and -inf; it comes after every rule of radiance_range_error;
//   - occlusion_visibility: the quotient of two integers exact in float32, in [0, 1], 0 and 1 at the
//     ends, monotone in the visible count, equal to the double quotient rounded once, for sample
//     counts up to RADIANCE_MAX_SAMPLES;
//   - the BOUND forms are distinct and BOUND_NONE is 0 (the unbounded kernels' default).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../julia-raytracer_amd/csrc/jt_radiance.h"

namespace {

long cases = 0, bad = 0;
void check(bool ok, const char* what, double a = 0, double b = 0) {
    cases++;
    if (!ok && bad++ < 20) std::fprintf(stderr, "bounded_rules_check: %s (%g %g)\n", what, a, b);
}

void check_segment() {
    const float eps = 0.0001f;
    volatile float one = 1.0f;
    const float want = one - eps;  // one float32 subtraction at run time
    check(jtq::SEGMENT_TMAX == want, "SEGMENT_TMAX is not 1 - ray_eps in float32", jtq::SEGMENT_TMAX, want);
    check(jtq::SEGMENT_TMAX < 1.0f && jtq::SEGMENT_TMAX > 1.0f - 2 * eps, "SEGMENT_TMAX outside (1 - 2 eps, 1)", jtq::SEGMENT_TMAX);
    check(jtq::BOUND_NONE == 0 && jtq::BOUND_ARRAY != jtq::BOUND_NONE && jtq::BOUND_SEGMENT != jtq::BOUND_NONE &&
              jtq::BOUND_ARRAY != jtq::BOUND_SEGMENT,
          "the BOUND forms");
}

void check_radius() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float ok : {std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::min(), 1e-6f, 0.25f, 1.0f, 3.5e3f,
                     std::numeric_limits<float>::max(), inf})
        check(jtr::occlusion_radius_error(ok) == nullptr, "a radius above 0 refused", ok);
    for (float no : {0.0f, -0.0f, -std::numeric_limits<float>::denorm_min(), -1.0f, -inf, nan, -nan}) {
        const char* m = jtr::occlusion_radius_error(no);
        check(m != nullptr && std::strstr(m, "radius") == m, "a radius that is not above 0 accepted, or a message that does not name it", no);
    }
    // the order: a call that breaks a range rule and the radius rule reports the range rule
    check(jtr::radiance_range_error(-1, 0, 0, 1) != nullptr && jtr::radiance_range_error(4, 0, 3, 3) != nullptr &&
              jtr::radiance_range_error(4, 0, 0, 1) == nullptr,
          "radiance_range_error");
}

void check_visibility() {
    const int64_t max = jtr::RADIANCE_MAX_SAMPLES;
    check((int64_t)(float)max == max && (int64_t)(float)(max - 1) == max - 1, "2^24 samples are not exact in float32");
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)5, (int64_t)7, (int64_t)16, (int64_t)1000, (int64_t)1024, (int64_t)65537, max - 1, max}) {
        check(jtr::occlusion_visibility(0, (int)n) == 0.0f, "none visible is not 0", (double)n);
        check(jtr::occlusion_visibility((int)n, (int)n) == 1.0f, "all visible is not 1", (double)n);
        float prev = -1.0f;
        const int64_t step = n <= 4096 ? 1 : n / 1021;
        for (int64_t v = 0; v <= n; v += step) {
            const float q = jtr::occlusion_visibility((int)v, (int)n);
            check(q >= 0.0f && q <= 1.0f, "visibility outside [0, 1]", (double)v, (double)n);
            check(q == (float)((double)v / (double)n), "visibility is not the once-rounded quotient", (double)v, (double)n);
            check(q >= prev, "visibility not monotone in the count", (double)v, (double)n);
            prev = q;
        }
    }
    check(jtr::occlusion_visibility(3, 5) == 0.6f, "3 of 5");
}

}  // namespace

int main() {
    check_segment();
    check_radius();
    check_visibility();
    std::printf("bounded_rules_check: %ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
