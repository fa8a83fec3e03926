// Host check of csrc/jt_sh.h, the spherical-harmonic basis jt_probe_sh projects onto
// (tests/test_sh_host.py builds and runs it; no device).
//   sh_check IN OUT   IN: n x 3 float32 directions; OUT: n x 9 float32, sh_basis of every one, for
//                     the bit comparison with jtrace/sh.py
// and, on every run, the header's own rules: the record layout, the constants against their closed
// forms, the fold step and its -0 rule. Prints "<checks> checks, <bad> bad".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../julia-raytracer_amd/csrc/jt_sh.h"

static int checks = 0, bad = 0;
static void check(bool ok, const char* what) {
    checks++;
    if (!ok) {
        bad++;
        std::printf("FAIL %s\n", what);
    }
}
static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    using namespace jtsh;
    // the layout: nine float4 per probe, coefficient-major
    check(SH_COEFFS == 9 && SH_CHANNELS == 4 && SH_RECORD == 36, "record size");
    check(sh_index(0, 0, 0) == 0 && sh_index(0, 1, 0) == 4 && sh_index(0, 8, 3) == 35 && sh_index(1, 0, 0) == 36, "sh_index");
    check(sh_index(((int64_t)1 << 30) - 1, 8, 3) == ((int64_t)36 << 30) - 1, "sh_index past 2^31");
    // the constants are the closed forms to six digits
    const double pi = 3.14159265358979323846;
    const double want[5] = {0.5 / std::sqrt(pi), std::sqrt(3.0) / (2 * std::sqrt(pi)), std::sqrt(15.0) / (2 * std::sqrt(pi)),
                            std::sqrt(5.0) / (4 * std::sqrt(pi)), std::sqrt(15.0) / (4 * std::sqrt(pi))};
    const float have[5] = {SH_C0, SH_C1, SH_C2, SH_C3, SH_C4};
    for (int k = 0; k < 5; k++) check(std::fabs(have[k] - want[k]) <= 5e-7, "constant");
    // the basis on the axes, evaluated at compile time as well
    constexpr Basis up = sh_basis(0.0f, 0.0f, 1.0f);
    static_assert(up.y[0] == SH_C0 && up.y[2] == SH_C1 && up.y[6] == SH_C3 * 2.0f, "constexpr basis");
    check(up.y[1] == 0 && up.y[3] == 0 && up.y[4] == 0 && up.y[5] == 0 && up.y[7] == 0 && up.y[8] == 0, "basis at +z");
    const Basis mx = sh_basis(-1.0f, 0.0f, 0.0f);
    check(mx.y[3] == -SH_C1 && mx.y[8] == SH_C4 && mx.y[6] == -SH_C3, "basis at -x");
    // the fold: the first step turns a product of -0 into +0, a later step is the plain expression
    const float v = 0.0f * -SH_C1;
    check(bits(v) == 0x80000000u, "the bare product is -0");
    check(bits(sh_fold(0.0f, 0.0f, -SH_C1, 1.0f, 0.0f)) == 0u, "the first fold step gives +0");
    check(sh_fold(0.0f, 2.0f, 0.5f, 1.0f, 0.0f) == 1.0f, "first step value");
    const float w = 1.0f / 3.0f, omw = 1 - w;
    check(bits(sh_fold(0.7f, 1.3f, -0.4f, w, omw)) == bits(0.7f * omw + (1.3f * -0.4f) * w), "later step");

    if (argc == 3) {
        std::FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 2;
        std::vector<float> d;
        float buf[3];
        while (std::fread(buf, sizeof(float), 3, in) == 3) d.insert(d.end(), buf, buf + 3);
        std::fclose(in);
        std::FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        for (size_t i = 0; i + 2 < d.size(); i += 3) {
            const Basis b = sh_basis(d[i], d[i + 1], d[i + 2]);
            if (std::fwrite(b.y, sizeof(float), SH_COEFFS, out) != (size_t)SH_COEFFS) return 2;
        }
        std::fclose(out);
        std::printf("%zu directions\n", d.size() / 3);
    }
    std::printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
