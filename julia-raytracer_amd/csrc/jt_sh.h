// jt_sh.h — the real spherical harmonics of bands 0..2 that jt_probe_sh projects onto
// (include/jtrace.h): the constants, the basis at a direction and the layout of a
// probe's record. Plain C++ (no HIP runtime), shared by radiance_kernel's epilogue
// (jt_radiance.hip) and the host check (tests/sh_check.cpp). Not part of the ABI.
//
// Every operation is a rounded float32 operation in the association written here; the units that
// include this header are compiled without contraction (-ffp-contract=off), so no product is fused
// into a sum. jtrace/sh.py restates the same expressions in numpy.
#pragma once

#include <stdint.h>

namespace jtsh {

constexpr int SH_COEFFS = 9;                        // bands 0, 1, 2
constexpr int SH_CHANNELS = 4;                      // r, g, b and the coverage flag
constexpr int SH_RECORD = SH_COEFFS * SH_CHANNELS;  // floats of a probe: 144 bytes, nine float4

constexpr float SH_C0 = 0.282095f;  // 1 / (2 sqrt pi)
constexpr float SH_C1 = 0.488603f;  // sqrt 3 / (2 sqrt pi)
constexpr float SH_C2 = 1.092548f;  // sqrt 15 / (2 sqrt pi)
constexpr float SH_C3 = 0.315392f;  // sqrt 5 / (4 sqrt pi)
constexpr float SH_C4 = 0.546274f;  // sqrt 15 / (4 sqrt pi)

// sh[(9 i + k) * 4 + c]: coefficient k, channel c of probe i
constexpr int64_t sh_index(int64_t probe, int k, int c) { return (probe * SH_COEFFS + k) * SH_CHANNELS + c; }

struct Basis {
    float y[SH_COEFFS];
};

// Y_0 .. Y_8 at the unit direction (x, y, z): constexpr, so a host and a device function alike
constexpr Basis sh_basis(float x, float y, float z) {
    return Basis{{SH_C0, SH_C1 * y, SH_C1 * z, SH_C1 * x, SH_C2 * (x * y), SH_C2 * (y * z), SH_C3 * (3.0f * (z * z) - 1.0f),
                  SH_C2 * (x * z), SH_C4 * (x * x - y * y)}};
}

// One step of a probe's running mean, per coefficient and channel: the integrator's own
// acc * (1 - w) + target * w on the product target * Y_k. The first step of a probe runs it from
// acc = 0 with w = 1, so a product of -0 comes out as +0: 0 * 0 + (-0) * 1.
constexpr float sh_fold(float acc, float target, float yk, float w, float omw) { return acc * omw + (target * yk) * w; }

}  // namespace jtsh
