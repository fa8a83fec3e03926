// shade_bake_check.cpp — the baked hemisphere basis of the FT_NONE kernels (csrc/jt_bsdf.h BakedBasis,
// basis_baked, sample_matte_baked; csrc/jt_kernels.h bake_shading) against basis_fromz, on the host's
// restatement of the device's float operations (csrc/jt_internal.h; -ffp-contract=off).
// tests/test_shade_bake.py builds it with the host compiler under -fsanitize=address,undefined and
// runs it. No Python, no HIP runtime, no GPU. Every comparison is of bits; a NaN only has to be a NaN.
//
//   (a) basis_fromz(-n) is (X, -Y, -Z) of basis_fromz(n), with Y.y' = 0 - Y.y: every entry but Y.y
//       changes or keeps its sign bit exactly; Y.y' equals -Y.y wherever Y.y != 0, and is +0 in both
//       orientations where it cancels (n = (+-0, +-1, +-0)) — counted, and seen at least once.
//   (b) the nine entries of both orientations from the six stored ones (basis_baked).
//   (c) for outgoing directions o: eval_shading's orientation (dot(n, o) >= 0 ? n : -n) followed by
//       up_normal on the oriented normal (dot <= 0 ? -N : N) is n or -n as the XOR of the two
//       predicates says, and basis_baked with that XOR is basis_fromz(up_normal(...)).
// Normals: every combination of {+0, -0, 1, -1} per component (the axes with all zero signs, (0,0,-1)
// where sign + z = -2, z = +-0, the zero vectors), denormal components, and 1.2 million random ones:
// unit vectors as the layout stores them, with components snapped to +-0, and unnormalised ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../julia-raytracer_amd/csrc/jt_internal.h"

namespace {

using jt::f3;
using jt::mk3;

struct m3 {
    f3 x, y, z;
};
// basis_fromz (csrc/jt_bsdf.h, src/shading.jl:724-732)
m3 basis_fromz(f3 v) {
    const f3 z = jt::normalize(v);
    const float sign = std::copysign(1.0f, z.z);
    const float a = -1.0f / (sign + z.z);
    const float b = z.x * z.y * a;
    return m3{mk3(1.0f + sign * z.x * z.x * a, sign * b, -sign * z.x), mk3(b, sign + z.y * z.y * a, -z.y), z};
}
// BakedBasis / basis_baked (csrc/jt_bsdf.h)
struct Baked {
    float xx, yx, yy;
    f3 z;
};
Baked bake(f3 n) {  // bake_shading's element loop
    const m3 b = basis_fromz(n);
    return Baked{b.x.x, b.y.x, b.y.y, b.z};
}
m3 basis_baked(const Baked& k, bool flip) {
    const f3 z = flip ? -k.z : k.z;
    const float b = flip ? -k.yx : k.yx;
    const float sign = std::copysign(1.0f, z.z);
    return m3{mk3(k.xx, sign * b, -sign * z.x), mk3(b, flip ? 0.0f - k.yy : k.yy, -z.y), z};
}
f3 up_normal(f3 normal, f3 outgoing) { return jt::dot(normal, outgoing) <= 0 ? -normal : normal; }

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
bool same(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }
bool same(f3 a, f3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
bool same(const m3& a, const m3& b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }

long normals = 0, cases = 0, bad = 0, yy_zero = 0;

void report(const char* what, f3 n, f3 o) {
    if (bad++ < 10)
        std::fprintf(stderr, "shade_bake_check: %s: n = %a %a %a, o = %a %a %a\n", what, n.x, n.y, n.z, o.x, o.y, o.z);
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t next_u32() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
float uniform(float lo, float hi) { return lo + (hi - lo) * ((float)(next_u32() >> 8) * (1.0f / 16777216.0f)); }

void check(f3 n) {
    normals++;
    const f3 zero = mk3(0, 0, 0);
    const m3 p = basis_fromz(n), m = basis_fromz(-n);
    // (a)
    cases++;
    if (!same(m.x, p.x) || !same(m.z, -p.z) || !same(m.y.x, -p.y.x) || !same(m.y.z, -p.y.z) || !same(m.y.y, 0.0f - p.y.y))
        report("(a) basis_fromz(-n) is not (X, -Y, -Z) with Y.y' = 0 - Y.y", n, zero);
    if (!same(m.y.y, -p.y.y)) {  // the exception: a cancelled Y.y is +0 in both orientations
        yy_zero++;
        if (p.y.y != 0 || bits(p.y.y) != 0 || bits(m.y.y) != 0) report("(a) Y.y' != -Y.y away from Y.y = +0", n, zero);
    }
    // (b)
    const Baked k = bake(n);
    cases++;
    if (!same(basis_baked(k, false), p)) report("(b) the basis of n from the stored six", n, zero);
    if (!same(basis_baked(k, true), m)) report("(b) the basis of -n from the stored six", n, zero);
    // (c): random directions, directions at right angles to n (dot exactly +-0 or a rounding
    // residue of either sign), +-n itself and the zero vectors
    f3 os[12];
    int no = 0;
    for (int q = 0; q < 4; q++) os[no++] = mk3(uniform(-1, 1), uniform(-1, 1), uniform(-1, 1));
    os[no++] = mk3(n.y, -n.x, 0.0f);
    os[no++] = mk3(-n.y, n.x, -0.0f);
    os[no++] = mk3(0.0f, n.z, -n.y);
    os[no++] = jt::cross(n, os[0]);
    os[no++] = n;
    os[no++] = -n;
    os[no++] = zero;
    os[no++] = -zero;
    for (int q = 0; q < no; q++) {
        const f3 o = os[q];
        cases++;
        const bool flip1 = !(jt::dot(n, o) >= 0);  // eval_shading
        const f3 normal = flip1 ? -n : n;
        const bool flip2 = jt::dot(normal, o) <= 0;  // up_normal, as sample_bsdfcos calls it
        const f3 up = up_normal(normal, o);
        const bool flip = flip1 != flip2;
        if (!same(up, flip ? -n : n)) report("(c) up_normal of the oriented normal is not the XOR's orientation of n", n, o);
        if (!same(basis_baked(k, flip), basis_fromz(up))) report("(c) basis_baked(XOR) is not basis_fromz(up)", n, o);
    }
}

}  // namespace

int main() {
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f};
    for (float x : vals)
        for (float y : vals)
            for (float z : vals) check(mk3(x, y, z));
    const float dmin = std::numeric_limits<float>::denorm_min();
    const float tiny[] = {dmin, -dmin, 1e-40f, -1e-40f, std::numeric_limits<float>::min(), 0.0f, -0.0f, 1.0f, -1.0f};
    for (float x : tiny)
        for (float y : tiny)
            for (float z : tiny) check(mk3(x, y, z));
    for (int k = 0; k < 1200000; k++) {
        f3 n = mk3(uniform(-1, 1), uniform(-1, 1), uniform(-1, 1));
        const uint32_t r = next_u32();
        if ((r & 7u) != 0) n = jt::normalize(n);  // a stored element normal: normalised (twice, in the layout)
        if ((r & 8u) != 0) n = jt::normalize(n);
        // snap components to +-0: normals in a coordinate plane or along an axis, every zero sign
        if ((r & 0x30u) == 0x10u) n.z = (r & 0x40u) ? -0.0f : 0.0f;
        if ((r & 0x300u) == 0x100u) n.x = (r & 0x400u) ? -0.0f : 0.0f;
        if ((r & 0x3000u) == 0x1000u) n.y = (r & 0x4000u) ? -0.0f : 0.0f;
        if ((r & 0x30000u) == 0x10000u) n.z = (r & 0x40000u) ? -1.0f : 1.0f;
        check(n);
    }
    std::printf("shade_bake_check: %ld normals, %ld cases, %ld bad; Y.y cancelled to +0 in both orientations: %ld\n", normals,
                cases, bad, yy_zero);
    if (yy_zero == 0) {
        std::fprintf(stderr, "shade_bake_check: no normal with a cancelled Y.y was seen\n");
        return 1;
    }
    return bad ? 1 : 0;
}
