// jt_sample_ray.h — a sample's ray of the calls on the caller's own records: the one arm
// radiance_kernel, hemisphere_kernel and sphere_kernel (jt_radiance.hip) and occlusion_kernel
// (jt_intersect.hip) share, so the stream and the two draws of jt_irradiance, jt_hemisphere_rays,
// jt_ambient_occlusion, jt_probe_sh and jt_sphere_rays cannot drift apart. A per-lane device function.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_bsdf.h"
#include "jt_radiance.h"

namespace jtk {
using namespace jtd;

// The stream of (record, sample), the sample prologue's four draws, which a camera would have used
// for the image and the lens position, and (o, d) from record `rec` of `recs`, whose stride is the
// source's (jtr::source_stride). SOURCE_RAY: the record is the ray and the draws are discarded.
// SOURCE_HEMISPHERE: the record is (position, normal); o is the position as given and d the matte
// lobe's own cosine-weighted direction about the normal (sample_hemisphere_cos, jt_bsdf.h) for the
// first draw, the second discarded. SOURCE_SPHERE: the record is the position alone; o is the
// position as given and d the uniform draw over the sphere (sample_sphere, jt_bsdf.h) for the first
// draw, the second discarded. Either way the stream is left after the prologue, where
// trace_sample's path begins.
template <int SOURCE>
__device__ __forceinline__ void radiance_ray(const DParams& P, const float* recs, long long stream_base, int rec, int sample, Rng& rng,
                                             v3& o, v3& d) {
    rng = rng_init(P.seed, (int)(stream_base + rec), sample);  // < 2^31: RADIANCE_MAX_STREAM
    const v2 ruv = rand2f(rng);
    (void)rand2f(rng);
    const float* const r = recs + (size_t)rec * jtr::source_stride(SOURCE);
    o = V3(r[0], r[1], r[2]);
    if constexpr (SOURCE == jtr::SOURCE_SPHERE) {
        d = sample_sphere(ruv);
    } else {
        d = V3(r[3], r[4], r[5]);
        if constexpr (SOURCE == jtr::SOURCE_HEMISPHERE) d = sample_hemisphere_cos(d, ruv);
    }
}

}  // namespace jtk
