// jt_denoise.h — the two denoisers' checks and launches, thin fronts of the one parameter check
// and the one launch loop in jt_denoise.hip; the kernels (demodulate_kernel<GUIDED>,
// atrous_kernel<GUIDED, LAST>), the host-array entries and the context's half (jt_denoise,
// jt_denoise_guided, jt_get_denoised) are there too. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_internal.h"

namespace jt {

// JT_ERR_INVALID naming the field, before any device work
int denoise_check_params(const jt_denoise_params* p);
int denoise_check_size(int32_t width, int32_t height);

// The filter of include/jtrace.h (jt_denoise) over device arrays of width * height float4:
// image RGBA, albedo and normal xyz (w ignored), two scratch buffers and the result. Every
// launch goes on `stream`, nothing waits: the caller synchronises. out may not alias an input.
hipError_t denoise_launch(hipStream_t stream, const float4* image, const float4* albedo, const float4* normal, int width,
                          int height, const jt_denoise_params& p, float4* ping, float4* pong, float4* out);

// The variance-guided filter (jt_denoise_guided): the same contract, with `variance` the
// variance of the mean per channel as jt_get_variance returns it (w ignored). Also refuses a
// sigma_variance^2 * variance_floor that underflows: every tap divides by at least that.
int denoise_guided_check_params(const jt_denoise_guided_params* p);
hipError_t denoise_guided_launch(hipStream_t stream, const float4* image, const float4* variance, const float4* albedo,
                                 const float4* normal, int width, int height, const jt_denoise_guided_params& p,
                                 float4* ping, float4* pong, float4* out);

}  // namespace jt
