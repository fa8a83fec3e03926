// jt_accum.h — the kernels that turn stream means into the running means, for the device context
// (jt_trace.hip): the combine of a context's k > 1 streams and the chain of a one-stream context's
// chunk. The kernels are in jt_accum.hip. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "jt_launch.h"

namespace jt {

// Both enqueue one launch over the slots of P's tiles on `stream` (none for a launch without
// tiles); nothing waits, the caller synchronises.
// aov false: the image; true: albedo, normal and hits
hipError_t combine_launch(hipStream_t stream, const jtd::DParams& P, const jtk::DAccum& A, const jtk::DCombine& cw, bool aov);
// folds the m one-sample streams of A's stream means into the running means that hold n0 samples
hipError_t chain_launch(hipStream_t stream, const jtd::DParams& P, const jtk::DAccum& A, int n0, int m);

}  // namespace jt
