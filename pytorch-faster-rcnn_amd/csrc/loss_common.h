// Pieces the fused loss files share (losses.hip, gfl.hip): the launch shape, the workspace
// layout behind frh_loss_workspace(), torch's BCE-with-logits / sigmoid forms, the block sum and
// the status-word read.  Moved here from losses.hip unchanged.
#pragma once
#include "common.h"

#include <math.h>

namespace frh {

constexpr int kLossThreads = 256;
constexpr int kMaxPartials = 256;        // forward grid cap = partial slots
constexpr int kCounterBytes = 256;       // arrival counter block at the workspace start
constexpr int kLossPartialArrays = 4;    // [kMaxPartials] f32 arrays behind the counter block

// torch: binary_cross_entropy_with_logits = (1 - t) * x - log_sigmoid(x),
// log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|)).
__device__ __forceinline__ float bce_logits(float x, float t) {
  float ls = fminf(x, 0.0f) - log1pf(expf(-fabsf(x)));
  return (1.0f - t) * x - ls;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float block_sum_f(float v, float* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  const int w = threadIdx.x >> 6;
  if (lane_id() == 0) scratch[w] = v;
  __syncthreads();
  float t = 0.0f;
  if (threadIdx.x == 0)
    for (int j = 0; j < kLossThreads / kWave; ++j) t += scratch[j];
  return t;
}

// A nonzero device status word (an in-launch wait of an earlier one-launch kernel ran out,
// include/frcnn_amd.h FRH_DEVERR_*) makes the loss NaN: the outputs it was computed from are
// undefined, and the step's own loss read carries the failure without an extra host sync.
__device__ __forceinline__ bool status_set(const int32_t* status) {
  return status && __hip_atomic_load(const_cast<int32_t*>(status), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

}  // namespace frh
