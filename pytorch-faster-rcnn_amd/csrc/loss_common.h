// Pieces the fused loss files share (losses.hip, gfl.hip, fcos.hip): the launch shape, the
// workspace layout behind frh_loss_workspace() with its size check and split, torch's
// BCE-with-logits / sigmoid forms, the focal element, the block sums, the arrival-counter fan-in
// and the status-word read.
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

// sigmoid_focal_loss element (losses.py:48-61) and its derivative (from losses.hip, shared with
// fcos.hip so both evaluate the same element).
__device__ __forceinline__ float focal_elem(float x, float t, float alpha, float gamma, float* dx) {
  float p = sigmoidf(x);
  float pt = p * t + (1.0f - p) * (1.0f - t);
  float at = alpha * t + (1.0f - alpha) * (1.0f - t);
  float q = 1.0f - pt;
  float qg = powf(q, gamma);
  float w = at * qg;
  float bce = bce_logits(x, t);
  if (dx) {
    // d/dx [bce * at * q^gamma] = (p - t) * w + bce * at * gamma * q^(gamma-1) * (-dpt/dx),
    // dpt/dx = p (1 - p) (2t - 1).  gamma == 0: q^0 is the constant 1 and the term is 0, as torch's
    // pow backward has it; gamma * q^(gamma-1) would be 0 * inf = NaN where q == 0 (|x| >= 17)
    float dq = gamma == 0.0f ? 0.0f : gamma * powf(q, gamma - 1.0f);
    float dpt = p * (1.0f - p) * (2.0f * t - 1.0f);
    *dx = (p - t) * w - bce * at * dq * dpt;
  }
  return bce * w;
}

// The arrival-counter fan-in of every fused forward, over N sums (MI355X_MICROARCH.md hand-off
// table, row 1: one signalling lane per workgroup, one unsharded counter, the last adder told by
// its add's return value).  Thread 0 holds the workgroup's partials p; every workgroup stores
// them write-through into slot blockIdx.x of its N arrays, drains and adds to the counter.  The
// workgroup whose add returns gridDim.x - 1 gets true (in all its threads) and, in res, sum q
// over the first nb[q] workgroups in a fixed order (double: one slot per thread, then a tree), so
// a call is deterministic.  Its thread 0 writes the outputs and then resets the counter.
// partial: kLossPartialArrays arrays of kMaxPartials floats, array q at q * kMaxPartials.
template <int N>
__device__ inline bool fan_in(const float (&p)[N], const int (&nb)[N], uint32_t* counter, float* partial,
                              double (&res)[N]) {
  static_assert(N <= kLossPartialArrays, "the workspace holds kLossPartialArrays partial arrays");
  __shared__ double s[kLossThreads];
  __shared__ int last;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q)
      __hip_atomic_store(partial + q * kMaxPartials + blockIdx.x, p[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return false;  // workgroup-uniform: the barriers below are reached by all threads or none
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const float* a = partial + q * kMaxPartials;
    double v = 0.0;
    for (int j = threadIdx.x; j < nb[q]; j += kLossThreads)
      v += (double)__hip_atomic_load(const_cast<float*>(a + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kLossThreads / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
      __syncthreads();
    }
    res[q] = s[0];
    __syncthreads();
  }
  return true;
}

// sum of an int over the workgroup, in thread 0 (from gfl.hip)
__device__ __forceinline__ int block_sum_i(int v, int* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  if (lane_id() == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
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

// Host side.  The forward grid: one workgroup per kLossThreads items, at least one, capped at the
// partial slots.
inline int loss_grid(int64_t work) {
  int64_t b = (work + kLossThreads - 1) / kLossThreads;
  if (b < 1) b = 1;
  return (int)(b < kMaxPartials ? b : kMaxPartials);
}

constexpr size_t kLossWorkspaceBytes = kCounterBytes + kLossPartialArrays * kMaxPartials * sizeof(float);

struct LossWorkspace {
  uint32_t* counter;  // zero between calls
  float* partial;
};

// the caller's workspace, checked and split; `what` names the loss in the message
inline int32_t split_workspace(void* workspace, size_t ws_bytes, const char* what, LossWorkspace* ws) {
  FRH_REQUIRE(workspace && ws_bytes >= kLossWorkspaceBytes, "%s: workspace too small", what);
  char* w = static_cast<char*>(workspace);
  *ws = LossWorkspace{reinterpret_cast<uint32_t*>(w), reinterpret_cast<float*>(w + kCounterBytes)};
  return FRH_OK;
}

}  // namespace frh
