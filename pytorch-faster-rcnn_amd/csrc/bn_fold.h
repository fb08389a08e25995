// The frozen-BatchNorm epilogue arithmetic, once: every kernel that applies an eval-mode BN
// (frh_bn_act, frh_bn_act_maxpool, the 1x1 conv's epilogue and input side, the RoI conv's
// epilogue) folds and applies it through the functions below, so all of them round the same
// operations in the same order and give the bits of frh_bn_act.
//   y = act(x * s[c] + b[c] (+ skip)),  s = gamma / sqrt(var + eps),  b = beta - mean * s
// s and b come from the BN parameters inside the kernel (no host-side folding, so trainable
// gamma / beta stay live).
#pragma once
#include <math.h>

#include "common.h"

namespace frh {

// One BN's parameters as the entries receive them.  mean == nullptr: no BN; gamma / beta are
// each nullable (affine=False).
struct FrozenBN {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float eps;
};

#define FRH_REQUIRE_BN_PAIR(p) \
  FRH_REQUIRE(((p).mean == nullptr) == ((p).var == nullptr), "mean and var must both be given or both be NULL")

// channel c of p as y = x * s + b (p.mean given)
__device__ __forceinline__ void bn_fold(const FrozenBN& p, int c, float& s, float& b) {
  const float sc = (p.gamma ? p.gamma[c] : 1.0f) / sqrtf(p.var[c] + p.eps);
  s = sc;
  b = (p.beta ? p.beta[c] : 0.0f) - p.mean[c] * sc;
}

// v * s + b where there is a BN, + skip where there is one, max(., 0) where relu: in this order,
// one rounding each.  s, b and skip come by address and are read only where their flag is set:
// an entry called without a BN (or a skip) never filled them.
__device__ __forceinline__ float bn_apply(float v, bool bn, const float* s, const float* b, bool has_skip,
                                          const float* skip, bool relu) {
  if (bn) v = v * *s + *b;
  if (has_skip) v = v + *skip;
  if (relu) v = fmaxf(v, 0.0f);
  return v;
}

__device__ __forceinline__ float4 bn_apply(float4 v, bool bn, const float* sp, const float* bp, bool has_skip,
                                           const float4* skip, bool relu) {
  if (bn) {
    const float s = *sp, b = *bp;
    v = make_float4(v.x * s + b, v.y * s + b, v.z * s + b, v.w * s + b);
  }
  if (has_skip) v = make_float4(v.x + skip->x, v.y + skip->y, v.z + skip->z, v.w + skip->w);
  if (relu) v = make_float4(fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f), fmaxf(v.z, 0.0f), fmaxf(v.w, 0.0f));
  return v;
}

}  // namespace frh
