// frh_conv3x3_nchw_bn_act: the bottlenecks' 3x3 / stride-1 / padding-1 convolutions (conv2) on
// contiguous NCHW f32 as Winograd F(2x2, 3x3) on the f32 MFMA, with the frozen-BN (+ ReLU)
// epilogue on the accumulators (kernels: conv3x3_nchw_kernels.h).  Two launches: the weight
// transform into the caller's workspace, redone on every call (the entry keeps no state, so a
// replayed graph follows weights an optimizer updated in place), then the convolution.
#include "conv3x3_nchw_kernels.h"

using namespace frh;

extern "C" size_t frh_conv3x3_nchw_workspace(int32_t cin, int32_t cout) {
  return cin > 0 && cout > 0 ? (size_t)16 * cin * cout * sizeof(float) : 0;
}

extern "C" int32_t frh_conv3x3_nchw_bn_act(const float* x, const float* w, const float* gamma, const float* beta,
                                           const float* mean, const float* var, float eps, float* y,
                                           float* workspace, int64_t n, int32_t cin, int32_t cout, int32_t h,
                                           int32_t wd, int32_t relu, void* stream) {
  return conv3x3_nchw_launch("frh_conv3x3_nchw_bn_act", -1, x, w, y, {gamma, beta, mean, var, eps}, workspace, n, cin,
                             cout, h, wd, relu, stream);
}
