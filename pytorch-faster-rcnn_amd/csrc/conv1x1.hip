// frh_conv1x1_bn_act: the bottleneck's 1x1 / stride-1 convolutions with the frozen-BN
// (+ residual) (+ ReLU) epilogue fused into the GEMM (kernel: conv1x1_kernels.h).  The raw conv output never goes to HBM, and the separate frh_bn_act
// launch that read it back is gone.
#include "conv1x1_kernels.h"

using namespace frh;

extern "C" int32_t frh_conv1x1_bn_act(const float* x, const float* w, const float* skip, float* y, const float* gamma,
                                      const float* beta, const float* mean, const float* var, float eps, int64_t n,
                                      int32_t cin, int32_t cout, int64_t hw, int32_t relu, void* stream) {
  return conv1x1_launch("frh_conv1x1_bn_act", conv1x1_pick_step(cin), x, w, skip, y, {gamma, beta, mean, var, eps}, n,
                        cin, cout, hw, relu, stream);
}

// frh_conv1x1_bn_act_pre: the same kernel with the BN (+ ReLU) that precedes the convolution
// applied to the X tile on its way into LDS (a bottleneck's bn2 in front of conv3): the
// frh_bn_act pass after the 3x3 conv is gone.
extern "C" int32_t frh_conv1x1_bn_act_pre(const float* x, const float* w, const float* skip, float* y,
                                          const float* gamma, const float* beta, const float* mean, const float* var,
                                          float eps, const float* pre_gamma, const float* pre_beta,
                                          const float* pre_mean, const float* pre_var, float pre_eps, int32_t pre_relu,
                                          int64_t n, int32_t cin, int32_t cout, int64_t hw, int32_t relu,
                                          void* stream) {
  FRH_REQUIRE(pre_mean && pre_var, "the input BN needs its mean and var");
  return conv1x1_launch("frh_conv1x1_bn_act_pre", conv1x1_pick_step(cin), x, w, skip, y,
                        {gamma, beta, mean, var, eps}, n, cin, cout, hw, relu, stream,
                        {pre_gamma, pre_beta, pre_mean, pre_var, pre_eps}, pre_relu);
}

// frh_conv1x1_s2_bn_act: the same kernel with its X tile gathered from x[:, :, ::2, ::2] (the
// stride-2 projections): no layout transposes around a GEMM, no separate frh_bn_act pass.
extern "C" int32_t frh_conv1x1_s2_bn_act(const float* x, const float* w, const float* skip, float* y,
                                         const float* gamma, const float* beta, const float* mean, const float* var,
                                         float eps, int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd,
                                         int32_t relu, void* stream) {
  FRH_REQUIRE(h >= 1 && wd >= 1, "bad sizes");
  FRH_REQUIRE(wd % 8 == 0, "input width %d must be a multiple of 8 (output width a multiple of 4)", wd);
  return conv1x1_launch("frh_conv1x1_s2_bn_act", conv1x1_pick_step(cin), x, w, skip, y,
                        {gamma, beta, mean, var, eps}, n, cin, cout, (int64_t)((h + 1) / 2) * (wd / 2), relu, stream,
                        /*pre=*/{}, /*pre_relu=*/0, /*in_h=*/h, /*in_w=*/wd);
}
