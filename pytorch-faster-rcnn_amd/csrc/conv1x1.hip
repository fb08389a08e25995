// frh_conv1x1_bn_act: the bottleneck's 1x1 / stride-1 convolutions with the frozen-BN
// (+ residual) (+ ReLU) epilogue fused into the GEMM (kernel: conv1x1_kernels.h).  The raw conv output never goes to HBM, and the separate frh_bn_act
// launch that read it back is gone.
#include "conv1x1_kernels.h"

using namespace frh;

extern "C" int32_t frh_conv1x1_bn_act(const float* x, const float* w, const float* skip, float* y, const float* gamma,
                                      const float* beta, const float* mean, const float* var, float eps, int64_t n,
                                      int32_t cin, int32_t cout, int64_t hw, int32_t relu, void* stream) {
  return conv1x1_launch(conv1x1_pick_step(cin), x, w, skip, y, gamma, beta, mean, var, eps, n, cin, cout, hw, relu,
                        stream);
}
