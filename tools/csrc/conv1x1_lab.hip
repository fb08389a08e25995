// TOOLS-ONLY: frh_conv1x1_bn_act with the cin step (16 or 32) chosen by the caller
// (tools/bench_conv1x1.py times both per shape to check the product's choice).
#include "conv1x1_kernels.h"
#include "frcnn_tools.h"

using namespace frh;

extern "C" int32_t frh_conv1x1_bn_act_step(int32_t step, const float* x, const float* w, const float* skip, float* y,
                                           const float* gamma, const float* beta, const float* mean, const float* var,
                                           float eps, int64_t n, int32_t cin, int32_t cout, int64_t hw, int32_t relu,
                                           void* stream) {
  return conv1x1_launch("frh_conv1x1_bn_act_step", step, x, w, skip, y, {gamma, beta, mean, var, eps}, n, cin, cout,
                        hw, relu, stream);
}
