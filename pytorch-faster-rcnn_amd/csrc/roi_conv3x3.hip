// frh_roi_conv3x3_bn_act: the Double-Head regression branch's 3x3 / stride-1 / padding-1 conv
// over every RoI's 7 x 7 tile (reference lib/heads/double_head.py:63-76,119-122), NCHW f32 in
// and out, with the eval-mode BN (+ ReLU) epilogue fused into the GEMM on the f32 MFMA (kernels:
// roi_conv3x3_kernels.h).  The weight repack into the workspace is the call's first launch and
// is redone on every call: no state is kept between calls.
#include "roi_conv3x3_kernels.h"

using namespace frh;

extern "C" size_t frh_roi_conv3x3_workspace(int32_t cin, int32_t cout) {
  return cin > 0 && cout > 0 ? (size_t)9 * cin * cout * sizeof(float) : 0;
}

extern "C" int32_t frh_roi_conv3x3_bn_act(const float* x, const float* w, float* y, const float* gamma,
                                          const float* beta, const float* mean, const float* var, float eps,
                                          int64_t r, int32_t cin, int32_t cout, int32_t relu, float* workspace,
                                          void* stream) {
  return roi_conv3x3_launch(x, w, y, {gamma, beta, mean, var, eps}, r, cin, cout, relu, workspace, stream);
}
