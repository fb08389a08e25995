// TOOLS-ONLY: frh_conv3x3_nchw_bn_act with the kernel form (0 .. 2: (NT, NC) = (2, 1), (1, 2),
// (1, 1)) chosen by the caller (tools/bench_conv3x3_nchw.py times every form per class to
// fill the product's table; tests/test_gpu_conv3x3_nchw.py reaches every form with it).
#include "conv3x3_nchw_kernels.h"
#include "frcnn_tools.h"

using namespace frh;

extern "C" int32_t frh_conv3x3_nchw_bn_act_form(int32_t form, const float* x, const float* w, const float* gamma,
                                                const float* beta, const float* mean, const float* var, float eps,
                                                float* y, float* workspace, int64_t n, int32_t cin, int32_t cout,
                                                int32_t h, int32_t wd, int32_t relu, void* stream) {
  FRH_REQUIRE(form >= 0, "form %d: 0 to %d", form, kNwForms - 1);
  return conv3x3_nchw_launch("frh_conv3x3_nchw_bn_act_form", form, x, w, y, {gamma, beta, mean, var, eps}, workspace,
                             n, cin, cout, h, wd, relu, stream);
}
