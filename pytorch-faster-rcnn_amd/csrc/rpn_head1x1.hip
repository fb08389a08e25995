// frh_rpn_head1x1_levels: the RPN head's classifier and regressor (two 1x1 convolutions with
// 3 and 12 output channels in cfg2) over every pyramid level in one launch (kernel:
// rpn_head1x1_kernels.h).  The hidden levels are read once for both convolutions, the bias is
// added on the accumulator, and nothing is split over cin: ten GEMM-shaped launches, their bias
// passes and their output clears are gone.
#include "rpn_head1x1_kernels.h"

using namespace frh;

extern "C" int32_t frh_rpn_head1x1_levels(int32_t num_levels, const void* const* xs, void* const* cls_outs,
                                          void* const* reg_outs, const float* w_cls, const float* b_cls,
                                          const float* w_reg, const float* b_reg, int64_t n, int32_t cin,
                                          int32_t c_cls, int32_t c_reg, const int32_t* level_hw,
                                          const int64_t* level_strides, void* stream) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kRhMaxLevels, "1 to %d levels, got %d", kRhMaxLevels, num_levels);
  FRH_REQUIRE(xs && cls_outs && reg_outs && level_hw && level_strides, "null pointer argument");
  RpnHeadLevelDesc d[kRhMaxLevels];
  for (int i = 0; i < num_levels; ++i)
    d[i] = {static_cast<const float*>(xs[i]),
            static_cast<float*>(cls_outs[i]),
            static_cast<float*>(reg_outs[i]),
            level_hw[2 * i],
            level_hw[2 * i + 1],
            level_strides[3 * i],
            level_strides[3 * i + 1],
            level_strides[3 * i + 2]};
  return rpn_head1x1_launch(num_levels, d, w_cls, b_cls, w_reg, b_reg, n, cin, c_cls, c_reg, stream);
}
