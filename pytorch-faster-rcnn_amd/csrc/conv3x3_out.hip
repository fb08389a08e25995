// frh_conv3x3_out_levels: the prediction convs of a one-stage head (RetinaHead's retina_cls /
// retina_reg, FCOSHead's fcos_cls / fcos_reg / fcos_center: 3x3 / stride 1 / padding 1 with 1 to
// 192 output channels) over every pyramid level in one launch (kernel: conv3x3_out_kernels.h).
// Two convs that read the same tower share the launch, so each level is read once for both;
// the bias, the per-level scale and the exp are applied on the accumulators.
#include "conv3x3_out_kernels.h"

using namespace frh;

extern "C" int32_t frh_conv3x3_out_levels(int32_t num_levels, const void* const* xs, void* const* ys0,
                                          void* const* ys1, const float* w0, const float* b0, const float* w1,
                                          const float* b1, const void* const* scales0, const void* const* scales1,
                                          int32_t exp0, int32_t exp1, int64_t n, int32_t cin, int32_t c0, int32_t c1,
                                          const int32_t* level_hw, const int64_t* level_strides, void* stream) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kCoMaxLevels, "1 to %d levels, got %d", kCoMaxLevels, num_levels);
  FRH_REQUIRE(xs && ys0 && (c1 == 0 || ys1) && level_hw && level_strides, "null pointer argument");
  ConvOutLevelDesc d[kCoMaxLevels];
  for (int i = 0; i < num_levels; ++i)
    d[i] = {static_cast<const float*>(xs[i]),
            static_cast<float*>(ys0[i]),
            c1 != 0 ? static_cast<float*>(ys1[i]) : nullptr,
            scales0 ? static_cast<const float*>(scales0[i]) : nullptr,
            scales1 && c1 != 0 ? static_cast<const float*>(scales1[i]) : nullptr,
            level_hw[2 * i],
            level_hw[2 * i + 1],
            level_strides[3 * i],
            level_strides[3 * i + 1],
            level_strides[3 * i + 2]};
  return conv3x3_out_launch(num_levels, d, w0, b0, w1, b1, exp0, exp1, n, cin, c0, c1, stream);
}
