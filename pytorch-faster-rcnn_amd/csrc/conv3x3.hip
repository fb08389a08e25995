// frh_conv3x3_bias_act, frh_conv3x3_bias_act_levels, frh_conv3x3_bias_act_pool: the FPN output
// convs, the RPN head's shared conv and VGG16's convs (3x3 / stride 1 / padding 1, channels-last
// f32; _pool with the 2x2 max pool that follows in its epilogue) as Winograd F(2x2, 3x3) on the
// f32 MFMA with the bias (+ ReLU) epilogue on the accumulators (kernels:
// conv3x3_wino_kernels.h).  The _levels form runs every pyramid level in one launch, with
// shared (RPN head) or per-level (FPN) weights: the small levels alone have far fewer
// workgroups than the chip has CUs.
#include "conv3x3_wino_kernels.h"

using namespace frh;

extern "C" size_t frh_conv3x3_workspace(int32_t cin, int32_t cout) {
  return cin > 0 && cout > 0 ? (size_t)16 * cin * cout * sizeof(float) : 0;
}

extern "C" int32_t frh_conv3x3_bias_act(const float* x, const float* w, const float* bias, float* y, float* workspace,
                                        int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd, int64_t sn,
                                        int64_t sy, int64_t sx, int32_t relu, void* stream) {
  const Conv3x3LevelDesc d = {x, w, bias, y, h, wd, sn, sy, sx};
  return conv3x3_launch("frh_conv3x3_bias_act", 1, &d, workspace, (int64_t)16 * cin * cout, n, cin, cout, relu,
                        stream);
}

// The VGG16 layers ahead of a max pool: the same launch with the pooled epilogue, y
// [n, h / 2, wd / 2, cout].
extern "C" int32_t frh_conv3x3_bias_act_pool(const float* x, const float* w, const float* bias, float* y,
                                             float* workspace, int64_t n, int32_t cin, int32_t cout, int32_t h,
                                             int32_t wd, int64_t sn, int64_t sy, int64_t sx, int32_t relu,
                                             void* stream) {
  const Conv3x3LevelDesc d = {x, w, bias, y, h, wd, sn, sy, sx};
  return conv3x3_launch<true>("frh_conv3x3_bias_act_pool", 1, &d, workspace, (int64_t)16 * cin * cout, n, cin, cout,
                              relu, stream);
}

extern "C" int32_t frh_conv3x3_bias_act_levels(int32_t num_levels, const void* const* xs, const void* const* weights,
                                               const void* const* biases, void* const* ys, float* workspace,
                                               size_t workspace_bytes, int64_t n, int32_t cin, int32_t cout,
                                               const int32_t* level_hw, const int64_t* level_strides, int32_t relu,
                                               void* stream) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kWgMaxLevels, "1 to %d levels, got %d", kWgMaxLevels, num_levels);
  FRH_REQUIRE(xs && weights && biases && ys && level_hw && level_strides, "null pointer argument");
  Conv3x3LevelDesc d[kWgMaxLevels];
  for (int i = 0; i < num_levels; ++i)
    d[i] = {static_cast<const float*>(xs[i]),
            static_cast<const float*>(weights[i]),
            static_cast<const float*>(biases[i]),
            static_cast<float*>(ys[i]),
            level_hw[2 * i],
            level_hw[2 * i + 1],
            level_strides[3 * i],
            level_strides[3 * i + 1],
            level_strides[3 * i + 2]};
  return conv3x3_launch("frh_conv3x3_bias_act_levels", num_levels, d, workspace,
                        (int64_t)(workspace_bytes / sizeof(float)), n, cin, cout, relu, stream);
}
