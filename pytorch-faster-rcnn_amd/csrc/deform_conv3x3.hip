// frh_deform_conv3x3_act, frh_deform_conv3x3_act_levels: the Guided Anchoring adaption layer
// (reference lib/heads/guided_head.py:92-96,404-405: offset_layer, a 1x1 conv without bias on the
// detached shape map, then DeformConv(cin, cout, 3, padding=1, deformable_groups) and ReLU) as a
// gather-fed implicit GEMM on the f32 MFMA (kernels: deform_conv3x3_kernels.h).  offset_w ==
// NULL: `offset` is the explicit [n, 18 dg, h, w] map; otherwise `offset` is the 2-channel shape
// map and offset_w the offset layer's weight, and the offsets are formed in registers.  The
// weight repack into the workspace is the call's first launch and is redone on every call: no
// state is kept between calls.
#include "deform_conv3x3_kernels.h"

using namespace frh;

extern "C" size_t frh_deform_conv3x3_workspace(int32_t cin, int32_t cout) {
  return cin > 0 && cout > 0 ? (size_t)9 * cin * cout * sizeof(float) : 0;
}

extern "C" int32_t frh_deform_conv3x3_act(const float* x, const float* offset, const float* offset_w, const float* w,
                                          float* y, float* workspace, int64_t n, int32_t cin, int32_t cout,
                                          int32_t dg, int32_t h, int32_t wd, int64_t sn, int64_t sy, int64_t sx,
                                          const int64_t* offset_strides, int32_t relu, void* stream) {
  FRH_REQUIRE(offset_strides, "null pointer argument");
  const DeformConvLevelDesc d = {x, offset, y, h, wd, sn, sy, sx, offset_strides[0], offset_strides[1],
                                 offset_strides[2], offset_strides[3]};
  return deform_conv3x3_launch("frh_deform_conv3x3_act", 1, &d, offset_w, w, workspace, n, cin, cout, dg, relu,
                               stream);
}

extern "C" int32_t frh_deform_conv3x3_act_levels(int32_t num_levels, const void* const* xs,
                                                 const void* const* offsets, const float* offset_w, const float* w,
                                                 void* const* ys, float* workspace, int64_t n, int32_t cin,
                                                 int32_t cout, int32_t dg, const int32_t* level_hw,
                                                 const int64_t* level_strides, const int64_t* offset_strides,
                                                 int32_t relu, void* stream) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kDcMaxLevels, "1 to %d levels, got %d", kDcMaxLevels, num_levels);
  FRH_REQUIRE(xs && offsets && ys && level_hw && level_strides && offset_strides, "null pointer argument");
  DeformConvLevelDesc d[kDcMaxLevels];
  for (int i = 0; i < num_levels; ++i)
    d[i] = {static_cast<const float*>(xs[i]),
            static_cast<const float*>(offsets[i]),
            static_cast<float*>(ys[i]),
            level_hw[2 * i],
            level_hw[2 * i + 1],
            level_strides[3 * i],
            level_strides[3 * i + 1],
            level_strides[3 * i + 2],
            offset_strides[4 * i],
            offset_strides[4 * i + 1],
            offset_strides[4 * i + 2],
            offset_strides[4 * i + 3]};
  return deform_conv3x3_launch("frh_deform_conv3x3_act_levels", num_levels, d, offset_w, w, workspace, n, cin, cout,
                               dg, relu, stream);
}
