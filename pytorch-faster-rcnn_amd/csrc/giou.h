// giou_loss (reference lib/losses.py:13-30) of two boxes and its derivative with respect to one
// coordinate of the first, for the fused head losses (gfl.hip, fcos.hip).  Moved here from
// gfl.hip's eval_positive, statement for statement: no +1 widths, the intersection zeroed unless
// tl < br strictly on both axes, torch's tie subgradients of max / min (a half each).
#pragma once
#include "common.h"

namespace frh {

// derivative weights of torch.max / torch.min of two operands with respect to the first (ties: half)
__device__ __forceinline__ float dmax_a(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }
__device__ __forceinline__ float dmin_a(float a, float b) { return a < b ? 1.0f : (a == b ? 0.5f : 0.0f); }

__device__ __forceinline__ float sel4(int s, float v0, float v1, float v2, float v3) {
  return s == 0 ? v0 : (s == 1 ? v1 : (s == 2 ? v2 : v3));
}

struct Giou {
  float iou;   // plain IoU of the two boxes
  float loss;  // 1 - (iou - (area_c - area_u) / area_c)
  float iw, ih, msk, wa, ha, cw, ch, area_i, area_u, area_c;  // what the derivative reuses
};

// boxes a = (a0, a1, a2, a3) and b = (b0, b1, b2, b3) as (x1, y1, x2, y2)
__device__ __forceinline__ Giou giou_eval(float a0, float a1, float a2, float a3, float b0, float b1, float b2,
                                          float b3) {
  Giou r;
  const float tl0 = fmaxf(a0, b0), tl1 = fmaxf(a1, b1), br0 = fminf(a2, b2), br1 = fminf(a3, b3);
  r.iw = br0 - tl0;
  r.ih = br1 - tl1;
  r.msk = (tl0 < br0 && tl1 < br1) ? 1.0f : 0.0f;
  r.area_i = (r.iw * r.ih) * r.msk;
  r.wa = a2 - a0;
  r.ha = a3 - a1;
  const float area_a = r.wa * r.ha, area_b = (b2 - b0) * (b3 - b1);
  r.area_u = (area_a + area_b) - r.area_i;
  r.iou = r.area_i / r.area_u;
  r.cw = fmaxf(a2, b2) - fminf(a0, b0);
  r.ch = fmaxf(a3, b3) - fminf(a1, b1);
  r.area_c = r.cw * r.ch;
  r.loss = 1.0f - (r.iou - (r.area_c - r.area_u) / r.area_c);
  return r;
}

// d giou_loss / d a_side = -d iou - d (area_u / area_c)
__device__ __forceinline__ float giou_dside(const Giou& r, int side, float a0, float a1, float a2, float a3, float b0,
                                            float b1, float b2, float b3) {
  const float dA = sel4(side, -r.ha, -r.wa, r.ha, r.wa);
  const float dI = sel4(side, -(r.msk * r.ih) * dmax_a(a0, b0), -(r.msk * r.iw) * dmax_a(a1, b1),
                        (r.msk * r.ih) * dmin_a(a2, b2), (r.msk * r.iw) * dmin_a(a3, b3));
  const float dC = sel4(side, -r.ch * dmin_a(a0, b0), -r.cw * dmin_a(a1, b1), r.ch * dmax_a(a2, b2),
                        r.cw * dmax_a(a3, b3));
  const float dU = dA - dI;
  const float diou = (dI * r.area_u - r.area_i * dU) / (r.area_u * r.area_u);
  const float dratio = (dU * r.area_c - r.area_u * dC) / (r.area_c * r.area_c);
  return -diou - dratio;
}

}  // namespace frh
