// Pieces the two LTRB target assigners share (atss.hip, fcos.hip): the level table of the
// level-concatenated cells, the painted image area (paint_value, fcos_head.py:90-94), a cell's
// ltrb against a box (bbox2ltrb, :78-87) and the centerness of an ltrb (:56-59).  Moved here
// from atss.hip unchanged, so both assigners round exactly as the reference does.
#pragma once
#include <math.h>

#include "common.h"

namespace frh {

constexpr int kLtrbMaxLevels = 16;

// the members every assigner's argument struct starts its level table with
struct LevelTable {
  int L;
  int64_t N;                         // cells of all levels
  int64_t off[kLtrbMaxLevels + 1];   // first cell of level l
  int gh[kLtrbMaxLevels], gw[kLtrbMaxLevels];
  float stride[kLtrbMaxLevels];
};

// host: fill the table from grid_hw[2l..2l+1] = (H_l, W_l) and strides[l]
inline int32_t set_levels(LevelTable* t, int32_t num_levels, const int32_t* grid_hw, const float* strides) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kLtrbMaxLevels, "num_levels %d not in [1, %d]", num_levels,
              kLtrbMaxLevels);
  FRH_REQUIRE(grid_hw && strides, "null host array");
  t->L = num_levels;
  int64_t n = 0;
  for (int l = 0; l < num_levels; ++l) {
    FRH_REQUIRE(grid_hw[2 * l] >= 1 && grid_hw[2 * l + 1] >= 1, "empty grid at level %d", l);
    FRH_REQUIRE(strides[l] > 0.0f, "stride must be positive");
    t->off[l] = n;
    t->gh[l] = grid_hw[2 * l];
    t->gw[l] = grid_hw[2 * l + 1];
    t->stride[l] = strides[l];
    n += (int64_t)t->gh[l] * t->gw[l];
  }
  t->off[num_levels] = n;
  FRH_REQUIRE(n < ((int64_t)1 << 31), "too many cells");
  t->N = n;
  return FRH_OK;
}

__device__ __forceinline__ int level_of(const LevelTable& t, int64_t c) {
  int l = 0;
  while (l + 1 < t.L && c >= t.off[l + 1]) ++l;
  return l;
}

// cell c of the concatenation -> its level and (y, x) there
__device__ __forceinline__ int cell_yx(const LevelTable& t, int64_t c, int* y, int* x) {
  const int l = level_of(t, c);
  const int64_t i = c - t.off[l];
  *y = (int)(i / t.gw[l]);
  *x = (int)(i - (int64_t)*y * t.gw[l]);
  return l;
}

// paint_value: [0, 0, img_w, img_h] * (1 / stride) in f32, round half-even, inclusive slice
// (Python slicing clips it to the grid)
__device__ __forceinline__ bool painted(const int32_t* img_hw, int b, float stride, int y, int x) {
  const float sc = (float)(1.0 / (double)stride);
  const int x2 = (int)rintf((float)img_hw[2 * b + 1] * sc), y2 = (int)rintf((float)img_hw[2 * b] * sc);
  return y <= y2 && x <= x2;
}

// bbox2ltrb at one cell: distances of the cell centre to the sides of bx = (x1, y1, x2, y2)
__device__ __forceinline__ void center_ltrb(float s, int y, int x, const float* bx, float* lt) {
  const float cx = (float)x * s + s / 2.0f, cy = (float)y * s + s / 2.0f;
  lt[0] = cx - bx[0];
  lt[1] = cy - bx[1];
  lt[2] = bx[2] - cx;
  lt[3] = bx[3] - cy;
}

// centerness on ltrb + 1e-6
__device__ __forceinline__ float ltrb_centerness(const float* lt) {
  const float l = lt[0] + 1e-6f, t = lt[1] + 1e-6f, r = lt[2] + 1e-6f, bb = lt[3] + 1e-6f;
  return sqrtf((fminf(l, r) / fmaxf(l, r)) * (fminf(t, bb) / fmaxf(t, bb)));
}

}  // namespace frh
