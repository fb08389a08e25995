// Guided Anchoring targets: the location targets and the shape targets of a whole batch in one
// launch.
//
// Reference: GuidedAnchor.loc_target_single_image (lib/heads/guided_head.py:342-397) and the
// painting part of shape_target_single_image_v2 (:195-231), with paint_value / paint_bbox
// (:23-39) and region.inside_grid_mask (lib/region.py:10-16).
//
// The reference loops over the gts of every image and paints rectangles into per-level maps,
// building each rectangle on the host from device scalars: several launches and a host
// synchronisation per gt, three passes.  The rectangle of gt g at ratio r on a level of stride
// s is, all in f32,
//   w = (x2 - x1 + 1) * r, h likewise, cx = (x2 + x1) / 2, cy likewise,
//   (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2) * (1 / s), rounded half to even,
// and a cell (y, x) is painted when rx1 <= x <= rx2 and ry1 <= y <= ry2 (an inclusive slice;
// Python clips it to the grid).  The passes never read what they paint over, so per cell the
// result is a rule: ga_targets_kernel is one thread per (image, cell) over the level-concatenated
// cells, the image's boxes and levels staged in LDS a chunk at a time, in the shape of
// fcos_assign_kernel.  No workspace, no atomics.
//
//   loc:  1 if a gt of this level has its centre region over the cell (the third pass paints
//         last); else -1 if a gt with |lvl - l| <= 1 has its ignore region over it (second
//         pass); else 0 inside the image's part of the grid, -1 outside it (first pass).
//   shape_mask / shape_box: 1 and the box of the highest-index gt of this level whose
//         shape-centre region covers the cell (painted in index order, the last one stays);
//         0 and zeros elsewhere.
//
// Precondition: gt coordinates are >= 0.  A negative rounded edge is a negative slice index in
// the reference, which wraps around the map; that is not reproduced here (a negative edge
// simply lies left of / above every cell).  The host mirror raises on negative coordinates.
//
// Numerics: f32 in the reference's operation order (-ffp-contract=off): bit-exact.  The level of
// each gt is an input (the mirror computes region.map_gt2level with torch): log2 is kept out of
// a bit-exact kernel.
#include "ltrb_common.h"

namespace frh {
namespace {

constexpr int kGaThreads = 256;
constexpr int kGaChunk = 256;  // gts staged in LDS per pass

struct GaArgs {
  int B, Gmax;
  LevelTable lv;
  const float* gts;
  int64_t gseg;
  const int32_t* ngt;
  const int32_t* glvl;
  const int32_t* img_hw;
  float center_ratio, ignore_ratio, shape_ratio;
  int64_t* loc;
  int64_t* smask;
  float* sbox;
};

// whether the region of box q at `ratio`, scaled by sc = 1 / stride, covers cell (y, x)
__device__ __forceinline__ bool ga_covers(const float4 q, float ratio, float sc, int y, int x) {
  float w = (q.z - q.x) + 1.0f, h = (q.w - q.y) + 1.0f;
  w = w * ratio, h = h * ratio;
  const float cx = (q.z + q.x) / 2.0f, cy = (q.w + q.y) / 2.0f;
  const float x1 = rintf((cx - w / 2.0f) * sc), y1 = rintf((cy - h / 2.0f) * sc);
  const float x2 = rintf((cx + w / 2.0f) * sc), y2 = rintf((cy + h / 2.0f) * sc);
  const float fx = (float)x, fy = (float)y;  // grids are far below 2^24: exact
  return x1 <= fx && fx <= x2 && y1 <= fy && fy <= y2;
}

__global__ void __launch_bounds__(kGaThreads) ga_targets_kernel(GaArgs a) {
  __shared__ float4 s_box[kGaChunk];
  __shared__ int s_lvl[kGaChunk];
  const int b = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * kGaThreads + threadIdx.x;
  const bool live = c < a.lv.N;
  int y = 0, x = 0, l = 0;
  if (live) l = cell_yx(a.lv, c, &y, &x);
  const float s = a.lv.stride[l];
  const float sc = (float)(1.0 / (double)s);
  int G = a.ngt[b];
  G = G < 0 ? 0 : (G > a.Gmax ? a.Gmax : G);
  const float* gt = a.gts + (int64_t)b * a.gseg;
  bool pos = false, ign = false;
  int owner = -1;
  float4 obox = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int g0 = 0; g0 < G; g0 += kGaChunk) {  // block-uniform
    const int n = G - g0 < kGaChunk ? G - g0 : kGaChunk;
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const int g = g0 + threadIdx.x;
      s_box[threadIdx.x] = make_float4(gt[g], gt[(int64_t)a.Gmax + g], gt[2 * (int64_t)a.Gmax + g],
                                       gt[3 * (int64_t)a.Gmax + g]);
      s_lvl[threadIdx.x] = a.glvl[(int64_t)b * a.Gmax + g];
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < n; ++j) {
        const int d = s_lvl[j] - l;
        if (d < -1 || d > 1) continue;
        const float4 q = s_box[j];
        if (ga_covers(q, a.ignore_ratio, sc, y, x)) ign = true;
        if (d != 0) continue;
        if (ga_covers(q, a.center_ratio, sc, y, x)) pos = true;
        if (ga_covers(q, a.shape_ratio, sc, y, x)) owner = g0 + j, obox = q;  // the later index stays
      }
  }
  if (!live) return;
  // inside_grid_mask: the first int(img / stride) + 1 rows / columns of the grid
  const double r = 1.0 / (double)s;
  const int in_h = (int)((double)a.img_hw[2 * b] * r) + 1, in_w = (int)((double)a.img_hw[2 * b + 1] * r) + 1;
  const bool in = y < in_h && x < in_w;
  const int64_t o = (int64_t)b * a.lv.N + c;
  a.loc[o] = pos ? 1 : (ign ? -1 : (in ? 0 : -1));
  a.smask[o] = owner >= 0 ? 1 : 0;
  reinterpret_cast<float4*>(a.sbox)[o] = obox;
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" int32_t frh_ga_targets(int32_t batch, int32_t num_levels, const int32_t* grid_hw, const float* strides,
                                  const float* gts, int64_t gt_seg_stride, const int32_t* num_gts,
                                  const int32_t* gt_levels, int32_t max_gts, const int32_t* img_hw,
                                  float center_ratio, float ignore_ratio, float shape_center_ratio, int64_t* loc,
                                  int64_t* shape_mask, float* shape_box, void* stream) {
  FRH_REQUIRE(batch >= 0 && max_gts >= 0, "negative batch or max_gts");
  GaArgs a;
  const int32_t lst = set_levels(&a.lv, num_levels, grid_hw, strides);
  if (lst != FRH_OK) return lst;
  if (batch == 0) return FRH_OK;
  FRH_REQUIRE(batch <= 65535, "batch %d exceeds the grid's y extent", batch);
  FRH_REQUIRE(num_gts && img_hw && loc && shape_mask && shape_box, "null pointer argument");
  FRH_REQUIRE(max_gts == 0 || (gts && gt_levels), "null gt pointer");
  FRH_REQUIRE(max_gts == 0 || gt_seg_stride >= 4 * (int64_t)max_gts, "gt_seg_stride %lld < 4 * max_gts",
              (long long)gt_seg_stride);
  FRH_REQUIRE_ALIGNED16(shape_box);
  a.B = batch;
  a.Gmax = max_gts;
  a.gts = gts;
  a.gseg = gt_seg_stride;
  a.ngt = num_gts;
  a.glvl = gt_levels;
  a.img_hw = img_hw;
  a.center_ratio = center_ratio;
  a.ignore_ratio = ignore_ratio;
  a.shape_ratio = shape_center_ratio;
  a.loc = loc;
  a.smask = shape_mask;
  a.sbox = shape_box;
  hipLaunchKernelGGL(ga_targets_kernel, dim3((unsigned)((a.lv.N + kGaThreads - 1) / kGaThreads), (unsigned)batch),
                     dim3(kGaThreads), 0, as_stream(stream), a);
  return check_launch("frh_ga_targets");
}
