// frh_deform_conv3x3_bwd: the backward of frh_deform_conv3x3_act for one level (kernels and
// their structure: deform_conv3x3_bwd_kernels.h).  Up to four launches, each skipped when its
// outputs are not wanted: the weight repack and the data launch (gx, goff), the weight launch
// into per-split slabs and the slab reduce (gw).  Workspace: the repacked weight, then the slabs.
#include "deform_conv3x3_bwd_kernels.h"

using namespace frh;

extern "C" size_t frh_deform_conv3x3_bwd_workspace(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd) {
  if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return 0;
  const int64_t tiles = (n * h * wd + kDcbCols - 1) / kDcbCols;
  return (size_t)(1 + dcb_splits(tiles)) * 9 * cin * cout * sizeof(float);
}

extern "C" int32_t frh_deform_conv3x3_bwd(const float* x, const float* offset, const float* offset_w, const float* w,
                                          const float* y, const float* gy, float* gx, float* goff, float* gw,
                                          float* workspace, int64_t n, int32_t cin, int32_t cout, int32_t dg,
                                          int32_t h, int32_t wd, int64_t sn, int64_t sy, int64_t sx,
                                          const int64_t* offset_strides, void* stream) {
  const char* const what = "frh_deform_conv3x3_bwd";
  FRH_REQUIRE(offset_strides, "null pointer argument");
  FRH_REQUIRE(n >= 0 && cin >= 1 && cout >= 1 && dg >= 1, "bad sizes");
  FRH_REQUIRE(cin % 16 == 0 && cout % 64 == 0, "cin %d must be a multiple of 16 and cout %d of 64", cin, cout);
  FRH_REQUIRE(cin % dg == 0 && (cin / dg) % 4 == 0, "cin / deformable_groups must be a multiple of 4 (cin %d, dg %d)",
              cin, dg);
  if (n == 0 || (!gx && !goff && !gw)) return FRH_OK;
  FRH_REQUIRE(x && offset && w && gy && workspace, "null pointer argument");
  FRH_REQUIRE(h >= 1 && wd >= 1, "empty map");
  FRH_REQUIRE_ALIGNED16(x, w, workspace, offset_w, y, gy, gx, gw);
  FRH_REQUIRE(sn >= 0 && sy >= 0 && sx >= cin && (sn | sy | sx) % 4 == 0,
              "x strides must be non-negative multiples of 4, the column stride >= cin");
  const int64_t xe = (n - 1) * sn + (h - 1) * sy + (wd - 1) * sx + cin;
  const int64_t P = n * h * wd;
  if (P >= ((int64_t)1 << 31) || xe >= ((int64_t)1 << 40)) {
    set_error("%s: the level is too large", what);
    return FRH_EUNSUPPORTED;
  }
  if (cout > kDcbMaxCout) {
    set_error("%s: cout %d above %d is not implemented", what, cout, kDcbMaxCout);
    return FRH_EUNSUPPORTED;
  }
  const int64_t tiles = (P + kDcbCols - 1) / kDcbCols;
  const int splits = dcb_splits(tiles);
  const int64_t welems = (int64_t)cin * cout * 9;
  const int64_t wb = welems * 4, wsb = wb * (1 + splits), xb = xe * 4, yb = P * cout * 4;
  const int och = offset_w ? 2 : 18 * dg;
  // the byte range the offsets span, for any (signed) strides
  int64_t olo = 0, ohi = 0;
  const int64_t ext[4] = {(n - 1) * offset_strides[0], (och - 1) * offset_strides[1], (h - 1) * offset_strides[2],
                          (wd - 1) * offset_strides[3]};
  for (int e = 0; e < 4; ++e) (ext[e] < 0 ? olo : ohi) += ext[e];
  const void* const in_p[6] = {x, offset + olo, w, gy, y, offset_w};
  const int64_t in_b[6] = {xb, (ohi - olo + 1) * 4, wb, yb, yb, (int64_t)36 * dg * 4};
  const void* const out_p[4] = {gx, goff, gw, workspace};
  const int64_t out_b[4] = {P * cin * 4, P * 18 * dg * 4, wb, wsb};
  for (int o = 0; o < 4; ++o) {
    if (!out_p[o]) continue;
    for (int i = 0; i < 6; ++i)
      FRH_REQUIRE(!in_p[i] || !ranges_overlap(out_p[o], out_b[o], in_p[i], in_b[i]),
                  "gx, goff, gw and the workspace must not overlap an input");
    for (int k = o + 1; k < 4; ++k)
      FRH_REQUIRE(!out_p[k] || !ranges_overlap(out_p[o], out_b[o], out_p[k], out_b[k]),
                  "gx, goff, gw and the workspace must not overlap each other");
  }

  DcbArgs a;
  a.x = x, a.off = offset, a.ow = offset_w, a.wp = workspace, a.y = y, a.gy = gy;
  a.gx = gx, a.goff = goff, a.slab = workspace + welems;
  a.h = h, a.w = wd, a.sn = sn, a.sy = sy, a.sx = sx;
  a.on = offset_strides[0], a.oc = offset_strides[1], a.oy = offset_strides[2], a.ox = offset_strides[3];
  a.P = P, a.cin = cin, a.cout = cout, a.cpg = cin / dg, a.dg = dg;
  a.tiles = (int)tiles, a.tiles_per_split = dcb_tiles_per_split(tiles);
  hipStream_t s = as_stream(stream);
  const dim3 b(kDcbThreads);
  if (gx || goff) {
    const unsigned rp_blocks = (unsigned)((welems + 255) / 256 < 4096 ? (welems + 255) / 256 : 4096);
    hipLaunchKernelGGL(deform_conv3x3_bwd_repack_kernel, dim3(rp_blocks), dim3(256), 0, s, w, workspace, (int)cin,
                       (int)cout);
    const dim3 g((unsigned)tiles);
    const size_t lds = (size_t)kDcbCols * cout * sizeof(float);  // at most 64 KiB
    if (offset_w)
      hipLaunchKernelGGL((deform_conv3x3_bwd_data_kernel<true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((deform_conv3x3_bwd_data_kernel<false>), g, b, lds, s, a);
  }
  if (gw) {
    const dim3 g((unsigned)(9 * (cin / kDcbKc) * splits));
#define FRH_DCB_WEIGHT(RT_)                                                                    \
  do {                                                                                         \
    if (offset_w)                                                                              \
      hipLaunchKernelGGL((deform_conv3x3_bwd_weight_kernel<RT_, true>), g, b, 0, s, a);        \
    else                                                                                       \
      hipLaunchKernelGGL((deform_conv3x3_bwd_weight_kernel<RT_, false>), g, b, 0, s, a);       \
  } while (0)
    switch (cout / 64) {
      case 1: FRH_DCB_WEIGHT(1); break;
      case 2: FRH_DCB_WEIGHT(2); break;
      case 3: FRH_DCB_WEIGHT(3); break;
      default: FRH_DCB_WEIGHT(4); break;
    }
#undef FRH_DCB_WEIGHT
    const unsigned rd_blocks = (unsigned)((welems + 255) / 256 < 4096 ? (welems + 255) / 256 : 4096);
    hipLaunchKernelGGL(deform_conv3x3_bwd_reduce_kernel, dim3(rd_blocks), dim3(256), 0, s, a.slab, gw, welems, splits);
  }
  return check_launch(what);
}
