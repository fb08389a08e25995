// TOOLS-ONLY RoIAlign laboratory (see frcnn_tools.h).  The product kernels (csrc/roi_kernels.h)
// are frozen to their shipped forms; a variant here is either one of them at another value of its
// surviving knobs (slab size, waves per SIMD, waves per workgroup, stamped build) or a kernel
// measured and not adopted (roi_lab_kernels.h).  Variants whose knob was frozen are retired: the
// number stays reserved (roi_align.hip and profiles/ cite it) and the call fails.
//
// Forward variants (frh_roi_align_fwd_variant):
//   0 / 1    the pair kernel as dispatched / its stamped build
//   2-7      lab kernel roi_align_fwd_nhwc_kernel: 56 / 64 / 96 slab cells, 5 outputs in LDS,
//            6 stamped, 7 128 cells
//   8-11     quad kernel: 8 and 10 as dispatched (3 waves per SIMD), 9 stamped, 11 5 waves per SIMD
//   19       lab kernel roi_align_fwd_quad4_kernel (RoI setup shared by a 4-wave workgroup)
//   23 / 24  lab kernel roi_align_fwd_quadp_kernel (software-pipelined persistent), 8 / 12 waves per CU
//   25       quad kernel with a 16-KB slab
//   65 / 68  band kernel as dispatched / its stamped build
//   89       channel-group kernel as dispatched (4 waves, 120 cells, 5 waves per SIMD); 94 stamped
//   90       4 waves, 144 cells, registers as compiled; 91 8 waves, 120 cells; 95 124 cells
//   96-99    lab kernel roi_align_fwd_cgp_kernel (software-pipelined items): 2 / 3 / 4 items at
//            144 cells; 99: 2 at 116 cells
// Retired: 12-18, 20, 26-64, 66, 67, 80-88, 92, 93.
#include "frcnn_tools.h"
#include "roi_kernels.h"
#include "roi_lab_kernels.h"

using namespace frh;

extern "C" size_t frh_roi_align_workspace(int64_t num_rois) { return (size_t)(num_rois > 0 ? num_rois : 1) * 64; }

static bool fwd_variant_retired(int v) {
  return (v >= 12 && v <= 18) || v == 20 || (v >= 26 && v <= 64) || v == 66 || v == 67 || (v >= 80 && v <= 88) ||
         v == 92 || v == 93;
}

extern "C" int32_t frh_roi_align_fwd_variant(int32_t variant, int32_t num_levels, const float* const* feats,
                                             const int32_t* feat_hw, const int64_t* strides, const float* scales,
                                             int32_t batch, int32_t channels, const float* rois,
                                             const int64_t* roi_levels, int64_t num_rois, int32_t pooled_h,
                                             int32_t pooled_w, int32_t sampling_ratio, int32_t aligned, float* out,
                                             void* workspace, size_t ws_bytes, void* stream) {
  FRH_REQUIRE(!fwd_variant_retired(variant),
              "roi_align variant %d retired: its kernel parameter is frozen to the shipped value (last built at commit "
              "d6bef71)", variant);
  int32_t r = roi_common_checks(batch, channels, num_rois, pooled_h, pooled_w, rois);
  if (r) return r;
  FRH_REQUIRE((feats && out) || num_rois == 0, "null pointer argument");
  RoiLevels lv;
  r = make_levels(num_levels, feats, nullptr, feat_hw, strides, scales, &lv);
  if (r) return r;
  lv.B = batch;
  if (num_rois == 0) return FRH_OK;
  RoiCfg c{rois, roi_levels, num_rois, channels, pooled_h, pooled_w, sampling_ratio, aligned};
  hipStream_t st = as_stream(stream);
  if (variant == 23 || variant == 24) {  // software-pipelined persistent quad kernel (23: 8 waves per CU, 24: 12;
                                        // 2 waves per SIMD by registers: 24 queues its surplus)
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w), "the quad kernel does not take this shape");
    int dev = 0, ncu = 0;
    FRH_HIP(hipGetDevice(&dev));
    FRH_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const int wpc = variant == 23 ? 8 : 12;
    const dim3 gq((unsigned)(8 * ((ncu * wpc + 7) / 8)));
    hipLaunchKernelGGL((roi_align_fwd_quadp_kernel<kCpolNT>), gq, dim3(kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  if (variant == 65 || variant == 68) {  // the band kernel as dispatched (240 cells); 68: stamped (8 int64 per item)
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w) && band_fits(pooled_h, pooled_w, 240),
                "the band kernel does not take this shape");
    const int64_t tq = num_rois * ((channels + kQuadChunk - 1) / kQuadChunk);
    const dim3 gq((unsigned)(8 * ((tq + 7) / 8)));
    if (variant == 65)
      hipLaunchKernelGGL((roi_align_fwd_band_kernel<240, false, false>), gq, dim3(kWave), 0, st, lv, c, out);
    else
      hipLaunchKernelGGL((roi_align_fwd_band_kernel<240, false, true>), gq, dim3(kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  if ((variant >= 89 && variant <= 91) || (variant >= 94 && variant <= 99)) {  // channel-group kernel
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w) && cg_ok(channels, pooled_h, pooled_w, 116),
                "the channel-group kernel does not take this shape");
    const int64_t tg = num_rois * (channels / kCgChan);
    const dim3 gg((unsigned)(8 * ((tg + 7) / 8)));
    if (variant == 89)  // as dispatched: 120 cells (30 KB: 5 workgroups per CU by LDS), 5 waves per SIMD
      hipLaunchKernelGGL((roi_align_fwd_cg_kernel<4, 120, false, 5>), gg, dim3(4 * kWave), 0, st, lv, c, out);
    else if (variant == 90)  // 144 cells, registers as compiled
      hipLaunchKernelGGL((roi_align_fwd_cg_kernel<4, 144, false, 0>), gg, dim3(4 * kWave), 0, st, lv, c, out);
    else if (variant == 91)  // 8 waves, 120 cells (2 workgroups per CU)
      hipLaunchKernelGGL((roi_align_fwd_cg_kernel<8, 120, false, 5>), gg, dim3(8 * kWave), 0, st, lv, c, out);
    else if (variant == 94)  // variant 89, stamped (16 int64 per item after the output)
      hipLaunchKernelGGL((roi_align_fwd_cg_kernel<4, 120, false, 5, true>), gg, dim3(4 * kWave), 0, st, lv, c, out);
    else if (variant == 95)  // 124 cells (31 KB: 5 workgroups per CU), 5 waves per SIMD
      hipLaunchKernelGGL((roi_align_fwd_cg_kernel<4, 124, false, 5>), gg, dim3(4 * kWave), 0, st, lv, c, out);
    else {  // 96-99, software-pipelined, kItems items per workgroup:
            // 96 / 97 / 98: 2 / 3 / 4 items at 144 cells; 99: 2 at 116 cells
      const int ki = variant == 96 || variant == 99 ? 2 : variant == 97 ? 3 : 4;
      const int64_t per = (tg + 7) / 8, nwx = (per + ki - 1) / ki;
      const dim3 gp((unsigned)(8 * nwx));
      if (variant == 96)
        hipLaunchKernelGGL((roi_align_fwd_cgp_kernel<4, 144, 2>), gp, dim3(4 * kWave), 0, st, lv, c, out);
      else if (variant == 97)
        hipLaunchKernelGGL((roi_align_fwd_cgp_kernel<4, 144, 3>), gp, dim3(4 * kWave), 0, st, lv, c, out);
      else if (variant == 98)
        hipLaunchKernelGGL((roi_align_fwd_cgp_kernel<4, 144, 4>), gp, dim3(4 * kWave), 0, st, lv, c, out);
      else
        hipLaunchKernelGGL((roi_align_fwd_cgp_kernel<4, 116, 2, kCpolNT, false, 5>), gp, dim3(4 * kWave), 0, st, lv, c,
                           out);
    }
    return check_launch("frh_roi_align_fwd_variant");
  }
  if (variant == 25) {  // quad kernel with a 16-KB slab (10 waves per CU by LDS; D = 4 up to 256 cells)
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w, QuadLayout<1, 4096>::kCells),
                "the quad kernel does not take this shape");
    const int64_t tq = num_rois * ((channels + kQuadChunk - 1) / kQuadChunk);
    const dim3 gq((unsigned)(8 * ((tq + 7) / 8)));
    hipLaunchKernelGGL((roi_align_fwd_quad_kernel<false, 3, 4096>), gq, dim3(kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  if (variant == 19) {  // quad kernel, RoI setup shared by a 4-wave workgroup
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w), "the quad kernel does not take this shape");
    const int64_t tq = num_rois * ((channels + 16 * kQuadWave - 1) / (16 * kQuadWave));
    const dim3 gq((unsigned)(8 * ((tq + 7) / 8)));
    hipLaunchKernelGGL(roi_align_fwd_quad4_kernel, gq, dim3(4 * kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  if (variant >= 8 && variant <= 11) {  // channels-last quad kernel (8, 10: as dispatched; 9: stamped; 11: 5 waves/SIMD)
    const FwdCaps fq = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
    FRH_REQUIRE(quad_ok(fq, lv, channels, pooled_h, pooled_w), "the quad kernel does not take this shape");
    const int64_t tq = num_rois * ((channels + kQuadChunk - 1) / kQuadChunk);
    const dim3 gq((unsigned)(8 * ((tq + 7) / 8)));
    if (variant == 9)
      hipLaunchKernelGGL((roi_align_fwd_quad_kernel<true>), gq, dim3(kWave), 0, st, lv, c, out);
    else if (variant == 11)
      hipLaunchKernelGGL((roi_align_fwd_quad_kernel<false, 5>), gq, dim3(kWave), 0, st, lv, c, out);
    else
      hipLaunchKernelGGL((roi_align_fwd_quad_kernel<false, 3>), gq, dim3(kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  if (variant >= 2 && variant <= 7) {  // channels-last kernel: slab cells / outputs in VGPRs or in LDS
    FRH_REQUIRE(nhwc_ok(lv, channels, pooled_h, pooled_w, sampling_ratio), "the nhwc kernel does not take this shape");
    const int64_t tn = num_rois * (channels / kNhwcGroup);
    const dim3 gn((unsigned)(8 * ((tn + 7) / 8)));
    if (variant == 2)
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 56, kCpolNT, true>), gn, dim3(kWave), 0, st, lv, c, out);
    else if (variant == 3)
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 64, kCpolNT, true>), gn, dim3(kWave), 0, st, lv, c, out);
    else if (variant == 4)
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 96, kCpolNT, true>), gn, dim3(kWave), 0, st, lv, c, out);
    else if (variant == 5)
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 56, kCpolNT, false>), gn, dim3(kWave), 0, st, lv, c, out);
    else if (variant == 6)
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 56, kCpolNT, true, true>), gn, dim3(kWave), 0, st, lv, c, out);
    else
      hipLaunchKernelGGL((roi_align_fwd_nhwc_kernel<7, 7, 128, kCpolNT, true>), gn, dim3(kWave), 0, st, lv, c, out);
    return check_launch("frh_roi_align_fwd_variant");
  }
  FRH_REQUIRE(variant == 0 || variant == 1, "roi_align variant %d unknown", variant);
  const FwdCaps f = fwd_caps(lv, channels, pooled_h, pooled_w, sampling_ratio);
  FRH_REQUIRE(pair_ok(f, channels, pooled_h, pooled_w), "the pair kernel does not take this shape");
  const int64_t total = num_rois * ((channels + kPairChunk - 1) / kPairChunk);
  FRH_REQUIRE(total <= (int64_t)0x7fffffff - 7, "too many RoIs");
  const dim3 g1((unsigned)(8 * ((total + 7) / 8)));
  if (variant == 0)
    hipLaunchKernelGGL((roi_align_fwd_pair_kernel<false>), g1, dim3(kWave), 0, st, lv, c, out);
  else
    hipLaunchKernelGGL((roi_align_fwd_pair_kernel<true>), g1, dim3(kWave), 0, st, lv, c, out);
  return check_launch("frh_roi_align_fwd_variant");
}

// Backward A/B (channels-last gradients, sampling 2, 7 x 7 bins); no variant is retired: the
// product kernel keeps its kFixed and kNW parameters.
//   0 / 2    the product's roi_align_bwd_nhwc_kernel with one wave per (RoI, 64 channels): float
//            atomics / fixed point (absmax pass + conversion, as frh_roi_align_bwd_fixed)
//   1 / 3    lab kernel roi_align_bwd_nhwc_reg_kernel (grad_out in registers): float / fixed point
//   4 / 5    lab kernel roi_align_bwd_nhwc2_kernel (tap lists read by v_readlane): float / fixed point
//   6-8      its diagnostics: plain stores instead of atomics / no column loop / setup only
//   9-11     the product kernel with 2 / 4 (as dispatched) / 8 waves per RoI, float atomics
//   12       4 waves, fixed point (as frh_roi_align_bwd_fixed dispatches it)
// accs zeroed by the caller for the fixed-point variants, grads for the others.
extern "C" int32_t frh_roi_align_bwd_variant(int32_t variant, int32_t num_levels, float* const* grad_feats,
                                             int64_t* const* acc_feats, const int32_t* feat_hw, const int64_t* strides,
                                             const float* scales, int32_t batch, int32_t channels, const float* rois,
                                             const int64_t* roi_levels, int64_t num_rois, const float* grad_out,
                                             uint32_t* scale_word, void* stream) {
  int32_t r = roi_common_checks(batch, channels, num_rois, 7, 7, rois);
  if (r) return r;
  const bool fixed = variant == 2 || variant == 3 || variant == 5 || variant == 12;
  RoiLevels lv;
  r = make_levels(num_levels, nullptr, fixed ? reinterpret_cast<float* const*>(acc_feats) : grad_feats, feat_hw,
                  strides, scales, &lv);
  if (r) return r;
  lv.B = batch;
  for (int l = 0; l < lv.L; ++l) FRH_REQUIRE(lv.sc[l] == 1, "channels-last gradients only");
  hipStream_t st = as_stream(stream);
  int hb = 0;
  while (hb < 62 && (int64_t(1) << hb) < num_rois * 49) ++hb;
  RoiCfg c{rois, roi_levels, num_rois, channels, 7, 7, 2, 0, nullptr, scale_word, hb};
  const dim3 grid((unsigned)num_rois, (unsigned)((channels + kWave - 1) / kWave));
  if (fixed) {
    FRH_HIP(hipMemsetAsync(scale_word, 0, 4, st));
    const int64_t ng = num_rois * channels * 49;
    hipLaunchKernelGGL(roi_bwd_absmax_kernel, dim3((unsigned)std::min<int64_t>((ng / 4 + 255) / 256 + 1, kAbsmaxBlocks)),
                       dim3(kAbsmaxThreads), 0, st, grad_out, ng, scale_word);
  }
  if (variant == 0)
    hipLaunchKernelGGL(roi_align_bwd_nhwc_kernel<false>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 1)
    hipLaunchKernelGGL(roi_align_bwd_nhwc_reg_kernel<false>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 2)
    hipLaunchKernelGGL(roi_align_bwd_nhwc_kernel<true>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 3)
    hipLaunchKernelGGL(roi_align_bwd_nhwc_reg_kernel<true>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 4)  // round 6: tap lists read by v_readlane, row sums in registers
    hipLaunchKernelGGL(roi_align_bwd_nhwc2_kernel<false>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 5)
    hipLaunchKernelGGL(roi_align_bwd_nhwc2_kernel<true>, grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 6)  // diagnostic: variant 4 with plain stores instead of atomics (wrong sums)
    hipLaunchKernelGGL((roi_align_bwd_nhwc2_kernel<false, true>), grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 7)  // diagnostic: no column loop (row sums stored)
    hipLaunchKernelGGL((roi_align_bwd_nhwc2_kernel<false, true, 1>), grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 8)  // diagnostic: setup only (grad_out staging, tap entries, ranks)
    hipLaunchKernelGGL((roi_align_bwd_nhwc2_kernel<false, true, 2>), grid, dim3(kWave), 0, st, lv, c, grad_out);
  else if (variant == 9)  // product kernel, kNW waves per RoI
    hipLaunchKernelGGL((roi_align_bwd_nhwc_kernel<false, 2>), grid, dim3(2 * kWave), 0, st, lv, c, grad_out);
  else if (variant == 10)
    hipLaunchKernelGGL((roi_align_bwd_nhwc_kernel<false, 4>), grid, dim3(4 * kWave), 0, st, lv, c, grad_out);
  else if (variant == 11)
    hipLaunchKernelGGL((roi_align_bwd_nhwc_kernel<false, 8>), grid, dim3(8 * kWave), 0, st, lv, c, grad_out);
  else if (variant == 12)
    hipLaunchKernelGGL((roi_align_bwd_nhwc_kernel<true, 4>), grid, dim3(4 * kWave), 0, st, lv, c, grad_out);
  else
    FRH_REQUIRE(false, "backward variant %d unknown", variant);
  if (fixed) {
    for (int l = 0; l < lv.L; ++l) {
      const int64_t n = (int64_t)batch * channels * lv.h[l] * lv.w[l];
      hipLaunchKernelGGL(roi_bwd_fixed_to_f32_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)),
                         dim3(256), 0, st, reinterpret_cast<const long long*>(acc_feats[l]), grad_feats[l], n,
                         scale_word, hb);
    }
  }
  return check_launch("frh_roi_align_bwd_variant");
}
