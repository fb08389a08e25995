// Plain FCOS: the scale-range target assignment of a whole batch in one launch, and the head's
// focal / GIoU / centerness losses in one launch each way.
//
// Reference: FCOSHead.single_image_targets (lib/heads/fcos_head.py:371-416) with utils.sort_bbox
// (lib/utils.py:362-366), bbox2ltrb (:78-87), positive_ltrb (:51-53), centerness (:56-59) and
// paint_value (:90-94); the non-GFL arm of FCOSHead.calc_loss (:419-515) with sigmoid_focal_loss
// (lib/losses.py:33-61), giou_loss (:13-30) and CrossEntropyLoss(use_sigmoid=True) on one
// channel (:144-147).
//
// Targets.  The reference sorts an image's gts by descending area and then, per gt and level,
// builds an [H, W, 4] ltrb map and writes the label and the ltrb where all four distances are
// positive and the largest lies in the level's scale range: G x L steps of a handful of tiny
// launches, and the last gt painted -- the smallest -- owns a cell.  Per cell that is an arg-min:
// the matching gt of smallest area, the largest original index among equal areas (the stable
// sort keeps them in order, so the later one is painted later).  fcos_assign_kernel is one
// thread per (image, cell): the image's boxes and areas are staged in LDS a chunk at a time,
// every thread walks them and keeps its winner, then writes the cell's 28 bytes (the ltrb as
// one 16-byte store).  No workspace, no atomics, no hand-off between workgroups.
//
// Losses.  The reference reads the positive count back to the host, boolean-indexes six tensors
// and runs three loss modules.  fcos_loss_fwd_kernel is one pass with lane = position (coalesced
// along i for the head's [C, M] layout): the focal element of every class at every position
// with label >= 0 (focal_elem, the element frh_cls_loss_fwd kind 0 sums), and at the positives
// giou_loss of (-p_l, -p_t, p_r, p_b) against the normalised target times the centerness target,
// and the centerness BCE.  The workgroups' partials are finalised in a fixed order by the last
// one to arrive (fan_in, loss_common.h); no float atomics.  The backward recomputes and writes
// every gradient element exactly once.
//
// Numerics: f32 in the reference's operation order; the assignment is bit-exact, the loss sums
// differ from torch's reduction order in the last bits.
#include "giou.h"
#include "loss_common.h"
#include "ltrb_common.h"

#include <math.h>

namespace frh {
namespace {

constexpr int kFcosThreads = 256;
constexpr int kFcosChunk = 256;  // gts staged in LDS per pass

struct FcosAssignArgs {
  int B, Gmax;
  LevelTable lv;
  float thr[kLtrbMaxLevels + 1];  // level l takes thr[l] <= max(ltrb) < thr[l+1]
  const float* gts;
  int64_t gseg;
  const int32_t* ngt;
  const int64_t* labels;
  const int32_t* img_hw;
  int64_t* cls;
  float* reg;
  float* ctr;
};

__global__ void __launch_bounds__(kFcosThreads) fcos_assign_kernel(FcosAssignArgs a) {
  __shared__ float4 s_box[kFcosChunk];
  __shared__ float s_area[kFcosChunk];
  const int b = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * kFcosThreads + threadIdx.x;
  const bool live = c < a.lv.N;
  int y = 0, x = 0, l = 0;
  if (live) l = cell_yx(a.lv, c, &y, &x);
  const float s = a.lv.stride[l], lo = a.thr[l], hi = a.thr[l + 1];
  int G = a.ngt[b];
  G = G < 0 ? 0 : (G > a.Gmax ? a.Gmax : G);
  const float* gt = a.gts + (int64_t)b * a.gseg;
  int best = -1;
  float best_area = INFINITY;
  float bl[4] = {-1.0f, -1.0f, -1.0f, -1.0f};
  for (int g0 = 0; g0 < G; g0 += kFcosChunk) {  // block-uniform
    const int n = G - g0 < kFcosChunk ? G - g0 : kFcosChunk;
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const int g = g0 + threadIdx.x;
      const float4 bx = make_float4(gt[g], gt[(int64_t)a.Gmax + g], gt[2 * (int64_t)a.Gmax + g],
                                    gt[3 * (int64_t)a.Gmax + g]);
      s_box[threadIdx.x] = bx;
      s_area[threadIdx.x] = ((bx.z - bx.x) + 1.0f) * ((bx.w - bx.y) + 1.0f);  // sort_bbox's key
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < n; ++j) {
        const float4 q = s_box[j];
        const float bx[4] = {q.x, q.y, q.z, q.w};
        float lt[4];
        center_ltrb(s, y, x, bx, lt);
        const float mx = fmaxf(fmaxf(lt[0], lt[1]), fmaxf(lt[2], lt[3]));
        const bool match = lt[0] > 0.0f && lt[1] > 0.0f && lt[2] > 0.0f && lt[3] > 0.0f && mx >= lo && mx < hi;
        // painted in descending-area order: the smallest wins, the later of equal areas
        if (match && s_area[j] <= best_area) {
          best = g0 + j;
          best_area = s_area[j];
          bl[0] = lt[0], bl[1] = lt[1], bl[2] = lt[2], bl[3] = lt[3];
        }
      }
  }
  if (!live) return;
  const bool in = painted(a.img_hw, b, s, y, x);
  int64_t lab = in ? 0 : -1;
  float ct = in ? 0.0f : -1.0f;
  if (best >= 0) {
    lab = a.labels[(int64_t)b * a.Gmax + best];
    if (lab > 0) ct = ltrb_centerness(bl);
  }
  const int64_t o = (int64_t)b * a.lv.N + c;
  a.cls[o] = lab;
  a.ctr[o] = ct;
  reinterpret_cast<float4*>(a.reg)[o] = make_float4(bl[0], bl[1], bl[2], bl[3]);
}

struct FcosLossArgs {
  const float* cls;
  int64_t c, sk, si;     // class logit (k, i) at cls[k*sk + i*si]
  const float* reg;
  int64_t rss, rsi;      // ltrb prediction (s, i) at reg[s*rss + i*rsi]
  const float* ctr;
  int64_t csi;           // centerness logit i at ctr[i*csi]
  const int64_t* label;  // [m]: -1 ignored, 0 negative, > 0 the class
  const float* ltrb;     // [m, 4] pixels
  const float* ctr_t;    // [m]
  int64_t m;
  float reg_mean, reg_std, alpha, gamma;
};

struct FcosScale {
  float wc, wb, wt;
};

struct FcosBox {
  float a[4], b[4];
};

// the boxes (-l, -t, r, b) of the prediction and of the normalised target around (0, 0)
// (simple_ltrb2bbox, fcos_head.py:494-495)
__device__ __forceinline__ FcosBox fcos_boxes(const FcosLossArgs& a, int64_t i) {
  FcosBox r;
  const float4 t = reinterpret_cast<const float4*>(a.ltrb)[i];
  const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float p = a.reg[s * a.rss + i * a.rsi];
    const float y = (tv[s] - a.reg_mean) / a.reg_std;
    r.a[s] = s < 2 ? 0.0f - p : 0.0f + p;
    r.b[s] = s < 2 ? 0.0f - y : 0.0f + y;
  }
  return r;
}

__global__ void __launch_bounds__(kLossThreads) fcos_loss_fwd_kernel(FcosLossArgs a, FcosScale o, uint32_t* counter,
                                                                     float* partial, float* out,
                                                                     const int32_t* status) {
  __shared__ float scratch[kLossThreads / kWave];
  __shared__ int iscratch[kLossThreads / kWave];
  float acc_cls = 0.0f, acc_box = 0.0f, acc_ctr = 0.0f;
  int npos = 0;
  for (int64_t i = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; i < a.m;
       i += (int64_t)gridDim.x * kLossThreads) {
    const int64_t lab = a.label[i];
    if (lab < 0) continue;
    const float* col = a.cls + i * a.si;
    for (int64_t k = 0; k < a.c; ++k)
      acc_cls += focal_elem(col[k * a.sk], lab == k + 1 ? 1.0f : 0.0f, a.alpha, a.gamma, nullptr);
    if (lab > 0) {
      const FcosBox bx = fcos_boxes(a, i);
      const float t = a.ctr_t[i];
      const Giou gv = giou_eval(bx.a[0], bx.a[1], bx.a[2], bx.a[3], bx.b[0], bx.b[1], bx.b[2], bx.b[3]);
      acc_box += gv.loss * t;
      acc_ctr += bce_logits(a.ctr[i * a.csi], t);
      ++npos;
    }
  }
  const float pc = block_sum_f(acc_cls, scratch);
  __syncthreads();
  const float pb = block_sum_f(acc_box, scratch);
  __syncthreads();
  const float pt = block_sum_f(acc_ctr, scratch);
  const int np = block_sum_i(npos, iscratch);
  const int g = gridDim.x;
  const float p[4] = {pc, pb, pt, (float)np};  // the count is exact in f32: a workgroup counts fewer than 2^24
  const int nb[4] = {g, g, g, g};
  double res[4];
  if (!fan_in(p, nb, counter, partial, res)) return;
  if (threadIdx.x == 0) {
    // the modules' (sum * loss_weight) / num_pos in f32; max(num_pos, 1) where the reference divides by 0
    const float n = (float)res[3];
    const float d = fmaxf(n, 1.0f);
    out[0] = ((float)res[0] * o.wc) / d;
    out[1] = ((float)res[1] * o.wb) / d;
    out[2] = ((float)res[2] * o.wt) / d;
    out[3] = n;
    if (status_set(status)) out[0] = out[1] = out[2] = NAN;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(kLossThreads) fcos_loss_bwd_kernel(FcosLossArgs a, FcosScale o, const float* g,
                                                                     const float* fwd_out, float* gcls, int64_t gsk,
                                                                     int64_t gsi, float* greg, int64_t grs, int64_t gri,
                                                                     float* gctr, int64_t gci) {
  const float d = fmaxf(fwd_out[3], 1.0f);
  // the reference's Div then Mul backward of (sum * weight) / num_pos
  const float sc_cls = (g[0] / d) * o.wc;
  const float sc_box = (g[1] / d) * o.wb;
  const float sc_ctr = (g[2] / d) * o.wt;
  for (int64_t i = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; i < a.m;
       i += (int64_t)gridDim.x * kLossThreads) {
    const int64_t lab = a.label[i];
    const float* col = a.cls + i * a.si;
    float* gcol = gcls + i * gsi;
    for (int64_t k = 0; k < a.c; ++k) {
      float gx = 0.0f;
      if (lab >= 0) {
        float dx;
        focal_elem(col[k * a.sk], lab == k + 1 ? 1.0f : 0.0f, a.alpha, a.gamma, &dx);
        gx = sc_cls * dx;
      }
      gcol[k * gsk] = gx;
    }
    float gr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float gc = 0.0f;
    if (lab > 0) {
      const FcosBox bx = fcos_boxes(a, i);
      const float t = a.ctr_t[i];
      const Giou gv = giou_eval(bx.a[0], bx.a[1], bx.a[2], bx.a[3], bx.b[0], bx.b[1], bx.b[2], bx.b[3]);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float dbox = giou_dside(gv, s, bx.a[0], bx.a[1], bx.a[2], bx.a[3], bx.b[0], bx.b[1], bx.b[2], bx.b[3]);
        gr[s] = (sc_box * t) * (s < 2 ? -dbox : dbox);  // a = (-p_l, -p_t, p_r, p_b)
      }
      gc = sc_ctr * (sigmoidf(a.ctr[i * a.csi]) - t);   // d bce_with_logits / dx = sigmoid(x) - t
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) greg[s * grs + i * gri] = gr[s];
    gctr[i * gci] = gc;
  }
}

int32_t make_fcos_loss(FcosLossArgs* a, const float* cls, int64_t c, int64_t sk, int64_t si, const float* reg,
                       int64_t rss, int64_t rsi, const float* ctr, int64_t csi, const int64_t* label,
                       const float* ltrb, const float* ctr_t, int64_t m, float reg_mean, float reg_std, float alpha,
                       float gamma) {
  FRH_REQUIRE(c >= 1 && m >= 0, "fcos loss: bad shape (C %lld, M %lld)", (long long)c, (long long)m);
  FRH_REQUIRE(m < (int64_t(1) << 31), "fcos loss: too many positions");
  FRH_REQUIRE(m == 0 || (cls && reg && ctr && label && ltrb && ctr_t), "fcos loss: null input");
  FRH_REQUIRE(reg_std != 0.0f, "fcos loss: reg_std must be nonzero");
  FRH_REQUIRE_ALIGNED16(ltrb);
  *a = FcosLossArgs{cls, c, sk, si, reg, rss, rsi, ctr, csi, label, ltrb, ctr_t, m, reg_mean, reg_std, alpha, gamma};
  return FRH_OK;
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" {

int32_t frh_fcos_assign(int32_t batch, int32_t num_levels, const int32_t* grid_hw, const float* strides,
                        const float* scale_thr, const float* gts, int64_t gt_seg_stride, const int32_t* num_gts,
                        const int64_t* gt_labels, int32_t max_gts, const int32_t* img_hw, int64_t* cls, float* reg,
                        float* ctr, void* stream) {
  FRH_REQUIRE(batch >= 0 && max_gts >= 0, "negative sizes");
  FcosAssignArgs a{};
  const int32_t lst = set_levels(&a.lv, num_levels, grid_hw, strides);
  if (lst != FRH_OK) return lst;
  FRH_REQUIRE(scale_thr, "null host array");
  for (int l = 0; l <= num_levels; ++l) a.thr[l] = scale_thr[l];
  if (batch == 0) return FRH_OK;
  FRH_REQUIRE(batch <= 65535, "batch %d exceeds the grid's y extent", batch);
  FRH_REQUIRE(num_gts && img_hw && cls && reg && ctr, "null pointer argument");
  FRH_REQUIRE(max_gts == 0 || (gts && gt_labels), "null gt pointer");
  FRH_REQUIRE(max_gts == 0 || gt_seg_stride >= 4 * (int64_t)max_gts, "gt_seg_stride %lld < 4 * max_gts",
              (long long)gt_seg_stride);
  FRH_REQUIRE_ALIGNED16(reg);
  a.B = batch;
  a.Gmax = max_gts;
  a.gts = gts;
  a.gseg = gt_seg_stride;
  a.ngt = num_gts;
  a.labels = gt_labels;
  a.img_hw = img_hw;
  a.cls = cls;
  a.reg = reg;
  a.ctr = ctr;
  hipLaunchKernelGGL(fcos_assign_kernel, dim3((unsigned)((a.lv.N + kFcosThreads - 1) / kFcosThreads), (unsigned)batch),
                     dim3(kFcosThreads), 0, as_stream(stream), a);
  return check_launch("frh_fcos_assign");
}

int32_t frh_fcos_loss_fwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                          int64_t reg_ss, int64_t reg_si, const float* ctr, int64_t ctr_si, const int64_t* label,
                          const float* ltrb, const float* ctr_t, int64_t m, float reg_mean, float reg_std,
                          float alpha, float gamma, float cls_weight, float bbox_weight, float ctr_weight,
                          const int32_t* status, float* out, void* workspace, size_t ws_bytes, void* stream) {
  FcosLossArgs a;
  int32_t st = make_fcos_loss(&a, cls, c, cls_sk, cls_si, reg, reg_ss, reg_si, ctr, ctr_si, label, ltrb, ctr_t, m,
                              reg_mean, reg_std, alpha, gamma);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(out, "fcos loss: null output");
  LossWorkspace ws;
  st = split_workspace(workspace, ws_bytes, "fcos loss", &ws);
  if (st != FRH_OK) return st;
  const FcosScale o{cls_weight, bbox_weight, ctr_weight};
  hipLaunchKernelGGL(fcos_loss_fwd_kernel, dim3(loss_grid(m)), dim3(kLossThreads), 0, as_stream(stream), a, o,
                     ws.counter, ws.partial, out, status);
  return check_launch("frh_fcos_loss_fwd");
}

int32_t frh_fcos_loss_bwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                          int64_t reg_ss, int64_t reg_si, const float* ctr, int64_t ctr_si, const int64_t* label,
                          const float* ltrb, const float* ctr_t, int64_t m, float reg_mean, float reg_std,
                          float alpha, float gamma, float cls_weight, float bbox_weight, float ctr_weight,
                          const float* g, const float* fwd_out, float* grad_cls, int64_t gc_sk, int64_t gc_si,
                          float* grad_reg, int64_t gr_ss, int64_t gr_si, float* grad_ctr, int64_t gt_si,
                          void* stream) {
  FcosLossArgs a;
  const int32_t st = make_fcos_loss(&a, cls, c, cls_sk, cls_si, reg, reg_ss, reg_si, ctr, ctr_si, label, ltrb, ctr_t,
                                    m, reg_mean, reg_std, alpha, gamma);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(g && fwd_out && (m == 0 || (grad_cls && grad_reg && grad_ctr)), "fcos loss bwd: null gradient");
  if (m == 0) return FRH_OK;
  const FcosScale o{cls_weight, bbox_weight, ctr_weight};
  const int64_t nb = (m + kLossThreads - 1) / kLossThreads;
  hipLaunchKernelGGL(fcos_loss_bwd_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(kLossThreads), 0,
                     as_stream(stream), a, o, g, fwd_out, grad_cls, gc_sk, gc_si, grad_reg, gr_ss, gr_si, grad_ctr,
                     gt_si);
  return check_launch("frh_fcos_loss_bwd");
}

}  // extern "C"
