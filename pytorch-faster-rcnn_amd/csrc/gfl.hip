// Generalized Focal Loss head: the fused QFL / DFL / GIoU losses (forward and backward) and the
// DFL box decode.
//
// Reference: FCOSHead.calc_loss with use_qfl and use_dfl (lib/heads/fcos_head.py:419-515),
// QualityFocalLoss / generalized_focal_loss (lib/losses.py:221-247), DistributionFocalLoss /
// log_softmax_with_logits (:251-282), giou_loss / GIoULoss (:13-30, :196-205), utils.elem_iou
// (lib/utils.py:174-182), length2class / class2length (fcos_head.py:10-42); the decode is
// predict_single_image's use_dfl branch (fcos_head.py:579-600) with ltrb2bbox (:63-75) and
// utils.clamp_bbox (lib/utils.py:109-120).  The reference reads the positive count back to the
// host, boolean-indexes six tensors, builds a two-hot target, transposes [4*bins, m] to
// [4m, bins], runs a log-softmax, a second softmax, an expectation, two box builds, an IoU and a
// GIoU, scatters the quality into an [M] vector and builds an [M, C+1] QFL target: a few dozen
// elementwise launches and a host sync per step.
//
// The forward is ONE launch.  A wave takes 64 consecutive positions at a time, in two phases:
//   1. its positives, one after the other (they are sparse: about 1 % of the positions), with
//      lane = regression channel = bin*4 + side: 16 bins x 4 sides is exactly one wave64, so the
//      per-side softmax statistics are xor-shuffles over the lane offsets 4, 8, 16, 32.  Each
//      positive's quality q and w * giou_loss are parked in the register of the lane that owns
//      that position in phase 2; the DFL terms stay in the lanes (bins) that produced them.
//   2. the class stream with lane = position (coalesced along i for the [C, M] layout the head
//      produces): the QFL element of every class, its target q taken from the lane's register.
// One launch and not two (positives first, then a class stream reading q from memory) because
// phase 2 needs q only for the 64 positions its own wave has just handled: the hand-over is a
// register, there is no [M] quality buffer to write, re-read and size a workspace for, and one
// launch less on a path that is launch-bound at the head's size (44 k positions, 3.5 MB of
// class logits).  The per-lane sums are reduced per workgroup and the workgroups' partials are
// finalised in a fixed order by the last workgroup to arrive (the arrival-counter fan-in of
// loss_common.h: fan_in), so a call is deterministic; no float atomics.
//
// The backward has the same two phases and recomputes q and w (constants of the gradient, as
// the reference detaches them): phase 1 writes the 4*bins regression gradients of a positive
// (lane = channel), the lanes of the other positions write their zeros (lane = position), phase
// 2 writes the class gradients.  Every element is written exactly once, no atomics.
//
// Numerics: f32 in the reference's operation order where that is free (the clamp bound and the
// bin positions b*stride are rounded from the double product as torch rounds its Python
// scalars; left = trunc(f32 division)); the sums differ from torch's reduction order in the
// last bits.  One step is wider than the reference's f32: the normalised target y and the two
// DFL weights y_right - y and y - y_left are formed in double and then rounded, because the
// DFL loss is divided by the constant 4 and not by num_pos, so y's own f32 rounding would show
// in its gradient.  At left == bins-1 the reference indexes past the last bin and raises; here the
// right-hand DFL term is dropped and no such lane exists to be read (include/frcnn_amd.h).
#include "giou.h"
#include "loss_common.h"

#include <math.h>

namespace frh {
namespace {

struct GflArgs {
  const float* cls;
  int64_t c, sk, si;    // class logit (k, i) at cls[k*sk + i*si]
  const float* reg;
  int64_t rsc, rsi;     // regression logit (ch, i) at reg[ch*rsc + i*rsi], ch = bin*4 + side
  const int64_t* label; // [m]: -1 ignored, 0 negative, > 0 the class
  const float* ltrb;    // [m, 4] pixels
  int64_t m;
  int32_t bins, norm_prob;
  float reg_mean, reg_std, beta;
  float stride;         // f32(stride): what torch's tensor-with-Python-scalar ops compute with
  float top;            // f32((bins-1) * stride), the clamp bound of length2class
  double stride_d;
};

struct GflScale {
  float wc, wd, wb, dfl_avg;
};

// all lanes of one side (lane & 3) end with the reduction over that side's bins (lane >> 2)
__device__ __forceinline__ float side_max(float v) {
#pragma unroll
  for (int o = 4; o < kWave; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float side_sum(float v) {
#pragma unroll
  for (int o = 4; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ float qfl_pow(float d, float beta) { return beta == 2.0f ? d * d : powf(d, beta); }

struct PosEval {
  float w;      // max_k sigmoid(cls(k, j))                         (wave-uniform)
  float q;      // IoU of the decoded and the target box            (wave-uniform)
  float giou;   // giou_loss of the two boxes                       (wave-uniform)
  float dfl;    // this lane's share of the position's DFL `loss` (before the minus sign)
  float g_dfl;  // kGrad: d(sum of the position's DFL `loss`) / d(this lane's logit)
  float g_box;  // kGrad: d(giou_loss) / d(this lane's logit)
};

// One positive position j, evaluated by a whole wave (wave-uniform call), lane = channel.
template <bool kGrad>
__device__ __forceinline__ PosEval eval_positive(const GflArgs& a, int64_t j, int lane) {
  PosEval r;
  const int side = lane & 3, bin = lane >> 2;
  const bool act = lane < 4 * a.bins;
  float w = 0.0f;  // sigmoid > 0
  for (int64_t k = lane; k < a.c; k += kWave) w = fmaxf(w, sigmoidf(a.cls[k * a.sk + j * a.si]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w = fmaxf(w, __shfl_xor(w, o, kWave));
  r.w = w;

  const float x = act ? a.reg[lane * a.rsc + j * a.rsi] : -INFINITY;
  const float mx = side_max(x);
  const float e = act ? expf(x - mx) : 0.0f;
  const float s = side_sum(e);
  const float p = e / s;                                         // softmax(-1)
  const float posb = (float)((double)bin * a.stride_d);          // class2length's rand_var
  const float len = side_sum(p * posb);
  // the normalised target in double: y sits next to a bin bound in the DFL weights below, and
  // the f32 rounding of y alone (6e-8 at y ~ 1) is what would limit the DFL gradient against an
  // f64 evaluation; its f32 value (the correctly rounded quotient) is the reference's y
  const double yd = ((double)a.ltrb[j * 4 + side] - (double)a.reg_mean) / (double)a.reg_std;
  const float y = (float)yd;

  // DistributionFocalLoss: this lane is bin `bin` of side `side`
  const float yc = fminf(fmaxf(y, 0.0f), a.top);
  const int left = (int)(yc / a.stride);
  const float yl = (float)left * a.stride, yr = (float)(left + 1) * a.stride;  // f32, as the reference's
  const float wl = (float)((double)yr - yd), wr = (float)(yd - (double)yl);    // y_right - y, y - y_left
  const float lsm = (x - mx) - logf(s);
  const bool is_l = act && bin == left, is_r = act && bin == left + 1;  // no lane is bin `bins`
  float t = is_l ? wl * lsm : (is_r ? wr * lsm : 0.0f);
  if (a.norm_prob) t = t / a.stride;
  r.dfl = t;

  // boxes (-l, -t, r, b) of the expectation and of the target (simple_ltrb2bbox around (0, 0))
  const float l0 = __shfl(len, 0, kWave), l1 = __shfl(len, 1, kWave), l2 = __shfl(len, 2, kWave),
              l3 = __shfl(len, 3, kWave);
  const float y0 = __shfl(y, 0, kWave), y1 = __shfl(y, 1, kWave), y2 = __shfl(y, 2, kWave), y3 = __shfl(y, 3, kWave);
  const float a0 = 0.0f - l0, a1 = 0.0f - l1, a2 = 0.0f + l2, a3 = 0.0f + l3;
  const float b0 = 0.0f - y0, b1 = 0.0f - y1, b2 = 0.0f + y2, b3 = 0.0f + y3;
  const Giou gv = giou_eval(a0, a1, a2, a3, b0, b1, b2, b3);  // giou.h
  r.q = gv.iou;
  r.giou = gv.loss;
  r.g_dfl = r.g_box = 0.0f;
  if constexpr (kGrad) {
    const float dbox = giou_dside(gv, side, a0, a1, a2, a3, b0, b1, b2, b3);  // d giou_loss / d a_side
    const float dlen = side < 2 ? -dbox : dbox;       // a = (-len_l, -len_t, len_r, len_b)
    r.g_box = act ? (p * (posb - len)) * dlen : 0.0f; // through the softmax expectation
    // d/dx_b of wl * logsm[left] + wr * logsm[left+1], d logsm[c] / d x_b = [b == c] - p_b
    float g = wl * ((is_l ? 1.0f : 0.0f) - p);
    if (left + 1 < a.bins) g += wr * ((is_r ? 1.0f : 0.0f) - p);
    if (a.norm_prob) g = g / a.stride;
    r.g_dfl = act ? g : 0.0f;
  }
  return r;
}

// The last workgroup to arrive sums the four partial arrays in a fixed order (loss_common.h:
// fan_in) and scales as the reference's modules do: (sum * loss_weight) / avg_factor in f32.
__device__ void gfl_fan_in(float pc, float pd, float pb, int np, uint32_t* counter, float* partial,
                           const GflScale& o, float* out, const int32_t* status) {
  const int g = gridDim.x;
  const float p[4] = {pc, pd, pb, (float)np};  // the count is exact in f32: a workgroup counts fewer than 2^24
  const int nb[4] = {g, g, g, g};
  double res[4];
  if (!fan_in(p, nb, counter, partial, res)) return;
  if (threadIdx.x == 0) {
    const float npos = (float)res[3];
    const float d = fmaxf(npos, 1.0f);
    out[0] = ((float)res[0] * o.wc) / d;
    out[1] = (-(float)res[1] * o.wd) / o.dfl_avg;
    out[2] = ((float)res[2] * o.wb) / d;
    out[3] = npos;
    if (status_set(status)) out[0] = out[1] = out[2] = NAN;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(kLossThreads) gfl_loss_fwd_kernel(GflArgs a, GflScale o, uint32_t* counter,
                                                                    float* partial, float* out,
                                                                    const int32_t* status) {
  __shared__ float scratch[kLossThreads / kWave];
  __shared__ int iscratch[kLossThreads / kWave];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  constexpr int kWaves = kLossThreads / kWave;
  float acc_cls = 0.0f, acc_dfl = 0.0f, acc_box = 0.0f;
  int npos = 0;
  const int64_t nchunks = (a.m + kWave - 1) / kWave;
  for (int64_t ch = (int64_t)blockIdx.x * kWaves + wave; ch < nchunks; ch += (int64_t)gridDim.x * kWaves) {
    const int64_t i = ch * kWave + lane;
    const int64_t lab = i < a.m ? a.label[i] : -1;
    uint64_t pm = __ballot(lab > 0);
    float q = 0.0f;
    while (pm) {  // wave-uniform
      const int pl = __builtin_ctzll(pm);
      pm &= pm - 1;
      const PosEval r = eval_positive<false>(a, ch * kWave + pl, lane);
      acc_dfl += r.dfl;
      if (lane == pl) {
        q = r.q;
        acc_box += r.giou * r.w;
        ++npos;
      }
    }
    if (lab >= 0) {
      const float* col = a.cls + i * a.si;
      for (int64_t k = 0; k < a.c; ++k) {
        const float x = col[k * a.sk];
        const float t = lab == k + 1 ? q : 0.0f;
        acc_cls += qfl_pow(fabsf(t - sigmoidf(x)), a.beta) * bce_logits(x, t);
      }
    }
  }
  const float pc = block_sum_f(acc_cls, scratch);
  __syncthreads();
  const float pd = block_sum_f(acc_dfl, scratch);
  __syncthreads();
  const float pb = block_sum_f(acc_box, scratch);
  const int np = block_sum_i(npos, iscratch);
  gfl_fan_in(pc, pd, pb, np, counter, partial, o, out, status);
}

__global__ void __launch_bounds__(kLossThreads) gfl_loss_bwd_kernel(GflArgs a, GflScale o, const float* g,
                                                                    const float* fwd_out, float* gcls, int64_t gsk,
                                                                    int64_t gsi, float* greg, int64_t grc,
                                                                    int64_t gri) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  constexpr int kWaves = kLossThreads / kWave;
  const float d = fmaxf(fwd_out[3], 1.0f);
  // the reference's Div then Mul backward of (sum * weight) / avg_factor
  const float sc_cls = (g[0] / d) * o.wc;
  const float sc_dfl = -((g[1] / o.dfl_avg) * o.wd);
  const float sc_box = (g[2] / d) * o.wb;
  const int nch = 4 * a.bins;
  const int64_t nchunks = (a.m + kWave - 1) / kWave;
  for (int64_t ch = (int64_t)blockIdx.x * kWaves + wave; ch < nchunks; ch += (int64_t)gridDim.x * kWaves) {
    const int64_t i = ch * kWave + lane;
    const int64_t lab = i < a.m ? a.label[i] : -1;
    uint64_t pm = __ballot(lab > 0);
    float q = 0.0f;
    while (pm) {  // wave-uniform
      const int pl = __builtin_ctzll(pm);
      pm &= pm - 1;
      const int64_t j = ch * kWave + pl;
      const PosEval r = eval_positive<true>(a, j, lane);
      if (lane < nch) greg[lane * grc + j * gri] = sc_dfl * r.g_dfl + sc_box * (r.w * r.g_box);
      if (lane == pl) q = r.q;
    }
    if (i >= a.m) continue;
    if (!(lab > 0))
      for (int c = 0; c < nch; ++c) greg[c * grc + i * gri] = 0.0f;
    const float* col = a.cls + i * a.si;
    float* gcol = gcls + i * gsi;
    for (int64_t k = 0; k < a.c; ++k) {
      float gx = 0.0f;
      if (lab >= 0) {
        const float x = col[k * a.sk];
        const float t = lab == k + 1 ? q : 0.0f;
        const float p = sigmoidf(x);
        const float df = t - p, ad = fabsf(df);
        const float sgn = df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f);
        const float f = qfl_pow(ad, a.beta);
        // d/dx |t - p|^beta = beta |t - p|^(beta-1) sign(t - p) (-p (1 - p)); d bce / dx = p - t
        const float dpw = a.beta == 2.0f ? 2.0f * ad : a.beta * powf(ad, a.beta - 1.0f);
        const float dfdx = (dpw * sgn) * (-(p * (1.0f - p)));
        gx = sc_cls * (f * (p - t) + bce_logits(x, t) * dfdx);
      }
      gcol[k * gsk] = gx;
    }
  }
}

struct DecodeArgs {
  const float* reg;
  int32_t batch, bins, h, w;
  int64_t sb, sc, sy, sx;
  double stride_d;
  float reg_std, reg_mean, cell, xmax, ymax;
  float* boxes;  // [batch, 4, h*w]
};

// side s of the box of cell (y, x): ltrb2bbox then clamp_bbox
__device__ __forceinline__ float decode_coord(const DecodeArgs& a, int side, float len, int y, int x) {
  const float ltrb = len * a.reg_std + a.reg_mean;
  const float ctr = (float)((side & 1) ? y : x) * a.cell + a.cell / 2.0f;
  const float v = side < 2 ? ctr - ltrb : ltrb + ctr;
  const float hi = (side & 1) ? a.ymax : a.xmax;
  return fminf(fmaxf(v, 0.0f), hi);
}

constexpr int kMaxBins = kWave / 4;

// lane = position: reads coalesced along x for NCHW-like layouts (sx == 1)
__global__ void __launch_bounds__(kLossThreads) dfl_decode_pos_kernel(DecodeArgs a) {
  const int64_t hw = (int64_t)a.h * a.w, total = hw * a.batch;
  for (int64_t e = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kLossThreads) {
    const int64_t b = e / hw, pos = e - b * hw;
    const int y = (int)(pos / a.w), x = (int)(pos - (int64_t)y * a.w);
    const float* base = a.reg + b * a.sb + y * a.sy + x * a.sx;
#pragma unroll
    for (int side = 0; side < 4; ++side) {
      float v[kMaxBins];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < kMaxBins; ++k) {
        v[k] = k < a.bins ? base[(k * 4 + side) * a.sc] : -INFINITY;
        mx = fmaxf(mx, v[k]);
      }
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < kMaxBins; ++k) {
        v[k] = k < a.bins ? expf(v[k] - mx) : 0.0f;
        s += v[k];
      }
      float len = 0.0f;
#pragma unroll
      for (int k = 0; k < kMaxBins; ++k)
        if (k < a.bins) len += (v[k] / s) * (float)((double)k * a.stride_d);
      a.boxes[(b * 4 + side) * hw + pos] = decode_coord(a, side, len, y, x);
    }
  }
}

// lane = channel, one position per wave and pass: a position's 4*bins logits are contiguous in
// channels-last maps (sc == 1), one coalesced 256-byte read
__global__ void __launch_bounds__(kLossThreads) dfl_decode_chan_kernel(DecodeArgs a) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  constexpr int kWaves = kLossThreads / kWave;
  const int side = lane & 3, bin = lane >> 2;
  const bool act = lane < 4 * a.bins;
  const float posb = (float)((double)bin * a.stride_d);
  const int64_t hw = (int64_t)a.h * a.w, total = hw * a.batch;
  for (int64_t e = (int64_t)blockIdx.x * kWaves + wave; e < total; e += (int64_t)gridDim.x * kWaves) {
    const int64_t b = e / hw, pos = e - b * hw;
    const int y = (int)(pos / a.w), x = (int)(pos - (int64_t)y * a.w);
    const float v = act ? a.reg[b * a.sb + y * a.sy + x * a.sx + lane * a.sc] : -INFINITY;
    const float mx = side_max(v);
    const float ex = act ? expf(v - mx) : 0.0f;
    const float s = side_sum(ex);
    const float len = side_sum((ex / s) * posb);
    if (lane < 4) a.boxes[(b * 4 + side) * hw + pos] = decode_coord(a, side, len, y, x);
  }
}

int32_t make_gfl(GflArgs* a, const float* cls, int64_t c, int64_t sk, int64_t si, const float* reg, int32_t bins,
                 int64_t rsc, int64_t rsi, const int64_t* label, const float* ltrb, int64_t m, float reg_mean,
                 float reg_std, double stride, int32_t norm_prob, float beta) {
  FRH_REQUIRE(bins >= 1 && c >= 1 && m >= 0, "gfl loss: bad shape (C %lld, bins %d, M %lld)", (long long)c, bins,
              (long long)m);
  if (bins * 4 > kWave) {
    set_error("gfl loss: 4 * bins = %d exceeds one wave (64 lanes)", bins * 4);
    return FRH_EUNSUPPORTED;
  }
  FRH_REQUIRE(m < (int64_t(1) << 31), "gfl loss: too many positions");
  FRH_REQUIRE(m == 0 || (cls && reg && label && ltrb), "gfl loss: null input");
  FRH_REQUIRE(stride > 0.0 && reg_std != 0.0f, "gfl loss: stride must be > 0 and reg_std nonzero");
  *a = GflArgs{cls, c, sk, si, reg, rsc, rsi, label, ltrb, m, bins, norm_prob ? 1 : 0, reg_mean, reg_std, beta,
               (float)stride, (float)((double)(bins - 1) * stride), stride};
  return FRH_OK;
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" {

int32_t frh_gfl_loss_fwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg, int32_t bins,
                         int64_t reg_sc, int64_t reg_si, const int64_t* label, const float* ltrb, int64_t m,
                         float reg_mean, float reg_std, double stride, int32_t norm_prob, float beta,
                         float cls_weight, float dfl_weight, float bbox_weight, float dfl_avg_factor,
                         const int32_t* status, float* out, void* workspace, size_t ws_bytes, void* stream) {
  GflArgs a;
  int32_t st = make_gfl(&a, cls, c, cls_sk, cls_si, reg, bins, reg_sc, reg_si, label, ltrb, m, reg_mean, reg_std,
                        stride, norm_prob, beta);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(out, "gfl loss: null output");
  FRH_REQUIRE(dfl_avg_factor != 0.0f, "gfl loss: dfl_avg_factor must be nonzero");
  LossWorkspace ws;
  st = split_workspace(workspace, ws_bytes, "gfl loss", &ws);
  if (st != FRH_OK) return st;
  const GflScale o{cls_weight, dfl_weight, bbox_weight, dfl_avg_factor};
  hipLaunchKernelGGL(gfl_loss_fwd_kernel, dim3(loss_grid(m)), dim3(kLossThreads), 0, as_stream(stream), a, o,
                     ws.counter, ws.partial, out, status);
  return check_launch("frh_gfl_loss_fwd");
}

int32_t frh_gfl_loss_bwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg, int32_t bins,
                         int64_t reg_sc, int64_t reg_si, const int64_t* label, const float* ltrb, int64_t m,
                         float reg_mean, float reg_std, double stride, int32_t norm_prob, float beta,
                         float cls_weight, float dfl_weight, float bbox_weight, float dfl_avg_factor, const float* g,
                         const float* fwd_out, float* grad_cls, int64_t gc_sk, int64_t gc_si, float* grad_reg,
                         int64_t gr_sc, int64_t gr_si, void* stream) {
  GflArgs a;
  int32_t st = make_gfl(&a, cls, c, cls_sk, cls_si, reg, bins, reg_sc, reg_si, label, ltrb, m, reg_mean, reg_std,
                        stride, norm_prob, beta);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(dfl_avg_factor != 0.0f, "gfl loss: dfl_avg_factor must be nonzero");
  FRH_REQUIRE(g && fwd_out && (m == 0 || (grad_cls && grad_reg)), "gfl loss bwd: null gradient");
  if (m == 0) return FRH_OK;
  const GflScale o{cls_weight, dfl_weight, bbox_weight, dfl_avg_factor};
  hipLaunchKernelGGL(gfl_loss_bwd_kernel, dim3(loss_grid(m)), dim3(kLossThreads), 0, as_stream(stream), a, o, g,
                     fwd_out, grad_cls, gc_sk, gc_si, grad_reg, gr_sc, gr_si);
  return check_launch("frh_gfl_loss_bwd");
}

int32_t frh_dfl_decode(const float* reg, int32_t batch, int32_t bins, int32_t h, int32_t w, int64_t sb, int64_t sc,
                       int64_t sy, int64_t sx, double stride, float reg_std, float reg_mean, float cell, float img_h,
                       float img_w, float* boxes, void* stream) {
  FRH_REQUIRE(batch >= 0 && bins >= 1 && h >= 0 && w >= 0, "dfl decode: bad shape");
  if (bins * 4 > kWave) {
    set_error("dfl decode: 4 * bins = %d exceeds one wave (64 lanes)", bins * 4);
    return FRH_EUNSUPPORTED;
  }
  const int64_t total = (int64_t)batch * h * w;
  FRH_REQUIRE(total < (int64_t(1) << 31), "dfl decode: too many positions");
  if (total == 0) return FRH_OK;
  FRH_REQUIRE(reg && boxes, "dfl decode: null pointer");
  const DecodeArgs a{reg, batch, bins, h, w, sb, sc, sy, sx, stride, reg_std, reg_mean, cell, img_w - 1.0f,
                     img_h - 1.0f, boxes};
  hipStream_t s = as_stream(stream);
  if (sc == 1 && sx != 1) {
    const int64_t nb = (total + 3) / 4;
    hipLaunchKernelGGL(dfl_decode_chan_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(kLossThreads), 0, s, a);
  } else {
    const int64_t nb = (total + kLossThreads - 1) / kLossThreads;
    hipLaunchKernelGGL(dfl_decode_pos_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(kLossThreads), 0, s, a);
  }
  return check_launch("frh_dfl_decode");
}

}  // extern "C"
