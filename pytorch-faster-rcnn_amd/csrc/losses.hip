// Fused detection losses: classification (sigmoid focal,
// sigmoid BCE, softmax cross-entropy) and masked / class-selected smooth-L1
// and balanced L1, forward sums and backward gradients, straight from the
// head outputs.
//
// Reference: lib/losses.py:33-61 (sigmoid_focal_loss), :77-83
// (smooth_l1_loss_v2), :126-156 (CrossEntropyLoss), :158-180
// (balanced_l1_loss / BalancedL1Loss), and their callers
// AnchorHead.calc_loss (lib/heads/anchor_head.py:113-139) and
// BBoxHead.calc_loss (lib/heads/bbox_head.py:56-87).  The reference builds a
// one-hot target, a sigmoid, pt, a focal weight, BCE-with-logits and a sum as
// separate tensors (about a dozen elementwise passes over [n, C] forward and
// as many backward), gathers the labelled class's deltas with an advanced
// index and masks negatives by boolean indexing (a host sync).  Here each loss
// is one streaming pass: the element (i, k) of the logits is read through
// explicit strides (so the channel-major [C, S] views the target gathers
// produce need no copy), the one-hot target is the comparison label[i] == k+1,
// and the per-block partial sums are finalised in a fixed order by the last
// workgroup (deterministic; no float atomics).  Backward recomputes the
// element's derivative and writes g * dL/dx, reading the upstream gradient
// from device memory (no host sync).
//
// The forward's finalisation rides in the same launch: the arrival-counter
// fan-in of loss_common.h (fan_in) over one sum, or over two for the one-launch
// head loss; the last workgroup to arrive writes the loss and resets the
// counter (grids capped at 256 workgroups).  Each loss family has one
// accumulation loop (cls_accumulate, l1_accumulate) that its own kernel and
// the head-loss kernel both call, so the two sum the same elements in the same
// order by construction.
//
// Bytes per element: forward 4 (logit) + 8/C (label); backward 4 + 4 + 8/C.
// Numerics follow torch's formulas (binary_cross_entropy_with_logits via
// log_sigmoid, pow backward, log_softmax backward); sums differ from torch's
// reduction order in the last bits, gradients agree to a few ulp.
#include "loss_common.h"

#include <math.h>

#include <algorithm>
#include <type_traits>

namespace frh {
namespace {

enum ClsKind { kFocal = 0, kSigmoidBce = 1, kSoftmaxCe = 2 };

struct ClsArgs {
  const float* x;
  int64_t n, c, sr, sc;  // logit (i, k) at x[i*sr + k*sc]
  const void* target;    // int64 labels [n] (or float32 [n] for kSigmoidBce, C == 1)
  int32_t tfloat;
  float alpha, gamma;
  int32_t i_fast;        // element order: i fastest (channel-major views) or k fastest
};

__device__ __forceinline__ float target_at(const ClsArgs& a, int64_t i) {
  return a.tfloat ? static_cast<const float*>(a.target)[i]
                  : static_cast<float>(static_cast<const int64_t*>(a.target)[i]);
}

__device__ __forceinline__ int64_t label_at(const ClsArgs& a, int64_t i) {
  return static_cast<const int64_t*>(a.target)[i];
}

// rows labelled < 0 are padding rows of a fixed-capacity target buffer (frh_anchor_target /
// frh_bbox_target past their device count): they contribute nothing, forward or backward
// (the reference's sampled targets never carry such labels)
__device__ __forceinline__ bool ignored(const ClsArgs& a, int64_t i) { return !a.tfloat && label_at(a, i) < 0; }

// focal_elem: the sigmoid_focal_loss element and its derivative, loss_common.h

__device__ __forceinline__ void elem_index(const ClsArgs& a, int64_t e, int64_t* i, int64_t* k) {
  if (a.i_fast) {
    *k = e / a.n;
    *i = e - *k * a.n;
  } else {
    *i = e / a.c;
    *k = e - *i * a.c;
  }
}

// target of element (i, k): C == 1 sigmoid takes the label value itself
// (label.view(-1, 1).float(), losses.py:142), otherwise one-hot[:, 1:].
__device__ __forceinline__ float elem_target(const ClsArgs& a, int64_t i, int64_t k) {
  if (a.c == 1) return target_at(a, i);
  return label_at(a, i) == k + 1 ? 1.0f : 0.0f;
}

// where a one-sum forward leaves its loss
struct FanIn {
  LossWorkspace ws;
  float* out;
  const int32_t* status;  // nullable: the caller's device status word; nonzero -> NaN loss
};

// Thread 0 holds the workgroup's partial sum; the last workgroup to arrive writes the loss.
__device__ __forceinline__ void finalize_one(float block_total, const FanIn& f) {
  const float p[1] = {block_total};
  const int nb[1] = {(int)gridDim.x};
  double res[1];
  if (!fan_in(p, nb, f.ws.counter, f.ws.partial, res)) return;
  if (threadIdx.x == 0) {
    f.out[0] = status_set(f.status) ? NAN : (float)res[0];
    __hip_atomic_store(f.ws.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// This thread's share of the classification sum as workgroup b of nb: the softmax kind strides
// over rows, the sigmoid kinds over elements.
template <int kKind>
__device__ __forceinline__ float cls_accumulate(const ClsArgs& a, int b, int nb) {
  float acc = 0.0f;
  if constexpr (kKind == kSoftmaxCe) {
    for (int64_t i = b * (int64_t)kLossThreads + threadIdx.x; i < a.n; i += (int64_t)nb * kLossThreads) {
      if (ignored(a, i)) continue;
      const float* row = a.x + i * a.sr;
      float m = -INFINITY;
      for (int64_t k = 0; k < a.c; ++k) m = fmaxf(m, row[k * a.sc]);
      float s = 0.0f;
      for (int64_t k = 0; k < a.c; ++k) s += expf(row[k * a.sc] - m);
      int64_t l = label_at(a, i);
      float xl = (l >= 0 && l < a.c) ? row[l * a.sc] : NAN;
      acc += (logf(s) + m) - xl;  // -log_softmax(x)[label]
    }
  } else {
    const int64_t total = a.n * a.c;
    for (int64_t e = b * (int64_t)kLossThreads + threadIdx.x; e < total; e += (int64_t)nb * kLossThreads) {
      int64_t i, k;
      elem_index(a, e, &i, &k);
      if (ignored(a, i)) continue;
      float x = a.x[i * a.sr + k * a.sc];
      float t = elem_target(a, i, k);
      acc += kKind == kFocal ? focal_elem(x, t, a.alpha, a.gamma, nullptr) : bce_logits(x, t);
    }
  }
  return acc;
}

template <int kKind>
__global__ void __launch_bounds__(kLossThreads) cls_loss_fwd_kernel(ClsArgs a, FanIn f) {
  __shared__ float scratch[kLossThreads / kWave];
  finalize_one(block_sum_f(cls_accumulate<kKind>(a, blockIdx.x, gridDim.x), scratch), f);
}

template <int kKind>
__global__ void __launch_bounds__(kLossThreads) cls_loss_bwd_kernel(ClsArgs a, const float* gout, float* gx,
                                                                     int64_t gsr, int64_t gsc) {
  const float g = *gout;
  if constexpr (kKind == kSoftmaxCe) {
    for (int64_t i = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; i < a.n;
         i += (int64_t)gridDim.x * kLossThreads) {
      if (ignored(a, i)) {
        for (int64_t k = 0; k < a.c; ++k) gx[i * gsr + k * gsc] = 0.0f;
        continue;
      }
      const float* row = a.x + i * a.sr;
      float m = -INFINITY;
      for (int64_t k = 0; k < a.c; ++k) m = fmaxf(m, row[k * a.sc]);
      float s = 0.0f;
      for (int64_t k = 0; k < a.c; ++k) s += expf(row[k * a.sc] - m);
      float ls = logf(s);
      int64_t l = label_at(a, i);
      // log_softmax backward: g_k - exp(logp_k) * sum(g), with g = -g at the label
      for (int64_t k = 0; k < a.c; ++k) {
        float sm = expf((row[k * a.sc] - m) - ls);
        gx[i * gsr + k * gsc] = (k == l ? -g : 0.0f) + sm * g;
      }
    }
  } else {
    const int64_t total = a.n * a.c;
    for (int64_t e = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * kLossThreads) {
      int64_t i, k;
      elem_index(a, e, &i, &k);
      if (ignored(a, i)) {
        gx[i * gsr + k * gsc] = 0.0f;
        continue;
      }
      float x = a.x[i * a.sr + k * a.sc];
      float t = elem_target(a, i, k);
      float d;
      if (kKind == kFocal)
        focal_elem(x, t, a.alpha, a.gamma, &d);
      else
        d = sigmoidf(x) - t;
      gx[i * gsr + k * gsc] = g * d;
    }
  }
}

struct L1Args {
  const float* x;
  int64_t xs_i, xs_j, xs_l;  // x(i, j) at x[i*xs_i + j*xs_j + label[i]*xs_l]
  const float* y;
  int64_t ys_i, ys_j;
  const int64_t* label;      // optional: rows with label <= 0 contribute nothing
  int64_t n, m, n_sel;       // rows, columns per row, selectable classes (label < n_sel)
  float beta;
};

// row i of a regression loss: masked out, or the offset of its (class-selected) first element
__device__ __forceinline__ bool l1_row(const L1Args& a, int64_t i, int64_t* off) {
  int64_t l = a.label ? a.label[i] : 0;
  if (a.label && l <= 0) return false;
  *off = i * a.xs_i + (a.xs_l ? l * a.xs_l : 0);
  return true;
}

// The regression element as a function of d = |x - y| and its slope; the kernels below are
// shared by every such loss (strided access, label mask / class select, status-word NaN,
// in-launch finalisation).
struct SmoothL1Elem {  // smooth_l1_loss_v2 (losses.py:77-83)
  float beta;
  __device__ __forceinline__ float value(float d) const { return d < beta ? (d * d) / (2.0f * beta) : d - 0.5f * beta; }
  __device__ __forceinline__ float slope(float d) const { return d < beta ? (2.0f * d) / (2.0f * beta) : 1.0f; }
};

// balanced_l1_loss (losses.py:158-168), in the reference's operation order with its Python
// scalars rounded to f32 as torch does: d < beta ? alpha / b * (b * d + 1) * log(b * d / beta + 1)
// - alpha * d : gamma * d + gamma / b - alpha * beta, b = e^(gamma / alpha) - 1.
struct BalancedL1Elem {
  float beta, alpha, gamma, b, a_over_b, g_over_b, ab;
  __device__ __forceinline__ float value(float d) const {
    const float bd = b * d;
    return d < beta ? (a_over_b * (bd + 1.0f)) * logf(bd / beta + 1.0f) - alpha * d : (gamma * d + g_over_b) - ab;
  }
  // d/dd of the above: alpha * log(b d / beta + 1) + alpha (b d + 1) / (b d + beta) - alpha, or gamma
  __device__ __forceinline__ float slope(float d) const {
    const float bd = b * d;
    return d < beta ? (alpha * logf(bd / beta + 1.0f) + (alpha * (bd + 1.0f)) / (bd + beta)) - alpha : gamma;
  }
};

// this thread's share of the regression sum as workgroup b of nb
template <class Elem>
__device__ __forceinline__ float l1_accumulate(const L1Args& a, const Elem& el, int b, int nb) {
  float acc = 0.0f;
  const int64_t total = a.n * a.m;
  for (int64_t e = b * (int64_t)kLossThreads + threadIdx.x; e < total; e += (int64_t)nb * kLossThreads) {
    int64_t i = e / a.m, j = e - i * a.m, off;
    if (!l1_row(a, i, &off)) continue;
    if (a.xs_l && (a.label[i] >= a.n_sel)) {
      acc += NAN;
      continue;
    }
    float d = fabsf(a.x[off + j * a.xs_j] - a.y[i * a.ys_i + j * a.ys_j]);
    acc += el.value(d);
  }
  return acc;
}

template <class Elem>
__global__ void __launch_bounds__(kLossThreads) l1_fwd_kernel(L1Args a, Elem el, FanIn f) {
  __shared__ float scratch[kLossThreads / kWave];
  finalize_one(block_sum_f(l1_accumulate(a, el, blockIdx.x, gridDim.x), scratch), f);
}

// gx must be zero-filled by the caller: only the selected, unmasked elements are written.
template <class Elem>
__global__ void __launch_bounds__(kLossThreads) l1_bwd_kernel(L1Args a, Elem el, const float* gout, float* gx,
                                                              int64_t gs_i, int64_t gs_j, int64_t gs_l) {
  const float g = *gout;
  const int64_t total = a.n * a.m;
  for (int64_t e = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kLossThreads) {
    int64_t i = e / a.m, j = e - i * a.m, off;
    if (!l1_row(a, i, &off)) continue;
    int64_t l = a.xs_l ? a.label[i] : 0;
    if (l >= a.n_sel) continue;
    float diff = a.x[off + j * a.xs_j] - a.y[i * a.ys_i + j * a.ys_j];
    float d = fabsf(diff);
    float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
    float dd = el.slope(d);
    gx[i * gs_i + j * gs_j + l * gs_l] = g * dd * sgn;
  }
}

// Classification + regression loss of one head in ONE launch (AnchorHead / BBoxHead
// calc_loss with a sampler: anchor_head.py:113-139, bbox_head.py:56-87).  Workgroup b
// takes the cls elements of workgroup b of cls_loss_fwd_kernel's grid (b < nbc) and the
// smooth-L1 elements of workgroup b of l1_fwd_kernel<SmoothL1Elem>'s grid (b < nbr); the last
// workgroup to arrive sums each loss's nbc / nbr partials in fan_in's fixed order, so both
// sums equal the separate launches' bit for bit, and applies the heads' scaling as torch
// does it: loss = (sum * loss_weight) / avg_factor in f32.
struct DetScale {
  float wc, dc, wr, dr;
  float* out;             // [2]: cls, reg
  const int32_t* ndev;    // nullable: avg_factor = this device count for both (0 -> zero losses)
  const int32_t* status;  // nullable: device status word; nonzero -> NaN losses
};

template <int kKind>
__global__ void __launch_bounds__(kLossThreads) det_loss_fwd_kernel(ClsArgs a, int nbc, L1Args r, int nbr,
                                                                    LossWorkspace ws, DetScale o) {
  __shared__ float scratch[kLossThreads / kWave];
  const int b = blockIdx.x;
  const float acc = b < nbc ? cls_accumulate<kKind>(a, b, nbc) : 0.0f;
  const float accr = b < nbr ? l1_accumulate(r, SmoothL1Elem{r.beta}, b, nbr) : 0.0f;
  const float pc = block_sum_f(acc, scratch);
  __syncthreads();
  const float p[2] = {pc, block_sum_f(accr, scratch)};
  const int nb[2] = {nbc, nbr};
  double sum[2];
  if (!fan_in(p, nb, ws.counter, ws.partial, sum)) return;
  if (threadIdx.x == 0) {
    const float res[2] = {(float)sum[0], (float)sum[1]};
    if (o.ndev) {
      const int32_t nd = *o.ndev;
      const float d = (float)nd;
      o.out[0] = nd ? (res[0] * o.wc) / d : 0.0f;
      o.out[1] = nd ? (res[1] * o.wr) / d : 0.0f;
    } else {
      o.out[0] = (res[0] * o.wc) / o.dc;
      o.out[1] = (res[1] * o.wr) / o.dr;
    }
    if (status_set(o.status)) o.out[0] = o.out[1] = NAN;
    __hip_atomic_store(ws.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// f(std::integral_constant<int, kind>()) for a kind that check_cls has passed
template <class F>
void dispatch_kind(int32_t kind, F f) {
  if (kind == kFocal)
    f(std::integral_constant<int, kFocal>());
  else if (kind == kSigmoidBce)
    f(std::integral_constant<int, kSigmoidBce>());
  else
    f(std::integral_constant<int, kSoftmaxCe>());
}

// the grid of a classification forward or backward: softmax strides over rows
int cls_grid(int32_t kind, const ClsArgs& a) { return loss_grid(kind == kSoftmaxCe ? a.n : a.n * a.c); }

int32_t check_cls(int32_t kind, const ClsArgs& a) {
  FRH_REQUIRE(kind >= kFocal && kind <= kSoftmaxCe, "cls loss: unknown kind %d", kind);
  FRH_REQUIRE(a.n >= 0 && a.c >= 1, "cls loss: bad shape [%lld, %lld]", (long long)a.n, (long long)a.c);
  FRH_REQUIRE(a.n * a.c < (int64_t(1) << 40), "cls loss: too many elements");
  FRH_REQUIRE(a.n == 0 || (a.x && a.target), "cls loss: null input");
  FRH_REQUIRE(!a.tfloat || (kind == kSigmoidBce && a.c == 1),
              "cls loss: float targets only for single-channel sigmoid BCE");
  return FRH_OK;
}

ClsArgs make_cls(const float* x, int64_t n, int64_t c, int64_t sr, int64_t sc, const void* target,
                 int32_t tfloat, float alpha, float gamma) {
  ClsArgs a;
  a.x = x;
  a.n = n;
  a.c = c;
  a.sr = sr;
  a.sc = sc;
  a.target = target;
  a.tfloat = tfloat;
  a.alpha = alpha;
  a.gamma = gamma;
  a.i_fast = (sr < sc) ? 1 : 0;
  return a;
}

int32_t check_l1(const L1Args& a) {
  FRH_REQUIRE(a.n >= 0 && a.m >= 1, "smooth l1: bad shape");
  FRH_REQUIRE(a.beta > 0.0f, "smooth l1: beta must be > 0");
  FRH_REQUIRE(a.n == 0 || (a.x && a.y), "smooth l1: null input");
  FRH_REQUIRE(a.xs_l == 0 || a.label, "smooth l1: class selection needs labels");
  FRH_REQUIRE(a.n_sel >= 1, "smooth l1: n_sel must be >= 1");
  return FRH_OK;
}

L1Args make_l1(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* y, int64_t ys_i,
               int64_t ys_j, const int64_t* label, int64_t n, int64_t m, int64_t n_sel, float beta) {
  L1Args a;
  a.x = x;
  a.xs_i = xs_i;
  a.xs_j = xs_j;
  a.xs_l = xs_l;
  a.y = y;
  a.ys_i = ys_i;
  a.ys_j = ys_j;
  a.label = label;
  a.n = n;
  a.m = m;
  a.n_sel = n_sel;
  a.beta = beta;
  return a;
}

// The element of an entry's (beta, alpha, gamma): smooth L1 takes beta alone.
int32_t make_elem(float beta, float, float, SmoothL1Elem* el) {
  *el = SmoothL1Elem{beta};
  return FRH_OK;
}

int32_t make_elem(float beta, float alpha, float gamma, BalancedL1Elem* el) {
  FRH_REQUIRE(alpha > 0.0f && gamma > 0.0f, "balanced l1: alpha and gamma must be > 0");
  const double b = exp((double)gamma / (double)alpha) - 1.0;
  *el = BalancedL1Elem{beta, alpha, gamma, (float)b, (float)((double)alpha / b), (float)((double)gamma / b),
                       (float)((double)alpha * (double)beta)};
  return FRH_OK;
}

// The bodies of frh_smooth_l1_* and frh_balanced_l1_*; `what` names the loss in a refusal, `entry`
// the entry point in a launch error.
template <class Elem>
int32_t l1_fwd(const L1Args& a, float alpha, float gamma, const int32_t* status, float* out, void* workspace,
               size_t ws_bytes, void* stream, const char* what, const char* entry) {
  int32_t st = check_l1(a);
  if (st != FRH_OK) return st;
  Elem el;
  st = make_elem(a.beta, alpha, gamma, &el);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(out, "%s: null output", what);
  LossWorkspace ws;
  st = split_workspace(workspace, ws_bytes, what, &ws);
  if (st != FRH_OK) return st;
  hipLaunchKernelGGL(l1_fwd_kernel<Elem>, dim3(loss_grid(a.n * a.m)), dim3(kLossThreads), 0, as_stream(stream), a, el,
                     FanIn{ws, out, status});
  return check_launch(entry);
}

template <class Elem>
int32_t l1_bwd(const L1Args& a, float alpha, float gamma, const float* grad_out, float* grad_x, int64_t gs_i,
               int64_t gs_j, int64_t gs_l, void* stream, const char* entry) {
  int32_t st = check_l1(a);
  if (st != FRH_OK) return st;
  Elem el;
  st = make_elem(a.beta, alpha, gamma, &el);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(grad_out && (a.n == 0 || grad_x), "l1 bwd: null gradient");
  if (a.n == 0) return FRH_OK;
  hipLaunchKernelGGL(l1_bwd_kernel<Elem>, dim3(loss_grid(a.n * a.m)), dim3(kLossThreads), 0, as_stream(stream), a, el,
                     grad_out, grad_x, gs_i, gs_j, gs_l);
  return check_launch(entry);
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" {

size_t frh_loss_workspace(void) { return kLossWorkspaceBytes; }

int32_t frh_cls_loss_fwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr, int64_t sc,
                         const void* target, int32_t target_is_float, float alpha, float gamma,
                         const int32_t* status, float* out, void* workspace, size_t ws_bytes, void* stream) {
  ClsArgs a = make_cls(x, n, c, sr, sc, target, target_is_float, alpha, gamma);
  int32_t st = check_cls(kind, a);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(out, "cls loss: null output");
  LossWorkspace ws;
  st = split_workspace(workspace, ws_bytes, "cls loss", &ws);
  if (st != FRH_OK) return st;
  const FanIn f{ws, out, status};
  dispatch_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(cls_loss_fwd_kernel<k()>, dim3(cls_grid(kind, a)), dim3(kLossThreads), 0, as_stream(stream), a,
                       f);
  });
  return check_launch("frh_cls_loss_fwd");
}

int32_t frh_cls_loss_bwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr, int64_t sc,
                         const void* target, int32_t target_is_float, float alpha, float gamma,
                         const float* grad_out, float* grad_x, int64_t gsr, int64_t gsc, void* stream) {
  ClsArgs a = make_cls(x, n, c, sr, sc, target, target_is_float, alpha, gamma);
  int32_t st = check_cls(kind, a);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(grad_out && (n == 0 || grad_x), "cls loss bwd: null gradient");
  if (n == 0) return FRH_OK;
  dispatch_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(cls_loss_bwd_kernel<k()>, dim3(cls_grid(kind, a)), dim3(kLossThreads), 0, as_stream(stream), a,
                       grad_out, grad_x, gsr, gsc);
  });
  return check_launch("frh_cls_loss_bwd");
}

int32_t frh_smooth_l1_fwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* y, int64_t ys_i,
                          int64_t ys_j, const int64_t* label, int64_t n, int64_t m, int64_t n_sel, float beta,
                          const int32_t* status, float* out, void* workspace, size_t ws_bytes, void* stream) {
  return l1_fwd<SmoothL1Elem>(make_l1(x, xs_i, xs_j, xs_l, y, ys_i, ys_j, label, n, m, n_sel, beta), 0.0f, 0.0f,
                              status, out, workspace, ws_bytes, stream, "smooth l1", "frh_smooth_l1_fwd");
}

int32_t frh_balanced_l1_fwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* y, int64_t ys_i,
                            int64_t ys_j, const int64_t* label, int64_t n, int64_t m, int64_t n_sel, float beta,
                            float alpha, float gamma, const int32_t* status, float* out, void* workspace,
                            size_t ws_bytes, void* stream) {
  return l1_fwd<BalancedL1Elem>(make_l1(x, xs_i, xs_j, xs_l, y, ys_i, ys_j, label, n, m, n_sel, beta), alpha, gamma,
                                status, out, workspace, ws_bytes, stream, "balanced l1", "frh_balanced_l1_fwd");
}

int32_t frh_det_loss_fwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr, int64_t sc,
                         const void* target, int32_t target_is_float, float alpha, float gamma, float cls_weight,
                         float cls_div, const float* rx, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* ry,
                         int64_t ys_i, int64_t ys_j, const int64_t* label, int64_t rn, int64_t rm, int64_t n_sel,
                         float beta, float reg_weight, float reg_div, const int32_t* div_count,
                         const int32_t* status, float* out, void* workspace, size_t ws_bytes, void* stream) {
  ClsArgs a = make_cls(x, n, c, sr, sc, target, target_is_float, alpha, gamma);
  int32_t st = check_cls(kind, a);
  if (st != FRH_OK) return st;
  L1Args r = make_l1(rx, xs_i, xs_j, xs_l, ry, ys_i, ys_j, label, rn, rm, n_sel, beta);
  st = check_l1(r);
  if (st != FRH_OK) return st;
  FRH_REQUIRE(out, "det loss: null output");
  LossWorkspace ws;
  st = split_workspace(workspace, ws_bytes, "det loss", &ws);
  if (st != FRH_OK) return st;
  const int nbc = cls_grid(kind, a), nbr = loss_grid(rn * rm);
  const DetScale o{cls_weight, cls_div, reg_weight, reg_div, out, div_count, status};
  dispatch_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(det_loss_fwd_kernel<k()>, dim3((unsigned)std::max(nbc, nbr)), dim3(kLossThreads), 0,
                       as_stream(stream), a, nbc, r, nbr, ws, o);
  });
  return check_launch("frh_det_loss_fwd");
}

int32_t frh_smooth_l1_bwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* y, int64_t ys_i,
                          int64_t ys_j, const int64_t* label, int64_t n, int64_t m, int64_t n_sel, float beta,
                          const float* grad_out, float* grad_x, int64_t gs_i, int64_t gs_j, int64_t gs_l,
                          void* stream) {
  return l1_bwd<SmoothL1Elem>(make_l1(x, xs_i, xs_j, xs_l, y, ys_i, ys_j, label, n, m, n_sel, beta), 0.0f, 0.0f,
                              grad_out, grad_x, gs_i, gs_j, gs_l, stream, "frh_smooth_l1_bwd");
}

int32_t frh_balanced_l1_bwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l, const float* y, int64_t ys_i,
                            int64_t ys_j, const int64_t* label, int64_t n, int64_t m, int64_t n_sel, float beta,
                            float alpha, float gamma, const float* grad_out, float* grad_x, int64_t gs_i,
                            int64_t gs_j, int64_t gs_l, void* stream) {
  return l1_bwd<BalancedL1Elem>(make_l1(x, xs_i, xs_j, xs_l, y, ys_i, ys_j, label, n, m, n_sel, beta), alpha, gamma,
                                grad_out, grad_x, gs_i, gs_j, gs_l, stream, "frh_balanced_l1_bwd");
}

}  // extern "C"
