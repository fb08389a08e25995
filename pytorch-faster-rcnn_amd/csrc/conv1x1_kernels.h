// 1x1 / stride-1 convolution on NCHW f32 with the frozen-BN (+ residual) (+ ReLU) epilogue
// of bn_act.hip applied to the accumulator tile: per image a GEMM
//   Y[cout, hw] = W[cout, cin] . X[cin, hw]
// on v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fmaf chain).  cout is the MFMA row
// (register) dimension, so s[co] / b[co] are per-register constants; pixels are the column
// (lane) dimension, so X fragments, skip reads and Y stores are 128-byte row segments of the
// NCHW planes.
//
// Work split: 256 threads = 2 x 2 waves, one 32 x 32 accumulator tile each; the workgroup
// owns a 64 (cout) x 64 (pixels) output tile of one image and walks cin in steps of BK (32,
// or 16 for short sums).  Measured on MI355X at the ResNet-50 shapes, 64 x 64 beat 64 x 128
// and 128 x 128 workgroup tiles at every shape: the kernel runs on the many small workgroups
// a CU holds at once (4 to 6 per SIMD), not on reuse inside one.  Both operands go global ->
// registers -> LDS (two buffers, one barrier per step; the loads of step t + 1 are in flight
// while step t runs its MFMAs):
//   W tile [64][BK] at pitch BK + 4 floats: a lane's 8 k-values are two ds_read_b128, and the
//     16 rows of one ds_read_b128 lane group start in 16 distinct 4-bank groups;
//   X tile [BK][64] at pitch 68: a ds_read_b32 is served per lane half, each half reading 32
//     consecutive floats of one row.
// Inside a step lane half h owns k = h BK/2 .. h BK/2 + BK/2 - 1 (a fixed permutation of the
// k order: the sum is over the same products, and the order is the same on every launch).
// s and b of the tile's 64 channels are computed once per workgroup into LDS (bn_fold.h holds
// the BN arithmetic of every form).  Workgroups are numbered cout-tile fastest and dealt to the
// 8 XCDs in contiguous chunks, so the cout tiles that re-read one X tile run on one L2.
//
// Two input-side forms of the same kernel (template flags; the plain instantiations compile
// to what they were):
//   PRE: the frozen BN (+ ReLU) that precedes the convolution (a bottleneck's bn2 in front of
//     conv3) applied to the X registers between the global load and the LDS write, s_in / b_in
//     of all cin channels computed once per workgroup into LDS: the bits of frh_bn_act
//     followed by the plain kernel, without that pass.
//   S2: the X tile gathered from x[:, :, ::2, ::2] of an NCHW input (a stride-2 projection).
//     With w_out % 4 == 0 a thread's four output pixels lie in one input row and are the
//     .x / .z of two aligned float4 loads: the bits of the plain kernel on a contiguous copy
//     of the subsampled input.
#pragma once
#include "bn_fold.h"

namespace frh {

constexpr int kCxThreads = 256;
constexpr int kCxTile = 64;  // outputs per workgroup: kCxTile channels x kCxTile pixels
constexpr int kCxXcds = 8;
constexpr int kCxPreMax = 512;  // cin bound of the PRE form (s_in / b_in in LDS: 4 KB)

struct Conv1x1Args {
  const float* x;
  const float* w;
  const float* skip;
  float* y;
  FrozenBN bn;
  int cin, cout;
  int64_t hw;
  int mt, pt;     // cout tiles, pixel tiles per image
  int64_t total;  // mt * pt * n
  int64_t chunk;  // ceil(total / kCxXcds)
  int relu;
  // PRE: the BN in front of the convolution
  FrozenBN pre;
  int pre_relu;
  // S2: the input plane (hw is the output plane, w_out its row length)
  int64_t in_hw;
  int in_w, w_out;
};

template <int BK, bool PRE = false, bool S2 = false>
__global__ void __launch_bounds__(kCxThreads) conv1x1_bn_act_kernel(const Conv1x1Args a) {
  constexpr int T = kCxTile, PA = BK + 4, PB = T + 4, HK = BK / 2;
  constexpr int NV = T * (BK / 4) / kCxThreads;  // float4 of W, and of X, per thread per step
  static_assert(NV == 1 || NV == 2, "staging registers are written out for one or two float4");
  constexpr int A_ROWS = kCxThreads / (BK / 4), B_ROWS = kCxThreads / (T / 4);
  __shared__ __attribute__((aligned(16))) float As[2][T * PA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * PB];
  __shared__ float bn_s[T], bn_b[T];
  __shared__ float pre_s[PRE ? kCxPreMax : 1], pre_b[PRE ? kCxPreMax : 1];

  // XCD x takes logical workgroups [x * chunk, (x + 1) * chunk)
  const int64_t wg = (int64_t)(blockIdx.x % kCxXcds) * a.chunk + blockIdx.x / kCxXcds;
  if (wg >= a.total) return;
  const int m_tile = (int)(wg % a.mt);
  const int64_t rest = wg / a.mt;
  const int p_tile = (int)(rest % a.pt);
  const int64_t img = rest / a.pt;
  const int m0 = m_tile * T;
  const int64_t p0 = (int64_t)p_tile * T;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;

  // read in the epilogue, after the main loop's barriers
  const bool bn = a.bn.mean != nullptr;
  if (bn && tid < T) bn_fold(a.bn, m0 + tid, bn_s[tid], bn_b[tid]);

  if constexpr (PRE) {
    for (int c = tid; c < a.cin; c += kCxThreads) bn_fold(a.pre, c, pre_s[c], pre_b[c]);
    __syncthreads();  // step 0 transforms its registers before the loop's first barrier
  }

  // staging: thread t moves float4 t (and t + 256) of each tile; W rows are BK / 4 float4
  // long, X rows 16.  Pixels past the plane's end stay zero (their columns are never stored,
  // so what the PRE transform makes of those zeros does not matter).
  const int a_row = tid / (BK / 4), a_q = tid % (BK / 4);
  const int b_row = tid / (T / 4), b_q = tid % (T / 4);
  const float* wp = a.w + (int64_t)(m0 + a_row) * a.cin + a_q * 4;
  const bool p_ok = p0 + b_q * 4 < a.hw;
  const float* xp;
  if constexpr (S2) {
    const int64_t pq = p0 + b_q * 4, oy = pq / a.w_out, ox = pq - oy * a.w_out;
    xp = a.x + (img * a.cin + b_row) * a.in_hw + 2 * oy * a.in_w + 2 * ox;
  } else {
    xp = a.x + (img * a.cin + b_row) * a.hw + p0 + b_q * 4;
  }
  const int64_t xs = S2 ? a.in_hw : a.hw;  // X plane stride
  const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 ra0, ra1 = z4, rb0 = z4, rb1 = z4;
  float4 rc0 = z4, rc1 = z4;  // S2: input columns 4 .. 7 of the thread's eight
#define FRH_CX_LOAD(k0)                                                                         \
  do {                                                                                          \
    ra0 = *reinterpret_cast<const float4*>(wp + (k0));                                          \
    if (NV > 1) ra1 = *reinterpret_cast<const float4*>(wp + (int64_t)A_ROWS * a.cin + (k0));    \
    if (p_ok) {                                                                                 \
      rb0 = *reinterpret_cast<const float4*>(xp + (int64_t)(k0)*xs);                            \
      if (NV > 1) rb1 = *reinterpret_cast<const float4*>(xp + (int64_t)((k0) + B_ROWS) * xs);   \
      if (S2) {                                                                                 \
        rc0 = *reinterpret_cast<const float4*>(xp + (int64_t)(k0)*xs + 4);                      \
        if (NV > 1) rc1 = *reinterpret_cast<const float4*>(xp + (int64_t)((k0) + B_ROWS) * xs + 4); \
      }                                                                                         \
    }                                                                                           \
  } while (0)

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  const int steps = a.cin / BK;
  FRH_CX_LOAD(0);
  for (int t = 0; t < steps; ++t) {
    const int buf = t & 1;
    // buffer buf was last read in step t - 2, which every wave left before the barrier of step t - 1
    *reinterpret_cast<float4*>(&As[buf][a_row * PA + a_q * 4]) = ra0;
    if (NV > 1) *reinterpret_cast<float4*>(&As[buf][(a_row + A_ROWS) * PA + a_q * 4]) = ra1;
    float4 vb0 = S2 ? make_float4(rb0.x, rb0.z, rc0.x, rc0.z) : rb0;
    float4 vb1 = S2 ? make_float4(rb1.x, rb1.z, rc1.x, rc1.z) : rb1;
    if constexpr (PRE) {
      const int c = t * BK + b_row;
      vb0 = bn_apply(vb0, true, &pre_s[c], &pre_b[c], false, nullptr, a.pre_relu);
      if (NV > 1) vb1 = bn_apply(vb1, true, &pre_s[c + B_ROWS], &pre_b[c + B_ROWS], false, nullptr, a.pre_relu);
    }
    *reinterpret_cast<float4*>(&Bs[buf][b_row * PB + b_q * 4]) = vb0;
    if (NV > 1) *reinterpret_cast<float4*>(&Bs[buf][(b_row + B_ROWS) * PB + b_q * 4]) = vb1;
    __syncthreads();
    if (t + 1 < steps) FRH_CX_LOAD((t + 1) * BK);  // in flight behind this step's MFMAs
#pragma unroll
    for (int q = 0; q < HK / 8; ++q) {
      const float* ap = &As[buf][(wm * 32 + j) * PA + h * HK + q * 8];
      const float4 lo = *reinterpret_cast<const float4*>(ap);
      const float4 hi = *reinterpret_cast<const float4*>(ap + 4);
      const float af[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      float bf[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) bf[s] = Bs[buf][(h * HK + q * 8 + s) * PB + wn * 32 + j];
#pragma unroll
      for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
    }
  }
#undef FRH_CX_LOAD

  // epilogue: bn_fold.h's bn_apply on the accumulator; register r of the 32 x 32 tile is row
  // mfma32_row(r) + 4 h, column j.
  const int64_t p = p0 + wn * 32 + j;
  if (p >= a.hw) return;
  const int lrow = wm * 32 + 4 * h;
  const int64_t off = (img * a.cout + m0 + lrow) * a.hw + p;
  float k[16];
  if (a.skip) {
#pragma unroll
    for (int r = 0; r < 16; ++r) k[r] = a.skip[off + (int64_t)mfma32_row(r) * a.hw];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int lr = lrow + mfma32_row(r);
    a.y[off + (int64_t)mfma32_row(r) * a.hw] =
        bn_apply(acc[r], bn, &bn_s[lr], &bn_b[lr], a.skip != nullptr, &k[r], a.relu);
  }
}

// cin per step: 32 from cin = 128 on, 16 for shorter sums (and for cin % 32 != 0); measured,
// tools/bench_conv1x1.py.
inline int conv1x1_pick_step(int32_t cin) { return cin >= 128 && cin % 32 == 0 ? 32 : 16; }

// The input-side forms: pre.mean != NULL is PRE, in_w > 0 is S2 (x is [n, cin, in_h, in_w] with
// in_w % 8 == 0, hw the output plane ((in_h + 1) / 2) * (in_w / 2)); not both.
inline int32_t conv1x1_launch(const char* what, int step, const float* x, const float* w, const float* skip, float* y,
                              FrozenBN bn, int64_t n, int32_t cin, int32_t cout, int64_t hw, int32_t relu,
                              void* stream, FrozenBN pre = {}, int32_t pre_relu = 0, int32_t in_h = 0,
                              int32_t in_w = 0) {
  const bool s2 = in_w > 0;
  FRH_REQUIRE(n >= 0 && cin >= 1 && cout >= 1 && hw >= 0, "bad sizes");
  if (n == 0 || hw == 0) return FRH_OK;
  FRH_REQUIRE(x && w && y, "null pointer argument");
  FRH_REQUIRE_BN_PAIR(bn);
  FRH_REQUIRE(hw % 4 == 0, "plane size %lld must be a multiple of 4", (long long)hw);
  FRH_REQUIRE(cin % 16 == 0 && cout % kCxTile == 0, "cin %d must be a multiple of 16 and cout %d of 64", cin, cout);
  FRH_REQUIRE_ALIGNED16(x, y, skip, w);
  const int64_t in_hw = s2 ? (int64_t)in_h * in_w : hw, yb = n * cout * hw * 4;
  FRH_REQUIRE(!ranges_overlap(y, yb, x, n * cin * in_hw * 4) && !ranges_overlap(y, yb, w, (int64_t)cout * cin * 4) &&
                  !(skip && ranges_overlap(y, yb, skip, yb)),
              "y must not alias x, w or skip");
  FRH_REQUIRE((step == 16 || step == 32) && cin % step == 0, "step %d does not fit cin %d", step, cin);
  FRH_REQUIRE(!(pre.mean && s2), "the input BN and the stride-2 gather are separate forms");
  FRH_REQUIRE(!pre.mean || cin <= kCxPreMax, "cin %d above the input BN form's bound %d", cin, kCxPreMax);
  Conv1x1Args a;
  a.x = x, a.w = w, a.skip = skip, a.y = y, a.bn = bn, a.pre = pre, a.pre_relu = pre_relu;
  a.in_hw = in_hw, a.in_w = in_w, a.w_out = in_w / 2;
  a.cin = cin, a.cout = cout, a.hw = hw, a.relu = relu;
  a.mt = cout / kCxTile;
  const int64_t pt = (hw + kCxTile - 1) / kCxTile;
  FRH_REQUIRE(pt < ((int64_t)1 << 31), "too many pixel tiles");
  a.pt = (int)pt;
  a.total = (int64_t)a.mt * pt * n;
  a.chunk = (a.total + kCxXcds - 1) / kCxXcds;
  FRH_REQUIRE(a.chunk * kCxXcds < ((int64_t)1 << 31), "too many blocks");
  const dim3 grid((unsigned)(a.chunk * kCxXcds)), block(kCxThreads);
  auto go = [&](auto k16, auto k32) {
    hipLaunchKernelGGL(step == 32 ? k32 : k16, grid, block, 0, as_stream(stream), a);
  };
  if (pre.mean)
    go(conv1x1_bn_act_kernel<16, true, false>, conv1x1_bn_act_kernel<32, true, false>);
  else if (s2)
    go(conv1x1_bn_act_kernel<16, false, true>, conv1x1_bn_act_kernel<32, false, true>);
  else
    go(conv1x1_bn_act_kernel<16, false, false>, conv1x1_bn_act_kernel<32, false, false>);
  return check_launch(what);
}

}  // namespace frh
