// 3x3 / stride-1 / padding-1 convolution on contiguous NCHW f32 with the frozen-BN (+ ReLU)
// epilogue of bn_act.hip on the accumulators (the bottlenecks' conv2), as Winograd
// F(2x2, 3x3) with the matrices of conv3x3_wino_kernels.h:
//   U = G g G^T      per (cin, cout): the 4 x 4 transformed filter (conv3x3_nchw_weights_kernel)
//   V = B^T d B      per (cin, tile): the 4 x 4 transformed input patch of a 2 x 2 output tile
//   M_p = U_p . V_p  per Winograd position p of 16: a GEMM [cout, cin] x [cin, tile]
//   Y = A^T M A      per (cout, tile): the 2 x 2 outputs, then BN, then ReLU
//
// The 16 GEMMs run on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain).  cout is the
// MFMA row (register) dimension and tiles are the column (lane) dimension, as in the 1x1
// kernel: lane (q = lane >> 4, t = lane & 15) holds channels 4 q .. 4 q + 3 of a 16-channel
// block for tile t of a run of 16 tiles along w, for all 16 positions.  So the output
// transform, s[co] / b[co] and the ReLU are register-local, a patch row is a run along w of one
// NCHW plane (16 lanes read 128 contiguous bytes) and so is an output row.
//
// Forms 0 .. 2: one wave is one work item and waves do not talk to each other: there is no LDS
// and no barrier.  (Forms 3 and 4 split cin across the waves of a workgroup; see
// conv3x3_nchw_wg_kernel.)  A wave owns NT vertically adjacent 16-tile runs (a 32 x 2 NT pixel block of one
// image) x NC 16-channel blocks, 64 NT NC accumulator registers, and walks cin in steps of 4
// (the MFMA's k): in a step lane (q, t) loads the (2 NT + 2) x 4 patch of channel k + q
// around its tiles (an aligned float2 and the two neighbours per row), zeroes what lies
// outside the plane, applies B^T d B in registers (the B operand: V_p[k + q][t]), loads
// U[k + q][co][0 .. 15] for its row of each channel block (64 contiguous bytes, the order the
// weights kernel wrote: the A operand U_p[co][k + q]) and issues 16 NT NC MFMAs.  The loads of
// step s + 1 are issued before the MFMAs of step s.  The template is instantiated at
// (NT, NC) = (2, 1) and (1, 2): 128 accumulators, two waves per SIMD; and (1, 1): 64, three.
// The smallest form costs more loads and transform arithmetic per MFMA and gives the chip twice
// as many work items; conv3x3_nchw_pick_form holds the measured choice per class.
// The four waves of a workgroup are consecutive work items, channel block fastest, so they
// read the same patch through one L1.
//
// Pixels outside the plane are the zero padding: their loads go to a clamped address and are
// zeroed; stores past the plane's edge are masked; tile blocks that overhang the plane are
// normal.  Fixed summation order (cin ascending; in the split forms each range ascending, then the
// ranges in order), no atomics: the same inputs give the same bits on every launch and an
// image's bits do not depend on n.
#pragma once
#include "bn_fold.h"
#include "cdna.h"

namespace frh {

constexpr int kNwThreads = 256;  // four independent waves
constexpr int kNwForms = 5;  // 0 .. 2: one wave per work item; 3, 4: cin split across a workgroup

struct Conv3x3NchwArgs {
  const float* x;
  const float* u;  // transformed weights [cin][cout][16]
  float* y;
  FrozenBN bn;
  int32_t cin, cout, h, w;
  int32_t cb, bx, by;  // channel blocks; tile blocks across and down one image
  int32_t relu;
  int32_t total;       // work items: cb * bx * by * n
};

// U = G g G^T of w [cout][cin][3][3] into [cin][cout][16] (position a * 4 + b).  One thread per
// (cout, cin): 9 floats in (a wave reads 2304 contiguous bytes), four float4 out.
static __global__ void __launch_bounds__(256) conv3x3_nchw_weights_kernel(const float* __restrict__ w, float* __restrict__ u,
                                                                   int cin, int cout) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)cin * cout) return;
  const int ci = (int)(idx % cin), co = (int)(idx / cin);
  const float* wp = w + idx * 9;
  float g[3][3];
#pragma unroll
  for (int i = 0; i < 9; ++i) g[i / 3][i % 3] = wp[i];
  float t[4][3];  // G g
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const float s = g[0][kx] + g[2][kx];
    t[0][kx] = g[0][kx];
    t[1][kx] = (s + g[1][kx]) * 0.5f;
    t[2][kx] = (s - g[1][kx]) * 0.5f;
    t[3][kx] = g[2][kx];
  }
  float* up = u + ((int64_t)ci * cout + co) * 16;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float s = t[a][0] + t[a][2];
    *reinterpret_cast<float4*>(up + a * 4) =
        make_float4(t[a][0], (s + t[a][1]) * 0.5f, (s - t[a][1]) * 0.5f, t[a][2]);
  }
}

// Loads go through buffer descriptors: a step's four channel planes (or its four rows of U) are
// one wave-uniform descriptor in SGPRs and the lane's part is a 32-bit offset, so a load is
// buffer_load with no per-lane 64-bit address (as plain pointers the compiler kept one 64-bit
// lane address per load, formed by a 64-bit add each step, and an integer turned pointer made
// them flat loads, which count in lgkmcnt as well as vmcnt).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int nw_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float nw_ld1(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ f32x2 nw_ld2(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ f32x4 nw_ld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

template <int NT, int NC>
__global__ void __launch_bounds__(kNwThreads, NT * NC == 1 ? 3 : 2) conv3x3_nchw_wino_kernel(const Conv3x3NchwArgs a) {
  constexpr int R = 2 * NT + 2;  // patch rows of the NT stacked tiles
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = (int)blockIdx.x * (kNwThreads / 64) + wave;
  if (item >= a.total) return;
  const int cbi = item % a.cb;
  int rest = item / a.cb;
  const int bxi = rest % a.bx;
  rest /= a.bx;
  const int byi = rest % a.by;
  const int64_t img = rest / a.by;

  const int q = lane >> 4, t = lane & 15;
  const int H = a.h, W = a.w, HW = H * W;
  const int ty0 = byi * NT;         // first tile row
  const int c0 = (bxi * 16 + t) * 2;  // first output column of the lane's tiles

  // the patch's columns c0 - 1 .. c0 + 2: an aligned pair and two neighbours, each clamped into
  // the plane (W is even, so the pair is inside it or outside it as a whole)
  const bool ok_c = c0 < W, ok_l = c0 >= 1 && c0 - 1 < W, ok_r = c0 + 2 < W;
  const int cc = min(c0, W - 2), cl = min(max(c0 - 1, 0), W - 1), cr = min(c0 + 2, W - 1);
  // byte offsets of the lane's loads inside the four channel planes of a step (32-bit: the
  // step's base pointer is wave-uniform)
  uint32_t oc[R], ol[R], orr[R];
  bool rok[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int iy = 2 * ty0 - 1 + r;
    rok[r] = iy >= 0 && iy < H;
    const int row = q * HW + min(max(iy, 0), H - 1) * W;
    oc[r] = (uint32_t)(row + cc) * 4u, ol[r] = (uint32_t)(row + cl) * 4u, orr[r] = (uint32_t)(row + cr) * 4u;
  }
  const char* xs = reinterpret_cast<const char*>(a.x + img * a.cin * HW);  // the image, wave-uniform
  const int64_t xstep = (int64_t)16 * HW;                                  // bytes per step
  const char* us = reinterpret_cast<const char*>(a.u);
  const uint32_t ou = (uint32_t)((q * a.cout + (cbi * NC * 16 + t)) * 16) * 4u;
  const int64_t ustep = (int64_t)4 * a.cout * 64;

  f32x4 acc[NT][NC][16];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int nc = 0; nc < NC; ++nc)
#pragma unroll
      for (int p = 0; p < 16; ++p) acc[nt][nc][p] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // One step's loads: the patch (pair, left, right per row) and the U rows.  Two sets, named
  // so that the loads of step s + 1 have registers of their own while step s is transformed.
  struct Loads {
    f32x2 c[R];
    float l[R], r[R];
    f32x4 u[NC][4];
  };
  Loads la, lb;
  auto load = [&](Loads & L, int s) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t xp = uniform_rsrc(xs + s * xstep, xstep);
    const __amdgpu_buffer_rsrc_t up = uniform_rsrc(us + s * ustep, ustep);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      L.c[r] = nw_ld2(xp, oc[r]);
      L.l[r] = nw_ld1(xp, ol[r]);
      L.r[r] = nw_ld1(xp, orr[r]);
    }
#pragma unroll
    for (int nc = 0; nc < NC; ++nc)
#pragma unroll
      for (int i = 0; i < 4; ++i) L.u[nc][i] = nw_ld4(up, ou + nc * 1024 + i * 16);
  };

  const int last = a.cin / 4 - 1;
  // Step s from the landed set `cur`: the patch, zero outside the plane, V = B^T d B per tile;
  // then the loads of step s + 1 into `nxt`, issued before this step's MFMAs and waited for at
  // the next step's transform (past the last step the last one again: valid addresses, nobody
  // reads the result); then the MFMAs.  The scheduling barriers keep the three parts in this
  // order: without them the compiler sinks the loads to their first use.
  auto step = [&](const Loads& cur, Loads& nxt, int s) __attribute__((always_inline)) {
    float d[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      d[r][0] = rok[r] && ok_l ? cur.l[r] : 0.0f;
      d[r][1] = rok[r] && ok_c ? cur.c[r].x : 0.0f;
      d[r][2] = rok[r] && ok_c ? cur.c[r].y : 0.0f;
      d[r][3] = rok[r] && ok_r ? cur.r[r] : 0.0f;
    }
    float v[NT][16];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float e[4][4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        e[0][c] = d[2 * nt][c] - d[2 * nt + 2][c];
        e[1][c] = d[2 * nt + 1][c] + d[2 * nt + 2][c];
        e[2][c] = d[2 * nt + 2][c] - d[2 * nt + 1][c];
        e[3][c] = d[2 * nt + 1][c] - d[2 * nt + 3][c];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[nt][i * 4 + 0] = e[i][0] - e[i][2];
        v[nt][i * 4 + 1] = e[i][1] + e[i][2];
        v[nt][i * 4 + 2] = e[i][2] - e[i][1];
        v[nt][i * 4 + 3] = e[i][1] - e[i][3];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    load(nxt, min(s + 1, last));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int nc = 0; nc < NC; ++nc)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[nt][nc][p] =
              __builtin_amdgcn_mfma_f32_16x16x4f32(cur.u[nc][p >> 2][p & 3], v[nt][p], acc[nt][nc][p], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };

  load(la, 0);
  for (int s = 0;; s += 2) {
    step(la, lb, s);
    if (s >= last) break;
    step(lb, la, s + 1);
    if (s + 1 >= last) break;
  }

  // epilogue: Y = A^T M A, bn_fold.h's bn_apply, stores of float2 output rows.  Register i of a
  // 16 x 16 tile is row (channel) 4 q + i, column (tile) t.
  const bool bn = a.bn.mean != nullptr;
  if (c0 >= W) return;
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    const int co0 = cbi * NC * 16 + nc * 16 + 4 * q;
    float bs[4] = {1.0f, 1.0f, 1.0f, 1.0f}, bb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bn) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bn_fold(a.bn, co0 + i, bs[i], bb[i]);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int oy = (ty0 + nt) * 2;
      if (oy >= H) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s0[4], s1[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          s0[b] = (acc[nt][nc][b][i] + acc[nt][nc][4 + b][i]) + acc[nt][nc][8 + b][i];
          s1[b] = (acc[nt][nc][4 + b][i] - acc[nt][nc][8 + b][i]) - acc[nt][nc][12 + b][i];
        }
        float2 o0, o1;
        o0.x = bn_apply((s0[0] + s0[1]) + s0[2], bn, &bs[i], &bb[i], false, nullptr, a.relu);
        o0.y = bn_apply((s0[1] - s0[2]) - s0[3], bn, &bs[i], &bb[i], false, nullptr, a.relu);
        o1.x = bn_apply((s1[0] + s1[1]) + s1[2], bn, &bs[i], &bb[i], false, nullptr, a.relu);
        o1.y = bn_apply((s1[1] - s1[2]) - s1[3], bn, &bs[i], &bb[i], false, nullptr, a.relu);
        float* yp = a.y + ((img * a.cout + co0 + i) * H + oy) * W + c0;
        *reinterpret_cast<float2*>(yp) = o0;
        if (oy + 1 < H) *reinterpret_cast<float2*>(yp + W) = o1;
      }
    }
  }
}

// The workgroup forms (form indices 3 and up): cin split across the waves of a workgroup.  S
// waves own the same channel blocks and 16-tile run and disjoint, contiguous cin ranges (whole
// chunks of 16 cin), so a wave's serial MFMA chain is 1 / S of the one-wave forms' and there are
// S times as many waves; a workgroup is S x TR waves, TR consecutive tile runs of the batch.
// Each wave applies A^T M A to its partial M (the transform is linear: 16 accumulators become 4
// values), waves 1 .. S - 1 leave their 16 NC values per lane in LDS, and after one barrier
// wave 0 adds them in the order 0, 1, .., S - 1 and runs the epilogue: no atomics, no
// workspace, the same bits on every launch and for every n.  U has one register set, used in
// place; the patch has two.  Every wave reaches the barrier: a wave whose tile run lies past
// the last one works on the last run with its stores masked, a wave whose cin range is empty
// adds nothing.  (The forms that share U through LDS, with and without the split, lost at
// every class and live in tools/csrc/conv3x3_nchw_lab.hip)
struct NwPatch {
  f32x2 c[4];
  float l[4], r[4];
};

template <int NC, int S, int TR>
__global__ void __launch_bounds__(64 * S * TR, 2) conv3x3_nchw_wg_kernel(const Conv3x3NchwArgs a) {
  constexpr int NCO = 16 * NC;
  static_assert(S > 1, "a workgroup form splits cin");
  __shared__ float lds[TR * (S - 1) * NCO * 64];  // the partial Y of waves 1 .. S - 1

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ks = wave % S, tr = wave / S;
  const int cbi = (int)blockIdx.x % a.cb;
  const int runs = a.total / a.cb;
  const int run = ((int)blockIdx.x / a.cb) * TR + tr;
  const bool live = run < runs;
  int rest = min(run, runs - 1);
  const int bxi = rest % a.bx;
  rest /= a.bx;
  const int byi = rest % a.by;
  const int64_t img = rest / a.by;

  const int q = lane >> 4, t = lane & 15;
  const int H = a.h, W = a.w, HW = H * W;
  const int c0 = (bxi * 16 + t) * 2;
  const bool ok_c = c0 < W, ok_l = c0 >= 1 && c0 - 1 < W, ok_r = c0 + 2 < W;
  const int cc = min(c0, W - 2), cl = min(max(c0 - 1, 0), W - 1), cr = min(c0 + 2, W - 1);
  uint32_t oc[4], ol[4], orr[4];
  bool rok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int iy = 2 * byi - 1 + r;
    rok[r] = iy >= 0 && iy < H;
    const int row = q * HW + min(max(iy, 0), H - 1) * W;
    oc[r] = (uint32_t)(row + cc) * 4u, ol[r] = (uint32_t)(row + cl) * 4u, orr[r] = (uint32_t)(row + cr) * 4u;
  }
  const char* xs = reinterpret_cast<const char*>(a.x + img * a.cin * HW);
  const int64_t xstep = (int64_t)16 * HW;

  // the wave's cin range in steps of 4: whole chunks of 16 cin, [s0, s1), possibly empty
  const int K4 = a.cin / 4;
  const int cpg = ((K4 + 3) / 4 + S - 1) / S;
  const int s0 = ks * cpg * 4;
  const int s1 = min(K4, s0 + cpg * 4);

  f32x4 acc[NC][16];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc)
#pragma unroll
    for (int p = 0; p < 16; ++p) acc[nc][p] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // the patch of step s (any step past the last loads the last: valid addresses, nobody reads it)
  auto load_patch = [&](NwPatch & P, int s) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t xp = uniform_rsrc(xs + min(s, K4 - 1) * xstep, xstep);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P.c[r] = nw_ld2(xp, oc[r]);
      P.l[r] = nw_ld1(xp, ol[r]);
      P.r[r] = nw_ld1(xp, orr[r]);
    }
  };
  // V = B^T d B of a landed patch, zero outside the plane
  auto transform = [&](const NwPatch& P, float* v) __attribute__((always_inline)) {
    float d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r][0] = rok[r] && ok_l ? P.l[r] : 0.0f;
      d[r][1] = rok[r] && ok_c ? P.c[r].x : 0.0f;
      d[r][2] = rok[r] && ok_c ? P.c[r].y : 0.0f;
      d[r][3] = rok[r] && ok_r ? P.r[r] : 0.0f;
    }
    float e[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      e[0][c] = d[0][c] - d[2][c];
      e[1][c] = d[1][c] + d[2][c];
      e[2][c] = d[2][c] - d[1][c];
      e[3][c] = d[1][c] - d[3][c];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i * 4 + 0] = e[i][0] - e[i][2];
      v[i * 4 + 1] = e[i][1] + e[i][2];
      v[i * 4 + 2] = e[i][2] - e[i][1];
      v[i * 4 + 3] = e[i][1] - e[i][3];
    }
  };
  {
    // U from global memory, one register set used in place: the rows of quad i (positions
    // 4 i .. 4 i + 3) of step s + 1 are loaded right behind the MFMAs of quad i of step s, which
    // were their registers' last readers.  The patch has two sets, as in the one-wave forms.
    NwPatch pa, pb;
    f32x4 u[NC][4];
    const char* us = reinterpret_cast<const char*>(a.u);
    const uint32_t ou = (uint32_t)((q * a.cout + (cbi * NCO + t)) * 16) * 4u;
    const int64_t ustep = (int64_t)4 * a.cout * 64;
    const int last = s1 - 1;
    auto load_u = [&](int s, int i) __attribute__((always_inline)) {
      const __amdgpu_buffer_rsrc_t up = uniform_rsrc(us + s * ustep, ustep);
#pragma unroll
      for (int nc = 0; nc < NC; ++nc) u[nc][i] = nw_ld4(up, ou + nc * 1024 + i * 16);
    };
    auto step = [&](const NwPatch& cur, NwPatch& nxt, int s) __attribute__((always_inline)) {
      float v[16];
      transform(cur, v);
      __builtin_amdgcn_sched_barrier(0);
      const int sn = min(s + 1, last);
      load_patch(nxt, sn);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int nc = 0; nc < NC; ++nc)
            acc[nc][4 * i + b] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[nc][i][b], v[4 * i + b], acc[nc][4 * i + b], 0, 0, 0);
        load_u(sn, i);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (s0 < s1) {
      load_patch(pa, s0);
#pragma unroll
      for (int i = 0; i < 4; ++i) load_u(s0, i);
      for (int s = s0;; s += 2) {
        step(pa, pb, s);
        if (s >= last) break;
        step(pb, pa, s + 1);
        if (s + 1 >= last) break;
      }
    }
  }

  // Y = A^T M A of the wave's partial M: 16 NC values per lane (channel block, register i =
  // channel 4 q + i, then the 2 x 2 outputs)
  float o[NC][4][4];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t0[4], t1[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        t0[b] = (acc[nc][b][i] + acc[nc][4 + b][i]) + acc[nc][8 + b][i];
        t1[b] = (acc[nc][4 + b][i] - acc[nc][8 + b][i]) - acc[nc][12 + b][i];
      }
      o[nc][i][0] = (t0[0] + t0[1]) + t0[2];
      o[nc][i][1] = (t0[1] - t0[2]) - t0[3];
      o[nc][i][2] = (t1[0] + t1[1]) + t1[2];
      o[nc][i][3] = (t1[1] - t1[2]) - t1[3];
    }
  {
    // the partial Y of waves 1 .. S - 1 through LDS, added by wave 0 in wave order
    float* red = lds + (tr * (S - 1) * NCO * 64 + lane);
    if (ks > 0) {
#pragma unroll
      for (int e = 0; e < NCO; ++e) red[((ks - 1) * NCO + e) * 64] = o[e / 16][(e / 4) % 4][e % 4];
    }
    __syncthreads();
    if (ks == 0) {
#pragma unroll
      for (int k = 1; k < S; ++k)
#pragma unroll
        for (int e = 0; e < NCO; ++e) o[e / 16][(e / 4) % 4][e % 4] += red[((k - 1) * NCO + e) * 64];
    }
  }
  if (ks != 0 || !live || c0 >= W) return;  // no barrier follows

  const bool bn = a.bn.mean != nullptr;
  const int oy = byi * 2;
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    const int co0 = cbi * NCO + nc * 16 + 4 * q;
    float bs[4] = {1.0f, 1.0f, 1.0f, 1.0f}, bb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bn) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bn_fold(a.bn, co0 + i, bs[i], bb[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float2 o0, o1;
      o0.x = bn_apply(o[nc][i][0], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o0.y = bn_apply(o[nc][i][1], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o1.x = bn_apply(o[nc][i][2], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o1.y = bn_apply(o[nc][i][3], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      float* yp = a.y + ((img * a.cout + co0 + i) * H + oy) * W + c0;
      *reinterpret_cast<float2*>(yp) = o0;
      if (oy + 1 < H) *reinterpret_cast<float2*>(yp + W) = o1;
    }
  }
}

// The forms: tile rows NT and channel blocks NC per wave; for the workgroup forms the cin split
// S and the tile runs TR per workgroup.
struct NwForm {
  int nt, nc, s, tr;
};
constexpr NwForm kNwFormTable[kNwForms] = {{2, 1, 1, 1}, {1, 2, 1, 1}, {1, 1, 1, 1}, {1, 1, 4, 1}, {1, 1, 2, 2}};

// The measured form per class (tools/bench_conv3x3_nchw.py).  Two channel
// blocks per wave are fastest at 64 channels, two tile rows at 256, cin split in two at 128 and
// in four at 512; classes outside the table take the one-wave form with the most work items.
inline int conv3x3_nchw_pick_form(int32_t cin, int32_t cout) {
  if (cin == 64 && cout % 32 == 0) return 1;
  return cin == 128 ? 4 : cin == 256 ? 0 : cin == 512 ? 3 : 2;
}

// The host checks of every form with NT tile rows and NC channel blocks per wave, and the
// kernel arguments.  run = false: nothing to do (an empty tensor).
inline int32_t conv3x3_nchw_prepare(int NT, int NC, const float* x, const float* w, float* y, FrozenBN bn, float* ws,
                                    int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t relu,
                                    Conv3x3NchwArgs& a, bool& run) {
  run = false;
  FRH_REQUIRE(n >= 0 && n < (1 << 20) && cin >= 1 && cout >= 1 && h >= 0 && wd >= 0, "bad sizes");
  FRH_REQUIRE_BN_PAIR(bn);
  FRH_REQUIRE(wd % 2 == 0, "width %d must be even (float2 rows)", wd);
  FRH_REQUIRE(cin % 4 == 0 && cout % (16 * NC) == 0, "cin %d must be a multiple of 4 and cout %d of %d", cin, cout,
              16 * NC);
  const int64_t hw = (int64_t)h * wd;
  FRH_REQUIRE(hw < (1 << 27) && cin * hw < ((int64_t)1 << 31) && cout * hw < ((int64_t)1 << 31) &&
                  (int64_t)cin * cout < (1 << 24),
              "one image spans too many elements");
  if (n == 0 || h == 0 || wd == 0) return FRH_OK;
  FRH_REQUIRE(x && w && y && ws, "null pointer argument");
  FRH_REQUIRE_ALIGNED16(x, y, w, ws);
  const int64_t xb = n * cin * hw * 4, yb = n * cout * hw * 4, wb = (int64_t)cout * cin * 9 * 4,
                ub = (int64_t)cout * cin * 16 * 4;
  FRH_REQUIRE(!ranges_overlap(y, yb, x, xb) && !ranges_overlap(y, yb, w, wb) && !ranges_overlap(y, yb, ws, ub),
              "y must not alias x, w or the workspace");
  FRH_REQUIRE(!ranges_overlap(ws, ub, x, xb) && !ranges_overlap(ws, ub, w, wb), "the workspace must not alias x or w");
  a.x = x, a.u = ws, a.y = y, a.bn = bn, a.cin = cin, a.cout = cout, a.h = h, a.w = wd, a.relu = relu;
  a.cb = cout / (16 * NC);
  a.bx = (wd + 31) / 32;
  a.by = (h + 2 * NT - 1) / (2 * NT);
  const int64_t total = (int64_t)a.cb * a.bx * a.by * n;
  FRH_REQUIRE(total < ((int64_t)1 << 30), "too many work items");
  a.total = (int32_t)total;
  run = true;
  return FRH_OK;
}

// form < 0: the table's choice.
inline int32_t conv3x3_nchw_launch(const char* what, int form, const float* x, const float* w, float* y, FrozenBN bn,
                                   float* ws, int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd,
                                   int32_t relu, void* stream) {
  FRH_REQUIRE(form < kNwForms, "form %d: there are %d", form, kNwForms);
  if (form < 0) form = conv3x3_nchw_pick_form(cin, cout);
  const NwForm f = kNwFormTable[form];
  Conv3x3NchwArgs a;
  bool run = false;
  const int32_t st = conv3x3_nchw_prepare(f.nt, f.nc, x, w, y, bn, ws, n, cin, cout, h, wd, relu, a, run);
  if (st != FRH_OK || !run) return st;
  const int64_t total = a.total;
  hipLaunchKernelGGL(conv3x3_nchw_weights_kernel, dim3((unsigned)(((int64_t)cin * cout + 255) / 256)), dim3(256), 0,
                     as_stream(stream), w, ws, cin, cout);
  if (form < 3) {
    const dim3 grid((unsigned)((total + kNwThreads / 64 - 1) / (kNwThreads / 64))), block(kNwThreads);
    switch (form) {
      case 0: hipLaunchKernelGGL((conv3x3_nchw_wino_kernel<2, 1>), grid, block, 0, as_stream(stream), a); break;
      case 1: hipLaunchKernelGGL((conv3x3_nchw_wino_kernel<1, 2>), grid, block, 0, as_stream(stream), a); break;
      default: hipLaunchKernelGGL((conv3x3_nchw_wino_kernel<1, 1>), grid, block, 0, as_stream(stream), a); break;
    }
    return check_launch(what);
  }
  // a workgroup takes f.tr consecutive tile runs of the batch x one group of channel blocks
  const int64_t runs = total / a.cb;
  const dim3 grid((unsigned)((runs + f.tr - 1) / f.tr * a.cb)), block((unsigned)(64 * f.s * f.tr));
  if (form == 3)
    hipLaunchKernelGGL((conv3x3_nchw_wg_kernel<1, 4, 1>), grid, block, 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL((conv3x3_nchw_wg_kernel<1, 2, 2>), grid, block, 0, as_stream(stream), a);
  return check_launch(what);
}

}  // namespace frh
