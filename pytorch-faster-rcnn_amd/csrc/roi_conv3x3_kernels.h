// 3x3 / stride-1 / padding-1 convolution over RoI tiles: x [r, cin, 7, 7] -> y [r, cout, 7, 7],
// NCHW f32 on both sides (RoIAlign writes the one, the following Linear's columns are in the
// order of the other), with the eval-mode BN (+ ReLU) epilogue of bn_act.hip on the accumulators.
//
// As a GEMM: rows are cout, columns are (RoI, position), K = (ci, tap), on
// v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fmaf chain).  cout is the MFMA row (register)
// dimension, so s[co] / b[co] are per-register constants and a store instruction writes 32
// consecutive positions of one output plane.
//
// Work split: a workgroup of WM waves owns WM x 32 output channels of kRcRois = 4 RoIs: 196
// columns in 7 column blocks of 32 (the last 28 columns idle).  Wave w owns channel rows
// 32 w .. 32 w + 31 and all seven column blocks (7 x 16 accumulator registers), so one weight
// fragment feeds seven MFMAs.  The workgroup walks cin in chunks of kRcKc = 8 channels; per
// chunk it holds in LDS (one buffer each, a barrier before and after the chunk's MFMAs; the
// global loads of chunk t + 1 are in flight in registers behind the MFMAs of chunk t, and the
// 128-channel form fits two workgroups on a CU, 256 registers and 47 KiB each, so one
// workgroup's MFMAs cover the other's barriers and LDS writes: measured 7 % faster at r = 1000
// than two LDS buffers with one workgroup per CU):
//   X: the 4 x 8 tiles as zero-bordered 9 x 9 planes [roi][ci][81].  A lane's (RoI, y, x) is
//      fixed for the whole kernel, the nine taps are nine constant offsets from its base address,
//      and no lane tests a border.  The borders are zeroed once: staging writes interiors only.
//   W: [tap][q][h][co] with co fastest (ci = 2 q + h inside the chunk): the 32 lanes of an MFMA
//      half read 32 consecutive floats.  The repack launch writes the workspace in exactly this
//      order, one contiguous slab per (channel block, chunk), so staging is a float4 copy.
// Inside a chunk the sum runs tap-major, then q, with lane half h on the odd / even channel: a
// fixed permutation of the (ci, tap) order, the same for every column, launch and r.  Columns of
// an MFMA never mix, so a RoI's bits do not depend on its neighbours, its index or r.
#pragma once
#include "bn_fold.h"

namespace frh {

constexpr int kRcRois = 4;                             // RoIs per workgroup
constexpr int kRcKc = 8;                               // input channels per chunk
constexpr int kRcTile = 49, kRcPlane = 81;             // 7 x 7 tile, 9 x 9 zero-bordered plane
constexpr int kRcCols = kRcRois * kRcTile;             // 196 live columns
constexpr int kRcBlocks = (kRcCols + 31) / 32;         // 7 column blocks
constexpr int kRcXs = kRcRois * kRcKc * kRcPlane;      // floats of one X buffer
constexpr int kRcXq = kRcKc * kRcTile / 4;             // float4 per RoI per chunk (98)

struct RoiConvArgs {
  const float* x;
  const float* wp;  // repacked weights (workspace)
  float* y;
  FrozenBN bn;
  int64_t r;
  int cin, cout;
  int mt;  // channel blocks of WM * 32
  int relu;
};

// ws[mb][t][tap][q][h][co] = w[mb * MB + co][t * 8 + 2 q + h][tap]
__global__ void __launch_bounds__(256) roi_conv3x3_repack_kernel(const float* __restrict__ w, float* __restrict__ ws,
                                                                 int cin, int cout, int MB) {
  const int64_t total = (int64_t)cin * cout * 9;
  const int chunks = cin / kRcKc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % MB);
    int64_t k = i / MB;
    const int h = (int)(k & 1);
    k >>= 1;
    const int q = (int)(k & 3);
    k >>= 2;
    const int tap = (int)(k % 9);
    k /= 9;
    const int t = (int)(k % chunks);
    const int mb = (int)(k / chunks);
    ws[i] = w[((int64_t)(mb * MB + co) * cin + t * kRcKc + 2 * q + h) * 9 + tap];
  }
}

template <int WM>
__global__ void __launch_bounds__(WM * 64, WM == 4 ? 2 : 1) roi_conv3x3_bn_act_kernel(const RoiConvArgs a) {
  constexpr int NT = WM * 64, MB = WM * 32;
  constexpr int AS = 9 * kRcKc * MB;            // floats of one W buffer
  constexpr int AV = AS / 4 / NT;               // float4 of W per thread per chunk (9)
  constexpr int XV = (kRcRois * kRcXq + NT - 1) / NT;  // float4 of X per thread per chunk
  static_assert(AS / 4 % NT == 0, "W slab must split evenly over the threads");
  __shared__ __attribute__((aligned(16))) float As[AS];
  __shared__ __attribute__((aligned(16))) float Bs[kRcXs];
  __shared__ float bn_s[MB], bn_b[MB];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  const int mb = (int)(blockIdx.x % a.mt);
  const int64_t roi0 = (int64_t)(blockIdx.x / a.mt) * kRcRois;
  const int m0 = mb * MB;

  // read in the epilogue, after the main loop's barriers
  const bool bn = a.bn.mean != nullptr;
  if (bn && tid < MB) bn_fold(a.bn, m0 + tid, bn_s[tid], bn_b[tid]);
  for (int i = tid; i < kRcXs; i += NT) Bs[i] = 0.0f;
  __syncthreads();  // the zero borders stand before any interior is written

  // X staging: float4 v of the chunk (v < 392) is RoI v / 98, elements 4 (v % 98) .. + 3 of that
  // RoI's 8 x 49 contiguous floats; element e is channel e / 49, position e % 49.
  const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const float* xsrc[XV];
  int xdst[XV][4];
  bool xok[XV];
#pragma unroll
  for (int u = 0; u < XV; ++u) {
    const int v = tid + u * NT;
    const int rl = v / kRcXq, e0 = (v % kRcXq) * 4;
    xok[u] = v < kRcRois * kRcXq && roi0 + rl < a.r;
    xsrc[u] = a.x + ((roi0 + rl) * a.cin) * kRcTile + e0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int e = e0 + s, ci = e / kRcTile, p = e % kRcTile;
      xdst[u][s] = v < kRcRois * kRcXq ? (rl * kRcKc + ci) * kRcPlane + (p / 7 + 1) * 9 + p % 7 + 1 : -1;
    }
  }
  const int chunks = a.cin / kRcKc;
  const f32x4* wsrc = reinterpret_cast<const f32x4*>(a.wp + (int64_t)mb * chunks * AS) + tid;
  f32x4 ra[AV], rx[XV];
  auto load = [&](int t) {
#pragma unroll
    for (int u = 0; u < AV; ++u) ra[u] = wsrc[(int64_t)t * (AS / 4) + u * NT];
#pragma unroll
    for (int u = 0; u < XV; ++u)
      rx[u] = xok[u] ? *reinterpret_cast<const f32x4*>(xsrc[u] + (int64_t)t * (kRcKc * kRcTile)) : z4;
  };

  // this lane's seven columns: block cb, column j -> (RoI, y, x); idle columns read column 0
  int bbase[kRcBlocks];
#pragma unroll
  for (int cb = 0; cb < kRcBlocks; ++cb) {
    int col = cb * 32 + j;
    if (col >= kRcCols) col = 0;
    const int rl = col / kRcTile, p = col % kRcTile;
    bbase[cb] = (rl * kRcKc + h) * kRcPlane + (p / 7) * 9 + p % 7;
  }
  const int abase = h * MB + wave * 32 + j;

  f32x16 acc[kRcBlocks];
#pragma unroll
  for (int cb = 0; cb < kRcBlocks; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;

  load(0);
  for (int t = 0; t < chunks; ++t) {
#pragma unroll
    for (int u = 0; u < AV; ++u) *reinterpret_cast<f32x4*>(&As[(tid + u * NT) * 4]) = ra[u];
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      if (xdst[u][0] >= 0) {
        Bs[xdst[u][0]] = rx[u].x;
        Bs[xdst[u][1]] = rx[u].y;
        Bs[xdst[u][2]] = rx[u].z;
        Bs[xdst[u][3]] = rx[u].w;
      }
    }
    __syncthreads();
    if (t + 1 < chunks) load(t + 1);  // in flight behind this chunk's MFMAs
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {  // rolled: the unrolled nine taps hold more fragments than two waves per SIMD leave room for
      const float* ap = &As[ky * 3 * kRcKc * MB + abase];
      const float* bp = &Bs[ky * 9];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int q = 0; q < kRcKc / 2; ++q) {
          const float af = ap[(kx * (kRcKc / 2) + q) * 2 * MB];
          float bf[kRcBlocks];
#pragma unroll
          for (int cb = 0; cb < kRcBlocks; ++cb) bf[cb] = bp[bbase[cb] + 2 * q * kRcPlane + kx];
#pragma unroll
          for (int cb = 0; cb < kRcBlocks; ++cb)
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf[cb], acc[cb], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // every wave has read this chunk before the next one is written
  }

  // epilogue: bn_fold.h's bn_apply on the accumulators; register r of a 32 x 32 tile is row
  // mfma32_row(r) + 4 h, column j.
  const int lrow = wave * 32 + 4 * h;
#pragma unroll
  for (int cb = 0; cb < kRcBlocks; ++cb) {
    const int col = cb * 32 + j;
    const int rl = col / kRcTile, p = col % kRcTile;
    if (col >= kRcCols || roi0 + rl >= a.r) continue;
    float* yp = a.y + ((roi0 + rl) * a.cout + m0 + lrow) * kRcTile + p;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dr = mfma32_row(r);
      yp[dr * kRcTile] = bn_apply(acc[cb][r], bn, &bn_s[lrow + dr], &bn_b[lrow + dr], false, nullptr, a.relu);
    }
  }
}

inline int32_t roi_conv3x3_launch(const float* x, const float* w, float* y, FrozenBN bn, int64_t r, int32_t cin,
                                  int32_t cout, int32_t relu, float* workspace, void* stream) {
  FRH_REQUIRE(r >= 0 && cin >= 1 && cout >= 1, "bad sizes");
  FRH_REQUIRE(cin % 16 == 0 && cout % 64 == 0, "cin %d must be a multiple of 16 and cout %d of 64", cin, cout);
  if (r == 0) return FRH_OK;
  FRH_REQUIRE(x && w && y && workspace, "null pointer argument");
  FRH_REQUIRE_BN_PAIR(bn);
  FRH_REQUIRE_ALIGNED16(x, y, w, workspace);
  FRH_REQUIRE(r < ((int64_t)1 << 40), "too many RoIs");
  const int64_t xb = r * cin * kRcTile * 4, yb = r * cout * kRcTile * 4, wb = (int64_t)cin * cout * 9 * 4;
  FRH_REQUIRE(!ranges_overlap(y, yb, x, xb) && !ranges_overlap(y, yb, workspace, wb) && !ranges_overlap(y, yb, w, wb),
              "y must not overlap x, w or the workspace");
  FRH_REQUIRE(!ranges_overlap(workspace, wb, x, xb) && !ranges_overlap(workspace, wb, w, wb),
              "the workspace must not overlap x or w");
  const int wm = cout % 128 == 0 ? 4 : 2;
  RoiConvArgs a;
  a.x = x, a.wp = workspace, a.y = y, a.bn = bn;
  a.r = r, a.cin = cin, a.cout = cout, a.relu = relu;
  a.mt = cout / (wm * 32);
  const int64_t blocks = (r + kRcRois - 1) / kRcRois * a.mt;
  FRH_REQUIRE(blocks < ((int64_t)1 << 31), "too many blocks");
  const int64_t welems = (int64_t)cin * cout * 9;
  const unsigned rp_blocks = (unsigned)((welems + 255) / 256 < 4096 ? (welems + 255) / 256 : 4096);
  hipLaunchKernelGGL(roi_conv3x3_repack_kernel, dim3(rp_blocks), dim3(256), 0, as_stream(stream), w, workspace,
                     (int)cin, (int)cout, wm * 32);
  if (wm == 4)
    hipLaunchKernelGGL((roi_conv3x3_bn_act_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL((roi_conv3x3_bn_act_kernel<2>), dim3((unsigned)blocks), dim3(128), 0, as_stream(stream), a);
  return check_launch("frh_roi_conv3x3_bn_act");
}

}  // namespace frh
