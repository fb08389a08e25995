// The prediction convs of a one-stage head (3x3 / stride 1 / padding 1; 1 to 192 output
// channels, one conv or two that read the same input) over every level of the pyramid in one
// launch: per pixel
//   out[co] = epilogue((sum_{tap, ci} w[co, tap, ci] * x[pixel + tap, ci]) + bias[co]),
// as a direct convolution on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain) with
// pixels as the MFMA rows and output channels as its columns.  No Winograd, no weight
// transform, no workspace, no atomics and no split over cin: every output element is one sum
// in one order -- 16-channel group ascending, then tap 0..8 (row-major), then channel
// 16 j + 4 g + i of the group in the order i, g -- the same for every level, pixel, width,
// companion conv and launch.  Channels past cin, columns past c0 + c1 and pixels outside the
// image are staged as zeros (they add +0); the latter are the convolution's zero padding.
//
// Work split: 256 threads = 4 waves; a tile is 4 rows x 16 columns of one image of one level
// (wave r owns row r = one MFMA row block), tiles numbered level by level; blockIdx.y picks a
// group of NCB 16-column blocks of the c0 + c1 output columns (the two convs' columns side by
// side: conv 1 starts at column c0).  Per chunk of KC input channels the workgroup stages the
// tile's 6 x 18 halo [pixel][KC] and the group's weights [tap][column][KC] into LDS (global ->
// registers -> LDS, the next chunk's loads in flight behind this chunk's MFMAs); LDS pitches
// KC + 4 floats: the 16 rows of a ds_read_b128 lane group start in 16 distinct 4-bank groups.
#pragma once
#include "common.h"

namespace frh {

constexpr int kCoThreads = 256;
constexpr int kCoTH = 4, kCoTW = 16;  // the tile: one row of 16 pixels per wave
constexpr int kCoHW = kCoTW + 2, kCoHalo = (kCoTH + 2) * kCoHW;
constexpr int kCoMaxLevels = 8;
constexpr int kCoMaxCout = 192;
constexpr int kCoGroupBlocks = 4;  // 16-column blocks of one workgroup, at most

struct ConvOutLevel {
  const float* x;
  float* y0;
  float* y1;
  const float* s0;  // per-channel scales of this level, or NULL
  const float* s1;
  int64_t sn, sy, sx;
  int32_t h, w;
  int32_t tiles_x, tiles_img;  // tiles per tile row, per image
  int32_t first, pad_;         // its first tile
};

struct ConvOutArgs {
  ConvOutLevel lv[kCoMaxLevels];
  const float* w0;
  const float* b0;
  const float* w1;
  const float* b1;
  int32_t levels, cin, c0, c1, exp0, exp1;
};

template <int NCB, int KC>
__global__ void __launch_bounds__(kCoThreads) conv3x3_out_kernel(const ConvOutArgs a) {
  constexpr int XP = KC + 4, Q = KC / 4, NC = NCB * 16;
  constexpr int XF = kCoHalo * Q, WF = 9 * NC * Q;  // float4 of a chunk's halo, of its weights
  constexpr int XL = (XF + kCoThreads - 1) / kCoThreads, WL = (WF + kCoThreads - 1) / kCoThreads;
  __shared__ __attribute__((aligned(16))) float Xs[kCoHalo * XP];
  __shared__ __attribute__((aligned(16))) float Ws[9 * NC * XP];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

  const int tile = blockIdx.x;
  ConvOutLevel L = a.lv[0];
#pragma unroll
  for (int i = 1; i < kCoMaxLevels; ++i)
    if (i < a.levels && tile >= a.lv[i].first) L = a.lv[i];
  const int t = tile - L.first;
  const int img = t / L.tiles_img, trem = t - img * L.tiles_img;
  const int ty = trem / L.tiles_x, tx = trem - ty * L.tiles_x;
  const int y0 = ty * kCoTH, x0 = tx * kCoTW;
  const int ctot = a.c0 + a.c1, cbase = blockIdx.y * NC;

  // thread t moves float4 t, t + 256, ... of the [108 pixels][KC] halo and of the
  // [9 taps][NC columns][KC] weights; what lies outside (image, cin, c0 + c1) stays zero
  int64_t xoff[XL];
  int xch[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int f = i * kCoThreads + tid, pix = f / Q, hy = pix / kCoHW, hx = pix - hy * kCoHW;
    const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
    xch[i] = (f % Q) * 4;
    xoff[i] = (f < XF && yy >= 0 && yy < L.h && xx >= 0 && xx < L.w)
                  ? (int64_t)img * L.sn + (int64_t)yy * L.sy + (int64_t)xx * L.sx + xch[i]
                  : -1;
  }
  const float* wp[WL];
  int wch[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int f = i * kCoThreads + tid, row = f / Q, tap = row / NC, c = cbase + (row - tap * NC);
    wch[i] = (f % Q) * 4;
    const float* r = nullptr;
    if (f < WF && c < ctot)
      r = c < a.c0 ? a.w0 + ((int64_t)c * 9 + tap) * a.cin : a.w1 + ((int64_t)(c - a.c0) * 9 + tap) * a.cin;
    wp[i] = r ? r + wch[i] : nullptr;
  }

  float4 xb[XL], wb[WL];
  auto load = [&](int kc) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      float4 v = z4;
      if (xoff[i] >= 0 && kc + xch[i] < a.cin) v = *reinterpret_cast<const float4*>(L.x + xoff[i] + kc);
      xb[i] = v;
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      float4 v = z4;
      if (wp[i] && kc + wch[i] < a.cin) v = *reinterpret_cast<const float4*>(wp[i] + kc);
      wb[i] = v;
    }
  };

  f32x4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int chunks = (a.cin + KC - 1) / KC;
  load(0);
  for (int c = 0; c < chunks; ++c) {
    if (c > 0) __syncthreads();  // every wave has left the previous chunk's reads
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int f = i * kCoThreads + tid;
      if (f < XF) *reinterpret_cast<float4*>(&Xs[(f / Q) * XP + (f % Q) * 4]) = xb[i];
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int f = i * kCoThreads + tid;
      if (f < WF) *reinterpret_cast<float4*>(&Ws[(f / Q) * XP + (f % Q) * 4]) = wb[i];
    }
    __syncthreads();
    if (c + 1 < chunks) load((c + 1) * KC);  // in flight behind this chunk's MFMAs
    const int groups = (min(KC, a.cin - c * KC) + 15) / 16;
    for (int j = 0; j < groups; ++j) {
      const float* xr = &Xs[(wave * kCoHW + p) * XP + 16 * j + 4 * g];
      const float* wr = &Ws[p * XP + 16 * j + 4 * g];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + ((tap / 3) * kCoHW + tap % 3) * XP);
        float4 wv[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) wv[cb] = *reinterpret_cast<const float4*>(wr + (tap * NC + cb * 16) * XP);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv[cb].x, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv[cb].y, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv[cb].z, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv[cb].w, acc[cb], 0, 0, 0);
      }
    }
  }

  // register r of a 16 x 16 block is pixel 4 g + r of the wave's row, column p of the block
  const int yy = y0 + wave;
  if (yy >= L.h) return;
  const int64_t row0 = ((int64_t)img * L.h + yy) * L.w;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int c = cbase + cb * 16 + p;
    if (c >= ctot) continue;
    const bool first = c < a.c0;
    const int ck = first ? c : c - a.c0, cw = first ? a.c0 : a.c1;
    const float* bp = first ? a.b0 : a.b1;
    const float* sp = first ? L.s0 : L.s1;
    float* out = first ? L.y0 : L.y1;
    const bool ex = (first ? a.exp0 : a.exp1) != 0;
    const float b = bp ? bp[ck] : 0.0f;
    const float s = sp ? sp[ck] : 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int xx = x0 + 4 * g + r;
      if (xx >= L.w) continue;
      float v = acc[cb][r] + b;
      if (sp) v = v * s;
      if (ex) v = expf(v);
      out[(row0 + xx) * cw + ck] = v;
    }
  }
}

// One level of a launch, as the entry receives it.
struct ConvOutLevelDesc {
  const float* x;
  float* y0;
  float* y1;
  const float* s0;
  const float* s1;
  int32_t h, w;
  int64_t sn, sy, sx;
};

inline int32_t conv3x3_out_launch(int32_t levels, const ConvOutLevelDesc* d, const float* w0, const float* b0,
                                  const float* w1, const float* b1, int32_t exp0, int32_t exp1, int64_t n,
                                  int32_t cin, int32_t c0, int32_t c1, void* stream) {
  FRH_REQUIRE(levels >= 1 && levels <= kCoMaxLevels, "1 to %d levels, got %d", kCoMaxLevels, levels);
  FRH_REQUIRE(n >= 0 && n < (1 << 20) && cin >= 8 && cin < (1 << 20) && c0 >= 1 && c1 >= 0, "bad sizes");
  FRH_REQUIRE(cin % 8 == 0, "cin %d must be a multiple of 8", cin);
  FRH_REQUIRE(c0 + c1 <= kCoMaxCout, "%d + %d output channels, at most %d together", c0, c1, kCoMaxCout);
  FRH_REQUIRE(w0 && (c1 == 0 || w1), "null pointer argument");
  FRH_REQUIRE_ALIGNED16(w0, w1);
  ConvOutArgs a;
  a.levels = 0, a.cin = cin, a.c0 = c0, a.c1 = c1, a.exp0 = exp0, a.exp1 = exp1;
  a.w0 = w0, a.b0 = b0, a.w1 = c1 ? w1 : nullptr, a.b1 = c1 ? b1 : nullptr;
  int64_t total = 0;
  int64_t xbytes[kCoMaxLevels], ybytes[kCoMaxLevels];
  for (int i = 0; i < levels; ++i) {
    const ConvOutLevelDesc& s = d[i];
    FRH_REQUIRE(s.h >= 0 && s.w >= 0 && s.h < (1 << 20) && s.w < (1 << 20), "bad sizes");
    if (n == 0 || s.h == 0 || s.w == 0) continue;
    FRH_REQUIRE(s.x && s.y0 && (c1 == 0 || s.y1), "null pointer argument");
    FRH_REQUIRE_ALIGNED16(s.x);
    // the stride of an extent of 1 is never used (torch leaves it arbitrary)
    const int64_t sn = n > 1 ? s.sn : 0, sy = s.h > 1 ? s.sy : 0, sx = s.w > 1 ? s.sx : 0;
    FRH_REQUIRE(sn >= 0 && sy >= 0 && sx >= 0 && (sn | sy | sx) % 4 == 0,
                "x strides must be non-negative multiples of 4 elements");
    ConvOutLevel& L = a.lv[a.levels];
    L.x = s.x, L.y0 = s.y0, L.y1 = c1 ? s.y1 : nullptr, L.s0 = s.s0, L.s1 = c1 ? s.s1 : nullptr;
    L.sn = sn, L.sy = sy, L.sx = sx, L.h = s.h, L.w = s.w, L.pad_ = 0;
    L.tiles_x = (s.w + kCoTW - 1) / kCoTW;
    L.tiles_img = L.tiles_x * ((s.h + kCoTH - 1) / kCoTH);
    L.first = (int32_t)total;
    total += n * L.tiles_img;
    FRH_REQUIRE(total < ((int64_t)1 << 30), "too many tiles");
    xbytes[a.levels] = ((n - 1) * sn + (s.h - 1) * sy + (s.w - 1) * sx + cin) * (int64_t)sizeof(float);
    ybytes[a.levels] = n * s.h * s.w * (int64_t)sizeof(float);  // per output channel
    ++a.levels;
  }
  if (a.levels == 0) return FRH_OK;
  const int64_t w0b = (int64_t)c0 * 9 * cin * 4, w1b = (int64_t)c1 * 9 * cin * 4;
  for (int i = 0; i < a.levels; ++i) {
    const ConvOutLevel& O = a.lv[i];
    const void* outs[2] = {O.y0, O.y1};
    const int64_t ob[2] = {ybytes[i] * c0, ybytes[i] * c1};
    for (int k = 0; k < (c1 ? 2 : 1); ++k) {
      for (int j = 0; j < a.levels; ++j)
        FRH_REQUIRE(!ranges_overlap(outs[k], ob[k], a.lv[j].x, xbytes[j]), "the outputs must not overlap the inputs");
      FRH_REQUIRE(!ranges_overlap(outs[k], ob[k], w0, w0b) && !(c1 && ranges_overlap(outs[k], ob[k], w1, w1b)),
                  "the outputs must not overlap the weights");
    }
  }
  for (int i = a.levels; i < kCoMaxLevels; ++i) a.lv[i] = a.lv[0];
  // the c0 + c1 columns in 16-column blocks, split evenly over as few groups of at most
  // kCoGroupBlocks as hold them
  const int blocks = (c0 + c1 + 15) / 16;
  const int groups = (blocks + kCoGroupBlocks - 1) / kCoGroupBlocks;
  const int per = (blocks + groups - 1) / groups;
  const dim3 grid((unsigned)total, (unsigned)groups), block(kCoThreads);
  hipStream_t st = as_stream(stream);
  switch (per) {
    case 1: hipLaunchKernelGGL((conv3x3_out_kernel<1, 32>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((conv3x3_out_kernel<2, 32>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((conv3x3_out_kernel<3, 16>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((conv3x3_out_kernel<4, 16>), grid, block, 0, st, a); break;
  }
  return check_launch("frh_conv3x3_out_levels");
}

}  // namespace frh
