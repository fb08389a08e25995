// The RPN head's two 1x1 convolutions (classifier and regressor) over every level of the
// pyramid in one launch: per pixel
//   out[co] = (sum_ci w[co, ci] * x[ci]) + bias[co],   co over the c_cls + c_reg <= 16 channels,
// on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain) with pixels as the MFMA rows
// and the 16 padded output channels as its columns.  The levels are channels-last (channel
// stride 1, explicit image / row / column strides), so a pixel's cin channels are one
// contiguous row; each is read from memory once and feeds both convolutions, and each output
// element is written once.  No atomics and no split over cin: every output is one sum in one
// order (channel 16 j + 4 g + i in the order j, i, g; the padding channels add +0), the same
// for every level, pixel and launch.
//
// Work split: 256 threads = 4 waves; a tile is 64 consecutive pixels of one level's flattened
// [n, h, w] index (16 per wave = one MFMA row block), so small and ragged levels fill their
// tiles, and the outputs of a tile are contiguous in the channels-last outputs.  Tiles are
// numbered level by level, so the small levels ride in the tail of the large ones, and a
// workgroup takes per_wg consecutive ones (the launch: one resident round of workgroups).
// Both weights (zero-padded to 16 rows) and the biases are staged into LDS once per
// workgroup.  X goes global -> registers -> LDS in chunks of 128 channels, the next
// chunk's loads in flight behind this chunk's MFMAs: a wave's load instruction covers the
// contiguous 512-byte half rows of two pixels (the other half is the next chunk), never a lane
// walking its own pixel.  LDS pitches 260 / 132 floats: the 16 rows of a ds_read_b128 lane
// group start in 16 distinct 4-bank groups.
#pragma once
#include "common.h"

namespace frh {

constexpr int kRhThreads = 256;
constexpr int kRhPix = 64;       // pixels per tile
constexpr int kRhCols = 16;      // output channels (MFMA columns), c_cls + c_reg padded
constexpr int kRhKC = 128;       // channels per staged chunk
constexpr int kRhMaxCin = 256;   // the weights' LDS image
constexpr int kRhMaxLevels = 8;
constexpr int kRhWP = kRhMaxCin + 4, kRhXP = kRhKC + 4;
constexpr int kRhLoads = kRhPix * (kRhKC / 4) / kRhThreads;  // float4 per thread per chunk

struct RpnHeadLevel {
  const float* x;
  float* cls;
  float* reg;
  int64_t sn, sy, sx;
  int64_t pixels;  // n * h * w
  int32_t h, w;
  int32_t first;  // its first tile
};

struct RpnHeadArgs {
  RpnHeadLevel lv[kRhMaxLevels];
  const float* w_cls;
  const float* b_cls;
  const float* w_reg;
  const float* b_reg;
  int32_t levels, cin, c_cls, c_reg;
  int32_t total, per_wg;  // tiles, tiles per workgroup
};

__global__ void __launch_bounds__(kRhThreads) rpn_head1x1_kernel(const RpnHeadArgs a) {
  __shared__ __attribute__((aligned(16))) float Ws[kRhCols * kRhWP];
  __shared__ __attribute__((aligned(16))) float Xs[kRhPix * kRhXP];
  __shared__ int64_t in_off[kRhPix];
  __shared__ float bias_s[kRhCols];
  __shared__ RpnHeadLevel lvs[kRhMaxLevels];  // the level table, read by a tile's level index

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int cout = a.c_cls + a.c_reg;

  // both weights as one [16][cin] image, zero outside (rows past cout, channels past cin)
  for (int f = tid; f < kRhCols * (kRhMaxCin / 4); f += kRhThreads) {
    const int co = f / (kRhMaxCin / 4), c = (f % (kRhMaxCin / 4)) * 4;
    float4 v = z4;
    if (c < a.cin && co < cout)
      v = *reinterpret_cast<const float4*>(co < a.c_cls ? a.w_cls + (int64_t)co * a.cin + c
                                                         : a.w_reg + (int64_t)(co - a.c_cls) * a.cin + c);
    *reinterpret_cast<float4*>(&Ws[co * kRhWP + c]) = v;
  }
  if (tid < kRhCols) {
    float b = 0.0f;
    if (tid < a.c_cls)
      b = a.b_cls ? a.b_cls[tid] : 0.0f;
    else if (tid < cout)
      b = a.b_reg ? a.b_reg[tid - a.c_cls] : 0.0f;
    bias_s[tid] = b;
  }

#pragma unroll
  for (int i = 0; i < kRhMaxLevels; ++i)
    if (tid == i) {
      lvs[i].x = a.lv[i].x, lvs[i].cls = a.lv[i].cls, lvs[i].reg = a.lv[i].reg;
      lvs[i].sn = a.lv[i].sn, lvs[i].sy = a.lv[i].sy, lvs[i].sx = a.lv[i].sx, lvs[i].pixels = a.lv[i].pixels;
      lvs[i].h = a.lv[i].h, lvs[i].w = a.lv[i].w, lvs[i].first = a.lv[i].first;
    }

  const int chunks = (a.cin + kRhKC - 1) / kRhKC;
  const int tile_end = min(a.total, (int)(blockIdx.x + 1) * a.per_wg);
  for (int tile = blockIdx.x * a.per_wg; tile < tile_end; ++tile) {
    int li = 0;
#pragma unroll
    for (int i = 1; i < kRhMaxLevels; ++i)
      if (i < a.levels && tile >= a.lv[i].first) li = i;

    __syncthreads();  // the previous tile's reads of in_off and Xs; the first tile: Ws, bias_s, lvs
    const RpnHeadLevel& L = lvs[li];
    const int64_t lin0 = (int64_t)(tile - L.first) * kRhPix;
    const float* const lx = L.x;
    const int64_t pixels = L.pixels;
    if (tid < kRhPix) {
      const int64_t lin = lin0 + tid;
      int64_t off = -1;  // past the level's end: staged as zeros, never stored
      if (lin < pixels) {
        const int64_t hw = (int64_t)L.h * L.w, img = lin / hw, rem = lin - img * hw;
        const int64_t y = rem / L.w, x = rem - y * L.w;
        off = img * L.sn + y * L.sy + x * L.sx;
      }
      in_off[tid] = off;
    }
    __syncthreads();

    // thread t moves float4 t, t + 256, ... of the [64 pixels][128 channels] chunk
    float4 rb[kRhLoads];
    auto load = [&](int c0) {
#pragma unroll
      for (int i = 0; i < kRhLoads; ++i) {
        const int f = i * kRhThreads + tid, row = f / (kRhKC / 4), ch = c0 + (f % (kRhKC / 4)) * 4;
        const int64_t off = in_off[row];
        float4 v = z4;
        if (off >= 0 && ch < a.cin) v = *reinterpret_cast<const float4*>(lx + off + ch);
        rb[i] = v;
      }
    };

    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    load(0);
    for (int c = 0; c < chunks; ++c) {
      if (c > 0) __syncthreads();  // every wave has left the previous chunk's reads of Xs
#pragma unroll
      for (int i = 0; i < kRhLoads; ++i) {
        const int f = i * kRhThreads + tid;
        *reinterpret_cast<float4*>(&Xs[(f / (kRhKC / 4)) * kRhXP + (f % (kRhKC / 4)) * 4]) = rb[i];
      }
      __syncthreads();
      if (c + 1 < chunks) load((c + 1) * kRhKC);  // in flight behind this chunk's MFMAs
      const int groups = (min(kRhKC, a.cin - c * kRhKC) + 15) / 16;
      const float* xr = &Xs[(wave * 16 + p) * kRhXP + 4 * g];
      const float* wr = &Ws[p * kRhWP + c * kRhKC + 4 * g];
      for (int j = 0; j < groups; ++j) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + 16 * j);
        const float4 wv = *reinterpret_cast<const float4*>(wr + 16 * j);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, wv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, wv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, wv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, wv.w, acc, 0, 0, 0);
      }
    }

    // register r of the 16 x 16 tile is pixel 4 g + r of the wave's 16, channel p
    const float b = bias_s[p];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t lin = lin0 + wave * 16 + 4 * g + r;
      if (lin >= pixels) continue;
      const float v = acc[r] + b;
      if (p < a.c_cls)
        L.cls[lin * a.c_cls + p] = v;
      else if (p < cout)
        L.reg[lin * a.c_reg + (p - a.c_cls)] = v;
    }
  }
}

// One level of a launch, as the entry receives it.
struct RpnHeadLevelDesc {
  const float* x;
  float* cls;
  float* reg;
  int32_t h, w;
  int64_t sn, sy, sx;
};

inline int32_t rpn_head1x1_launch(int32_t levels, const RpnHeadLevelDesc* d, const float* w_cls, const float* b_cls,
                                  const float* w_reg, const float* b_reg, int64_t n, int32_t cin, int32_t c_cls,
                                  int32_t c_reg, void* stream) {
  FRH_REQUIRE(levels >= 1 && levels <= kRhMaxLevels, "1 to %d levels, got %d", kRhMaxLevels, levels);
  FRH_REQUIRE(n >= 0 && n < (1 << 20) && cin >= 1 && c_cls >= 0 && c_reg >= 0 && c_cls + c_reg >= 1, "bad sizes");
  FRH_REQUIRE(c_cls + c_reg <= kRhCols, "%d + %d output channels, at most %d together", c_cls, c_reg, kRhCols);
  FRH_REQUIRE(cin % 8 == 0 && cin <= kRhMaxCin, "cin %d must be a multiple of 8 and at most %d", cin, kRhMaxCin);
  FRH_REQUIRE((c_cls == 0 || w_cls) && (c_reg == 0 || w_reg), "null pointer argument");
  FRH_REQUIRE_ALIGNED16(w_cls, w_reg);
  RpnHeadArgs a;
  a.levels = 0, a.cin = cin, a.c_cls = c_cls, a.c_reg = c_reg;
  a.w_cls = w_cls, a.b_cls = b_cls, a.w_reg = w_reg, a.b_reg = b_reg;
  int64_t total = 0;
  for (int i = 0; i < levels; ++i) {
    const RpnHeadLevelDesc& s = d[i];
    FRH_REQUIRE(s.h >= 0 && s.w >= 0, "bad sizes");
    if (n == 0 || s.h == 0 || s.w == 0) continue;
    FRH_REQUIRE(s.x && (c_cls == 0 || s.cls) && (c_reg == 0 || s.reg), "null pointer argument");
    FRH_REQUIRE_ALIGNED16(s.x);
    // the stride of an extent of 1 is never used (torch leaves it arbitrary)
    const int64_t sn = n > 1 ? s.sn : 0, sy = s.h > 1 ? s.sy : 0, sx = s.w > 1 ? s.sx : 0;
    FRH_REQUIRE(sn >= 0 && sy >= 0 && sx >= 0 && (sn | sy | sx) % 4 == 0,
                "x strides must be non-negative multiples of 4 elements");
    FRH_REQUIRE(s.cls != s.x && s.reg != s.x, "the outputs must not alias x");
    RpnHeadLevel& L = a.lv[a.levels++];
    L.x = s.x, L.cls = s.cls, L.reg = s.reg, L.sn = sn, L.sy = sy, L.sx = sx, L.h = s.h, L.w = s.w;
    L.pixels = n * s.h * s.w;
    FRH_REQUIRE(L.pixels < ((int64_t)1 << 31), "too many pixels in one level");
    L.first = (int32_t)total;
    total += (L.pixels + kRhPix - 1) / kRhPix;
    FRH_REQUIRE(total < ((int64_t)1 << 30), "too many tiles");
  }
  if (a.levels == 0) return FRH_OK;
  for (int i = a.levels; i < kRhMaxLevels; ++i) a.lv[i] = a.lv[0];
  a.total = (int32_t)total;
  // one resident round of workgroups where the launch is large enough for it, so that the
  // weights are staged as few times as the chip's width allows
  const int cap = resident_capacity(reinterpret_cast<const void*>(rpn_head1x1_kernel), kRhThreads);
  a.per_wg = cap > 0 ? (int32_t)((total + cap - 1) / cap) : 4;
  const int64_t grid = (total + a.per_wg - 1) / a.per_wg;
  hipLaunchKernelGGL(rpn_head1x1_kernel, dim3((unsigned)grid), dim3(kRhThreads), 0, as_stream(stream), a);
  return check_launch("frh_rpn_head1x1_levels");
}

}  // namespace frh
