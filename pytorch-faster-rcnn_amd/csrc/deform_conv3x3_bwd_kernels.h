// Backward of the deformable 3x3 convolution of deform_conv3x3_kernels.h (same definition, same
// sample-point arithmetic): given gy = dL/dy (masked by y > 0 where the forward applied ReLU),
//   G[n, c, k, p]  = sum_co w[co, c, k] gy[n, co, p]                       (a GEMM, K = cout)
//   gx             : every G adds G (hy hx, hy lx, ly hx, ly lx) to its four corners
//   goff[n, g 18 + 2 k, p]     = sum_{c in g} G dS/dpy,  dS/dpy = hx (v10 - v00) + lx (v11 - v01)
//   goff[n, g 18 + 2 k + 1, p] = sum_{c in g} G dS/dpx,  dS/dpx = hy (v01 - v00) + ly (v11 - v10)
//   gw[co, c, k]   = sum_{n, p} gy[n, co, p] S[n, c, k, p]                  (a GEMM, K = positions)
// Corners outside the map count as 0 and receive nothing; a sample whose float range test fails
// (NaN, infinite and huge offsets included) forms no address and contributes exact zeros to all
// three.  floor has derivative 0, so at an integer coordinate dS/dp is the one-sided value the
// formulas give: what autograd returns for the torch restatement.
//
// Data launch (gx, goff).  A workgroup of four waves owns kDcbCols = 64 consecutive positions.
// It stages its gy tile [64][cout] in LDS once (masked by y > 0; float4 slots XOR-swizzled by
// the row so that the 16 rows an MFMA operand load touches fall on different banks), then walks
// (tap, 16-channel chunk).  Per chunk each wave forms the G tile of its 16 positions x 16
// channels on v_mfma_f32_16x16x4_f32 (positions are the MFMA rows, K = cout; the repacked w is
// read as one contiguous 1-KiB line per 16 output channels): register r of lane (p = lane & 15,
// q = lane >> 4) is G of position 4 q + r, channel p.  The lane recomputes that position's sample
// point for its channel's group with the forward's arithmetic and
//   gx:   adds G * weight to each in-map corner with a no-return float atomic; one wave
//         instruction covers four runs of 16 consecutive channels (64 B) of one corner each;
//   goff: sums G dS/dp over the channels of a group in a fixed order -- a butterfly over the
//         four lanes of a channel quad, then the quads of the group in ascending channel order,
//         across chunks where a group spans several -- and stores each (n, g, k, p) once.  No
//         atomics: the same inputs give the same goff bits on every launch.
//
// Weight launch (gw).  Grid = (tap, 16-channel chunk) x position split.  A workgroup walks the
// 64-position tiles of its split; per tile thread (position, channel quad) gathers and blends
// its sample exactly as the forward does into Bs[position][16], and the waves run the
// gy^T S product on the 16 x 16 x 4 MFMA (rows = output channels, 16 RT per wave, K = positions
// in ascending order).  The split's partial gw goes to its slab of the workspace with plain
// stores; the reduce launch sums the slabs in split order.  No atomics: gw is bit-identical
// from launch to launch.
#pragma once
#include "common.h"

namespace frh {

constexpr int kDcbKc = 16;        // input channels per chunk
constexpr int kDcbCols = 64;      // positions per tile
constexpr int kDcbThreads = 256;
constexpr int kDcbMaxCout = 256;  // the gy tile of the data launch is 64 x cout floats of LDS
constexpr int kDcbMaxSplits = 32;

struct DcbArgs {
  const float* x;
  const float* off;  // explicit: [n, 18 dg, h, w]; guided: the shape map [n, 2, h, w]
  const float* ow;   // guided: offset-layer weight [18 dg, 2]
  const float* wp;   // repacked weights (workspace)
  const float* y;    // NULL: no ReLU mask
  const float* gy;
  float* gx;
  float* goff;
  float* slab;  // [splits][cout][cin][9]
  int h, w;
  int64_t sn, sy, sx;      // x strides (image, row, column), elements
  int64_t on, oc, oy, ox;  // off strides (image, channel, row, column), elements
  int64_t P;               // n * h * w
  int cin, cout, cpg, dg;
  int tiles, tiles_per_split;
};

// Position splits of the weight launch for P positions: a function of P alone, so that the
// workspace size and the launch agree.
inline int dcb_tiles_per_split(int64_t tiles) { return (int)((tiles + kDcbMaxSplits - 1) / kDcbMaxSplits); }
inline int dcb_splits(int64_t tiles) {
  const int tps = dcb_tiles_per_split(tiles);
  return tps > 0 ? (int)((tiles + tps - 1) / tps) : 0;
}

// wp[tap][cc][j][c][i] = w[16 j + i][16 cc + c][tap]
__global__ void __launch_bounds__(256) deform_conv3x3_bwd_repack_kernel(const float* __restrict__ w,
                                                                        float* __restrict__ wp, int cin, int cout) {
  const int64_t total = (int64_t)cin * cout * 9;
  const int cchunks = cin / kDcbKc, jb = cout / 16;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e & 15), c = (int)((e >> 4) & 15);
    int64_t k = e >> 8;
    const int j = (int)(k % jb);
    k /= jb;
    const int cc = (int)(k % cchunks);
    const int tap = (int)(k / cchunks);
    wp[e] = w[((int64_t)(16 * j + i) * cin + 16 * cc + c) * 9 + tap];
  }
}

// The sample point of the forward kernel: the float range test first, then floor, the blend
// weights and which corners lie in the map.
struct DcbPoint {
  float ly, lx, hy, hx;
  int y0, x0;
  bool yt, yb, xl, xr;
};

__device__ __forceinline__ bool dcb_point(float py, float px, int H, int W, DcbPoint& s) {
  // in float, before any conversion: NaN and far offsets fail here and form no address
  if (!(py > -1.0f && py < (float)H && px > -1.0f && px < (float)W)) return false;
  const float fy = floorf(py), fx = floorf(px);
  s.y0 = (int)fy, s.x0 = (int)fx;  // in [-1, H - 1] x [-1, W - 1]
  s.ly = py - fy, s.lx = px - fx;
  s.hy = 1.0f - s.ly, s.hx = 1.0f - s.lx;
  s.yt = s.y0 >= 0, s.yb = s.y0 + 1 <= H - 1, s.xl = s.x0 >= 0, s.xr = s.x0 + 1 <= W - 1;
  return true;
}

// the offsets (dy, dx) of offset channel pair och at a position: ob points at the position's
// channel 0 (explicit), or (s0, s1) is its shape (guided: the forward's f32 order)
template <bool GUIDED>
__device__ __forceinline__ void dcb_offsets(const DcbArgs& a, const float* ob, float s0, float s1, int och, float& dy,
                                            float& dx) {
  if (GUIDED) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(a.ow + 2 * och);
    dy = (q.x * s0) + (q.y * s1);
    dx = (q.z * s0) + (q.w * s1);
  } else {
    dy = ob[och * a.oc];
    dx = ob[(och + 1) * a.oc];
  }
}

// lanes p < 4 of a 16-lane row group store the (dy, dx) sums of position p of their four
__device__ __forceinline__ void dcb_store_goff(bool store, float* gp, int64_t HW, int p, f32x4 ady, f32x4 adx) {
  const float vy = p == 0 ? ady.x : p == 1 ? ady.y : p == 2 ? ady.z : ady.w;
  const float vx = p == 0 ? adx.x : p == 1 ? adx.y : p == 2 ? adx.z : adx.w;
  if (store) {
    gp[0] = vy;
    gp[HW] = vx;
  }
}

template <bool GUIDED>
__global__ void __launch_bounds__(kDcbThreads) deform_conv3x3_bwd_data_kernel(const DcbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gys[];  // [64][cout], float4 slots swizzled by the row
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int H = a.h, W = a.w, cout = a.cout, cin = a.cin;
  const int64_t HW = (int64_t)H * W;
  const int64_t pos0 = (int64_t)blockIdx.x * kDcbCols;
  const int c4n = cout / 4;  // float4 of a gy row

  for (int f = tid; f < kDcbCols * c4n; f += kDcbThreads) {
    const int row = f / c4n, col = f - row * c4n;
    const int64_t pos = pos0 + row;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (pos < a.P) {
      v = *reinterpret_cast<const f32x4*>(a.gy + pos * cout + 4 * col);
      if (a.y) {
        const f32x4 yv = *reinterpret_cast<const f32x4*>(a.y + pos * cout + 4 * col);
        v.x = yv.x > 0.0f ? v.x : 0.0f;
        v.y = yv.y > 0.0f ? v.y : 0.0f;
        v.z = yv.z > 0.0f ? v.z : 0.0f;
        v.w = yv.w > 0.0f ? v.w : 0.0f;
      }
    }
    *reinterpret_cast<f32x4*>(&gys[(row * c4n + (col ^ (row & 15))) * 4]) = v;
  }

  // this lane's four positions 4 q + r of the wave's 16
  bool live[4];
  int py0[4], px0[4];
  int64_t xo[4], cell0[4];
  const float* ob[4];
  float s0[4], s1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t gpos = pos0 + wave * 16 + 4 * q + r;
    live[r] = gpos < a.P;
    py0[r] = px0[r] = 0, xo[r] = cell0[r] = 0, ob[r] = a.off, s0[r] = s1[r] = 0.0f;
    if (live[r]) {
      const int64_t ni = gpos / HW;
      const int rem = (int)(gpos - ni * HW);
      py0[r] = rem / W;
      px0[r] = rem - py0[r] * W;
      xo[r] = ni * a.sn;
      cell0[r] = ni * HW;
      ob[r] = a.off + ni * a.on + py0[r] * a.oy + px0[r] * a.ox;
      if (GUIDED) s0[r] = ob[r][0], s1[r] = ob[r][a.oc];
    }
  }
  // the position whose goff this lane stores (lanes p < 4): 4 q + p
  const int64_t spos = pos0 + wave * 16 + 4 * q + (p & 3);
  const bool sstore = a.goff && p < 4 && spos < a.P;
  int64_t sbase = 0;
  if (sstore) {
    const int64_t ni = spos / HW;
    sbase = ni * 18 * a.dg * HW + (spos - ni * HW);
  }
  __syncthreads();

  const int cchunks = cin / kDcbKc, jb = cout / 16;
  const int arow = (wave * 16 + p) * c4n, aswz = p;  // (wave * 16 + p) & 15 == p
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3 - 1, kx = tap - (tap / 3) * 3 - 1;
    f32x4 ady = {0.0f, 0.0f, 0.0f, 0.0f}, adx = ady;
    int curg = -1;  // the group ady / adx are summing (wave-uniform)
    for (int cc = 0; cc < cchunks; ++cc) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      const f32x4* wsrc = reinterpret_cast<const f32x4*>(a.wp + (int64_t)(tap * cchunks + cc) * jb * 256) + p * 4 + q;
      for (int j0 = 0; j0 < jb; j0 += 4)  // jb is a multiple of 4
#pragma unroll
      for (int j = j0; j < j0 + 4; ++j) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(&gys[(arow + ((4 * j + q) ^ aswz)) * 4]);
        const f32x4 bv = wsrc[j * 64];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
      }
      const int c = cc * kDcbKc + p;
      const int och = (c / a.cpg) * 18 + 2 * tap;
      float cy[4], cx[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cy[r] = cx[r] = 0.0f;
        if (!live[r]) continue;
        float dy, dx;
        dcb_offsets<GUIDED>(a, ob[r], s0[r], s1[r], och, dy, dx);
        const float py = (float)(py0[r] + ky) + dy, px = (float)(px0[r] + kx) + dx;
        DcbPoint s;
        if (!dcb_point(py, px, H, W, s)) continue;
        const float G = acc[r];
        if (a.goff) {
          const float* xp = a.x + xo[r] + s.y0 * a.sy + s.x0 * a.sx + c;
          const float v00 = s.yt && s.xl ? xp[0] : 0.0f;
          const float v01 = s.yt && s.xr ? xp[a.sx] : 0.0f;
          const float v10 = s.yb && s.xl ? xp[a.sy] : 0.0f;
          const float v11 = s.yb && s.xr ? xp[a.sy + a.sx] : 0.0f;
          cy[r] = G * (s.hx * (v10 - v00) + s.lx * (v11 - v01));
          cx[r] = G * (s.hy * (v01 - v00) + s.ly * (v11 - v10));
        }
        if (a.gx) {
          float* gp = a.gx + (cell0[r] + (int64_t)s.y0 * W + s.x0) * cin + c;
          if (s.yt && s.xl) atomicAdd(gp, G * (s.hy * s.hx));
          if (s.yt && s.xr) atomicAdd(gp + cin, G * (s.hy * s.lx));
          if (s.yb && s.xl) atomicAdd(gp + (int64_t)W * cin, G * (s.ly * s.hx));
          if (s.yb && s.xr) atomicAdd(gp + (int64_t)(W + 1) * cin, G * (s.ly * s.lx));
        }
      }
      if (a.goff) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // the channel quad's sum, in every lane of the quad
          cy[r] += __shfl_xor(cy[r], 1, kWave);
          cx[r] += __shfl_xor(cx[r], 1, kWave);
          cy[r] += __shfl_xor(cy[r], 2, kWave);
          cx[r] += __shfl_xor(cx[r], 2, kWave);
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {  // quads in ascending channel order; a quad never straddles groups
          const int g = (cc * kDcbKc + 4 * qq) / a.cpg;
          if (g != curg) {
            if (curg >= 0) dcb_store_goff(sstore, a.goff + sbase + (int64_t)(curg * 18 + 2 * tap) * HW, HW, p, ady, adx);
            curg = g;
            ady = adx = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            ady[r] += __shfl(cy[r], (lane & 48) + 4 * qq, kWave);
            adx[r] += __shfl(cx[r], (lane & 48) + 4 * qq, kWave);
          }
        }
      }
    }
    if (a.goff && curg >= 0)
      dcb_store_goff(sstore, a.goff + sbase + (int64_t)(curg * 18 + 2 * tap) * HW, HW, p, ady, adx);
  }
}

template <int RT, bool GUIDED>
__global__ void __launch_bounds__(kDcbThreads) deform_conv3x3_bwd_weight_kernel(const DcbArgs a) {
  __shared__ __attribute__((aligned(16))) float Bs[kDcbCols * kDcbKc];  // [position][channel]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int H = a.h, W = a.w, cout = a.cout;
  const int64_t HW = (int64_t)H * W;
  const int cchunks = a.cin / kDcbKc;
  const int col = (int)(blockIdx.x % (9 * cchunks)), split = (int)(blockIdx.x / (9 * cchunks));
  const int tap = col / cchunks, cc = col - tap * cchunks;
  const int ky = tap / 3 - 1, kx = tap - (tap / 3) * 3 - 1;
  const int t0 = split * a.tiles_per_split;
  const int t1 = t0 + a.tiles_per_split < a.tiles ? t0 + a.tiles_per_split : a.tiles;

  // this thread's gather item, as in the forward: position pl of the tile, channels c0 .. c0 + 3
  const int pl = tid >> 2, c4 = tid & 3;
  const int c0 = cc * kDcbKc + c4 * 4;
  const int och = (c0 / a.cpg) * 18 + 2 * tap;
  const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};

  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = z4;

  for (int t = t0; t < t1; ++t) {
    const int64_t pos0 = (int64_t)t * kDcbCols;
    f32x4 b = z4;
    const int64_t gpos = pos0 + pl;
    if (gpos < a.P) {
      const int64_t ni = gpos / HW;
      const int rem = (int)(gpos - ni * HW);
      const int py0 = rem / W, px0 = rem - py0 * W;
      const float* ob = a.off + ni * a.on + py0 * a.oy + px0 * a.ox;
      float s0 = 0.0f, s1 = 0.0f, dy, dx;
      if (GUIDED) s0 = ob[0], s1 = ob[a.oc];
      dcb_offsets<GUIDED>(a, ob, s0, s1, och, dy, dx);
      const float py = (float)(py0 + ky) + dy, px = (float)(px0 + kx) + dx;
      DcbPoint s;
      if (dcb_point(py, px, H, W, s)) {
        const float* xp = a.x + ni * a.sn + s.y0 * a.sy + s.x0 * a.sx + c0;
        f32x4 v00 = z4, v01 = z4, v10 = z4, v11 = z4;
        if (s.yt && s.xl) v00 = *reinterpret_cast<const f32x4*>(xp);
        if (s.yt && s.xr) v01 = *reinterpret_cast<const f32x4*>(xp + a.sx);
        if (s.yb && s.xl) v10 = *reinterpret_cast<const f32x4*>(xp + a.sy);
        if (s.yb && s.xr) v11 = *reinterpret_cast<const f32x4*>(xp + a.sy + a.sx);
        b = (((s.hy * s.hx) * v00 + (s.hy * s.lx) * v01) + (s.ly * s.hx) * v10) + (s.ly * s.lx) * v11;
      }
    }
    __syncthreads();  // every wave has read the previous tile
    *reinterpret_cast<f32x4*>(&Bs[pl * kDcbKc + c4 * 4]) = b;
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kDcbCols / 4; ++kk) {
      const int64_t pos = pos0 + 4 * kk + q;
      const float bv = Bs[(4 * kk + q) * kDcbKc + p];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int co = (wave * RT + rt) * 16 + p;
        float av = 0.0f;
        if (pos < a.P) {
          av = a.gy[pos * cout + co];
          if (a.y) av = a.y[pos * cout + co] > 0.0f ? av : 0.0f;
        }
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[rt], 0, 0, 0);
      }
    }
  }

  // register r of tile rt: output channel (wave RT + rt) 16 + 4 q + r, input channel 16 cc + p
  float* slab = a.slab + (int64_t)split * cout * a.cin * 9;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = (wave * RT + rt) * 16 + 4 * q + r;
      slab[((int64_t)co * a.cin + cc * kDcbKc + p) * 9 + tap] = acc[rt][r];
    }
}

// gw[i] = slab[0][i] + slab[1][i] + ... in split order
__global__ void __launch_bounds__(256) deform_conv3x3_bwd_reduce_kernel(const float* __restrict__ slab,
                                                                        float* __restrict__ gw, int64_t elems,
                                                                        int splits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x) {
    float s = slab[i];
    for (int k = 1; k < splits; ++k) s += slab[(int64_t)k * elems + i];
    gw[i] = s;
  }
}

}  // namespace frh
