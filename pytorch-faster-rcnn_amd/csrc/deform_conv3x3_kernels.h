// Deformable (DCNv1) 3x3 / stride-1 / padding-1 / dilation-1 convolution without bias, x NHWC
// f32 (channel stride 1, any image / row / column strides) -> y contiguous NHWC, with an
// optional ReLU on the accumulators: the Guided Anchoring adaption layer.
//
// Definition (mmdet v1 / torchvision deform_conv2d).  Input channel c belongs to deformable
// group g = c / (cin / dg).  Tap k = 3 (ky + 1) + (kx + 1) of group g at output (y, x) samples
// x at (py, px) = (y + ky + dy, x + kx + dx), dy / dx = offset channels g * 18 + 2 k / + 1.  The
// sample is 0 unless -1 < py < H and -1 < px < W (tested in float, before any conversion to
// int: a non-finite or huge offset fails the test and forms no address); otherwise it is
// ((hy hx) v00 + (hy lx) v01) + (ly hx) v10 + (ly lx) v11 over the four neighbours, ly = py -
// floor(py), hy = 1 - ly, neighbours outside the map contributing 0.
//
// As a GEMM: rows are cout (A operand: the weights), columns are the positions of (image, y, x)
// (B operand: the blended samples), K = (tap, channel), on v_mfma_f32_32x32x2_f32 (exact f32, a
// k-ordered fmaf chain).  A workgroup of four waves owns MT = 256 / 128 / 64 output channels of
// kDcCols = 64 consecutive positions and walks K in 9 * cin / 16 chunks of one tap and kDcKc = 16
// channels.  Per chunk:
//   B: thread (position tid >> 2, channel quad tid & 3) computes its sample point, loads the
//      four corners as float4 (the four lanes of a position read 64 consecutive bytes of each
//      corner), blends them in registers and writes the four channels to Bs[channel][position]
//      (row length 66: the four quads of a wave half land 8 banks apart, no write conflict; an
//      MFMA half reads 32 consecutive floats).  The loads of chunk t + 1 are in flight behind
//      the MFMAs of chunk t.
//   A: As[channel][co], a float4 copy of the slab the repack launch wrote in this order.
// Offsets come from one of two sources behind the template flag: the explicit [n, 18 dg, h, w]
// map, or (guided) the 2-channel shape map s and the offset layer's weight ow [18 dg, 2], the
// offset being (ow[c][0] * s0) + (ow[c][1] * s1) in that f32 order -- the 1x1 convolution the
// reference runs first, whose 18 dg-channel output is then never written or read.
//
// The sum over K runs tap-major, then channel, lane half h on the odd / even channel of a pair:
// one fixed order for every column, level, launch and n.  Columns of an MFMA never mix, so a
// position's bits depend on nothing but its own inputs.  No atomics.
//
// K is not split: a workgroup runs its 9 * cin / 16 chunks (144 at cin = 256) one after another,
// so a call with few positions is latency-bound (about 270 us at 256 -> 256 however small the
// map: the three coarse FPN levels alone).  The _levels entry runs the small levels in the tail
// of the large ones' launch; per-level calls at small n * h * w pay that floor each.
#pragma once
#include "common.h"

namespace frh {

constexpr int kDcKc = 16;         // input channels per chunk
constexpr int kDcCols = 64;       // positions per workgroup
constexpr int kDcLd = 66;         // row length of the B slab
constexpr int kDcThreads = 256;
constexpr int kDcMaxLevels = 8;

struct DcLevel {
  const float* x;
  const float* off;  // explicit: [n, 18 dg, h, w]; guided: the shape map [n, 2, h, w]
  float* y;
  int h, w;
  int64_t sn, sy, sx;      // x strides (image, row, column), elements
  int64_t on, oc, oy, ox;  // off strides (image, channel, row, column), elements
  int64_t tile0;           // first position tile of this level
};

struct DcArgs {
  DcLevel lv[kDcMaxLevels];
  int L;
  const float* wp;  // repacked weights (workspace)
  const float* ow;  // guided: offset-layer weight [18 dg, 2]
  int64_t n;
  int cin, cout, cpg;  // cpg = cin / dg
  int mt;              // channel blocks of MT
  int relu;
};

// ws[mb][tap][cc][kk][co] = w[mb * MT + co][cc * 16 + kk][tap]
__global__ void __launch_bounds__(256) deform_conv3x3_repack_kernel(const float* __restrict__ w,
                                                                    float* __restrict__ ws, int cin, int cout,
                                                                    int MT) {
  const int64_t total = (int64_t)cin * cout * 9;
  const int cchunks = cin / kDcKc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % MT);
    int64_t k = i / MT;
    const int kk = (int)(k % kDcKc);
    k /= kDcKc;
    const int cc = (int)(k % cchunks);
    k /= cchunks;
    const int tap = (int)(k % 9);
    const int mb = (int)(k / 9);
    ws[i] = w[((int64_t)(mb * MT + co) * cin + cc * kDcKc + kk) * 9 + tap];
  }
}

template <int MT, bool GUIDED>
__global__ void __launch_bounds__(kDcThreads) deform_conv3x3_kernel(const DcArgs a) {
  constexpr int NT = kDcThreads;
  constexpr int RT = MT == 256 ? 2 : 1;   // 32-row tiles per wave
  constexpr int CB = MT == 64 ? 1 : 2;    // 32-column blocks per wave
  constexpr int AS = kDcKc * MT;          // floats of the W slab
  constexpr int AV = AS / 4 / NT;         // float4 of W per thread per chunk
  static_assert(AS / 4 % NT == 0, "W slab must split evenly over the threads");
  __shared__ __attribute__((aligned(16))) float As[AS];
  __shared__ float Bs[kDcKc * kDcLd];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  const int mb = (int)(blockIdx.x % a.mt);
  const int64_t tile = blockIdx.x / a.mt;
  int l = 0;
  while (l + 1 < a.L && tile >= a.lv[l + 1].tile0) ++l;
  const float* const xg = a.lv[l].x;
  const float* const og = a.lv[l].off;
  const int H = a.lv[l].h, W = a.lv[l].w;
  const int64_t sy = a.lv[l].sy, sx = a.lv[l].sx;
  const int64_t oc = a.lv[l].oc;
  const int64_t P = a.n * H * W;  // positions of this level
  const int64_t pos0 = (tile - a.lv[l].tile0) * kDcCols;
  const int m0 = mb * MT;
  const int wrow = MT == 64 ? (wave & 1) * 32 : wave * 32 * RT;  // first channel row of this wave
  const int wcb = MT == 64 ? (wave >> 1) : 0;                    // first column block of this wave

  // this thread's gather item: position pl of the tile, channels 4 c4 .. 4 c4 + 3 of every chunk
  const int pl = tid >> 2, c4 = tid & 3;
  const int64_t gpos = pos0 + pl;
  const bool live = gpos < P;
  int py0 = 0, px0 = 0;
  const float* xb = xg;   // the position's image
  const float* ob = og;   // the position's offsets: channel 0 at (y, x)
  if (live) {
    const int64_t ni = gpos / ((int64_t)H * W);
    const int rem = (int)(gpos - ni * H * W);
    py0 = rem / W;
    px0 = rem - py0 * W;
    xb = xg + ni * a.lv[l].sn;
    ob = og + ni * a.lv[l].on + py0 * a.lv[l].oy + px0 * a.lv[l].ox;
  }
  float s0 = 0.0f, s1 = 0.0f;
  if (GUIDED && live) s0 = ob[0], s1 = ob[oc];

  const int cchunks = a.cin / kDcKc;
  const int chunks = 9 * cchunks;
  const f32x4* wsrc = reinterpret_cast<const f32x4*>(a.wp + (int64_t)mb * chunks * AS) + tid;
  const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 ra[AV], rv[4];
  float rw[4];
  auto load = [&](int t) {
#pragma unroll
    for (int u = 0; u < AV; ++u) ra[u] = wsrc[(int64_t)t * (AS / 4) + u * NT];
    rv[0] = rv[1] = rv[2] = rv[3] = z4;
    rw[0] = rw[1] = rw[2] = rw[3] = 0.0f;
    if (!live) return;
    const int tap = t / cchunks, cc = t - tap * cchunks;
    const int ky = tap / 3 - 1, kx = tap - (tap / 3) * 3 - 1;
    const int c0 = cc * kDcKc + c4 * 4;
    const int och = (c0 / a.cpg) * 18 + 2 * tap;
    float dy, dx;
    if (GUIDED) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(a.ow + 2 * och);
      dy = (q.x * s0) + (q.y * s1);
      dx = (q.z * s0) + (q.w * s1);
    } else {
      dy = ob[och * oc];
      dx = ob[(och + 1) * oc];
    }
    const float py = (float)(py0 + ky) + dy, px = (float)(px0 + kx) + dx;
    // in float, before any conversion: NaN and far offsets fail here and form no address
    if (!(py > -1.0f && py < (float)H && px > -1.0f && px < (float)W)) return;
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = (int)fy, x0 = (int)fx;  // in [-1, H - 1] x [-1, W - 1]
    const float ly = py - fy, lx = px - fx;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    rw[0] = hy * hx, rw[1] = hy * lx, rw[2] = ly * hx, rw[3] = ly * lx;
    const bool yt = y0 >= 0, yb = y0 + 1 <= H - 1, xl = x0 >= 0, xr = x0 + 1 <= W - 1;
    const float* p = xb + y0 * sy + x0 * sx + c0;
    if (yt && xl) rv[0] = *reinterpret_cast<const f32x4*>(p);
    if (yt && xr) rv[1] = *reinterpret_cast<const f32x4*>(p + sx);
    if (yb && xl) rv[2] = *reinterpret_cast<const f32x4*>(p + sy);
    if (yb && xr) rv[3] = *reinterpret_cast<const f32x4*>(p + sy + sx);
  };

  const int abase = h * MT + wrow + j;
  const int bbase = h * kDcLd + wcb * 32 + j;
  const int bdst = c4 * 4 * kDcLd + pl;

  f32x16 acc[RT][CB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][cb][r] = 0.0f;

  load(0);
  for (int t = 0; t < chunks; ++t) {
#pragma unroll
    for (int u = 0; u < AV; ++u) *reinterpret_cast<f32x4*>(&As[(tid + u * NT) * 4]) = ra[u];
    {
      const f32x4 b = ((rw[0] * rv[0] + rw[1] * rv[1]) + rw[2] * rv[2]) + rw[3] * rv[3];
      Bs[bdst] = b.x;
      Bs[bdst + kDcLd] = b.y;
      Bs[bdst + 2 * kDcLd] = b.z;
      Bs[bdst + 3 * kDcLd] = b.w;
    }
    __syncthreads();
    if (t + 1 < chunks) load(t + 1);  // in flight behind this chunk's MFMAs
#pragma unroll
    for (int q = 0; q < kDcKc / 2; ++q) {
      float af[RT], bf[CB];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) af[rt] = As[abase + 2 * q * MT + rt * 32];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bf[cb] = Bs[bbase + 2 * q * kDcLd + cb * 32];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[rt][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[rt], bf[cb], acc[rt][cb], 0, 0, 0);
    }
    __syncthreads();  // every wave has read this chunk before the next one is written
  }

  // epilogue: registers 4 i .. 4 i + 3 of a 32 x 32 tile are rows 8 i + 4 h .. + 3 of column j:
  // four consecutive output channels of one position, one 16-byte store
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int64_t pos = pos0 + (wcb + cb) * 32 + j;
    if (pos >= P) continue;
    float* yp = a.lv[l].y + pos * a.cout + m0 + wrow + 4 * h;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = {acc[rt][cb][4 * i], acc[rt][cb][4 * i + 1], acc[rt][cb][4 * i + 2], acc[rt][cb][4 * i + 3]};
        if (a.relu) {
          v.x = v.x > 0.0f ? v.x : 0.0f;
          v.y = v.y > 0.0f ? v.y : 0.0f;
          v.z = v.z > 0.0f ? v.z : 0.0f;
          v.w = v.w > 0.0f ? v.w : 0.0f;
        }
        *reinterpret_cast<f32x4*>(yp + rt * 32 + 8 * i) = v;
      }
  }
}

struct DeformConvLevelDesc {
  const float* x;
  const float* off;
  float* y;
  int32_t h, w;
  int64_t sn, sy, sx;
  int64_t on, oc, oy, ox;
};

inline int32_t deform_conv3x3_launch(const char* what, int32_t num_levels, const DeformConvLevelDesc* d,
                                     const float* offset_w, const float* w, float* workspace, int64_t n,
                                     int32_t cin, int32_t cout, int32_t dg, int32_t relu, void* stream) {
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kDcMaxLevels, "1 to %d levels, got %d", kDcMaxLevels, num_levels);
  FRH_REQUIRE(n >= 0 && cin >= 1 && cout >= 1 && dg >= 1, "bad sizes");
  FRH_REQUIRE(cin % 16 == 0 && cout % 64 == 0, "cin %d must be a multiple of 16 and cout %d of 64", cin, cout);
  FRH_REQUIRE(cin % dg == 0 && (cin / dg) % 4 == 0, "cin / deformable_groups must be a multiple of 4 (cin %d, dg %d)",
              cin, dg);
  if (n == 0) return FRH_OK;
  FRH_REQUIRE(w && workspace, "null pointer argument");
  FRH_REQUIRE_ALIGNED16(w, workspace, offset_w);
  const int64_t wb = (int64_t)cin * cout * 9 * 4;
  FRH_REQUIRE(!ranges_overlap(workspace, wb, w, wb), "the workspace must not overlap w");
  const int mtile = cout % 256 == 0 ? 256 : (cout % 128 == 0 ? 128 : 64);
  DcArgs a;
  a.L = num_levels, a.wp = workspace, a.ow = offset_w, a.n = n;
  a.cin = cin, a.cout = cout, a.cpg = cin / dg, a.mt = cout / mtile, a.relu = relu;
  const int och = offset_w ? 2 : 18 * dg;
  int64_t tiles = 0;
  for (int i = 0; i < num_levels; ++i) {
    const DeformConvLevelDesc& v = d[i];
    FRH_REQUIRE(v.x && v.off && v.y, "null pointer argument (level %d)", i);
    FRH_REQUIRE(v.h >= 1 && v.w >= 1, "empty level %d", i);
    FRH_REQUIRE_ALIGNED16(v.x, v.y);
    FRH_REQUIRE(v.sn >= 0 && v.sy >= 0 && v.sx >= cin && (v.sn | v.sy | v.sx) % 4 == 0,
                "level %d: x strides must be non-negative multiples of 4, the column stride >= cin", i);
    const int64_t xe = (n - 1) * v.sn + (v.h - 1) * v.sy + (v.w - 1) * v.sx + cin;
    const int64_t p = n * v.h * v.w;
    if (p >= ((int64_t)1 << 31) || xe >= ((int64_t)1 << 40)) {
      set_error("%s: level %d is too large", what, i);
      return FRH_EUNSUPPORTED;
    }
    const int64_t xb = xe * 4, yb = p * cout * 4;
    // the byte range the offsets span, for any (signed) strides
    int64_t olo = 0, ohi = 0;
    const int64_t ext[4] = {(n - 1) * v.on, (och - 1) * v.oc, (v.h - 1) * v.oy, (v.w - 1) * v.ox};
    for (int e = 0; e < 4; ++e) (ext[e] < 0 ? olo : ohi) += ext[e];
    FRH_REQUIRE(!ranges_overlap(v.y, yb, v.x, xb) && !ranges_overlap(v.y, yb, workspace, wb) &&
                    !ranges_overlap(v.y, yb, w, wb) && !ranges_overlap(v.y, yb, v.off + olo, (ohi - olo + 1) * 4) &&
                    !ranges_overlap(workspace, wb, v.x, xb),
                "level %d: y must not overlap x, w, the offsets or the workspace", i);
    FRH_REQUIRE(!offset_w || !ranges_overlap(v.y, yb, offset_w, (int64_t)36 * dg * 4),
                "level %d: y must not overlap the offset-layer weight", i);
    for (int k = 0; k < num_levels; ++k) {  // another level's input or output
      if (k == i) continue;
      const int64_t kxb = ((n - 1) * d[k].sn + (d[k].h - 1) * d[k].sy + (d[k].w - 1) * d[k].sx + cin) * 4;
      FRH_REQUIRE(!ranges_overlap(v.y, yb, d[k].y, n * d[k].h * d[k].w * (int64_t)cout * 4) &&
                      !ranges_overlap(v.y, yb, d[k].x, kxb),
                  "level %d: y overlaps level %d", i, k);
    }
    a.lv[i] = {v.x, v.off, v.y, v.h, v.w, v.sn, v.sy, v.sx, v.on, v.oc, v.oy, v.ox, tiles};
    tiles += (p + kDcCols - 1) / kDcCols;
  }
  const int64_t blocks = tiles * a.mt;
  if (blocks >= ((int64_t)1 << 31)) {
    set_error("%s: too many blocks", what);
    return FRH_EUNSUPPORTED;
  }
  const int64_t welems = (int64_t)cin * cout * 9;
  const unsigned rp_blocks = (unsigned)((welems + 255) / 256 < 4096 ? (welems + 255) / 256 : 4096);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(deform_conv3x3_repack_kernel, dim3(rp_blocks), dim3(256), 0, s, w, workspace, (int)cin,
                     (int)cout, mtile);
  const dim3 g((unsigned)blocks), b(kDcThreads);
#define FRH_DC_LAUNCH(MT_)                                                                      \
  do {                                                                                          \
    if (offset_w)                                                                               \
      hipLaunchKernelGGL((deform_conv3x3_kernel<MT_, true>), g, b, 0, s, a);                    \
    else                                                                                        \
      hipLaunchKernelGGL((deform_conv3x3_kernel<MT_, false>), g, b, 0, s, a);                   \
  } while (0)
  if (mtile == 256)
    FRH_DC_LAUNCH(256);
  else if (mtile == 128)
    FRH_DC_LAUNCH(128);
  else
    FRH_DC_LAUNCH(64);
#undef FRH_DC_LAUNCH
  return check_launch(what);
}

}  // namespace frh
