// 3x3 / stride-1 / padding-1 convolution on channels-last f32 with the bias (+ ReLU) epilogue,
// as Winograd F(2x2, 3x3): 16 multiplies per 2 x 2 outputs and channel pair instead of 36.
//   U = G g G^T      per (cout, cin): the 4 x 4 transformed filter (conv3x3_bias_act_weights_kernel)
//   V = B^T d B      per (tile, cin): the 4 x 4 transformed input patch of a 2 x 2 output tile
//   M_p = V_p . U_p  per Winograd position p of 16: a GEMM [tile, cin] x [cin, cout]
//   Y = A^T M A      per (tile, cout): the 2 x 2 outputs, then + bias, then ReLU
// with the standard matrices  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],
// G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],  A^T = [1 1 1 0; 0 1 -1 -1].
//
// The 16 GEMMs run on v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fmaf chain).  A wave owns
// 32 tiles (MFMA rows, registers) x 32 output channels (MFMA columns, lanes) and holds one
// 32 x 32 accumulator per position: 256 accumulator registers, 16 independent MFMA chains, one
// wave per SIMD.  Every lane then holds the same (tile, cout) element of all 16 M_p, so the
// output transform, the bias and the ReLU are register-local, the stores are 128-byte channel
// runs of NHWC pixels, and M never leaves the registers.
//
// Workgroup: 256 threads = 2 x 2 waves = 64 tiles (8 x 8 tiles = 16 x 16 outputs of one image)
// x 64 output channels.  cin is walked in chunks of 8: 64 MFMAs per wave per chunk.  Per chunk
//   - every thread loads the 4 x 4 pixels x float2 of its tile's patch (four threads per tile
//     share the chunk's 8 channels), applies B^T d B and writes 16 float2 of V;
//   - every thread copies 8 float4 of the U chunk, which the weights kernel wrote in the LDS
//     image's own order.
// Both go global -> registers -> LDS, two LDS stages, one barrier per chunk: the loads of chunk
// t + 2 are in flight while chunk t runs its MFMAs, and chunk t + 1 is transformed and written
// between them.  LDS images: V [16][64 tiles][8 k] and U [16][64 cout][8 k]; lane half h owns
// k = 4 h .. 4 h + 3 of the chunk (a fixed permutation of the k order), one ds_read_b128 per
// operand and position.  A row's two 16-byte halves swap places when bit 3 of the row index is
// set: each 16-lane group of a ds_read_b128 then reads 16 distinct 4-bank groups.
//
// Pixels outside the image are the zero padding: their loads go to a clamped address and are
// zeroed; stores past the image's edge are masked.  Workgroups are numbered level by level,
// cout block slowest inside a level, and dealt to the 8 XCDs in contiguous chunks, so an XCD
// works through one 1-MB slice of U at a time.  Fixed summation order, no atomics, no split
// over cin: the same inputs give the same bits on every launch.
#pragma once
#include "common.h"

namespace frh {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));

constexpr int kWgThreads = 256;
constexpr int kWgBK = 8;        // cin per chunk
constexpr int kWgSide = 8;      // tiles per workgroup side (16 outputs)
constexpr int kWgCout = 64;     // output channels per workgroup
constexpr int kWgXcds = 8;
constexpr int kWgMaxLevels = 8;
constexpr int kWgSlab = 64 * kWgBK;             // floats of one position of V (or U) per chunk
constexpr int kWgStage = 2 * 16 * kWgSlab;      // floats of one LDS stage: V then U

struct Conv3x3Level {
  const float* x;
  const float* u;     // transformed weights [cin / 8][16][cout][8]
  const float* bias;  // nullable
  float* y;
  int64_t sn;         // x element strides: image, row, column (channel stride 1)
  int32_t sy, sx;
  int32_t h, w;
  int32_t by, bx;     // workgroup blocks down, across
  int32_t first;      // first logical workgroup of the level
};

struct Conv3x3Args {
  Conv3x3Level lv[kWgMaxLevels];
  int32_t levels, n, cin, cout, relu;
  int32_t total, chunk;  // logical workgroups; ceil(total / kWgXcds)
};

// float offset of (row r, k half kh) inside a [64][8] slab
__device__ __forceinline__ int wg_slab_off(int r, int kh) { return r * kWgBK + ((kh ^ ((r >> 3) & 1)) << 2); }

struct Conv3x3Weights {
  const float* w[kWgMaxLevels];
  float* u[kWgMaxLevels];
};

// U = G g G^T of w [cout][3][3][cin] into [cin / 8][16][cout][8], rows in wg_slab_off order,
// for weight blockIdx.y of the table.  One thread per (chunk, cout, k half): 9 float4 in,
// 16 float4 out, a wave's stores contiguous.
__global__ void __launch_bounds__(256) conv3x3_bias_act_weights_kernel(const Conv3x3Weights tab, int cin, int cout) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)(cin / kWgBK) * cout * 2) return;
  const float* w = tab.w[0];
  float* u = tab.u[0];
#pragma unroll
  for (int i = 1; i < kWgMaxLevels; ++i)
    if (i == (int)blockIdx.y) w = tab.w[i], u = tab.u[i];
  const int kh = (int)(idx & 1);
  const int co = (int)((idx >> 1) % cout);
  const int ch = (int)((idx >> 1) / cout);
  const float* wp = w + (int64_t)co * 9 * cin + ch * kWgBK + kh * 4;
  float g[3][3][4];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float4 v = *reinterpret_cast<const float4*>(wp + (ky * 3 + kx) * cin);
      g[ky][kx][0] = v.x, g[ky][kx][1] = v.y, g[ky][kx][2] = v.z, g[ky][kx][3] = v.w;
    }
  float t[4][3][4];  // G g
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = g[0][kx][c] + g[2][kx][c];
      t[0][kx][c] = g[0][kx][c];
      t[1][kx][c] = (s + g[1][kx][c]) * 0.5f;
      t[2][kx][c] = (s - g[1][kx][c]) * 0.5f;
      t[3][kx][c] = g[2][kx][c];
    }
  float* up = u + ((int64_t)ch * 16 * cout + co) * kWgBK + ((kh ^ ((co >> 3) & 1)) << 2);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float o[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = t[a][0][c] + t[a][2][c];
      o[0][c] = t[a][0][c];
      o[1][c] = (s + t[a][1][c]) * 0.5f;
      o[2][c] = (s - t[a][1][c]) * 0.5f;
      o[3][c] = t[a][2][c];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
      *reinterpret_cast<float4*>(up + (int64_t)(a * 4 + b) * cout * kWgBK) =
          make_float4(o[b][0], o[b][1], o[b][2], o[b][3]);
  }
}

__global__ void __launch_bounds__(kWgThreads) conv3x3_bias_act_wino_kernel(const Conv3x3Args a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kWgStage];  // 128 KB: two stages of V, U

  // XCD x takes logical workgroups [x * chunk, (x + 1) * chunk)
  const int wg = (int)(blockIdx.x % kWgXcds) * a.chunk + (int)(blockIdx.x / kWgXcds);
  if (wg >= a.total) return;
  Conv3x3Level L = a.lv[0];
#pragma unroll
  for (int i = 1; i < kWgMaxLevels; ++i)
    if (i < a.levels && wg >= a.lv[i].first) L = a.lv[i];
  const int H = L.h, W = L.w;
  int rest = wg - L.first;
  const int bx = rest % L.bx;
  rest /= L.bx;
  const int by = rest % L.by;
  rest /= L.by;
  const int img = rest % a.n;
  const int cb = rest / a.n;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;

  // ---- staging roles
  // V: tile T = tid >> 2 (8 x 8, row-major), channels 2 c2, 2 c2 + 1 of the chunk: the whole
  // 4 x 4 patch as 16 float2, B^T d B on both channels, 16 ds_write_b64.
  const int T = tid >> 2, c2 = tid & 3;
  const int iy0 = (by * kWgSide + (T >> 3)) * 2 - 1;
  const int ix0 = (bx * kWgSide + (T & 7)) * 2 - 1;
  // wave-uniform bases; the lane's part is a 32-bit byte offset (no address arithmetic per load)
  const char* xb = reinterpret_cast<const char*>(L.x + (int64_t)img * L.sn);
  uint32_t xoff[4][4];
  bool xok[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int iy = iy0 + r, ix = ix0 + c;
      xok[r][c] = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
      xoff[r][c] = (uint32_t)(cy * L.sy + cx * L.sx + c2 * 2) * 4u;  // bytes
    }
  const int v_off = wg_slab_off(T, c2 >> 1) + (c2 & 1) * 2;
  // U: float4 q * 256 + tid of the chunk's [16][64][8] image, q = 0 .. 7
  const char* ub = reinterpret_cast<const char*>(L.u + (int64_t)cb * kWgCout * kWgBK);
  const uint32_t u_src = (uint32_t)((tid >> 7) * a.cout * kWgBK + (tid & 127) * 4) * 4u;
  const int64_t u_pos = (int64_t)2 * a.cout * kWgBK * 4;     // two positions on, bytes
  const int64_t u_chunk = (int64_t)16 * a.cout * kWgBK * 4;  // one chunk on
  const int u_off = 16 * kWgSlab + (tid >> 7) * kWgSlab + (tid & 127) * 4;
  // MFMA operands: A = V rows (tiles wm * 32 + j), B = U rows (channels wn * 32 + j), k half h
  const int a_off = wg_slab_off(wm * 32 + j, h);
  const int b_off = 16 * kWgSlab + wg_slab_off(wn * 32 + j, h);

  // staging registers (named: an indexed array of them ends up in LDS)
  wg_f32x2 x00, x01, x02, x03, x10, x11, x12, x13, x20, x21, x22, x23, x30, x31, x32, x33;
  float4 u0, u1, u2, u3, u4, u5, u6, u7;
#define FRH_WG_LX(r, c) x##r##c = *reinterpret_cast<const wg_f32x2*>(xs_ + xoff[r][c])
#define FRH_WG_LU(q) *reinterpret_cast<const float4*>(up_ + (q) * u_pos + u_src)
#define FRH_WG_LOAD(t)                                                                   \
  do {                                                                                   \
    const char* xs_ = xb + (t) * (kWgBK * 4);                                               \
    FRH_WG_LX(0, 0), FRH_WG_LX(0, 1), FRH_WG_LX(0, 2), FRH_WG_LX(0, 3);                  \
    FRH_WG_LX(1, 0), FRH_WG_LX(1, 1), FRH_WG_LX(1, 2), FRH_WG_LX(1, 3);                  \
    FRH_WG_LX(2, 0), FRH_WG_LX(2, 1), FRH_WG_LX(2, 2), FRH_WG_LX(2, 3);                  \
    FRH_WG_LX(3, 0), FRH_WG_LX(3, 1), FRH_WG_LX(3, 2), FRH_WG_LX(3, 3);                  \
    const char* up_ = ub + (t) * u_chunk;                                                \
    u0 = FRH_WG_LU(0), u1 = FRH_WG_LU(1), u2 = FRH_WG_LU(2), u3 = FRH_WG_LU(3);          \
    u4 = FRH_WG_LU(4), u5 = FRH_WG_LU(5), u6 = FRH_WG_LU(6), u7 = FRH_WG_LU(7);          \
  } while (0)

  // the U copy and B^T d B of the staged patch into stage ST: columns first (e = B^T d), then
  // rows, each V row written as soon as it is complete
#define FRH_WG_Z(r, c) (xok[r][c] ? x##r##c : z2)
#define FRH_WG_VROW(vp, e0, e1, e2, e3)                                   \
  do {                                                                    \
    *reinterpret_cast<wg_f32x2*>(vp) = (e0) - (e2);                       \
    *reinterpret_cast<wg_f32x2*>((vp) + kWgSlab) = (e1) + (e2);           \
    *reinterpret_cast<wg_f32x2*>((vp) + 2 * kWgSlab) = (e2) - (e1);       \
    *reinterpret_cast<wg_f32x2*>((vp) + 3 * kWgSlab) = (e1) - (e3);       \
  } while (0)
#define FRH_WG_STORE(ST)                                                                             \
  do {                                                                                               \
    float* sp = lds + (ST) * kWgStage;                                                               \
    float* uq = sp + u_off;                                                                          \
    *reinterpret_cast<float4*>(uq) = u0, *reinterpret_cast<float4*>(uq + 2 * kWgSlab) = u1;          \
    *reinterpret_cast<float4*>(uq + 4 * kWgSlab) = u2, *reinterpret_cast<float4*>(uq + 6 * kWgSlab) = u3;   \
    *reinterpret_cast<float4*>(uq + 8 * kWgSlab) = u4, *reinterpret_cast<float4*>(uq + 10 * kWgSlab) = u5;  \
    *reinterpret_cast<float4*>(uq + 12 * kWgSlab) = u6, *reinterpret_cast<float4*>(uq + 14 * kWgSlab) = u7; \
    const wg_f32x2 z2 = {0.0f, 0.0f};                                                                \
    const wg_f32x2 d00 = FRH_WG_Z(0, 0), d01 = FRH_WG_Z(0, 1), d02 = FRH_WG_Z(0, 2), d03 = FRH_WG_Z(0, 3); \
    const wg_f32x2 d10 = FRH_WG_Z(1, 0), d11 = FRH_WG_Z(1, 1), d12 = FRH_WG_Z(1, 2), d13 = FRH_WG_Z(1, 3); \
    const wg_f32x2 d20 = FRH_WG_Z(2, 0), d21 = FRH_WG_Z(2, 1), d22 = FRH_WG_Z(2, 2), d23 = FRH_WG_Z(2, 3); \
    const wg_f32x2 d30 = FRH_WG_Z(3, 0), d31 = FRH_WG_Z(3, 1), d32 = FRH_WG_Z(3, 2), d33 = FRH_WG_Z(3, 3); \
    float* vp = sp + v_off;                                                                          \
    FRH_WG_VROW(vp, d00 - d20, d01 - d21, d02 - d22, d03 - d23);                                     \
    FRH_WG_VROW(vp + 4 * kWgSlab, d10 + d20, d11 + d21, d12 + d22, d13 + d23);                       \
    FRH_WG_VROW(vp + 8 * kWgSlab, d20 - d10, d21 - d11, d22 - d12, d23 - d13);                       \
    FRH_WG_VROW(vp + 12 * kWgSlab, d10 - d30, d11 - d31, d12 - d32, d13 - d33);                      \
  } while (0)

#define FRH_WG_MFMA(ST, p)                                                          \
  do {                                                                              \
    const float* sp = lds + (ST) * kWgStage + (p) * kWgSlab;                        \
    const float4 av = *reinterpret_cast<const float4*>(sp + a_off);                 \
    const float4 bv = *reinterpret_cast<const float4*>(sp + b_off);                 \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[p], 0, 0, 0);     \
  } while (0)

  // One chunk: its 64 MFMAs from stage ST; the next chunk (in registers since the last step)
  // transformed into the other stage; the chunk after that loaded.  The other stage was last
  // read one chunk ago, which every wave left before that step's barrier.  The stage is a
  // literal so that the LDS reads and writes of a step are provably disjoint, and the
  // scheduling groups spread the staging work over the MFMAs' issue gaps: per position the
  // operand reads of the next one, then per MFMA two VALU and one memory instruction -- the U
  // copy's LDS writes and the selects that free the staging registers first, the 24 loads of
  // the chunk after next from the 17th MFMA on (most of a step ahead of their use), V's LDS
  // writes last.
#define FRH_WG_GROUPS(N, MEM, ID)                                                     \
  _Pragma("unroll") for (int p = 0; p < (N); ++p) {                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, ID);                             \
    _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                 \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, ID);                           \
      __builtin_amdgcn_sched_group_barrier(0x002, 2, ID);                           \
      __builtin_amdgcn_sched_group_barrier(MEM, 1, ID);                             \
    }                                                                               \
  }
#define FRH_WG_STEP(ST, STORE, LOAD, t)                                             \
  do {                                                                              \
    _Pragma("unroll") for (int p = 0; p < 16; ++p) FRH_WG_MFMA(ST, p);              \
    if (STORE) FRH_WG_STORE((ST) ^ 1);                                              \
    if (LOAD) FRH_WG_LOAD((t) + 2);                                                 \
    if (STORE) {                                                                    \
      __builtin_amdgcn_sched_group_barrier(0x100, 4, ST);                           \
      FRH_WG_GROUPS(4, 0x200, ST);                                                     \
      FRH_WG_GROUPS(6, 0x020, ST);                                                     \
      FRH_WG_GROUPS(6, 0x200, ST);                                                     \
    }                                                                               \
    if (STORE) {                                                                    \
      __syncthreads();                                                              \
      __builtin_amdgcn_sched_barrier(0);                                            \
    }                                                                               \
  } while (0)

  wg_f32x16 acc[16];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;

  const int steps = a.cin / kWgBK;
  FRH_WG_LOAD(0);
  FRH_WG_STORE(0);
  if (steps > 1) FRH_WG_LOAD(1);
  __syncthreads();
  int t = 0;
  for (; t + 3 < steps; t += 2) {
    FRH_WG_STEP(0, true, true, t);
    FRH_WG_STEP(1, true, true, t + 1);
  }
  // one to three chunks left, t even
  if (t + 3 == steps) {
    FRH_WG_STEP(0, true, true, t);
    FRH_WG_STEP(1, true, false, t + 1);
    FRH_WG_STEP(0, false, false, t + 2);
  } else if (t + 2 == steps) {
    FRH_WG_STEP(0, true, false, t);
    FRH_WG_STEP(1, false, false, t + 1);
  } else {
    FRH_WG_STEP(0, false, false, t);
  }
#undef FRH_WG_LX
#undef FRH_WG_LU
#undef FRH_WG_LOAD
#undef FRH_WG_Z
#undef FRH_WG_VROW
#undef FRH_WG_STORE
#undef FRH_WG_MFMA
#undef FRH_WG_GROUPS
#undef FRH_WG_STEP

  // epilogue: Y = A^T M A, + bias, ReLU.  Register r of a 32 x 32 tile is row (tile)
  // (r & 3) + 8 (r >> 2) + 4 h: tile row r >> 2 of the wave's four, tile column (r & 3) + 4 h.
  const int co = cb * kWgCout + wn * 32 + j;
  const bool has_bias = L.bias != nullptr;
  const float bias = has_bias ? L.bias[co] : 0.0f;
  float* yb = L.y + (int64_t)img * H * W * a.cout + co;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int oy = (by * kWgSide + wm * 4 + (r >> 2)) * 2;
    const int ox = (bx * kWgSide + (r & 3) + 4 * h) * 2;
    float s0[4], s1[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      s0[b] = (acc[b][r] + acc[4 + b][r]) + acc[8 + b][r];
      s1[b] = (acc[4 + b][r] - acc[8 + b][r]) - acc[12 + b][r];
    }
    float o[2][2];
    o[0][0] = (s0[0] + s0[1]) + s0[2];
    o[0][1] = (s0[1] - s0[2]) - s0[3];
    o[1][0] = (s1[0] + s1[1]) + s1[2];
    o[1][1] = (s1[1] - s1[2]) - s1[3];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float v = o[dy][dx];
        if (has_bias) v = v + bias;
        if (a.relu) v = fmaxf(v, 0.0f);
        if (oy + dy < H && ox + dx < W) yb[((int64_t)(oy + dy) * W + (ox + dx)) * a.cout] = v;
      }
  }
}

// One level of a launch, as the entries receive it.
struct Conv3x3LevelDesc {
  const float* x;
  const float* wt;  // the Conv2d weight [cout][3][3][cin]
  const float* bias;
  float* y;
  int32_t h, w;
  int64_t sn, sy, sx;
};

// Runs `levels` levels in one launch of the main kernel, after one launch that transforms each
// distinct weight (consecutive levels with the same w share one) into its slot of ws
// ([16 * cin * cout] floats each; ws_floats is what the caller provides).
inline int32_t conv3x3_launch(const char* what, int32_t levels, const Conv3x3LevelDesc* d, float* ws,
                              int64_t ws_floats, int64_t n, int32_t cin, int32_t cout, int32_t relu, void* stream) {
  FRH_REQUIRE(levels >= 1 && levels <= kWgMaxLevels, "1 to %d levels, got %d", kWgMaxLevels, levels);
  FRH_REQUIRE(n >= 0 && n < (1 << 20) && cin >= 1 && cout >= 1 && cout <= (1 << 20), "bad sizes");
  FRH_REQUIRE(cin % kWgBK == 0 && cout % kWgCout == 0, "cin %d must be a multiple of %d and cout %d of %d", cin,
              kWgBK, cout, kWgCout);
  FRH_REQUIRE(ws, "null pointer argument");
  FRH_REQUIRE((uintptr_t)ws % 16 == 0, "tensors must be 16-byte aligned");
  const int64_t slot = (int64_t)16 * cin * cout;
  Conv3x3Weights tab = {};
  int slots = 0;
  Conv3x3Args a;
  a.levels = 0, a.n = (int32_t)n, a.cin = cin, a.cout = cout, a.relu = relu;
  int64_t total = 0;
  for (int i = 0; i < levels; ++i) {
    const Conv3x3LevelDesc& s = d[i];
    FRH_REQUIRE(s.h >= 0 && s.w >= 0, "bad sizes");
    if (n == 0 || s.h == 0 || s.w == 0) continue;
    FRH_REQUIRE(s.x && s.y && s.wt, "null pointer argument");
    FRH_REQUIRE(((uintptr_t)s.x | (uintptr_t)s.y | (uintptr_t)s.bias | (uintptr_t)s.wt) % 16 == 0,
                "tensors must be 16-byte aligned");
    if (slots == 0 || tab.w[slots - 1] != s.wt) {
      FRH_REQUIRE((slots + 1) * slot <= ws_floats, "workspace holds %lld floats, %d weights need %lld",
                  (long long)ws_floats, slots + 1, (long long)((slots + 1) * slot));
      tab.w[slots] = s.wt, tab.u[slots] = ws + slots * slot;
      ++slots;
    }
    FRH_REQUIRE(s.sn >= 0 && s.sy >= 0 && s.sx >= cin && (s.sn | s.sy | s.sx) % 4 == 0,
                "x strides must be multiples of 4 elements and the column stride at least cin");
    const int64_t span = (int64_t)(s.h - 1) * s.sy + (int64_t)(s.w - 1) * s.sx + cin;
    FRH_REQUIRE(span < ((int64_t)1 << 30), "one image of x spans too many elements");
    const int64_t x_end = (n - 1) * s.sn + span, y_end = n * s.h * s.w * cout;
    FRH_REQUIRE(s.y + y_end <= s.x || s.x + x_end <= s.y, "y must not alias x");
    FRH_REQUIRE(s.y + y_end <= ws || ws + ws_floats <= s.y, "y must not alias the workspace");
    Conv3x3Level& L = a.lv[a.levels++];
    L.x = s.x, L.u = tab.u[slots - 1], L.bias = s.bias, L.y = s.y;
    L.sn = s.sn, L.sy = (int32_t)s.sy, L.sx = (int32_t)s.sx, L.h = s.h, L.w = s.w;
    L.by = (s.h + 2 * kWgSide - 1) / (2 * kWgSide), L.bx = (s.w + 2 * kWgSide - 1) / (2 * kWgSide);
    L.first = (int32_t)total;
    total += (int64_t)L.by * L.bx * n * (cout / kWgCout);
    FRH_REQUIRE(total < ((int64_t)1 << 30), "too many blocks");
  }
  if (a.levels == 0) return FRH_OK;
  a.total = (int32_t)total;
  a.chunk = (int32_t)((total + kWgXcds - 1) / kWgXcds);
  const int64_t wt = (int64_t)(cin / kWgBK) * cout * 2;
  hipLaunchKernelGGL(conv3x3_bias_act_weights_kernel, dim3((unsigned)((wt + 255) / 256), (unsigned)slots), dim3(256),
                     0, as_stream(stream), tab, cin, cout);
  hipLaunchKernelGGL(conv3x3_bias_act_wino_kernel, dim3((unsigned)(a.chunk * kWgXcds)), dim3(kWgThreads), 0,
                     as_stream(stream), a);
  return check_launch(what);
}

}  // namespace frh
