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
//   - every wave moves 8 KB of the U chunk, which the weights kernel wrote in the LDS image's
//     own order, straight into LDS with 8 LDS-DMA instructions (global_load_lds_dwordx4).
// Two LDS stages of each, one barrier per chunk.  While chunk t runs its MFMAs, U of chunk
// t + 1 is in flight into the other U stage, the patch of chunk t + 2 is in flight into one of
// two register sets, and the patch of chunk t + 1 (the other set, landed one step ago) is
// transformed and written; the patch loads of a step are issued in its first 8 MFMAs, the DMA
// in four pieces over the next 8, and all are waited for once, before its closing barrier.
// The prologue is step -1 and past the last chunk the
// prefetches repeat it, so every chunk count runs the same loop body and nothing is peeled.
// LDS images: V [16][64 tiles][8 k] and U [16][64 cout][8 k]; lane half h owns
// k = 4 h .. 4 h + 3 of the chunk (a fixed permutation of the k order), one ds_read_b128 per
// operand and position.  A row's two 16-byte halves swap places when bit 3 of the row index is
// set: each 16-lane group of a ds_read_b128 then reads 16 distinct 4-bank groups.
//
// Pixels outside the image are the zero padding: their loads go to a clamped address and are
// zeroed; stores past the image's edge are masked.  Workgroups are numbered level by level,
// cout block slowest inside a level, and dealt to the 8 XCDs in contiguous chunks, so an XCD
// works through one 1-MB slice of U at a time.  Fixed summation order, no atomics, no split
// over cin: the same inputs give the same bits on every launch.
//
// Pooled form (kPool, frh_conv3x3_bias_act_pool): tiles start at even coordinates, so the four
// outputs a lane forms per accumulator register are exactly one window of a 2 x 2 / stride-2
// max pool.  The epilogue forms them as the unpooled one does (same expressions, same order,
// then bias, then ReLU), keeps the largest and stores it at (oy / 2, ox / 2) of a
// [n, H / 2, W / 2, cout] output: a quarter of the stores, and no full-resolution map in
// memory.  An odd last row or column is a neighbour of the convolution and has no window, so
// the workgroup grid covers 2 (H / 2) x 2 (W / 2) outputs.  The main loop is the same text; the
// unpooled instantiation has no run-time trace of the pooled one.
#pragma once
#include "common.h"

namespace frh {

typedef float wg_f32x2 __attribute__((ext_vector_type(2)));

constexpr int kWgThreads = 256;
constexpr int kWgBK = 8;        // cin per chunk
constexpr int kWgSide = 8;      // tiles per workgroup side (16 outputs)
constexpr int kWgCout = 64;     // output channels per workgroup
constexpr int kWgXcds = 8;
constexpr int kWgMaxLevels = 8;
constexpr int kWgSlab = 64 * kWgBK;             // floats of one position of V (or U) per chunk
constexpr int kWgImage = 16 * kWgSlab;          // floats of one LDS stage of V (or U)

typedef uint32_t wg_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* wg_lds_ptr;

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
static __global__ void __launch_bounds__(256) conv3x3_bias_act_weights_kernel(const Conv3x3Weights tab, int cin, int cout) {
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

// A raw buffer descriptor over the memory from p on (p wave-uniform; both halves are read from
// the first lane so that the compiler keeps it in SGPRs): loads through it take a 32-bit lane
// offset and a scalar offset, no per-lane 64-bit address.  No range: every offset the kernel
// forms is inside the tensor.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_buffer(const void* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, -1, 0x00020000);
}

// p (wave-uniform) as an integer the compiler keeps in SGPRs
__device__ __forceinline__ uint64_t wg_uniform64(const void* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

template <bool kPool>
static __global__ void __launch_bounds__(kWgThreads) conv3x3_bias_act_wino_kernel(const Conv3x3Args a) {
  // 128 KB, one array: U stages 0, 1 (the LDS-DMA's targets), then V stages 0, 1
  __shared__ __attribute__((aligned(16))) float lds[4 * kWgImage];

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
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;

  // ---- staging roles
  // V: tile T = tid >> 2 (8 x 8, row-major), channels 2 c2, 2 c2 + 1 of the chunk: the whole
  // 4 x 4 patch as 16 float2, B^T d B on both channels, 16 ds_write_b64.
  const int T = tid >> 2, c2 = tid & 3;
  const int iy0 = (by * kWgSide + (T >> 3)) * 2 - 1;
  const int ix0 = (bx * kWgSide + (T & 7)) * 2 - 1;
  // the image as a buffer; the lane's part is a 32-bit byte offset, the chunk's a scalar one
  // (an image spans less than 2^32 bytes)
  const __amdgpu_buffer_rsrc_t xb = wg_buffer(L.x + (int64_t)img * L.sn);
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
  // U: the chunk's [16][64][8] image is 32 runs of 1 KB, in global memory (two per position,
  // positions cout * 32 bytes apart) as in LDS (contiguous); one LDS-DMA instruction moves a
  // run, lane l its 16 bytes at 16 l.  Wave w moves positions 4 w .. 4 w + 3.
  const int64_t u_pos = (int64_t)a.cout * kWgBK * 4;  // one position on, bytes
  const int64_t u_chunk = 16 * u_pos;                 // one chunk on
  const char* ub = reinterpret_cast<const char*>(L.u + (int64_t)cb * kWgCout * kWgBK) + wave * 4 * u_pos;
  const uint32_t u_lane = (uint32_t)lane * 16u;
  const uint32_t u_dst = (uint32_t)(uintptr_t)(wg_lds_ptr)lds + (uint32_t)wave * 4 * kWgSlab * 4;  // LDS bytes
  // MFMA operands: A = V rows (tiles wm * 32 + j), B = U rows (channels wn * 32 + j), k half h
  const int a_off = 2 * kWgImage + wg_slab_off(wm * 32 + j, h);
  const int b_off = wg_slab_off(wn * 32 + j, h);

  // two sets of patch registers (named: an indexed array of them ends up in LDS): chunk c
  // lives in set c & 1, loaded two steps before the step that multiplies it
  wg_f32x2 x000, x001, x002, x003, x010, x011, x012, x013, x020, x021, x022, x023, x030, x031, x032, x033;
  wg_f32x2 x100, x101, x102, x103, x110, x111, x112, x113, x120, x121, x122, x123, x130, x131, x132, x133;
  const wg_f32x2 z2 = {0.0f, 0.0f};
#define FRH_WG_LX(S, r, c) \
  x##S##r##c = __builtin_bit_cast(wg_f32x2, __builtin_amdgcn_raw_buffer_load_b64(xb, (int)xoff[r][c], xs_, 0))
#define FRH_WG_LOADX(S, t)                                                                       \
  do {                                                                                           \
    const int xs_ = (t) * (kWgBK * 4);                                                           \
    FRH_WG_LX(S, 0, 0), FRH_WG_LX(S, 0, 1), FRH_WG_LX(S, 0, 2), FRH_WG_LX(S, 0, 3);              \
    FRH_WG_LX(S, 1, 0), FRH_WG_LX(S, 1, 1), FRH_WG_LX(S, 1, 2), FRH_WG_LX(S, 1, 3);              \
    FRH_WG_LX(S, 2, 0), FRH_WG_LX(S, 2, 1), FRH_WG_LX(S, 2, 2), FRH_WG_LX(S, 2, 3);              \
    FRH_WG_LX(S, 3, 0), FRH_WG_LX(S, 3, 1), FRH_WG_LX(S, 3, 2), FRH_WG_LX(S, 3, 3);              \
  } while (0)

  // Position q (of the wave's four) of chunk t of U into U stage ST by LDS-DMA: one M0 value
  // (the LDS address of the position's run pair) and two instructions, no registers; four such
  // pieces move the wave's 8 KB.  In assembly, because the compiler makes every LDS read after
  // a DMA it knows of wait for that DMA.  One statement for all eight instructions put 8 x
  // 60-185 cycles of DMA issue into a single 64-cycle MFMA gap; a piece per gap is covered by
  // its MFMA.  What orders a piece is held by operands alone:
  //  - the token chains every piece behind the barrier that freed its stage (FRH_WG_SYNC of the
  //    step before, after which no wave reads stage ST's U again until the next barrier) and
  //    ahead of the step's own FRH_WG_SYNC, and the pieces among themselves;
  //  - the compiler does not count these loads, so FRH_WG_SYNC's vmcnt(0) retires them, every
  //    step and before the epilogue: no DMA is in flight when the workgroup ends and the next
  //    one on the CU gets its LDS;
  //  - `after` is a value of the column stage of B^T d B, which is made from the step's selects,
  //    and these carry every s_waitcnt vmcnt(N) the compiler emits in a step (it counts the
  //    patch loads of the step before, which FRH_WG_SYNC has retired already).  So every piece
  //    sits behind the step's last counted wait, none of them is tightened by a load it does
  //    not count, and the pieces land in the VALU-only gaps behind the 16 patch loads (emitted:
  //    MFMA gaps 10, 12, 14, 16 of the step);
  //  - M0 is the compiler's register, so each piece puts it back.
  // The s_nop 4 covers a VALU-written SGPR (readfirstlane) read by the DMA, the s_nop 0 the
  // M0 write ahead of it: the compiler's hazard pass does not look into the statement.
#define FRH_WG_DMA_PIECE(ST, t, q, after)                                                        \
  do {                                                                                           \
    const uint64_t g_ = wg_uniform64(ub + (int64_t)(t) * u_chunk) + (q) * u_pos;                 \
    const uint32_t l_ = u_dst + (ST) * kWgImage * 4 + (q) * kWgSlab * 4;                         \
    uint32_t m0_;                                                                                \
    asm("s_nop 4\n\t"                                                                            \
        "s_mov_b32 %0, m0\n\t"                                                                   \
        "s_mov_b32 m0, %3\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %4\n\tglobal_load_lds_dwordx4 %2, %4 offset:1024\n\t"       \
        "s_mov_b32 m0, %0"                                                                       \
        : "=&s"(m0_), "+v"(token)                                                                \
        : "v"(u_lane), "s"(l_), "s"(g_), "v"(after));                                            \
  } while (0)

  // B^T d B of patch set S into V stage ST: the selects and the columns (e = B^T d) as values
  // of the enclosing block, which the DMA pieces are ordered behind, then the rows, each V row
  // written as soon as it is complete
#define FRH_WG_Z(S, r, c) (xok[r][c] ? x##S##r##c : z2)
#define FRH_WG_VCOLS(S)                                                                                    \
  const wg_f32x2 d00 = FRH_WG_Z(S, 0, 0), d01 = FRH_WG_Z(S, 0, 1), d02 = FRH_WG_Z(S, 0, 2), d03 = FRH_WG_Z(S, 0, 3); \
  const wg_f32x2 d10 = FRH_WG_Z(S, 1, 0), d11 = FRH_WG_Z(S, 1, 1), d12 = FRH_WG_Z(S, 1, 2), d13 = FRH_WG_Z(S, 1, 3); \
  const wg_f32x2 d20 = FRH_WG_Z(S, 2, 0), d21 = FRH_WG_Z(S, 2, 1), d22 = FRH_WG_Z(S, 2, 2), d23 = FRH_WG_Z(S, 2, 3); \
  const wg_f32x2 d30 = FRH_WG_Z(S, 3, 0), d31 = FRH_WG_Z(S, 3, 1), d32 = FRH_WG_Z(S, 3, 2), d33 = FRH_WG_Z(S, 3, 3); \
  const wg_f32x2 e00 = d00 - d20, e01 = d01 - d21, e02 = d02 - d22, e03 = d03 - d23;                       \
  const wg_f32x2 e10 = d10 + d20, e11 = d11 + d21, e12 = d12 + d22, e13 = d13 + d23;                       \
  const wg_f32x2 e20 = d20 - d10, e21 = d21 - d11, e22 = d22 - d12, e23 = d23 - d13;                       \
  const wg_f32x2 e30 = d10 - d30, e31 = d11 - d31, e32 = d12 - d32, e33 = d13 - d33
#define FRH_WG_VROW(vp, e0, e1, e2, e3)                                   \
  do {                                                                    \
    *reinterpret_cast<wg_f32x2*>(vp) = (e0) - (e2);                       \
    *reinterpret_cast<wg_f32x2*>((vp) + kWgSlab) = (e1) + (e2);           \
    *reinterpret_cast<wg_f32x2*>((vp) + 2 * kWgSlab) = (e2) - (e1);       \
    *reinterpret_cast<wg_f32x2*>((vp) + 3 * kWgSlab) = (e1) - (e3);       \
  } while (0)
#define FRH_WG_VROWS(ST)                                                  \
  do {                                                                    \
    float* vp = lds + (2 + (ST)) * kWgImage + v_off;                      \
    FRH_WG_VROW(vp, e00, e01, e02, e03);                                  \
    FRH_WG_VROW(vp + 4 * kWgSlab, e10, e11, e12, e13);                    \
    FRH_WG_VROW(vp + 8 * kWgSlab, e20, e21, e22, e23);                    \
    FRH_WG_VROW(vp + 12 * kWgSlab, e30, e31, e32, e33);                   \
  } while (0)

#define FRH_WG_MFMA(ST, p)                                                          \
  do {                                                                              \
    const float* sp = lds + (ST) * kWgImage + (p) * kWgSlab;                        \
    const float4 av = *reinterpret_cast<const float4*>(sp + a_off);                 \
    const float4 bv = *reinterpret_cast<const float4*>(sp + b_off);                 \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[p], 0, 0, 0);     \
  } while (0)

  // the step's DMA and patch loads landed, its LDS writes done, then the barrier
#define FRH_WG_SYNC()                                                                        \
  do {                                                                                       \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" : "+v"(token) : : "memory");    \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)

  // One step: chunk t's 64 MFMAs from stage ST.  Beside them U of chunk t + 1 goes by DMA into
  // the other U stage, the patch of chunk t + 2 is loaded into set ST, and the patch of chunk
  // t + 1 (set ST ^ 1, loaded one step ago) is transformed into the other V stage.  That stage
  // was last read one step ago, which every wave left before that step's barrier.  Past the
  // last chunk the prefetches repeat the last chunk (valid addresses, nobody reads the result),
  // so every step is this one body.  The stage is a literal so that the LDS reads and writes
  // of a step are provably disjoint, and the scheduling groups spread the staging work over
  // the MFMAs' issue gaps: per position the operand reads of the next one; in the first 8
  // MFMAs four VALU (the selects that read the landed set) and two patch loads each; then the
  // adds, four per MFMA as emitted, with one DMA piece in every second gap; V's LDS writes last.
#define FRH_WG_GROUPS(N, VALU, MEM, K, ID)                                          \
  _Pragma("unroll") for (int p = 0; p < (N); ++p) {                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, ID);                             \
    _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                 \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, ID);                           \
      __builtin_amdgcn_sched_group_barrier(0x002, VALU, ID);                        \
      __builtin_amdgcn_sched_group_barrier(MEM, K, ID);                             \
    }                                                                               \
  }
#define FRH_WG_STEP(ST, OT, t)                                                        \
  do {                                                                              \
    _Pragma("unroll") for (int p = 0; p < 16; ++p) FRH_WG_MFMA(ST, p);              \
    FRH_WG_LOADX(ST, min((t) + 2, last));                                           \
    FRH_WG_VCOLS(OT);                                                               \
    FRH_WG_DMA_PIECE(OT, min((t) + 1, last), 0, e03.y);                             \
    FRH_WG_DMA_PIECE(OT, min((t) + 1, last), 1, e13.y);                             \
    FRH_WG_DMA_PIECE(OT, min((t) + 1, last), 2, e23.y);                             \
    FRH_WG_DMA_PIECE(OT, min((t) + 1, last), 3, e33.y);                             \
    FRH_WG_VROWS(OT);                                                               \
    __builtin_amdgcn_sched_group_barrier(0x100, 4, ST);                             \
    FRH_WG_GROUPS(2, 4, 0x020, 2, ST);                                              \
    FRH_WG_GROUPS(14, 2, 0x200, 1, ST);                                             \
    FRH_WG_SYNC();                                                                  \
  } while (0)

  f32x16 acc[16];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;

  const int last = a.cin / kWgBK - 1;
  uint32_t token = 0;
  FRH_WG_DMA_PIECE(0, 0, 0, 0.0f);
  FRH_WG_DMA_PIECE(0, 0, 1, 0.0f);
  FRH_WG_DMA_PIECE(0, 0, 2, 0.0f);
  FRH_WG_DMA_PIECE(0, 0, 3, 0.0f);
  FRH_WG_LOADX(0, 0);
  FRH_WG_LOADX(1, min(1, last));
  {
    FRH_WG_VCOLS(0);
    FRH_WG_VROWS(0);
  }
  FRH_WG_SYNC();
  for (int t = 0;; t += 2) {
    FRH_WG_STEP(0, 1, t);
    if (t >= last) break;
    FRH_WG_STEP(1, 0, t + 1);
    if (t + 1 >= last) break;
  }
#undef FRH_WG_LX
#undef FRH_WG_LOADX
#undef FRH_WG_DMA_PIECE
#undef FRH_WG_Z
#undef FRH_WG_VCOLS
#undef FRH_WG_VROW
#undef FRH_WG_VROWS
#undef FRH_WG_MFMA
#undef FRH_WG_SYNC
#undef FRH_WG_GROUPS
#undef FRH_WG_STEP

  // epilogue: Y = A^T M A, + bias, ReLU.  Register r of a 32 x 32 tile is row (tile)
  // mfma32_row(r) + 4 h: tile row r >> 2 of the wave's four, tile column (r & 3) + 4 h.
  const int co = cb * kWgCout + wn * 32 + j;
  const bool has_bias = L.bias != nullptr;
  const float bias = has_bias ? L.bias[co] : 0.0f;
  // The one wait for the bias, in the block that dominates every store.  Without it the
  // compiler waits inside each conditional bias add, and past the join behind it the load
  // counts as pending again: s_waitcnt vmcnt(0) before all 64 stores, which also retires the
  // store before (stores count in vmcnt), so the stores went out one round trip at a time.
  asm volatile("" : : "v"(bias));
  const int PH = H >> 1, PW = W >> 1;  // the pooled extent (kPool)
  float* yb = kPool ? L.y + (int64_t)img * PH * PW * a.cout + co : L.y + (int64_t)img * H * W * a.cout + co;
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
    if constexpr (kPool) {
      // the window in row-major order, a later value replacing the kept one only when it is
      // larger: max_pool2d's own rule, so a tie of -0 and +0 resolves as it does there
      float m = 0.0f;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          float v = o[dy][dx];
          if (has_bias) v = v + bias;
          if (a.relu) v = fmaxf(v, 0.0f);
          m = (dy | dx) == 0 || v > m ? v : m;
        }
      const int py = oy >> 1, px = ox >> 1;
      if (py < PH && px < PW) yb[((int64_t)py * PW + px) * a.cout] = m;
    } else {
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
// ([16 * cin * cout] floats each; ws_floats is what the caller provides).  main_launch(grid, a)
// launches the main kernel: the product's below, a laboratory build of it in the tools library.
// kPool: the pooled form, y [n, h / 2, w / 2, cout]; a level with no whole window is skipped like
// an empty one.
template <bool kPool = false, class MainLaunch>
inline int32_t conv3x3_launch_with(const char* what, int32_t levels, const Conv3x3LevelDesc* d, float* ws,
                                   int64_t ws_floats, int64_t n, int32_t cin, int32_t cout, int32_t relu,
                                   void* stream, MainLaunch&& main_launch) {
  FRH_REQUIRE(levels >= 1 && levels <= kWgMaxLevels, "1 to %d levels, got %d", kWgMaxLevels, levels);
  FRH_REQUIRE(n >= 0 && n < (1 << 20) && cin >= 1 && cout >= 1 && cout <= (1 << 20), "bad sizes");
  FRH_REQUIRE(cin % kWgBK == 0 && cout % kWgCout == 0, "cin %d must be a multiple of %d and cout %d of %d", cin,
              kWgBK, cout, kWgCout);
  FRH_REQUIRE(ws, "null pointer argument");
  FRH_REQUIRE_ALIGNED16(ws);
  const int64_t slot = (int64_t)16 * cin * cout;
  Conv3x3Weights tab = {};
  int slots = 0;
  Conv3x3Args a;
  a.levels = 0, a.n = (int32_t)n, a.cin = cin, a.cout = cout, a.relu = relu;
  int64_t total = 0;
  for (int i = 0; i < levels; ++i) {
    const Conv3x3LevelDesc& s = d[i];
    FRH_REQUIRE(s.h >= 0 && s.w >= 0, "bad sizes");
    // the extent the workgroups cover and y's: the map, or its whole 2 x 2 windows
    const int32_t eh = kPool ? s.h / 2 * 2 : s.h, ew = kPool ? s.w / 2 * 2 : s.w;
    const int32_t yh = kPool ? s.h / 2 : s.h, yw = kPool ? s.w / 2 : s.w;
    if (n == 0 || eh == 0 || ew == 0) continue;
    FRH_REQUIRE(s.x && s.y && s.wt, "null pointer argument");
    FRH_REQUIRE_ALIGNED16(s.x, s.y, s.bias, s.wt);
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
    const int64_t x_end = (n - 1) * s.sn + span, y_end = n * yh * yw * cout;
    FRH_REQUIRE(!ranges_overlap(s.y, y_end * 4, s.x, x_end * 4), "y must not alias x");
    FRH_REQUIRE(!ranges_overlap(s.y, y_end * 4, ws, ws_floats * 4), "y must not alias the workspace");
    Conv3x3Level& L = a.lv[a.levels++];
    L.x = s.x, L.u = tab.u[slots - 1], L.bias = s.bias, L.y = s.y;
    L.sn = s.sn, L.sy = (int32_t)s.sy, L.sx = (int32_t)s.sx, L.h = s.h, L.w = s.w;
    L.by = (eh + 2 * kWgSide - 1) / (2 * kWgSide), L.bx = (ew + 2 * kWgSide - 1) / (2 * kWgSide);
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
  main_launch(dim3((unsigned)(a.chunk * kWgXcds)), a);
  return check_launch(what);
}

template <bool kPool = false>
inline int32_t conv3x3_launch(const char* what, int32_t levels, const Conv3x3LevelDesc* d, float* ws,
                              int64_t ws_floats, int64_t n, int32_t cin, int32_t cout, int32_t relu, void* stream) {
  return conv3x3_launch_with<kPool>(what, levels, d, ws, ws_floats, n, cin, cout, relu, stream,
                                    [&](dim3 grid, const Conv3x3Args& a) {
                                      hipLaunchKernelGGL(conv3x3_bias_act_wino_kernel<kPool>, grid, dim3(kWgThreads),
                                                         0, as_stream(stream), a);
                                    });
}

}  // namespace frh
