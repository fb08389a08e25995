// TOOLS-ONLY: laboratory builds of conv3x3_bias_act_wino_kernel (conv3x3_wino_kernels.h) for
// tools/bench_conv3x3_variants.py and tools/clock_conv3x3.py.  One kernel template holds the
// candidate forms of the chunk step; the product header holds only the form that was adopted
// (kDma 1, kNP 16, kIl 0, kEp 2; measurements: DESIGN section 4, Tried).
//   kIl   1: the MFMAs of two positions alternate (kNP 16 only)
//   kEp   where the lane's bias is loaded and waited for: 0 behind the main loop, waited for in
//         every conditional bias add; 1 before the main loop; 2 behind it with one wait
//   kDma  how the step's 8 LDS-DMA instructions of the U chunk are issued
//         0  one asm statement behind the step's last select (the form before the split)
//         1  four pieces of one M0 value and two DMAs, each behind one row of the column stage of
//            B^T d B: the VALU-only gaps after the patch loads
//         2  four pieces, each behind one row of the selects: gaps that also hold patch loads
//         3  eight pieces of one DMA, two behind each row of the column stage
//   kNP   positions whose MFMAs run before the step's barrier
//         16 the barrier closes the step (the form before the register tail)
//         12 .. 15  the operands of positions kNP .. 15 are read into registers before the
//            barrier, the next step's position-0 operands behind it, and the tail's MFMAs cover
//            the barrier's skew and that read's latency.  The compiler puts the barrier behind
//            the last operand read: emitted at MFMA 44, 48, 52, 52 for kNP 12, 13, 14, 15, the
//            next step's first read at MFMA 4 kNP
// A non-null `stamps` makes thread 0 of every workgroup store s_memtime and s_memrealtime at
// kernel entry, around the main loop and after the epilogue: 8 uint64 per logical workgroup.
#include "conv3x3_wino_kernels.h"
#include "frcnn_tools.h"

using namespace frh;

namespace {

template <int kDma, int kNP, int kIl, int kEp>
__global__ void __launch_bounds__(kWgThreads) wino_lab_kernel(const Conv3x3Args a, unsigned long long* stamps) {
  __shared__ __attribute__((aligned(16))) float lds[4 * kWgImage];

  const int wg = (int)(blockIdx.x % kWgXcds) * a.chunk + (int)(blockIdx.x / kWgXcds);
  if (wg >= a.total) return;
  const bool stamp = stamps != nullptr && threadIdx.x == 0;
#define LAB_STAMP(i)                                                  \
  do {                                                                \
    if (stamp) {                                                      \
      stamps[(int64_t)wg * 8 + 2 * (i)] = __builtin_amdgcn_s_memtime();         \
      stamps[(int64_t)wg * 8 + 2 * (i) + 1] = __builtin_amdgcn_s_memrealtime(); \
    }                                                                 \
  } while (0)
  LAB_STAMP(0);
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
  // with the tail the wave index has a known range: the compiler can then prove V's writes
  // disjoint from the operand reads of the other stage and place them in mid-step
  const int lane = tid & 63;
  const int wave = kNP == 16 ? __builtin_amdgcn_readfirstlane(tid >> 6) : (__builtin_amdgcn_readfirstlane(tid >> 6) & 3);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;

  const int T = tid >> 2, c2 = tid & 3;
  const int iy0 = (by * kWgSide + (T >> 3)) * 2 - 1;
  const int ix0 = (bx * kWgSide + (T & 7)) * 2 - 1;
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
      xoff[r][c] = (uint32_t)(cy * L.sy + cx * L.sx + c2 * 2) * 4u;
    }
  const int v_off = wg_slab_off(T, c2 >> 1) + (c2 & 1) * 2;
  const int64_t u_pos = (int64_t)a.cout * kWgBK * 4;
  const int64_t u_chunk = 16 * u_pos;
  const char* ub = reinterpret_cast<const char*>(L.u + (int64_t)cb * kWgCout * kWgBK) + wave * 4 * u_pos;
  const uint32_t u_lane = (uint32_t)lane * 16u;
  const uint32_t u_dst = (uint32_t)(uintptr_t)(wg_lds_ptr)lds + (uint32_t)wave * 4 * kWgSlab * 4;
  const int a_off = 2 * kWgImage + wg_slab_off(wm * 32 + j, h);
  const int b_off = wg_slab_off(wn * 32 + j, h);

  wg_f32x2 x000, x001, x002, x003, x010, x011, x012, x013, x020, x021, x022, x023, x030, x031, x032, x033;
  wg_f32x2 x100, x101, x102, x103, x110, x111, x112, x113, x120, x121, x122, x123, x130, x131, x132, x133;
  const wg_f32x2 z2 = {0.0f, 0.0f};
#define LAB_LX(S, r, c) \
  x##S##r##c = __builtin_bit_cast(wg_f32x2, __builtin_amdgcn_raw_buffer_load_b64(xb, (int)xoff[r][c], xs_, 0))
#define LAB_LOADX(S, t)                                                      \
  do {                                                                       \
    const int xs_ = (t) * (kWgBK * 4);                                       \
    LAB_LX(S, 0, 0), LAB_LX(S, 0, 1), LAB_LX(S, 0, 2), LAB_LX(S, 0, 3);      \
    LAB_LX(S, 1, 0), LAB_LX(S, 1, 1), LAB_LX(S, 1, 2), LAB_LX(S, 1, 3);      \
    LAB_LX(S, 2, 0), LAB_LX(S, 2, 1), LAB_LX(S, 2, 2), LAB_LX(S, 2, 3);      \
    LAB_LX(S, 3, 0), LAB_LX(S, 3, 1), LAB_LX(S, 3, 2), LAB_LX(S, 3, 3);      \
  } while (0)

  // the whole chunk in one statement (kDma 0)
#define LAB_DMA(ST, t, after)                                                                    \
  do {                                                                                           \
    const uint64_t g_ = wg_uniform64(ub + (int64_t)(t) * u_chunk);                               \
    const uint32_t l_ = u_dst + (ST) * kWgImage * 4;                                             \
    uint32_t m0_;                                                                                \
    asm("s_nop 4\n\t"                                                                            \
        "s_mov_b32 %0, m0\n\t"                                                                   \
        "s_mov_b32 m0, %3\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %7\n\tglobal_load_lds_dwordx4 %2, %7 offset:1024\n\t"       \
        "s_mov_b32 m0, %4\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %8\n\tglobal_load_lds_dwordx4 %2, %8 offset:1024\n\t"       \
        "s_mov_b32 m0, %5\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %9\n\tglobal_load_lds_dwordx4 %2, %9 offset:1024\n\t"       \
        "s_mov_b32 m0, %6\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %10\n\tglobal_load_lds_dwordx4 %2, %10 offset:1024\n\t"     \
        "s_mov_b32 m0, %0"                                                                       \
        : "=&s"(m0_), "+v"(token)                                                                \
        : "v"(u_lane), "s"(l_), "s"(l_ + kWgSlab * 4), "s"(l_ + 2 * kWgSlab * 4),                \
          "s"(l_ + 3 * kWgSlab * 4), "s"(g_), "s"(g_ + u_pos), "s"(g_ + 2 * u_pos),              \
          "s"(g_ + 3 * u_pos), "v"(after));                                                      \
  } while (0)
  // position q of the wave's four (one M0 value, two DMAs) and one 1-KB run of it
#define LAB_PIECE2(ST, t, q, after)                                                              \
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
#define LAB_PIECE1(ST, t, q, half, after)                                                        \
  do {                                                                                           \
    const uint64_t g_ = wg_uniform64(ub + (int64_t)(t) * u_chunk) + (q) * u_pos + (half) * 1024; \
    const uint32_t l_ = u_dst + (ST) * kWgImage * 4 + (q) * kWgSlab * 4 + (half) * 1024;         \
    uint32_t m0_;                                                                                \
    asm("s_nop 4\n\t"                                                                            \
        "s_mov_b32 %0, m0\n\t"                                                                   \
        "s_mov_b32 m0, %3\n\ts_nop 0\n\t"                                                        \
        "global_load_lds_dwordx4 %2, %4\n\t"                                                     \
        "s_mov_b32 m0, %0"                                                                       \
        : "=&s"(m0_), "+v"(token)                                                                \
        : "v"(u_lane), "s"(l_), "s"(g_), "v"(after));                                            \
  } while (0)

#define LAB_Z(S, r, c) (xok[r][c] ? x##S##r##c : z2)
#define LAB_VROW(vp, e0, e1, e2, e3)                                      \
  do {                                                                    \
    *reinterpret_cast<wg_f32x2*>(vp) = (e0) - (e2);                       \
    *reinterpret_cast<wg_f32x2*>((vp) + kWgSlab) = (e1) + (e2);           \
    *reinterpret_cast<wg_f32x2*>((vp) + 2 * kWgSlab) = (e2) - (e1);       \
    *reinterpret_cast<wg_f32x2*>((vp) + 3 * kWgSlab) = (e1) - (e3);       \
  } while (0)
  // the selects, the column stage e = B^T d (same operations as the product's), the DMA pieces
  // of chunk `tn` into U stage ST behind them, then the row stage into V stage ST
#define LAB_VSTORE_DMA(ST, S, tn, split)                                                                   \
  do {                                                                                                     \
    const wg_f32x2 d00 = LAB_Z(S, 0, 0), d01 = LAB_Z(S, 0, 1), d02 = LAB_Z(S, 0, 2), d03 = LAB_Z(S, 0, 3); \
    const wg_f32x2 d10 = LAB_Z(S, 1, 0), d11 = LAB_Z(S, 1, 1), d12 = LAB_Z(S, 1, 2), d13 = LAB_Z(S, 1, 3); \
    const wg_f32x2 d20 = LAB_Z(S, 2, 0), d21 = LAB_Z(S, 2, 1), d22 = LAB_Z(S, 2, 2), d23 = LAB_Z(S, 2, 3); \
    const wg_f32x2 d30 = LAB_Z(S, 3, 0), d31 = LAB_Z(S, 3, 1), d32 = LAB_Z(S, 3, 2), d33 = LAB_Z(S, 3, 3); \
    const wg_f32x2 e00 = d00 - d20, e01 = d01 - d21, e02 = d02 - d22, e03 = d03 - d23;                     \
    const wg_f32x2 e10 = d10 + d20, e11 = d11 + d21, e12 = d12 + d22, e13 = d13 + d23;                     \
    const wg_f32x2 e20 = d20 - d10, e21 = d21 - d11, e22 = d22 - d12, e23 = d23 - d13;                     \
    const wg_f32x2 e30 = d10 - d30, e31 = d11 - d31, e32 = d12 - d32, e33 = d13 - d33;                     \
    if (split) {                                                                                           \
      if constexpr (kDma == 0) {                                                                           \
        LAB_DMA(ST, tn, d33.y);                                                                            \
      } else if constexpr (kDma == 1) {                                                                    \
        LAB_PIECE2(ST, tn, 0, e03.y);                                                                      \
        LAB_PIECE2(ST, tn, 1, e13.y);                                                                      \
        LAB_PIECE2(ST, tn, 2, e23.y);                                                                      \
        LAB_PIECE2(ST, tn, 3, e33.y);                                                                      \
      } else if constexpr (kDma == 2) {                                                                    \
        LAB_PIECE2(ST, tn, 0, d03.y);                                                                      \
        LAB_PIECE2(ST, tn, 1, d13.y);                                                                      \
        LAB_PIECE2(ST, tn, 2, d23.y);                                                                      \
        LAB_PIECE2(ST, tn, 3, d33.y);                                                                      \
      } else {                                                                                             \
        LAB_PIECE1(ST, tn, 0, 0, e01.y);                                                                   \
        LAB_PIECE1(ST, tn, 0, 1, e03.y);                                                                   \
        LAB_PIECE1(ST, tn, 1, 0, e11.y);                                                                   \
        LAB_PIECE1(ST, tn, 1, 1, e13.y);                                                                   \
        LAB_PIECE1(ST, tn, 2, 0, e21.y);                                                                   \
        LAB_PIECE1(ST, tn, 2, 1, e23.y);                                                                   \
        LAB_PIECE1(ST, tn, 3, 0, e31.y);                                                                   \
        LAB_PIECE1(ST, tn, 3, 1, e33.y);                                                                   \
      }                                                                                                    \
    }                                                                                                      \
    float* vp = lds + (2 + (ST)) * kWgImage + v_off;                                                       \
    LAB_VROW(vp, e00, e01, e02, e03);                                                                      \
    LAB_VROW(vp + 4 * kWgSlab, e10, e11, e12, e13);                                                        \
    LAB_VROW(vp + 8 * kWgSlab, e20, e21, e22, e23);                                                        \
    LAB_VROW(vp + 12 * kWgSlab, e30, e31, e32, e33);                                                       \
  } while (0)

  // operands of position p from stage ST; its four MFMAs
#define LAB_READ(ST, p)                                                                               \
  do {                                                                                                \
    av[p] = *reinterpret_cast<const float4*>(lds + (ST) * kWgImage + (p) * kWgSlab + a_off);          \
    bv[p] = *reinterpret_cast<const float4*>(lds + (ST) * kWgImage + (p) * kWgSlab + b_off);          \
  } while (0)
#define LAB_MM(p)                                                                         \
  do {                                                                                    \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].x, bv[p].x, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].y, bv[p].y, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].z, bv[p].z, acc[p], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].w, bv[p].w, acc[p], 0, 0, 0);     \
  } while (0)

#define LAB_SYNC()                                                                           \
  do {                                                                                       \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" : "+v"(token) : : "memory");    \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)

  // the step as it was before the register tail (kNP 16)
#define LAB_GROUPS(N, VALU, MEM, K, ID)                                             \
  _Pragma("unroll") for (int p = 0; p < (N); ++p) {                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, ID);                             \
    _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                 \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, ID);                           \
      __builtin_amdgcn_sched_group_barrier(0x002, VALU, ID);                        \
      __builtin_amdgcn_sched_group_barrier(MEM, K, ID);                             \
    }                                                                               \
  }
#define LAB_STEP16(ST, OT, t)                                                       \
  do {                                                                              \
    _Pragma("unroll") for (int p = 0; p < 16; ++p) {                                \
      LAB_READ(ST, p);                                                              \
      LAB_MM(p);                                                                    \
    }                                                                               \
    LAB_LOADX(ST, min((t) + 2, last));                                              \
    LAB_VSTORE_DMA(OT, OT, min((t) + 1, last), true);                               \
    __builtin_amdgcn_sched_group_barrier(0x100, 4, ST);                             \
    LAB_GROUPS(2, 4, 0x020, 2, ST);                                                 \
    LAB_GROUPS(14, 2, 0x200, 1, ST);                                                \
    LAB_SYNC();                                                                     \
  } while (0)
  // the step with the register tail.  Before the barrier: the MFMAs of positions 0 .. kNP - 1
  // (position 0's operands were read behind the barrier before), the operand reads of every
  // other position of this stage, the staging (MFMAs 1-8 four selects and two patch loads
  // each, 9-24 four adds each, 25-32 one V write each).  Behind it: position 0 of the next
  // stage is read, then the tail's MFMAs.
#define LAB_STEPT(ST, OT, t)                                                        \
  do {                                                                              \
    _Pragma("unroll") for (int p = 1; p < 16; ++p) LAB_READ(ST, p);                 \
    _Pragma("unroll") for (int p = 0; p < kNP; ++p) LAB_MM(p);                      \
    LAB_LOADX(ST, min((t) + 2, last));                                              \
    LAB_VSTORE_DMA(OT, OT, min((t) + 1, last), true);                               \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, ST);                             \
    _Pragma("unroll") for (int p = 0; p < kNP; ++p) {                               \
      if (p + 2 <= 15) __builtin_amdgcn_sched_group_barrier(0x100, 2, ST);          \
      if (kNP < 14 && p >= 2 * kNP - 14) __builtin_amdgcn_sched_group_barrier(0x100, 2, ST); \
      _Pragma("unroll") for (int m = 0; m < 4; ++m) {                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, ST);                         \
        if (4 * p + m < 8) {                                                        \
          __builtin_amdgcn_sched_group_barrier(0x002, 4, ST);                       \
          __builtin_amdgcn_sched_group_barrier(0x020, 2, ST);                       \
        } else if (4 * p + m < 24) {                                                \
          __builtin_amdgcn_sched_group_barrier(0x002, 4, ST);                       \
        } else if (4 * p + m < 32) {                                                \
          __builtin_amdgcn_sched_group_barrier(0x200, 1, ST);                       \
        }                                                                           \
      }                                                                             \
    }                                                                               \
    LAB_SYNC();                                                                     \
    LAB_READ(OT, 0);                                                                \
    _Pragma("unroll") for (int p = kNP; p < 16; ++p) LAB_MM(p);                     \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 2 + ST);                         \
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * (16 - kNP), 2 + ST);            \
    __builtin_amdgcn_sched_barrier(0);                                              \
  } while (0)
  // kIl: the MFMAs of two positions alternate (x0 x1 y0 y1 ...: no accumulator's own order
  // changes), so that no MFMA follows the one whose result it accumulates onto
#define LAB_MM2(p, q)                                                                     \
  do {                                                                                    \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].x, bv[p].x, acc[p], 0, 0, 0);     \
    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].x, bv[q].x, acc[q], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].y, bv[p].y, acc[p], 0, 0, 0);     \
    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].y, bv[q].y, acc[q], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].z, bv[p].z, acc[p], 0, 0, 0);     \
    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].z, bv[q].z, acc[q], 0, 0, 0);     \
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p].w, bv[p].w, acc[p], 0, 0, 0);     \
    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].w, bv[q].w, acc[q], 0, 0, 0);     \
  } while (0)
#define LAB_STEP16I(ST, OT, t)                                                      \
  do {                                                                              \
    _Pragma("unroll") for (int p = 0; p < 16; p += 2) {                             \
      LAB_READ(ST, p);                                                              \
      LAB_READ(ST, p + 1);                                                          \
      LAB_MM2(p, p + 1);                                                            \
    }                                                                               \
    LAB_LOADX(ST, min((t) + 2, last));                                              \
    LAB_VSTORE_DMA(OT, OT, min((t) + 1, last), true);                               \
    __builtin_amdgcn_sched_group_barrier(0x100, 4, ST);                             \
    _Pragma("unroll") for (int pr = 0; pr < 8; ++pr) {                              \
      __builtin_amdgcn_sched_group_barrier(0x100, 4, ST);                           \
      _Pragma("unroll") for (int m = 0; m < 8; ++m) {                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, ST);                         \
        if (8 * pr + m < 8) {                                                       \
          __builtin_amdgcn_sched_group_barrier(0x002, 4, ST);                       \
          __builtin_amdgcn_sched_group_barrier(0x020, 2, ST);                       \
        } else {                                                                    \
          __builtin_amdgcn_sched_group_barrier(0x002, 2, ST);                       \
          __builtin_amdgcn_sched_group_barrier(0x200, 1, ST);                       \
        }                                                                           \
      }                                                                             \
    }                                                                               \
    LAB_SYNC();                                                                     \
  } while (0)
#define LAB_STEP(ST, OT, t)                  \
  do {                                       \
    if constexpr (kNP == 16 && kIl == 1) {   \
      LAB_STEP16I(ST, OT, t);                \
    } else if constexpr (kNP == 16) {        \
      LAB_STEP16(ST, OT, t);                 \
    } else {                                 \
      LAB_STEPT(ST, OT, t);                  \
    }                                        \
  } while (0)

  f32x16 acc[16];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;
  float4 av[16], bv[16];

  // kEp: where the lane's bias is loaded.  0 behind the main loop, as it was: the compiler
  // then waits vmcnt(0) before the bias add of every one of the 64 conditional stores, each
  // store behind the one before; 1 before the main loop (a register for its whole length);
  // 2 behind the loop with one wait before the first store
  const int co = cb * kWgCout + wn * 32 + j;
  const bool has_bias = L.bias != nullptr;
  float bias = 0.0f;
  if constexpr (kEp == 1) bias = has_bias ? L.bias[co] : 0.0f;
  const int last = a.cin / kWgBK - 1;
  uint32_t token = 0;
  if constexpr (kDma == 1) {  // as the product
    LAB_PIECE2(0, 0, 0, 0.0f);
    LAB_PIECE2(0, 0, 1, 0.0f);
    LAB_PIECE2(0, 0, 2, 0.0f);
    LAB_PIECE2(0, 0, 3, 0.0f);
  } else {
    LAB_DMA(0, 0, 0.0f);
  }
  LAB_LOADX(0, 0);
  LAB_LOADX(1, min(1, last));
  LAB_VSTORE_DMA(0, 0, 0, false);
  LAB_SYNC();
  if constexpr (kNP < 16) LAB_READ(0, 0);
  LAB_STAMP(1);
  for (int t = 0;; t += 2) {
    LAB_STEP(0, 1, t);
    if (t >= last) break;
    LAB_STEP(1, 0, t + 1);
    if (t + 1 >= last) break;
  }
  LAB_STAMP(2);

  if constexpr (kEp != 1) bias = has_bias ? L.bias[co] : 0.0f;
  // kEp 2: the one wait for the bias here, in the block that dominates every store
  if constexpr (kEp == 2) asm volatile("" : : "v"(bias));
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
  LAB_STAMP(3);
}

template <int kDma, int kNP, int kIl = 0, int kEp = 0>
void lab_launch(dim3 grid, const Conv3x3Args& a, unsigned long long* stamps, void* stream) {
  hipLaunchKernelGGL((wino_lab_kernel<kDma, kNP, kIl, kEp>), grid, dim3(kWgThreads), 0, as_stream(stream), a, stamps);
}

}  // namespace

extern "C" int32_t frh_conv3x3_bias_act_levels_variant(int32_t variant, uint64_t* stamps, int32_t num_levels,
                                                       const void* const* xs, const void* const* weights,
                                                       const void* const* biases, void* const* ys, float* workspace,
                                                       size_t workspace_bytes, int64_t n, int32_t cin, int32_t cout,
                                                       const int32_t* level_hw, const int64_t* level_strides,
                                                       int32_t relu, void* stream) {
  const char* what = "frh_conv3x3_bias_act_levels_variant";
  FRH_REQUIRE(num_levels >= 1 && num_levels <= kWgMaxLevels, "1 to %d levels, got %d", kWgMaxLevels, num_levels);
  FRH_REQUIRE(xs && weights && biases && ys && level_hw && level_strides, "null pointer argument");
  Conv3x3LevelDesc d[kWgMaxLevels];
  for (int i = 0; i < num_levels; ++i)
    d[i] = {static_cast<const float*>(xs[i]),
            static_cast<const float*>(weights[i]),
            static_cast<const float*>(biases[i]),
            static_cast<float*>(ys[i]),
            level_hw[2 * i],
            level_hw[2 * i + 1],
            level_strides[3 * i],
            level_strides[3 * i + 1],
            level_strides[3 * i + 2]};
  void (*fn)(dim3, const Conv3x3Args&, unsigned long long*, void*) = nullptr;
  switch (variant) {  // 10000 * kEp + 1000 * kIl + 100 * kDma + kNP
    case 16: fn = lab_launch<0, 16>; break;
    case 116: fn = lab_launch<1, 16>; break;
    case 10016: fn = lab_launch<0, 16, 0, 1>; break;
    case 10116: fn = lab_launch<1, 16, 0, 1>; break;
    case 20016: fn = lab_launch<0, 16, 0, 2>; break;
    case 20116: fn = lab_launch<1, 16, 0, 2>; break;
    case 10114: fn = lab_launch<1, 14, 0, 1>; break;
    case 1016: fn = lab_launch<0, 16, 1>; break;
    case 1116: fn = lab_launch<1, 16, 1>; break;
    case 216: fn = lab_launch<2, 16>; break;
    case 316: fn = lab_launch<3, 16>; break;
    case 15: fn = lab_launch<0, 15>; break;
    case 14: fn = lab_launch<0, 14>; break;
    case 13: fn = lab_launch<0, 13>; break;
    case 12: fn = lab_launch<0, 12>; break;
    case 115: fn = lab_launch<1, 15>; break;
    case 114: fn = lab_launch<1, 14>; break;
    case 113: fn = lab_launch<1, 13>; break;
    case 112: fn = lab_launch<1, 12>; break;
    default: FRH_REQUIRE(false, "variant %d: 100 * dma form + positions before the barrier", variant);
  }
  return conv3x3_launch_with(what, num_levels, d, workspace, (int64_t)(workspace_bytes / sizeof(float)), n, cin, cout,
                             relu, stream, [&](dim3 grid, const Conv3x3Args& a) {
                               fn(grid, a, reinterpret_cast<unsigned long long*>(stamps), stream);
                             });
}
