// TOOLS-ONLY RoIAlign kernels measured and not adopted, built on the product's
// pieces (roi_kernels.h).  Forward: roi_lab variant 19 (RoI setup shared by a 4-wave workgroup),
// 23 / 24 (software-pipelined persistent waves), 96-99 (the channel-group kernel with
// software-pipelined items), 2-7 (one wave per (RoI, 64 channels), lane = channel).  Backward: the
// register-resident and readlane forms of the channels-last kernel (backward variants 1 / 3, 4-8).
#pragma once
#include "roi_kernels.h"

namespace frh {

// The quad kernel with the RoI setup shared by a workgroup: 4 waves per (RoI, 64 channels),
// wave 0 computes the RoI's tap state (pair_setup) and hands it to the other three through
// LDS (18 dwords per lane), so the ~480-instruction setup runs once per 64 channels, not
// once per 16; each wave then stages and evaluates its own 16 channels.  Tools-only
// candidate (roi_lab variant 19).  Grid: 8 * ceil(K * groups / 8) workgroups of 256.
static __global__ void __launch_bounds__(4 * kWave) roi_align_fwd_quad4_kernel(RoiLevels lv, RoiCfg c, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float slab[4][kQuadSlab];
  __shared__ PairLane sp[kWave];
  __shared__ PairGeom sg;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)), lane = threadIdx.x & (kWave - 1);
  const uint32_t sbase = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)slab[wave]);
  const uint32_t NG = (uint32_t)(c.C + 16 * kQuadWave - 1) / (uint32_t)(16 * kQuadWave), K32 = (uint32_t)c.K;
  const uint32_t total = K32 * NG, per = (total + 7u) / 8u;
  const uint32_t w = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  const uint32_t wend = min((blockIdx.x & 7u) * per + per, total);
  if (w >= wend) return;
  const int grp = (int)(w / K32);
  const int64_t k0 = (int64_t)(w - (uint32_t)grp * K32);
  PairGeom G;
  PairLane P;
  if (wave == 0) {
    const RoiRaw raw = roi_fetch(c, k0);
    pair_setup<16>(lv, c, raw, lane, G, P);
    sp[lane] = P;
    if (lane == 0) sg = G;
  }
  __syncthreads();
  if (wave != 0) {
    P = sp[lane];
    G.empty = __builtin_amdgcn_readfirstlane(sg.empty);
    G.y0 = __builtin_amdgcn_readfirstlane(sg.y0), G.x0 = __builtin_amdgcn_readfirstlane(sg.x0);
    G.R = __builtin_amdgcn_readfirstlane(sg.R), G.Cs = __builtin_amdgcn_readfirstlane(sg.Cs);
    G.Cs2 = __builtin_amdgcn_readfirstlane(sg.Cs2);
    G.dy = __builtin_amdgcn_readfirstlane(sg.dy), G.dx = __builtin_amdgcn_readfirstlane(sg.dx);
    G.sy = __builtin_amdgcn_readfirstlane(sg.sy), G.sx = __builtin_amdgcn_readfirstlane(sg.sx);
    G.scs = __builtin_amdgcn_readfirstlane(sg.scs);
    G.inv = (uint32_t)__builtin_amdgcn_readfirstlane((int)sg.inv);
    G.extent = (uint32_t)__builtin_amdgcn_readfirstlane((int)sg.extent);
    const uint64_t b = reinterpret_cast<uint64_t>(sg.base);
    G.base = reinterpret_cast<const float*>(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b));
  }
  const int chunk = grp * 4 + wave;
  if (chunk * 4 * kQuadWave >= c.C) return;
  quad_body<false, kQuadSlab, false, false>(G, P, c, out, k0, chunk, w, sbase, 0, lane);
}

// ---------------------------------------------------------------------------
// Software-pipelined persistent quad kernel (tools-only candidate, roi_lab variant 23):
// each wave walks its XCD's items (RoI, 16 channels) as units of one channel quad, two
// 8-KB slabs: unit u+1's window DMA is in flight while unit u is evaluated, and the next
// item's setup runs while the current unit's DMA lands.  Same slab layout (D = 1: up to 512
// cells), operation order and outputs as the quad kernel; windows of more cells take the
// global gather per quad, empty RoIs store zeros.
struct QpItem {
  PairGeom G;
  PairLane P;
  int64_t k;
  int cw0, nq;
  int D;    // quads per stage (4, 2, 1: the quad kernel's slab layouts); 0: global gather
  int nst;  // stages
};

__device__ __forceinline__ void qp_load(const RoiLevels& lv, const RoiCfg& c, uint32_t w, uint32_t K32, int lane,
                                        QpItem& it) {
  const int ch = (int)(w / K32);
  it.k = (int64_t)(w - (uint32_t)ch * K32);
  it.cw0 = ch * 4 * kQuadWave;
  it.nq = min(kQuadWave, (c.C - it.cw0) / 4);
  const RoiRaw raw = roi_fetch(c, it.k);
  pair_setup<16>(lv, c, raw, lane, it.G, it.P);
  const int ncell = it.G.R * it.G.Cs2;
  it.D = it.G.empty ? 4 : ncell <= QuadLayout<4>::kCells ? 4 : ncell <= QuadLayout<2>::kCells ? 2
                                                     : ncell <= QuadLayout<1>::kCells ? 1 : 0;
  it.nst = it.D ? (it.nq + it.D - 1) / it.D : it.nq;
}

__device__ __forceinline__ bool qp_staged(const QpItem& it) { return !it.G.empty && it.D > 0; }

// stage s of a staged item: region d (RS(D) dwords) <- quad s * D + d of every window cell
__device__ __forceinline__ void qp_issue(const QpItem& it, int s, uint32_t sb, int lane) {
  const PairGeom& G = it.G;
  const int ncell = G.R * G.Cs2;
  const int nr = (ncell + kWave - 1) / kWave;
  const int RSb = 4 * ((kQuadSlab / it.D) / 256 * 256);  // region bytes
  const __amdgpu_buffer_rsrc_t fr = uniform_rsrc(G.base, (int64_t)G.extent);
  for (int d = 0; d < it.D; ++d) {
    const int soff = (it.cw0 + 4 * min(s * it.D + d, it.nq - 1)) * 4;
    for (int j = 0; j < nr; ++j) {
      int e = j * kWave + lane;
      e = e < ncell ? e : 0;
      const int r = (int)(((uint32_t)e * G.inv) >> 16), col = min(e - r * G.Cs2, G.Cs - 1);
      const int goff = (G.dy && G.dx) ? ((G.y0 + r) * G.sy + (G.x0 + col) * G.sx) * 4
                                      : __shfl(it.P.rsrc, r, kWave) + __shfl(it.P.csrc, col, kWave);
      lds_dma_at<16, 0>(fr, sb + (uint32_t)(d * RSb) + 1024u * (uint32_t)j, goff, soff);
    }
  }
}

// one quad of a staged item from its slab region at rb (byte address): the quad kernel's evaluation
__device__ __forceinline__ f32x4 qp_eval(const PairLane& P, uint32_t rb) {
  constexpr int SR = 2;
  f32x4 v[2][8];
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float ly_h[SR], ly_l[SR], lx_h[SR], lx_l[SR];
  uint32_t lb[SR][SR], ldq[SR], ldr[SR];
#pragma unroll
  for (int i = 0; i < SR; ++i) {
    ly_h[i] = P.fyh[i], ly_l[i] = P.fyl[i], lx_h[i] = P.fxh[i], lx_l[i] = P.fxl[i], ldq[i] = P.tdq[i], ldr[i] = P.tdr[i];
#pragma unroll
    for (int j = 0; j < SR; ++j) lb[i][j] = rb + P.tb0[i][j];
  }
  auto tap = [&](int iy, int ix, int q) -> uint32_t {
    return lb[iy][ix] + ((q & 1) ? ldq[ix] : 0u) + ((q & 2) ? ldr[iy] : 0u);
  };
#pragma unroll
  for (int ix = 0; ix < SR; ++ix)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[0][ix * 4 + q] = lds_read_b128<0>(tap(0, ix, q));
#pragma unroll
  for (int ix = 0; ix < SR; ++ix)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[1][ix * 4 + q] = lds_read_b128<0>(tap(1, ix, q));
  lds_wait4<8>(v[0]);
#pragma unroll
  for (int ix = 0; ix < SR; ++ix) {
    const float w[4] = {ly_h[0] * lx_h[ix], ly_h[0] * lx_l[ix], ly_l[0] * lx_h[ix], ly_l[0] * lx_l[ix]};
    acc = acc + quad_val(w, &v[0][ix * 4]);
  }
  lds_wait4<0>(v[1]);
#pragma unroll
  for (int ix = 0; ix < SR; ++ix) {
    const float w[4] = {ly_h[1] * lx_h[ix], ly_h[1] * lx_l[ix], ly_l[1] * lx_h[ix], ly_l[1] * lx_l[ix]};
    acc = acc + quad_val(w, &v[1][ix * 4]);
  }
  return acc * 0.25f;
}

// quad q of an item whose window does not fit the slab: taps gathered from global memory
__device__ __forceinline__ f32x4 qp_global(const QpItem& it, int q) {
  constexpr int SR = 2;
  const PairGeom& G = it.G;
  const PairLane& P = it.P;
  const __amdgpu_buffer_rsrc_t fr = uniform_rsrc(G.base, (int64_t)G.extent);
  const int soff = (it.cw0 + 4 * q) * 4;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int iy = 0; iy < SR; ++iy)
#pragma unroll
    for (int ix = 0; ix < SR; ++ix) {
      const uint32_t t0 = P.tb0[iy][ix] / 16u;
      const int r0 = (int)(t0 / (uint32_t)G.Cs2), c0 = (int)(t0 - (uint32_t)r0 * (uint32_t)G.Cs2);
      const int r1 = r0 + (int)(P.tdr[iy] / 16u / (uint32_t)G.Cs2), c1 = c0 + (int)(P.tdq[ix] / 16u);
      const int ro0 = __shfl(P.rsrc, r0, kWave), ro1 = __shfl(P.rsrc, r1, kWave);
      const int co0 = __shfl(P.csrc, c0, kWave), co1 = __shfl(P.csrc, c1, kWave);
      f32x4 x[4];
      const int offs[4] = {ro0 + co0, ro0 + co1, ro1 + co0, ro1 + co1};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(fr, offs[t], soff, 0);
        x[t] = f32x4{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
      }
      const float w[4] = {P.fyh[iy] * P.fxh[ix], P.fyh[iy] * P.fxl[ix], P.fyl[iy] * P.fxh[ix], P.fyl[iy] * P.fxl[ix]};
      acc = acc + quad_val(w, x);
    }
  return acc * 0.25f;
}

// s_waitcnt vmcnt(n) for n in {0, 4, 8, 12, 16} (the previous unit's store count)
__device__ __forceinline__ void qp_wait(int n) {
  if (n >= 16) wait_vmcnt<16>();
  else if (n >= 12) wait_vmcnt<12>();
  else if (n >= 8) wait_vmcnt<8>();
  else if (n >= 4) wait_vmcnt<4>();
  else wait_vmcnt<0>();
}

template <int kStAux = kCpolNT>
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) roi_align_fwd_quadp_kernel(RoiLevels lv, RoiCfg c, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float slab[2][kQuadSlab];
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t sb0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)slab[0]);
  const uint32_t sbs[2] = {sb0, sb0 + 4u * kQuadSlab};
  const uint32_t G = (uint32_t)(c.C + 4 * kQuadWave - 1) / (uint32_t)(4 * kQuadWave), K32 = (uint32_t)c.K;
  const uint32_t total = K32 * G, per = (total + 7u) / 8u;
  const uint32_t xcd = blockIdx.x & 7u, nw = gridDim.x >> 3;
  const uint32_t lo = xcd * per, hi = min(lo + per, total);
  uint32_t w = lo + (blockIdx.x >> 3);
  if (w >= hi) return;
  const int nbins = c.ph * c.pw;
  const int ovoff = lane < nbins ? lane * 4 : 0x40000000;
  const int ostep = nbins * 4;
  QpItem A, B;
  qp_load(lv, c, w, K32, lane, A);
  int s = 0, cur = 0, prev_stores = 0;
  if (qp_staged(A)) qp_issue(A, 0, sbs[0], lane);
  for (;;) {
    // the next unit: the next stage of this item, or stage 0 of the wave's next item
    const bool same = s + 1 < A.nst;
    const uint32_t wn = w + nw;
    const bool more = same || wn < hi;
    if (!same && more) qp_load(lv, c, wn, K32, lane, B);  // overlaps the current unit's DMA
    // this unit's DMA landed; the previous unit's output stores (younger: vector memory
    // operations complete in issue order) may still be in flight
    qp_wait(prev_stores);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (more) {
      if (same) {
        if (qp_staged(A)) qp_issue(A, s + 1, sbs[cur ^ 1], lane);
      } else if (qp_staged(B)) {
        qp_issue(B, 0, sbs[cur ^ 1], lane);
      }
    }
    const __amdgpu_buffer_rsrc_t orr = uniform_rsrc(out + (A.k * c.C + A.cw0) * nbins, (int64_t)4 * A.nq * nbins * 4);
    const int D = A.D ? A.D : 1;
    const int RSb = 4 * ((kQuadSlab / D) / 256 * 256);
    prev_stores = 0;
    for (int d = 0; d < D; ++d) {
      const int q = s * D + d;
      if (q >= A.nq) break;
      f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
      if (A.G.empty) {
      } else if (A.D) {
        r = qp_eval(A.P, sbs[cur] + (uint32_t)(d * RSb));
      } else {
        r = qp_global(A, q);
      }
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r.x), orr, ovoff, (4 * q) * ostep, kStAux);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r.y), orr, ovoff, (4 * q + 1) * ostep, kStAux);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r.z), orr, ovoff, (4 * q + 2) * ostep, kStAux);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r.w), orr, ovoff, (4 * q + 3) * ostep, kStAux);
      prev_stores += 4;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!more) break;
    cur ^= 1;
    if (same) {
      ++s;
    } else {
      A = B;
      s = 0;
      w = wn;
    }
  }
}

// Round-6 experiment (tools only; measured slower: the backward is bound by its atomics, not by
// the 8 waves per CU its LDS staging allows -- DESIGN §4).  The channels-last backward with 7 x 7 bins and the wave's grad_out held in registers (49 per lane:
// its channel's bins) instead of LDS: the kernel's LDS is the four tap-entry tables (< 0.5 KB),
// so residency is set by registers (~20 waves per CU against 8 with the 18.9-KB LDS staging).
// The bin row and column of a tap entry are wave-uniform, so the register operand is chosen by a
// uniform switch (static indices).  Same operation order as roi_align_bwd_nhwc_kernel: the same
// per-(RoI, row, column) sums, bit for bit.
template <bool kFixed = false>
__global__ void __launch_bounds__(kWave) roi_align_bwd_nhwc_reg_kernel(RoiLevels lv, RoiCfg c,
                                                                     const float* __restrict__ gout) {
  constexpr int P = 7, NB = P * P;
  __shared__ int ye[kSepEnt], xe[kSepEnt];  // sorted tap entries: position << 16 | bin index
  __shared__ float yws[kSepEnt], xws[kSepEnt];
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const int c0 = blockIdx.y * kWave, ch = c0 + lane;
  const bool live = ch < c.C;
  float gr[NB];  // grad_out of this lane's channel, bin py * 7 + px
  {
    const float* go = gout + (k * c.C + (live ? ch : c0)) * NB;
#pragma unroll
    for (int b = 0; b < NB; ++b) gr[b] = live ? go[b] : 0.0f;
  }
  const RoiGeom g = roi_geom(c, lv, k);
  const int l = g.lvl, H = lv.h[l], W = lv.w[l];
  constexpr int nye = 4 * P, nxe = 4 * P;
  auto entry = [&](int e, float start, float bin, int size, int* pos, float* w) {
    const Tap t = make_tap(start + (float)(e >> 2) * bin + ((float)((e >> 1) & 1) + 0.5f) * bin * 0.5f, size);
    *pos = t.valid ? ((e & 1) ? t.hi : t.lo) : -1;
    *w = (e & 1) ? t.l : t.h;
  };
  int yp = -1, xp = -1;
  float ywv = 0.0f, xwv = 0.0f;
  if (lane < nye) entry(lane, g.start_h, g.bin_h, H, &yp, &ywv);
  if (lane < nxe) entry(lane, g.start_w, g.bin_w, W, &xp, &xwv);
  const int ypm = yp < 0 ? (1 << 20) : yp, xpm = xp < 0 ? (1 << 20) : xp;
  int yr = 0, xr = 0;  // rank by (position, entry)
  for (int e = 0; e < nye; ++e) {
    const int pe = __shfl(ypm, e, kWave);
    yr += (pe < ypm || (pe == ypm && e < lane)) ? 1 : 0;
  }
  for (int e = 0; e < nxe; ++e) {
    const int pe = __shfl(xpm, e, kWave);
    xr += (pe < xpm || (pe == xpm && e < lane)) ? 1 : 0;
  }
  if (yp >= 0) ye[yr] = (yp << 16) | (lane >> 2), yws[yr] = ywv;
  if (xp >= 0) xe[xr] = (xp << 16) | (lane >> 2), xws[xr] = xwv;
  const int nyv = __popcll(__ballot(yp >= 0)), nxv = __popcll(__ballot(xp >= 0));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (nyv == 0 || nxv == 0) return;  // no valid tap: no gradient
  const int64_t base = (int64_t)g.b * lv.sb[l] + ch, sy = lv.sy[l], sx = lv.sx[l];
  const double fscale = kFixed ? bwd_fixed_scale(c.fix_max, c.fix_hb) : 0.0;
  if (kFixed && fscale < 0.0) return;  // non-finite gradient: the conversion writes NaN
  float R[P];
#pragma unroll
  for (int px = 0; px < P; ++px) R[px] = 0.0f;
  for (int i = 0; i < nyv; ++i) {
    const int yv = __builtin_amdgcn_readfirstlane(ye[i]), row = yv >> 16, py = yv & 0xffff;
    const float wy = yws[i];
    switch (py) {  // wave-uniform: static register operands
#define FRH_ROW_CASE(Q)                                                       \
  case Q:                                                                     \
    _Pragma("unroll") for (int px = 0; px < P; ++px) R[px] = R[px] + wy * gr[Q * P + px]; \
    break;
      FRH_ROW_CASE(0) FRH_ROW_CASE(1) FRH_ROW_CASE(2) FRH_ROW_CASE(3) FRH_ROW_CASE(4) FRH_ROW_CASE(5) FRH_ROW_CASE(6)
#undef FRH_ROW_CASE
      default: break;
    }
    if (i + 1 < nyv && (ye[i + 1] >> 16) == row) continue;  // the row continues (uniform)
    float acc = 0.0f;
    for (int jx = 0; jx < nxv; ++jx) {
      const int xv = __builtin_amdgcn_readfirstlane(xe[jx]), col = xv >> 16, px = xv & 0xffff;
      const float rv = px == 0 ? R[0] : px == 1 ? R[1] : px == 2 ? R[2] : px == 3 ? R[3] : px == 4 ? R[4]
                                                                                             : px == 5 ? R[5] : R[6];
      acc = acc + xws[jx] * rv;
      if (jx + 1 < nxv && (xe[jx + 1] >> 16) == col) continue;
      const float v = acc * 0.25f;  // / count (4 samples)
      acc = 0.0f;
      if (!live || v == 0.0f) continue;
      const int64_t e = base + (int64_t)row * sy + (int64_t)col * sx;
      if constexpr (kFixed)
        atomicAdd(reinterpret_cast<unsigned long long*>(lv.grad[l]) + e,
                  (unsigned long long)(long long)rint((double)v * fscale));
      else
        atomicAdd(lv.grad[l] + e, v);
    }
#pragma unroll
    for (int px = 0; px < P; ++px) R[px] = 0.0f;
  }
}

// ---------------------------------------------------------------------------
// The channel-group forward with kItems items per workgroup, software-pipelined (round 6): the
// next item's RoI record, window and sample tables (the ~1.5-2 us setup chain: scalar loads, tap
// math, tables) are computed while the current item's window DMA is in flight, and the slab is
// never idle during a setup.  Tables double-buffered; barriers wait for LDS only (the output
// stores drain in the background).  Item j of workgroup r of XCD x: x * per + r + j * nwx (per
// items per XCD, nwx workgroups per XCD), so the resident workgroups of an XCD stay on nearby
// RoIs of one channel group.  Same evaluation as roi_align_fwd_cg_kernel: bit-identical.
__device__ __forceinline__ void lds_only_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

struct CgItem {  // wave-uniform (SGPRs); the per-lane tables live in LDS (CgTab)
  const float* base;  // image b of the RoI's level
  uint32_t extent;    // feature bytes addressable from base
  int k, grp, state;  // state 0: none, 1: no valid sample (zeros), 2: staged and evaluated
  int R, Cs, dy, multi, rows_cap;
  float rcs;
};

// An item's LDS tables (written by wave 0 in cg_setup): the sample tables (y samples [0, 16), x
// [16, 32): slab row / column of the lo tap, hi - lo, l, h), the source byte offsets of the window
// rows (dense or tap-list) and columns, the tap-list rows (list bands), bin-row row spans.
struct CgTab {
  float4 smp[32];
  int rsrc[32], rsrcl[32], csrc[32];
  int brl[8], brh[8];
};

template <int kSlabCells>
__device__ __forceinline__ void cg_setup(const RoiLevels& lv, const RoiCfg& c, uint32_t w, uint32_t wend, CgTab* tb,
                                         int lane, int wave, CgItem& it) {
  constexpr int SR = 2;
  if (w >= wend) {
    it.state = 0;
    return;
  }
  const uint32_t K32 = (uint32_t)c.K;
  it.grp = (int)(w / K32);
  it.k = (int)(w - (uint32_t)it.grp * K32);
  const RoiRaw raw = roi_fetch(c, (int64_t)it.k);
  const RoiGeom g = roi_geom_raw(c, lv, raw);
  const int l = g.lvl;
  const int H = lv.h[l], W = lv.w[l];
  const int sy = (int)lv.sy[l], sx = (int)lv.sx[l];
  const bool isx = lane >= 32;
  const int e = lane & 31;
  const int nl = isx ? 2 * SR * c.pw : 2 * SR * c.ph;
  int trow = -1, tlo = 0x7fffffff, thi = -1;
  float tl = 0.f, th = 0.f;
  if (e < nl) {
    const int s = e >> 1, p = s >> 1, i = s & 1;
    const float v = isx ? g.start_w + (float)p * g.bin_w + ((float)i + 0.5f) * g.bin_w * 0.5f
                        : g.start_h + (float)p * g.bin_h + ((float)i + 0.5f) * g.bin_h * 0.5f;
    const Tap t = make_tap(v, isx ? W : H);
    if (t.valid) trow = (e & 1) ? t.hi : t.lo, tlo = t.lo, thi = t.hi, tl = t.l, th = t.h;
  }
  const uint64_t vm = __ballot(trow >= 0);
  const uint32_t vy = (uint32_t)vm, vx = (uint32_t)(vm >> 32);
  if (!vy || !vx) {
    it.state = 1;
    return;
  }
  it.state = 2;
  const int y0 = __builtin_amdgcn_readlane(tlo, __builtin_ctz(vy));
  const int y1 = __builtin_amdgcn_readlane(thi, 31 - __builtin_clz(vy));
  const int x0 = __builtin_amdgcn_readlane(tlo, 32 + __builtin_ctz(vx));
  const int x1 = __builtin_amdgcn_readlane(thi, 63 - __builtin_clz(vx));
  const int nly = 2 * SR * c.ph, nlx = 2 * SR * c.pw;
  const bool dy = y1 - y0 + 1 <= nly, dx = x1 - x0 + 1 <= nlx;
  it.dy = dy;
  it.R = dy ? y1 - y0 + 1 : nly;
  it.Cs = dx ? x1 - x0 + 1 : nlx;
  it.multi = it.R * it.Cs > kSlabCells;
  it.rcs = __builtin_amdgcn_rcpf((float)it.Cs);
  it.rows_cap = it.multi ? (int)(((float)kSlabCells + 0.5f) * it.rcs) : kSlabCells;
  it.base = lv.feat[l] + (int64_t)g.b * lv.sb[l];
  it.extent = (uint32_t)(((int64_t)(c.C - 1) + (int64_t)(H - 1) * sy + (int64_t)(W - 1) * sx + 1) * 4);
  if (wave == 0) {
    const bool dax = isx ? dx : dy;
    const int org = isx ? x0 : y0;
    const int src = (dax ? org + min(e, (isx ? it.Cs : it.R) - 1) : (trow >= 0 ? trow : org)) * (isx ? sx : sy) * 4;
    if (isx) {
      tb->csrc[e] = src;
    } else {
      tb->rsrc[e] = src;
      tb->rsrcl[e] = (trow >= 0 ? trow : org) * sy * 4;
    }
    const bool tv = e < nl && trow >= 0 && (e & 1) == 0;
    const int r0 = tv ? (dax ? tlo - org : e) : 0, dr = tv ? (dax ? thi - tlo : 1) : 0;
    if ((e & 1) == 0)
      tb->smp[(isx ? 16 : 0) + (e >> 1)] = float4{__int_as_float(r0), __int_as_float(dr), tv ? tl : 0.f, tv ? th : 0.f};
    if (it.multi) {
      const int rl = tv ? r0 : 0x7fffffff, rh = tv ? r0 + dr : -1;
      const int pr = min(lane, 15);
      const int a = min(__shfl(rl, 4 * pr, kWave), __shfl(rl, 4 * pr + 2, kWave));
      const int b = max(__shfl(rh, 4 * pr, kWave), __shfl(rh, 4 * pr + 2, kWave));
      if (lane < 8) tb->brl[lane] = a, tb->brh[lane] = b;
    }
  }
}

// one item: its bands (staging, evaluation), the output block; hook() runs once, right after
// the first band's DMA is issued (or at once for an item without a valid sample)
template <int kNW, int kSlabCells, int kStAux, bool kLd2, typename Hook>
__device__ __forceinline__ void cg_body(const RoiCfg& c, const CgItem& it, float* __restrict__ out, float* slab,
                                        uint32_t sbase, const CgTab* tb, int lane, int wave, Hook&& hook) {
  const uint32_t tbase = (uint32_t)reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) const float4*)reinterpret_cast<const float4*>(tb->smp));
  constexpr int SR = 2;
  constexpr int kJ = 16 / kNW;
  const int nbins = c.ph * c.pw;
  const int nq = nbins * kCgChan / 4;
  if (it.state == 1) {
    const __amdgpu_buffer_rsrc_t orr =
        uniform_rsrc(out + ((int64_t)it.k * c.C + (int64_t)it.grp * kCgChan) * nbins, (int64_t)nq * 16);
    for (int u = (int)threadIdx.x; u < nq; u += kNW * kWave)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, orr, u * 16, 0, kStAux);
    hook();
    return;
  }
  const int R = it.R, Cs = it.Cs;
  const float rcs = it.rcs;
  const int soff = it.grp * kCgChan * 4;
  const int q = lane & 15, b4 = lane >> 4;
  f32x4 res[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int pb = 0;
  bool first = true;
  while (pb < c.ph) {
    int rs = 0x7fffffff, re = -1, pe = pb;
    if (!it.multi) {
      rs = 0, re = R - 1, pe = c.ph;
    } else {
      while (pe < c.ph) {
        const int lo = __builtin_amdgcn_readfirstlane(tb->brl[pe]), hi = __builtin_amdgcn_readfirstlane(tb->brh[pe]);
        if (hi >= 0) {
          const int nrs = min(rs, lo), nre = max(re, hi);
          if (pe > pb && nre - nrs + 1 > it.rows_cap) break;
          rs = nrs, re = nre;
        }
        ++pe;
      }
      if (re < 0) rs = re = 0;
    }
    const bool lst = it.multi && it.dy && re - rs + 1 > it.rows_cap;
    if (lst) rs = 4 * pb, re = 4 * pb + 3, pe = pb + 1;
    const int nb = (re - rs + 1) * Cs;
    const int nj = (nb + 3) >> 2;
    for (int J = wave; J < nj; J += kNW) {
      int cell = 4 * J + b4;
      const bool in = cell < nb;
      cell = in ? cell : 0;
      const int r = (int)(((float)cell + 0.5f) * rcs), cc = cell - r * Cs;
      const int voff = (lst ? tb->rsrcl[rs + r] : tb->rsrc[rs + r]) + tb->csrc[cc] + q * 16;
      lds_dma_at<16, 0>(uniform_rsrc(it.base, (int64_t)it.extent), sbase + 1024u * (uint32_t)J,
                        in ? voff : 0x40000000, soff);
    }
    if (first) {
      hook();  // the next item's setup while this DMA is in flight
      first = false;
    }
    wait_vmcnt<0>();
    lds_only_barrier();  // every wave's DMA (and the tables) landed
    const int bin_lo = pb * c.pw, bin_hi = min(pe * c.pw, nbins);
    const int rsb = rs;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const int t = wave + kNW * j;
      if (4 * t + 3 < bin_lo || 4 * t >= bin_hi) continue;
      int b4o = b4;
      asm volatile("" : "+v"(b4o));
      const int bin = 4 * t + b4o;
      const bool act = bin >= bin_lo && bin < bin_hi;
      const int bq = act ? bin : bin_lo;
      const int py = (int)(((uint32_t)bq * ((65536u + (uint32_t)c.pw - 1u) / (uint32_t)c.pw)) >> 16), px = bq - py * c.pw;
      f32x4 Y[2], X[2];
      Y[0] = lds_read_b128<0>(tbase + 32u * (uint32_t)py);
      Y[1] = lds_read_b128<16>(tbase + 32u * (uint32_t)py);
      X[0] = lds_read_b128<256>(tbase + 32u * (uint32_t)px);
      X[1] = lds_read_b128<272>(tbase + 32u * (uint32_t)px);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Y[0]), "+v"(Y[1]), "+v"(X[0]), "+v"(X[1]) : : "memory");
      uint32_t ra[SR], rd[SR], ca[SR], cd[SR];
#pragma unroll
      for (int i = 0; i < SR; ++i) {
        const int ry = lst ? 4 * py + 2 * i - rsb : max(__float_as_int(Y[i].x) - rsb, 0);
        ra[i] = (uint32_t)(ry * Cs) * 256u;
        rd[i] = (uint32_t)((lst ? 1 : __float_as_int(Y[i].y)) * Cs) * 256u;
        ca[i] = (uint32_t)__float_as_int(X[i].x) * 256u;
        cd[i] = (uint32_t)__float_as_int(X[i].y) * 256u;
      }
      const uint32_t qb = sbase + 16u * (uint32_t)q;
      f32x4 v[2][8];
      auto load = [&](auto hh) {
        constexpr int iy = decltype(hh)::value;
#pragma unroll
        for (int ix = 0; ix < SR; ++ix) {
          const uint32_t a = qb + ra[iy] + ca[ix];
          v[iy][ix * 4 + 0] = lds_read_b128<0>(a);
          v[iy][ix * 4 + 1] = lds_read_b128<0>(a + cd[ix]);
          v[iy][ix * 4 + 2] = lds_read_b128<0>(a + rd[iy]);
          v[iy][ix * 4 + 3] = lds_read_b128<0>(a + rd[iy] + cd[ix]);
        }
      };
      load(std::integral_constant<int, 0>{});
      if constexpr (kLd2) load(std::integral_constant<int, 1>{});
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (kLd2) lds_wait4<8>(v[0]);
      else lds_wait4<0>(v[0]);
#pragma unroll
      for (int ix = 0; ix < SR; ++ix) {
        const float wq[4] = {Y[0].w * X[ix].w, Y[0].w * X[ix].z, Y[0].z * X[ix].w, Y[0].z * X[ix].z};
        acc = acc + quad_val(wq, &v[0][ix * 4]);
      }
      if constexpr (!kLd2) {
        asm volatile("" : "+v"(acc));
        load(std::integral_constant<int, 1>{});
      }
      lds_wait4<0>(v[1]);
#pragma unroll
      for (int ix = 0; ix < SR; ++ix) {
        const float wq[4] = {Y[1].w * X[ix].w, Y[1].w * X[ix].z, Y[1].z * X[ix].w, Y[1].z * X[ix].z};
        acc = acc + quad_val(wq, &v[1][ix * 4]);
      }
      if (act) res[j] = acc * 0.25f;
    }
    lds_only_barrier();  // the band's tap reads are done before the next band (or the outputs) overwrite the slab
    pb = pe;
  }
  float* ob = slab;
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    const int bin = 4 * (wave + kNW * j) + b4;
    if (bin < nbins) {
      ob[(4 * q + 0) * nbins + bin] = res[j].x;
      ob[(4 * q + 1) * nbins + bin] = res[j].y;
      ob[(4 * q + 2) * nbins + bin] = res[j].z;
      ob[(4 * q + 3) * nbins + bin] = res[j].w;
    }
  }
  lds_only_barrier();
  const __amdgpu_buffer_rsrc_t orr =
      uniform_rsrc(out + ((int64_t)it.k * c.C + (int64_t)it.grp * kCgChan) * nbins, (int64_t)nq * 16);
  const float4* o4 = reinterpret_cast<const float4*>(slab);
  for (int u = (int)threadIdx.x; u < nq; u += kNW * kWave) {
    const float4 v4 = o4[u];
    __builtin_amdgcn_raw_buffer_store_b128(
        u32x4{__float_as_uint(v4.x), __float_as_uint(v4.y), __float_as_uint(v4.z), __float_as_uint(v4.w)}, orr,
        u * 16, 0, kStAux);
  }
  lds_only_barrier();  // the output block's reads are done before the next item's DMA overwrites the slab
}

template <int kNW, int kSlabCells, int kItems, int kStAux = kCpolNT, bool kSpan = false, int kWpe = 0,
          bool kLd2 = false>
__global__ void __launch_bounds__(kNW * kWave) __attribute__((amdgpu_waves_per_eu(kWpe > 0 ? kWpe : 1)))
roi_align_fwd_cgp_kernel(RoiLevels lv, RoiCfg c, float* __restrict__ out) {
  static_assert(kNW == 2 || kNW == 4 || kNW == 8, "waves per workgroup");
  static_assert(kSlabCells >= 64 && kSlabCells % 4 == 0, "the output block [64][<= 64 bins] leaves through the slab");
  static_assert((kSlabCells + 3) / 4 <= 63 * kNW, "vmcnt is 6 bits");
  const int64_t t_start = kSpan ? (int64_t)__builtin_amdgcn_s_memrealtime() : 0;
  __shared__ __attribute__((aligned(16))) float slab[kSlabCells * kCgChan];
  __shared__ CgTab tab[2];  // double-buffered item tables
  const uint32_t sbase = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)slab);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t total = (uint32_t)c.K * ((uint32_t)c.C / kCgChan), per = (total + 7u) / 8u;
  const uint32_t nwx = (per + kItems - 1u) / kItems;  // workgroups per XCD
  const uint32_t x = blockIdx.x & 7u, r = blockIdx.x >> 3;
  const uint32_t wend = min(x * per + per, total);
  uint32_t w = x * per + r;
  CgItem cur, nxt;
  cg_setup<kSlabCells>(lv, c, w, wend, &tab[0], lane, wave, cur);
  lds_only_barrier();  // the first item's tables
  int b = 0;
  for (int j = 0; j < kItems && cur.state; ++j) {
    const uint32_t wn = j + 1 < kItems ? w + nwx : wend;
    nxt.state = 0;
    cg_body<kNW, kSlabCells, kStAux, kLd2>(c, cur, out, slab, sbase, &tab[b], lane, wave, [&] {
      cg_setup<kSlabCells>(lv, c, wn, wend, &tab[b ^ 1], lane, wave, nxt);
    });
    cur = nxt;
    w = wn;
    b ^= 1;
  }
  if (kSpan && threadIdx.x == 0) record_span(c, t_start);
}

// The channels-last backward with the tap lists in registers (round 6): the sorted y / x tap
// entries sit one per lane and are read by v_readlane with the wave-uniform loop index (a
// scalar, no LDS round trip), the row sums R[px] stay in registers and the column loop picks
// R[px] by a uniform select -- the round-5 kernel read each x entry, its weight and R[px]
// from LDS in a dependent chain (two LDS round trips per (row, column) pair: ~50 us of serial
// latency per wave on VOC-sized windows).  Same sums in the same order: each cell's
// contribution is bit-identical to roi_align_bwd_nhwc_kernel's.
// kStore (tools-only diagnostic): plain stores instead of the atomics (wrong sums): the kernel's
// time without the atomic traffic; kDiag (tools-only): 1 = no column loop (the row sums stored),
// 2 = return after the tap-entry setup
template <bool kFixed = false, bool kStore = false, int kDiag = 0>
__global__ void __launch_bounds__(kWave) roi_align_bwd_nhwc2_kernel(RoiLevels lv, RoiCfg c,
                                                                  const float* __restrict__ gout) {
  constexpr int kMaxP = 8;
  __shared__ __attribute__((aligned(16))) float gs[kMaxP * kMaxP * kWave];  // grad_out, [lane][bin]
  __shared__ int ye[kSepEnt], xe[kSepEnt];     // sorted tap entries: position << 16 | bin index
  __shared__ float yws[kSepEnt], xws[kSepEnt];
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const int c0 = blockIdx.y * kWave, ch = c0 + lane;
  const bool live = ch < c.C;
  const RoiGeom g = roi_geom(c, lv, k);
  const int l = g.lvl, H = lv.h[l], W = lv.w[l];
  const int ph = c.ph, pw = c.pw, nbins = ph * pw, nye = 4 * ph, nxe = 4 * pw;
  {  // the wave's contiguous [64][bins] grad_out block by LDS-DMA (as roi_align_bwd_nhwc_kernel)
    const float* go = gout + (k * c.C + c0) * nbins;
    const int nvalid = min(kWave, c.C - c0) * nbins;
    const __amdgpu_buffer_rsrc_t gr = uniform_rsrc(go, (int64_t)nvalid * 4);
    const uint32_t gsb = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)gs);
    for (int i0 = 0; i0 < nbins; i0 += 32) {
      const int i1 = min(nbins, i0 + 32);
      for (int i = i0; i < i1; ++i) lds_dma_at<4, 0>(gr, gsb + 256u * (uint32_t)i, lane * 4, i * 256);
      wait_vmcnt<0>();
    }
  }
  auto entry = [&](int e, float start, float bin, int size, int* pos, float* w) {
    const Tap t = make_tap(start + (float)(e >> 2) * bin + ((float)((e >> 1) & 1) + 0.5f) * bin * 0.5f, size);
    *pos = t.valid ? ((e & 1) ? t.hi : t.lo) : -1;
    *w = (e & 1) ? t.l : t.h;
  };
  int yp = -1, xp = -1;
  float ywv = 0.0f, xwv = 0.0f;
  if (lane < nye) entry(lane, g.start_h, g.bin_h, H, &yp, &ywv);
  if (lane < nxe) entry(lane, g.start_w, g.bin_w, W, &xp, &xwv);
  if (lane >= nye) yp = -1;
  if (lane >= nxe) xp = -1;
  const int ypm = yp < 0 ? (1 << 20) : yp, xpm = xp < 0 ? (1 << 20) : xp;
  int yr = 0, xr = 0;  // rank by (position, entry)
  for (int e = 0; e < nye; ++e) {
    const int pe = __shfl(ypm, e, kWave);
    yr += (pe < ypm || (pe == ypm && e < lane)) ? 1 : 0;
  }
  for (int e = 0; e < nxe; ++e) {
    const int pe = __shfl(xpm, e, kWave);
    xr += (pe < xpm || (pe == xpm && e < lane)) ? 1 : 0;
  }
  if (yp >= 0) ye[yr] = (yp << 16) | (lane >> 2), yws[yr] = ywv;
  if (xp >= 0) xe[xr] = (xp << 16) | (lane >> 2), xws[xr] = xwv;
  const int nyv = __popcll(__ballot(yp >= 0)), nxv = __popcll(__ballot(xp >= 0));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (nyv == 0 || nxv == 0) return;  // no valid tap: no gradient
  if (kDiag == 2) {
    if (ye[0] == 0x7fffffff) lv.grad[l][lane] = 1.0f;  // keep the setup alive
    return;
  }
  // lane i holds sorted entry i of each axis (read by v_readlane below)
  const int ye_l = lane < kSepEnt ? ye[lane] : 0, xe_l = lane < kSepEnt ? xe[lane] : 0;
  const float yw_l = lane < kSepEnt ? yws[lane] : 0.0f, xw_l = lane < kSepEnt ? xws[lane] : 0.0f;
  const int64_t base = (int64_t)g.b * lv.sb[l] + ch, sy = lv.sy[l], sx = lv.sx[l];
  const double fscale = kFixed ? bwd_fixed_scale(c.fix_max, c.fix_hb) : 0.0;
  if (kFixed && fscale < 0.0) return;  // non-finite gradient: the conversion writes NaN
  float R[kMaxP];
#pragma unroll
  for (int px = 0; px < kMaxP; ++px) R[px] = 0.0f;
  for (int i = 0; i < nyv; ++i) {
    const int yv = __builtin_amdgcn_readlane(ye_l, i), row = yv >> 16, py = yv & 0xffff;
    const float wy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yw_l), i));
    const float* gr = gs + lane * nbins + py * pw;
#pragma unroll
    for (int px = 0; px < kMaxP; ++px)
      if (px < pw) R[px] = R[px] + wy * gr[px];
    if (i + 1 < nyv && (__builtin_amdgcn_readlane(ye_l, i + 1) >> 16) == row) continue;  // the row continues
    if (kDiag == 1) {
      float t = 0.0f;
#pragma unroll
      for (int px = 0; px < kMaxP; ++px) t = t + R[px], R[px] = 0.0f;
      if (live) __builtin_nontemporal_store(t, lv.grad[l] + base + (int64_t)row * sy);
      continue;
    }
    float acc = 0.0f;
    for (int jx = 0; jx < nxv; ++jx) {
      const int xv = __builtin_amdgcn_readlane(xe_l, jx), col = xv >> 16, px = xv & 0xffff;
      const float wx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xw_l), jx));
      float r = R[0];
#pragma unroll
      for (int q = 1; q < kMaxP; ++q) r = px == q ? R[q] : r;  // uniform select
      acc = acc + wx * r;
      if (jx + 1 < nxv && (__builtin_amdgcn_readlane(xe_l, jx + 1) >> 16) == col) continue;
      const float v = acc * 0.25f;  // / count (4 samples)
      acc = 0.0f;
      if (!live || v == 0.0f) continue;
      const int64_t e = base + (int64_t)row * sy + (int64_t)col * sx;
      if constexpr (kStore)
        __builtin_nontemporal_store(v, lv.grad[l] + e);
      else if constexpr (kFixed)
        atomicAdd(reinterpret_cast<unsigned long long*>(lv.grad[l]) + e,
                  (unsigned long long)(long long)rint((double)v * fscale));
      else
        atomicAdd(lv.grad[l] + e, v);
    }
#pragma unroll
    for (int px = 0; px < kMaxP; ++px) R[px] = 0.0f;
  }
}

// ---------------------------------------------------------------------------
// Channels-last forward (features with unit channel stride: the FPN's NHWC outputs).
// One wave per (RoI, 64 channels), lane = channel: every tap is wave-uniform, so the
// sample geometry is computed once per wave (14 y- and 14 x-samples, one lane each,
// broadcast by v_readlane) and every feature access is a 256-B run of one cell's
// channels.  The RoI's tap cells (the dense window [y0, y1] x [x0, x1], or per axis the
// 2 * 2 * P (lo, hi) tap list when the window is wider -- as the pair kernel) are staged
// into the wave's LDS slab by 16-B LDS-DMA, one 1-KB instruction per 4 cells (full
// 128-B lines); a window with more than kCells cells is staged in bands of slab rows,
// each band holding whole sample rows.  Each sample's four taps are ds_read_b32 of
// consecutive channels (conflict-free); the bilinear sums run per lane in torchvision's
// operation order, so the result is bit-identical to the other kernels.  The 7 x 7
// outputs of the lane's channel collect in VGPRs and leave through the slab, transposed
// to [channel][bin], as 16-B stores of one contiguous 12.5-KB block.
constexpr int kNhwcGroup = 64;  // channels per wave

// kRegOut: the outputs stay in VGPRs until the end (LDS = the slab only) instead of a
// separate [channel][bin] LDS buffer.  kStamp (tools-only timing builds): lane 0 writes 8
// int64 per item after the output -- s_memrealtime at start / prologue done / first band
// landed / eval done / end, bands staged, cells of the first band, XCD.
template <int PH, int PW, int kCells, int kStAux, bool kRegOut = true, bool kStamp = false>
__global__ void __launch_bounds__(kWave) roi_align_fwd_nhwc_kernel(RoiLevels lv, RoiCfg c, float* __restrict__ out) {
  const int64_t t_start = kStamp ? (int64_t)__builtin_amdgcn_s_memrealtime() : 0;
  int64_t t_pro = 0, t_land = 0, t_eval = 0;
  int n_bands = 0, first_cells = 0;
  static_assert(2 * PH <= 32 && 2 * PW <= 32 && kCells % 4 == 0 && kCells >= 2 * 4 * PW, "tap lanes / DMA rounds");
  static_assert(!kRegOut || kCells >= PH * PW, "the outputs leave through the slab");
  constexpr int NLY = 4 * PH, NLX = 4 * PW;  // tap-list lengths
  constexpr int NB = PH * PW;
  __shared__ __attribute__((aligned(16))) float slab[kCells * kNhwcGroup];
  __shared__ __attribute__((aligned(16))) float obuf[kRegOut ? 4 : kNhwcGroup * NB];  // [channel][bin]
  const uint32_t sbase = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)slab);
  const int lane = threadIdx.x;
  // XCD x (= workgroup id mod 8) walks the x-th eighth of the group-major (group, RoI) list
  const uint32_t G = (uint32_t)c.C / kNhwcGroup, K32 = (uint32_t)c.K;
  const uint32_t total = K32 * G, per = (total + 7u) / 8u;
  const uint32_t w = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (w >= min((blockIdx.x & 7u) * per + per, total)) return;
  const int grp = (int)(w / K32);
  const int64_t k = (int64_t)(w - (uint32_t)grp * K32);
  const RoiRaw raw = roi_fetch(c, k);
  const RoiGeom g = roi_geom_raw(c, lv, raw);
  const int l = g.lvl, H = lv.h[l], W = lv.w[l];
  // lane s < 2 PH: y sample s (bin s / 2, sub-sample s % 2); lane 32 + s < 32 + 2 PW: x sample s
  const bool isy = lane < 2 * PH, isx = lane >= 32 && lane < 32 + 2 * PW;
  const int s = isy ? lane : lane - 32;
  Tap t{0, 0, 0.f, 0.f, 0};
  if (isy || isx) {
    const float st = isy ? g.start_h : g.start_w, bn = isy ? g.bin_h : g.bin_w;
    t = make_tap(st + (float)(s >> 1) * bn + ((float)(s & 1) + 0.5f) * bn * 0.5f, isy ? H : W);
  }
  const bool tv = (isy || isx) && t.valid;
  const int y0 = __builtin_amdgcn_readfirstlane(wave_min_i32(isy && tv ? t.lo : 1 << 30));
  const int y1 = __builtin_amdgcn_readfirstlane(wave_max_i32(isy && tv ? t.hi : -1));
  const int x0 = __builtin_amdgcn_readfirstlane(wave_min_i32(isx && tv ? t.lo : 1 << 30));
  const int x1 = __builtin_amdgcn_readfirstlane(wave_max_i32(isx && tv ? t.hi : -1));
  float* o = out + (k * c.C + (int64_t)grp * kNhwcGroup) * NB;  // [64][NB], contiguous
  const __amdgpu_buffer_rsrc_t orr = uniform_rsrc(o, (int64_t)kNhwcGroup * NB * 4);
  if (!(y1 >= y0 && x1 >= x0)) {  // no valid sample: every bin is 0
    for (int e = lane; e < kNhwcGroup * NB / 4; e += kWave)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, orr, e * 16, 0, kStAux);
    return;
  }
  const bool dy = y1 - y0 + 1 <= NLY, dx = x1 - x0 + 1 <= NLX;
  const int R = dy ? y1 - y0 + 1 : NLY, Cs = dx ? x1 - x0 + 1 : NLX;
  // per-lane sample data: slab indices (row of y sample / column of x sample) and factors,
  // zeroed (and pointed at index 0) for invalid samples
  const int i0 = !tv ? 0 : (isy ? (dy ? t.lo - y0 : 2 * s) : (dx ? t.lo - x0 : 2 * s));
  const int i1 = !tv ? 0 : (isy ? (dy ? t.hi - y0 : 2 * s + 1) : (dx ? t.hi - x0 : 2 * s + 1));
  const float fl = tv ? t.l : 0.f, fh = tv ? t.h : 0.f;
  // tap-list source rows / columns: list entry e of an axis is tap (e & 1 ? hi : lo) of sample e / 2
  // (the source lane supplies both taps; the destination picks by its own parity)
  const int ysrc_e = (lane < NLY) ? lane : 0, xsrc_e = (lane < NLX) ? lane : 0;
  const int ylo_s = __shfl(tv ? t.lo : y0, ysrc_e >> 1, kWave), yhi_s = __shfl(tv ? t.hi : y0, ysrc_e >> 1, kWave);
  const int xlo_s = __shfl(tv ? t.lo : x0, 32 + (xsrc_e >> 1), kWave);
  const int xhi_s = __shfl(tv ? t.hi : x0, 32 + (xsrc_e >> 1), kWave);
  const int ysrc = (ysrc_e & 1) ? yhi_s : ylo_s, xsrc = (xsrc_e & 1) ? xhi_s : xlo_s;
  const int64_t sy = lv.sy[l], sx = lv.sx[l];
  const float* base = lv.feat[l] + (int64_t)g.b * lv.sb[l];
  const __amdgpu_buffer_rsrc_t fr =
      uniform_rsrc(base, ((int64_t)(H - 1) * sy + (int64_t)(W - 1) * sx + c.C) * 4);
  const int rows_cap = kCells / Cs;  // >= 2: Cs <= NLX
  const uint32_t inv = (65536u + (uint32_t)Cs - 1u) / (uint32_t)Cs;  // e / Cs for e < 1024
  const int quad = (lane & 15) * 16, soff = grp * kNhwcGroup * 4;
  int band_lo = 0, band_hi = 0;
  if (kStamp) t_pro = (int64_t)__builtin_amdgcn_s_memrealtime();
  // sample row sr (in order): stage its band if needed, then acc[px] += its two samples of each bin column
  auto row = [&](int sr, float (&acc)[PW]) {
    // opaque copies: the broadcasts are re-read per row, not hoisted into ~60 live SGPRs
    int a0 = i0, a1 = i1, av = tv;
    float al = fl, ah = fh;
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(av), "+v"(al), "+v"(ah));
    int r0 = __builtin_amdgcn_readlane(a0, sr), r1 = __builtin_amdgcn_readlane(a1, sr);
    const float ly = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(al), sr));
    const float hy = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ah), sr));
    if (!__builtin_amdgcn_readlane(av, sr) && band_hi > band_lo) r0 = r1 = band_lo;  // zero weights: any cell
    if (r0 < band_lo || r1 >= band_hi) {  // stage the band of slab rows [r0, r0 + rows_cap)
      band_lo = r0;
      band_hi = min(r0 + rows_cap, R);
      const int ncell = (band_hi - band_lo) * Cs;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the previous band's tap reads are done
      __builtin_amdgcn_wave_barrier();
      for (int i = 0; 4 * i < ncell; ++i) {
        int e = 4 * i + (lane >> 4);
        e = e < ncell ? e : ncell - 1;
        const int rr = (int)(((uint32_t)e * inv) >> 16), cc = e - rr * Cs;
        const int yy = dy ? y0 + band_lo + rr : __shfl(ysrc, band_lo + rr, kWave);
        const int xx = dx ? x0 + cc : __shfl(xsrc, cc, kWave);
        lds_dma_at<16, 0>(fr, sbase + 1024u * (uint32_t)i, (int)(((int64_t)yy * sy + (int64_t)xx * sx) * 4) + quad,
                          soff);
      }
      wait_vmcnt<0>();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (kStamp) {
        if (n_bands == 0) t_land = (int64_t)__builtin_amdgcn_s_memrealtime(), first_cells = ncell;
        ++n_bands;
      }
    }
    const float* row0 = slab + (r0 - band_lo) * Cs * kNhwcGroup + lane;
    const float* row1 = slab + (r1 - band_lo) * Cs * kNhwcGroup + lane;
#pragma unroll
    for (int ix = 0; ix < 2 * PW; ++ix) {
      const int q0 = __builtin_amdgcn_readlane(a0, 32 + ix) * kNhwcGroup;
      const int q1 = __builtin_amdgcn_readlane(a1, 32 + ix) * kNhwcGroup;
      const float lx = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(al), 32 + ix));
      const float hx = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ah), 32 + ix));
      const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
      const float val = ((w1 * row0[q0] + w2 * row0[q1]) + w3 * row1[q0]) + w4 * row1[q1];
      acc[ix >> 1] = acc[ix >> 1] + val;
    }
  };
  float* ob = kRegOut ? slab : obuf;  // [channel][bin]
  if constexpr (kRegOut) {
    // the 7 x 7 outputs of this lane's channel in VGPRs: a dynamic bin-row loop shifts each
    // row's results into the tail of outv (static indices only), then out through the slab
    float outv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) outv[j] = 0.0f;
    for (int py = 0; py < PH; ++py) {
      float acc[PW];
#pragma unroll
      for (int px = 0; px < PW; ++px) acc[px] = 0.0f;
      row(2 * py, acc);
      row(2 * py + 1, acc);
#pragma unroll
      for (int j = 0; j < NB - PW; ++j) outv[j] = outv[j + PW];
#pragma unroll
      for (int px = 0; px < PW; ++px) outv[NB - PW + px] = acc[px] * 0.25f;  // count 4: / 4 == * 0.25
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int j = 0; j < NB; ++j) ob[lane * NB + j] = outv[j];  // stride NB (odd): no bank conflicts
  } else {
    for (int py = 0; py < PH; ++py) {
      float acc[PW];
#pragma unroll
      for (int px = 0; px < PW; ++px) acc[px] = 0.0f;
      row(2 * py, acc);
      row(2 * py + 1, acc);
#pragma unroll
      for (int px = 0; px < PW; ++px) ob[lane * NB + py * PW + px] = acc[px] * 0.25f;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (kStamp) t_eval = (int64_t)__builtin_amdgcn_s_memrealtime();
  const float4* s4 = reinterpret_cast<const float4*>(ob);
  for (int e = lane; e < kNhwcGroup * NB / 4; e += kWave) {
    const float4 q = s4[e];
    __builtin_amdgcn_raw_buffer_store_b128(
        u32x4{__float_as_uint(q.x), __float_as_uint(q.y), __float_as_uint(q.z), __float_as_uint(q.w)}, orr, e * 16, 0,
        kStAux);
  }
  if (kStamp && lane == 0) {
    int64_t* st = reinterpret_cast<int64_t*>(out + c.K * c.C * NB) + (int64_t)w * 8;
    st[0] = t_start;
    st[1] = t_pro;
    st[2] = t_land;
    st[3] = t_eval;
    st[4] = (int64_t)__builtin_amdgcn_s_memrealtime();
    st[5] = n_bands;
    st[6] = first_cells;
    st[7] = blockIdx.x & 7;
  }
}

// channels-last features: unit channel stride, 16-B aligned cells, 64-channel groups
static inline bool nhwc_ok(const RoiLevels& lv, int32_t channels, int32_t ph, int32_t pw, int32_t sr) {
  if (sr != 2 || ph != 7 || pw != 7 || channels % kNhwcGroup != 0) return false;
  for (int l = 0; l < lv.L; ++l) {
    const int64_t ext = ((int64_t)(lv.h[l] - 1) * lv.sy[l] + (int64_t)(lv.w[l] - 1) * lv.sx[l] + channels) * 4;
    if (lv.sc[l] != 1 || lv.sx[l] < channels || lv.sy[l] < lv.sx[l] || lv.sx[l] % 4 || lv.sy[l] % 4 ||
        lv.sb[l] % 4 || (reinterpret_cast<uintptr_t>(lv.feat[l]) & 15) || ext >= ((int64_t)1 << 31))
      return false;
  }
  return true;
}

}  // namespace frh
