// Candidate selection of the one-stage heads' inference for all (image, level) segments at once.
// Reference: lib/heads/fcos_head.py:570-621 (FCOS, FCOS-ATSS, GFL: decode, clamp, min-size
// filter, then top-k by (centerness x) best class score) and lib/heads/anchor_head.py:207-250
// (RetinaNet: top-k by best class score, decode, min-size mask).
//
// One memset and four launches, whatever B, L and C (seg_topk.h's multi-launch form; no
// workgroup waits on another):
//  1. keys    : per column the key max_c sigmoid(cls_c) (x sigmoid(ctr)) as (f32 bits + 1) << 2,
//               0 for a column the LTRB / DFL min-size filter drops, + first-level histogram.
//               Channels-last maps: lanes along the channels of a cell, reduced across the wave;
//               other layouts: lanes along columns, a loop over the channels.
//  2. refine, 3. collect : the k_l largest keys per segment, ties to the lowest column.
//  4. gather  : every workgroup orders its segment's records (key desc, column asc) in LDS and
//               writes its slice of the rows: box, every class score, factor, valid, column.
// The DFL expectation sums its bins in one fixed tree order in every path, so the outputs do
// not depend on the layout of the inputs.
#include <math.h>

#include "loss_common.h"
#include "seg_topk.h"

namespace frh {
namespace {

constexpr int kDcHistBits = 12;
constexpr int kDcMaxSort = 16384;  // records ordered in LDS per segment
constexpr int kDcMaxBins = kWave / 4;
constexpr int kDcCellsPerWg = 256;  // channels-last keys: 64 cells per wave
constexpr int kDcCellsPerIt = 8;    // ... 8 of them in flight
constexpr int kDcTile = 256;        // gather: rows per pass

struct DcArgs {
  const float* cls[FRH_MAX_LEVELS];
  const float* reg[FRH_MAX_LEVELS];
  const float* ctr[FRH_MAX_LEVELS];
  int64_t cst[FRH_MAX_LEVELS][4], rst[FRH_MAX_LEVELS][4], tst[FRH_MAX_LEVELS][4];  // element strides (b, c, y, x)
  int64_t aoff[FRH_MAX_LEVELS];  // first anchor column of the level (DELTA)
  int32_t h[FRH_MAX_LEVELS], w[FRH_MAX_LEVELS];
  int32_t k[FRH_MAX_LEVELS], row0[FRH_MAX_LEVELS];  // rows of the level and their first output row
  float cell[FRH_MAX_LEVELS];
  int L, A, C, mode, bins, has_ctr;
  const float* anchors;
  int64_t anchor_ld;
  float m[4], sd[4];
  float reg_std, reg_mean;
  double dfl_stride;
  int P;          // largest k_l: the record row length
  int64_t cap;    // output rows per image
  uint64_t* rec;  // [S][P] selection records key << 32 | ~column
  float* boxes;
  float* scores;
  float* factor;
  uint8_t* valid;
  int32_t* index;
};

struct DcImg {
  float hw[2 * 64];
  float min_size[64];
};

__device__ __forceinline__ int64_t dc_elem(const int64_t (&st)[4], int b, int ch, int y, int x) {
  return (int64_t)b * st[0] + (int64_t)ch * st[1] + (int64_t)y * st[2] + (int64_t)x * st[3];
}

// column i = a*H*W + y*W + x of a level
__device__ __forceinline__ void dc_column(int H, int W, int i, int* a, int* y, int* x) {
  const uint32_t hw = (uint32_t)H * (uint32_t)W, u = (uint32_t)i, aa = u / hw, sp = u - aa * hw;
  const uint32_t yy = sp / (uint32_t)W;
  *a = (int)aa;
  *y = (int)yy;
  *x = (int)(sp - yy * (uint32_t)W);
}

// scores are >= 0: their bits order like the values; + 1 keeps a zero score a candidate
__device__ __forceinline__ uint32_t dc_key(float s) { return (__float_as_uint(s) + 1u) << 2; }

// sum of 16 values in the order of a wave butterfly over the bin bits
__device__ __forceinline__ float dc_tree16(float (&t)[kDcMaxBins]) {
#pragma unroll
  for (int o = 1; o < kDcMaxBins; o <<= 1)
#pragma unroll
    for (int k = 0; k < kDcMaxBins; k += 2 * o) t[k] = t[k] + t[k + o];
  return t[0];
}

// ltrb2bbox + clamp_bbox of one side (fcos_head.py:66-71, frh_dfl_decode's decode_coord)
__device__ __forceinline__ float dc_coord(int side, float ltrb, int y, int x, float cell, float xmax, float ymax) {
  const float ctr = (float)((side & 1) ? y : x) * cell + cell / 2.0f;
  const float v = side < 2 ? ctr - ltrb : ltrb + ctr;
  return fminf(fmaxf(v, 0.0f), (side & 1) ? ymax : xmax);
}

// LTRB / DFL box of cell (y, x) of level l, image b
__device__ float4 dc_ltrb_box(const DcArgs& p, const DcImg& ia, int l, int b, int y, int x) {
  const float* reg = p.reg[l] + dc_elem(p.rst[l], b, 0, y, x);
  const int64_t sc = p.rst[l][1];
  float len[4];
  if (p.mode == FRH_DENSE_LTRB) {
#pragma unroll
    for (int s = 0; s < 4; ++s) len[s] = reg[s * sc];
  } else {
#pragma unroll 1  // one side at a time: all four unrolled cost 60 more VGPRs (occupancy 4 -> 2) in every mode
    for (int s = 0; s < 4; ++s) {
      float v[kDcMaxBins];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < kDcMaxBins; ++k) {
        v[k] = k < p.bins ? reg[(k * 4 + s) * sc] : -INFINITY;
        mx = fmaxf(mx, v[k]);
      }
      float e[kDcMaxBins], t[kDcMaxBins];
#pragma unroll
      for (int k = 0; k < kDcMaxBins; ++k) t[k] = e[k] = k < p.bins ? expf(v[k] - mx) : 0.0f;
      const float sum = dc_tree16(t);
#pragma unroll
      for (int k = 0; k < kDcMaxBins; ++k) t[k] = (e[k] / sum) * (float)((double)k * p.dfl_stride);
      len[s] = dc_tree16(t);
    }
  }
  const float xmax = ia.hw[2 * b + 1] - 1.0f, ymax = ia.hw[2 * b] - 1.0f;
  float c[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) c[s] = dc_coord(s, len[s] * p.reg_std + p.reg_mean, y, x, p.cell[l], xmax, ymax);
  return make_float4(c[0], c[1], c[2], c[3]);
}

// param2bbox + clamp of column i = (a, y, x) (utils.py:83-144, frh_param2bbox's arithmetic)
__device__ float4 dc_delta_box(const DcArgs& p, const DcImg& ia, int l, int b, int i, int a, int y, int x) {
  const int64_t ai = p.aoff[l] + i, ld = p.anchor_ld;
  const float* an = p.anchors;
  const float ax1 = an[ai], ay1 = an[ld + ai], ax2 = an[2 * ld + ai], ay2 = an[3 * ld + ai];
  float d[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) d[q] = p.reg[l][dc_elem(p.rst[l], b, q * p.A + a, y, x)];
  const float tx = d[0] * p.sd[0] + p.m[0];
  const float ty = d[1] * p.sd[1] + p.m[1];
  const float tw = d[2] * p.sd[2] + p.m[2];
  const float th = d[3] * p.sd[3] + p.m[3];
  const float bw = (ax2 - ax1) + 1.0f, bh = (ay2 - ay1) + 1.0f;
  const float bcx = (ax2 + ax1) / 2.0f, bcy = (ay2 + ay1) / 2.0f;
  const float cx = tx * bw + bcx, cy = ty * bh + bcy;
  const float ww = expf(tw) * bw, hh = expf(th) * bh;
  const float hw2 = ww / 2.0f, hh2 = hh / 2.0f;
  const float v[4] = {cx - hw2, cy - hh2, cx + hw2, cy + hh2};
  const float img_h = ia.hw[2 * b], img_w = ia.hw[2 * b + 1];
  const float hi[4] = {img_w - 1.0f, img_h - 1.0f, img_w - 1.0f, img_h - 1.0f};
  float box[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float c = (v[q] < 0.0f) ? 0.0f : v[q];
    box[q] = (c > hi[q]) ? hi[q] : c;
  }
  return make_float4(box[0], box[1], box[2], box[3]);
}

// fcos_head.py:600-603: strictly larger than min_size on both sides
__device__ __forceinline__ bool dc_ltrb_keeps(float4 bx, float min_size) {
  return (((bx.z - bx.x) + 1.0f) > min_size) && (((bx.w - bx.y) + 1.0f) > min_size);
}
// anchor_head.py:243-246: the mask applied after the decode, only when min_size > 0
__device__ __forceinline__ bool dc_delta_keeps(float4 bx, float min_size) {
  return !(min_size > 0.0f) || ((((bx.z - bx.x) + 1.0f) >= min_size) && (((bx.w - bx.y) + 1.0f) >= min_size));
}

// The key of column (a, y, x) from its best class score: x centerness, 0 when the LTRB / DFL
// min-size filter drops the column.
__device__ __forceinline__ uint32_t dc_finish_key(const DcArgs& p, const DcImg& ia, int l, int b, int y, int x,
                                                  float best) {
  float s = best;
  if (p.has_ctr) s = s * sigmoidf(p.ctr[l][dc_elem(p.tst[l], b, 0, y, x)]);
  if (p.mode != FRH_DENSE_DELTA && !dc_ltrb_keeps(dc_ltrb_box(p, ia, l, b, y, x), ia.min_size[b])) return 0u;
  return dc_key(s);
}

// whether level l's class map is read with lanes along channels
__host__ __device__ inline bool dc_chan_path(const DcArgs& p, int l) {
  return p.cst[l][1] == 1 && p.C * p.A > 1 && p.A <= kWave;
}
__host__ __device__ inline int dc_key_groups(const DcArgs& p, int l) {
  const int64_t hw = (int64_t)p.h[l] * p.w[l];
  return dc_chan_path(p, l) ? (int)((hw + kDcCellsPerWg - 1) / kDcCellsPerWg)
                            : (int)((hw * p.A + kTkChunk - 1) / kTkChunk);
}

// Grid (key groups, segments).
__global__ void __launch_bounds__(kTkThreads) dc_keys_kernel(DcArgs p, DcImg ia, TkBufs tb) {
  __shared__ uint32_t hist[1 << kDcHistBits];
  __shared__ uint32_t lm[kTkThreads / kWave][kDcCellsPerIt][kWave];
  const int seg = blockIdx.y, t = threadIdx.x;
  const int b = seg / p.L, l = seg % p.L;
  const int H = p.h[l], W = p.w[l], hw = H * W, n = p.A * hw;
  if ((int)blockIdx.x >= dc_key_groups(p, l)) return;  // workgroup-uniform
  tk_hist1_clear(hist, 1 << kDcHistBits);
  uint32_t* kk = const_cast<uint32_t*>(tb.keys) + (int64_t)seg * tb.ld;
  const float* cls = p.cls[l];
  const int64_t csc = p.cst[l][1];
  if (!dc_chan_path(p, l)) {
    // lanes along columns: 16 columns per thread, their loads of a channel in flight together
    const int base = (int)blockIdx.x * kTkChunk;
    int64_t off[kTkPerThread];
    float best[kTkPerThread];
#pragma unroll
    for (int r = 0; r < kTkPerThread; ++r) {
      const int i = base + r * kTkThreads + t;
      int a = 0, y = 0, x = 0;
      if (i < n) dc_column(H, W, i, &a, &y, &x);
      off[r] = dc_elem(p.cst[l], b, a, y, x);
      best[r] = 0.0f;
    }
    for (int c = 0; c < p.C; ++c) {
      float v[kTkPerThread];
#pragma unroll
      for (int r = 0; r < kTkPerThread; ++r)
        v[r] = base + r * kTkThreads + t < n ? cls[off[r] + (int64_t)c * p.A * csc] : 0.0f;
#pragma unroll
      for (int r = 0; r < kTkPerThread; ++r) best[r] = fmaxf(best[r], sigmoidf(v[r]));
    }
#pragma unroll 1
    for (int r = 0; r < kTkPerThread; ++r) {
      const int i = base + r * kTkThreads + t;
      uint32_t key = 0u;
      if (i < n) {
        int a, y, x;
        dc_column(H, W, i, &a, &y, &x);
        key = dc_finish_key(p, ia, l, b, y, x, best[r]);
        kk[i] = key;
      }
      tk_hist_add(hist, key != 0u, key >> (32 - kDcHistBits));
    }
  } else {
    // lanes along the C*A contiguous channels of a cell, 8 cells of the wave in flight; lane j
    // always holds anchor j % A (passes advance by a multiple of A)
    const int lane = lane_id(), wave = t / kWave;
    const int CA = p.C * p.A, step = (kWave / p.A) * p.A;
    const int cell0 = (int)blockIdx.x * kDcCellsPerWg + wave * kWave;
    uint32_t mine = 0u;  // A == 1: the best score bits of cell cell0 + lane
#pragma unroll 1
    for (int it = 0; it < kWave / kDcCellsPerIt; ++it) {
      int64_t off[kDcCellsPerIt];
      uint32_t lmax[kDcCellsPerIt];
#pragma unroll
      for (int u = 0; u < kDcCellsPerIt; ++u) {
        const int cell = min(cell0 + it * kDcCellsPerIt + u, hw - 1);
        const int y = cell / W, x = cell - y * W;
        off[u] = dc_elem(p.cst[l], b, 0, y, x);
        lmax[u] = 0u;
      }
      for (int ch0 = 0; ch0 < CA; ch0 += step) {
        const int ch = ch0 + lane;
        const bool ok = lane < step && ch < CA;
        float v[kDcCellsPerIt];
#pragma unroll
        for (int u = 0; u < kDcCellsPerIt; ++u) v[u] = ok ? cls[off[u] + ch] : 0.0f;
#pragma unroll
        for (int u = 0; u < kDcCellsPerIt; ++u) {
          const uint32_t sb = ok ? __float_as_uint(sigmoidf(v[u])) : 0u;
          lmax[u] = sb > lmax[u] ? sb : lmax[u];
        }
      }
      if (p.A == 1) {
#pragma unroll
        for (int u = 0; u < kDcCellsPerIt; ++u) {
          const uint32_t mx = wave_max_u32(lmax[u]);
          if (lane == it * kDcCellsPerIt + u) mine = mx;
        }
      } else {
        __syncthreads();  // lm free (every wave runs the same trip counts)
#pragma unroll
        for (int u = 0; u < kDcCellsPerIt; ++u) lm[wave][u][lane] = lmax[u];
        __syncthreads();
        const int items = kDcCellsPerIt * p.A;
        for (int q0 = 0; q0 < items; q0 += kWave) {
          const int q = q0 + lane, u = q / p.A, a = q - u * p.A;
          const int cell = cell0 + it * kDcCellsPerIt + u;
          const bool act = q < items && cell < hw;
          uint32_t key = 0u;
          if (act) {
            uint32_t mx = 0u;
            for (int j = a; j < step; j += p.A) mx = lm[wave][u][j] > mx ? lm[wave][u][j] : mx;
            const int y = cell / W, x = cell - y * W;
            key = dc_finish_key(p, ia, l, b, y, x, __uint_as_float(mx));
            kk[a * hw + cell] = key;
          }
          tk_hist_add(hist, key != 0u, key >> (32 - kDcHistBits));
        }
      }
    }
    if (p.A == 1) {
      const int cell = cell0 + lane;
      uint32_t key = 0u;
      if (cell < hw) {
        const int y = cell / W, x = cell - y * W;
        key = dc_finish_key(p, ia, l, b, y, x, __uint_as_float(mine));
        kk[cell] = key;
      }
      tk_hist_add(hist, key != 0u, key >> (32 - kDcHistBits));
    }
  }
  tk_hist1_flush(hist, 1 << kDcHistBits, tb.hist1 + (int64_t)seg * (1 << kDcHistBits));
}

// Top-k launches: grid (chunks of 4096, segments), 256 threads (seg_topk.h).
__global__ void __launch_bounds__(kTkThreads) dc_refine_kernel(DcArgs p, TkBufs tb) {
  __shared__ TkSmem sm;
  const int seg = blockIdx.y, l = seg % p.L;
  tk_refine_chunk(tb, seg, p.A * p.h[l] * p.w[l], p.k[l], sm);
}

struct DcPol {
  uint64_t* rec;
  int32_t* st;
  __device__ void select(int i, uint32_t key, int slot) {
    xwg_store(rec + slot, ((uint64_t)key << 32) | (uint32_t)~(uint32_t)i);
  }
  __device__ void finish(int kv) {
    if (threadIdx.x == 0) st[TK_K] = kv;  // the gather launch's count
  }
};

__global__ void __launch_bounds__(kTkThreads) dc_collect_kernel(DcArgs p, TkBufs tb) {
  __shared__ TkSmem sm;
  const int seg = blockIdx.y, l = seg % p.L;
  DcPol pol{p.rec + (int64_t)seg * p.P, tb.state + seg * TK_WORDS};
  tk_collect_chunk(tb, seg, p.A * p.h[l] * p.w[l], tk_plan_refined(tb, seg), pol, sm);
}

// Grid (row groups of `rows`, segments): every workgroup orders the segment's kv records in
// LDS and writes rows [x * rows, (x + 1) * rows) of the level's k_l.
__global__ void __launch_bounds__(kTkThreads) dc_gather_kernel(DcArgs p, DcImg ia, const int32_t* state, int rows) {
  extern __shared__ uint64_t skeys[];
  __shared__ int64_t roff[kDcTile];
  __shared__ int rlive[kDcTile];
  const int seg = blockIdx.y, t = threadIdx.x;
  const int b = seg / p.L, l = seg % p.L;
  const int k = p.k[l], r0 = (int)blockIdx.x * rows;
  if (r0 >= k) return;  // workgroup-uniform
  const int H = p.h[l], W = p.w[l];
  int kv = state[seg * TK_WORDS + TK_K];
  kv = kv < 0 ? 0 : (kv > k ? k : kv);
  const int P2 = next_pow2(kv > 1 ? kv : 1);
  const uint64_t* rec = p.rec + (int64_t)seg * p.P;
  for (int j = t; j < P2; j += kTkThreads) skeys[j] = j < kv ? rec[j] : 0ull;
  __syncthreads();
  if (kv > 1) block_bitonic_sort_desc(skeys, P2);
  const int rend = r0 + rows < k ? r0 + rows : k;
  const int64_t out0 = (int64_t)b * p.cap + p.row0[l];
  for (int tile = r0; tile < rend; tile += kDcTile) {
    const int j = tile + t;
    if (t < kDcTile && j < rend) {
      float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
      float fac = 0.0f;
      int idx = -1;
      int64_t off = 0;
      if (j < kv) {
        const int i = (int)~(uint32_t)skeys[j];
        int a, y, x;
        dc_column(H, W, i, &a, &y, &x);
        bool live = true;
        if (p.mode == FRH_DENSE_DELTA) {
          bx = dc_delta_box(p, ia, l, b, i, a, y, x);
          live = dc_delta_keeps(bx, ia.min_size[b]);
        } else {
          bx = dc_ltrb_box(p, ia, l, b, y, x);
        }
        if (live) {
          idx = i;
          off = dc_elem(p.cst[l], b, a, y, x);
          if (p.has_ctr) fac = sigmoidf(p.ctr[l][dc_elem(p.tst[l], b, 0, y, x)]);
        } else {
          bx = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      reinterpret_cast<float4*>(p.boxes)[out0 + j] = bx;
      if (p.factor) p.factor[out0 + j] = fac;
      p.valid[out0 + j] = idx >= 0 ? 1 : 0;
      p.index[out0 + j] = idx;
      roff[t] = off;
      rlive[t] = idx >= 0;
    }
    __syncthreads();
    const int nrow = rend - tile < kDcTile ? rend - tile : kDcTile;
    const int64_t cstep = (int64_t)p.A * p.cst[l][1];
    for (int e = t; e < nrow * p.C; e += kTkThreads) {
      const int r = e / p.C, c = e - r * p.C;
      const float v = rlive[r] ? sigmoidf(p.cls[l][roff[r] + c * cstep]) : 0.0f;
      p.scores[(out0 + tile + r) * p.C + c] = v;
    }
    __syncthreads();
  }
}

size_t dc_al(size_t v) { return (v + 255) & ~(size_t)255; }

struct DcLayout {
  int P;
  int64_t cap, nmax;
  size_t keys, cand, rec, zero, zero_bytes, total;
};

// k_l = min(pre_nms, n_l), n_l when pre_nms <= 0
int64_t dc_k(int64_t n, int32_t pre_nms) { return (pre_nms > 0 && pre_nms < n) ? pre_nms : n; }

DcLayout dc_layout(int32_t B, int32_t L, const int32_t* grid_hw, int32_t A, int32_t pre_nms) {
  DcLayout z{};
  z.P = 1;
  z.nmax = 1;
  for (int l = 0; l < L; ++l) {
    const int64_t n = (int64_t)A * grid_hw[2 * l] * grid_hw[2 * l + 1], k = dc_k(n, pre_nms);
    z.cap += k;
    if (k > z.P) z.P = (int)(k < (1 << 30) ? k : (1 << 30));
    if (n > z.nmax) z.nmax = n;
  }
  const size_t S = (size_t)B * L;
  z.keys = 0;
  z.cand = z.keys + dc_al(S * (size_t)z.nmax * sizeof(uint32_t));
  z.rec = z.cand + dc_al(S * (size_t)z.nmax * sizeof(uint64_t));
  z.zero = z.rec + dc_al(S * (size_t)z.P * sizeof(uint64_t));
  z.zero_bytes = tk_zero_bytes((int)S, kDcHistBits);
  z.total = z.zero + dc_al(z.zero_bytes);
  return z;
}

bool dc_shape_ok(int32_t B, int32_t L, const int32_t* grid_hw, int32_t A) {
  if (B < 1 || B > 64 || L < 1 || L > FRH_MAX_LEVELS || !grid_hw || A < 1) return false;
  for (int l = 0; l < L; ++l) {
    if (grid_hw[2 * l] < 1 || grid_hw[2 * l + 1] < 1) return false;
    if ((int64_t)A * grid_hw[2 * l] * grid_hw[2 * l + 1] >= ((int64_t)1 << 30)) return false;
  }
  return true;
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" size_t frh_dense_candidates_workspace(int32_t num_imgs, int32_t num_levels, const int32_t* grid_hw,
                                                 int32_t num_anchors, int32_t pre_nms) {
  if (!dc_shape_ok(num_imgs, num_levels, grid_hw, num_anchors)) return 0;
  return dc_layout(num_imgs, num_levels, grid_hw, num_anchors, pre_nms).total;
}

extern "C" int32_t frh_dense_candidates(int32_t num_imgs, int32_t num_levels, const float* const* cls_ptrs,
                                        const float* const* reg_ptrs, const float* const* ctr_ptrs,
                                        const int64_t* cls_strides, const int64_t* reg_strides,
                                        const int64_t* ctr_strides, const int32_t* grid_hw, int32_t num_anchors,
                                        int32_t num_classes, int32_t mode, const float* anchors, int64_t anchor_ld,
                                        const float* means, const float* stds, const float* cell_strides,
                                        int32_t bins, double dfl_stride, float reg_std, float reg_mean,
                                        const float* img_hw, const float* min_size, int32_t pre_nms,
                                        float* out_boxes, float* out_scores, float* out_factor, uint8_t* out_valid,
                                        int32_t* out_index, int64_t cap, void* workspace, size_t ws_bytes,
                                        void* stream) {
  FRH_REQUIRE(mode == FRH_DENSE_DELTA || mode == FRH_DENSE_LTRB || mode == FRH_DENSE_DFL,
              "dense candidates: unknown mode %d", mode);
  if (mode == FRH_DENSE_DFL && bins * 4 > kWave) {
    set_error("dense candidates: 4 * bins = %d exceeds one wave (64 lanes)", bins * 4);
    return FRH_EUNSUPPORTED;
  }
  FRH_REQUIRE(dc_shape_ok(num_imgs, num_levels, grid_hw, num_anchors),
              "dense candidates: bad shape (images %d in [1, 64], levels %d in [1, %d], anchors %d)", num_imgs,
              num_levels, FRH_MAX_LEVELS, num_anchors);
  FRH_REQUIRE(num_classes >= 1, "dense candidates: num_classes %d", num_classes);
  FRH_REQUIRE(cls_ptrs && reg_ptrs && cls_strides && reg_strides && img_hw && min_size && out_boxes && out_scores &&
                  out_valid && out_index,
              "dense candidates: null pointer argument");
  FRH_REQUIRE((ctr_ptrs != nullptr) == (out_factor != nullptr) && (!ctr_ptrs || ctr_strides),
              "dense candidates: centerness maps and the factor output come together");
  FRH_REQUIRE(!ctr_ptrs || num_anchors == 1, "dense candidates: centerness needs one column per cell");
  if (mode == FRH_DENSE_DELTA) {
    FRH_REQUIRE(anchors && means && stds, "dense candidates: DELTA needs anchors, means and stds");
  } else {
    FRH_REQUIRE(num_anchors == 1 && cell_strides, "dense candidates: LTRB / DFL need one column per cell and strides");
    FRH_REQUIRE(mode != FRH_DENSE_DFL || (bins >= 1 && dfl_stride > 0.0), "dense candidates: bad DFL bins / stride");
  }
  FRH_REQUIRE_ALIGNED16(out_boxes);
  const DcLayout z = dc_layout(num_imgs, num_levels, grid_hw, num_anchors, pre_nms);
  FRH_REQUIRE(z.P <= kDcMaxSort, "dense candidates: %d rows of one level exceed %d (set pre_nms)", z.P, kDcMaxSort);
  FRH_REQUIRE(cap == z.cap, "dense candidates: cap %lld, expected %lld", (long long)cap, (long long)z.cap);
  FRH_REQUIRE(workspace && ws_bytes >= z.total, "dense candidates: workspace too small");
  DcArgs p{};
  int64_t aoff = 0, row0 = 0;
  for (int l = 0; l < num_levels; ++l) {
    FRH_REQUIRE(cls_ptrs[l] && reg_ptrs[l] && (!ctr_ptrs || ctr_ptrs[l]), "dense candidates: null level %d", l);
    p.cls[l] = cls_ptrs[l];
    p.reg[l] = reg_ptrs[l];
    p.ctr[l] = ctr_ptrs ? ctr_ptrs[l] : nullptr;
    for (int q = 0; q < 4; ++q) {
      p.cst[l][q] = cls_strides[4 * l + q];
      p.rst[l][q] = reg_strides[4 * l + q];
      p.tst[l][q] = ctr_ptrs ? ctr_strides[4 * l + q] : 0;
    }
    p.h[l] = grid_hw[2 * l];
    p.w[l] = grid_hw[2 * l + 1];
    const int64_t n = (int64_t)num_anchors * p.h[l] * p.w[l];
    p.aoff[l] = aoff;
    aoff += n;
    p.k[l] = (int32_t)dc_k(n, pre_nms);
    p.row0[l] = (int32_t)row0;
    row0 += p.k[l];
    p.cell[l] = cell_strides ? cell_strides[l] : 0.0f;
    FRH_REQUIRE(mode == FRH_DENSE_DELTA || p.cell[l] > 0.0f, "dense candidates: stride must be positive");
  }
  FRH_REQUIRE(mode != FRH_DENSE_DELTA || anchor_ld >= aoff, "dense candidates: anchor_ld smaller than the columns");
  p.L = num_levels;
  p.A = num_anchors;
  p.C = num_classes;
  p.mode = mode;
  p.bins = bins;
  p.has_ctr = ctr_ptrs ? 1 : 0;
  p.anchors = anchors;
  p.anchor_ld = anchor_ld;
  for (int q = 0; q < 4; ++q) {
    p.m[q] = means ? means[q] : 0.0f;
    p.sd[q] = stds ? stds[q] : 1.0f;
  }
  p.reg_std = reg_std;
  p.reg_mean = reg_mean;
  p.dfl_stride = dfl_stride;
  p.P = z.P;
  p.cap = z.cap;
  char* ws = reinterpret_cast<char*>(workspace);
  p.rec = reinterpret_cast<uint64_t*>(ws + z.rec);
  p.boxes = out_boxes;
  p.scores = out_scores;
  p.factor = out_factor;
  p.valid = out_valid;
  p.index = out_index;
  DcImg ia{};
  for (int b = 0; b < num_imgs; ++b) {
    ia.hw[2 * b] = img_hw[2 * b];
    ia.hw[2 * b + 1] = img_hw[2 * b + 1];
    ia.min_size[b] = min_size[b];
  }
  const int S = num_imgs * num_levels;
  hipStream_t st = as_stream(stream);
  char* zb = ws + z.zero;
  TkBufs tb{reinterpret_cast<uint32_t*>(ws + z.keys), z.nmax, reinterpret_cast<uint32_t*>(zb), kDcHistBits,
            reinterpret_cast<uint32_t*>(zb + (size_t)S * (1 << kDcHistBits) * sizeof(uint32_t)),
            reinterpret_cast<int32_t*>(zb + (size_t)S * ((1 << kDcHistBits) + kTkBins2) * sizeof(uint32_t)),
            reinterpret_cast<uint64_t*>(ws + z.cand)};
  FRH_HIP(hipMemsetAsync(zb, 0, z.zero_bytes, st));
  int kg = 1;
  for (int l = 0; l < num_levels; ++l) {
    const int g = dc_key_groups(p, l);
    kg = g > kg ? g : kg;
  }
  const dim3 grid((unsigned)((z.nmax + kTkChunk - 1) / kTkChunk), (unsigned)S);
  hipLaunchKernelGGL(dc_keys_kernel, dim3((unsigned)kg, (unsigned)S), dim3(kTkThreads), 0, st, p, ia, tb);
  hipLaunchKernelGGL(dc_refine_kernel, grid, dim3(kTkThreads), 0, st, p, tb);
  hipLaunchKernelGGL(dc_collect_kernel, grid, dim3(kTkThreads), 0, st, p, tb);
  // rows per gather workgroup: at least 64, at most 16 workgroups per segment
  int rows = (z.P + 15) / 16;
  rows = rows < 64 ? 64 : rows;
  const size_t lds = (size_t)next_pow2(z.P) * sizeof(uint64_t);
  if (lds > 32768)
    FRH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dc_gather_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(dc_gather_kernel, dim3((unsigned)((z.P + rows - 1) / rows), (unsigned)S), dim3(kTkThreads), lds,
                     st, p, ia, tb.state, rows);
  return check_launch("frh_dense_candidates");
}
