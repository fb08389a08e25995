// BFP neck (Libra R-CNN's balanced feature pyramid, refine_type=None), forward and backward.
// Reference: lib/necks.py:93-141 (BFP.forward):
//   uniform_i = adaptive_max_pool2d(feats[i], size_r)        for i < r (finer levels)
//             = interpolate(feats[i], size_r, 'nearest')     for i > r (coarser levels)
//   refine    = sum(uniform_i, i != r) / (num_levels - 1)    (Python sum: 0 + u_0 + u_1 + ...)
//   out[i]    = feats[i] + interpolate(refine, size_i, 'nearest')      for i < r
//             = feats[i] + adaptive_max_pool2d(refine, size_i)         for i > r
//             = feats[i] + refine                                       for i = r
// The reference runs 2 (L - 1) resampling passes, L - 2 adds, a divide and L adds, each a
// read + write of a whole map.  Here the forward is two launches: the gather writes the
// refine map from every other level (one read of each), the scatter writes every output
// level (one read of the level, the small refine map from L2, one write).  Max and nearest
// are selections and the mean is the reference's adds in its order followed by one f32
// divide, so the outputs are bit-identical to the reference's CPU result.
//
// Index rules (torch's): adaptive window of output o is [floor(o*in/out), ceil((o+1)*in/out));
// nearest source of destination d is min(floor(d * (float)in / out), in - 1).  They are
// computed in the kernels (the row part from blockIdx, i.e. on the scalar unit): no tables,
// no workspace, nothing but launches on the stream.
//
// Maximum: torch's CPU scan, row-major over the window, `val > max || isnan(val)` (the first
// maximum wins, a NaN replaces anything).  With `argmax` given the winning cell's y*W + x is
// stored (int32, channels-last like the map it belongs to) for the backward: about 1/16 of
// level 0's bytes per finer level, against re-reading every finer level to recompute it.
//
// Backward (deterministic, no atomics): both adjoints are written as gathers.
//   launch 1, per refine cell: g = gout[r] + sum over the cells of the finer outputs whose
//     nearest source it is + sum over the coarser outputs' windows that contain it and whose
//     stored argmax it is; stores g / (L - 1), the gradient of the level sum.
//   launch 2, per cell of every level but r: gin = gout + (finer: the sum over the refine
//     windows that contain the cell and chose it; coarser: the sum over the refine cells
//     whose nearest source it is).  grad feats[r] = gout[r] (the caller's, no pass).
// Adaptive windows overlap when the sizes do not divide, so a cell can be the argmax of up to
// two windows per axis; nearest pre-images are contiguous ranges (the rule is monotone).
// Each sum runs in a fixed order.
//
// Layout: inputs through explicit (b, c, y, x) element strides (NHWC from the FPN, its
// stride-2 view of the last level, NCHW); every output is NHWC contiguous.  Lanes run along
// the channels: 16 B per lane when channels % 4 == 0 and the strides / pointers allow it,
// one float per lane otherwise.
#include <algorithm>

#include "common.h"

namespace frh {
namespace {

constexpr int kBfpThreads = 256;
constexpr int kBfpMaxSide = 32767;  // (o + 1) * in + out stays below 2^31

struct BfpMap {
  const float* p;
  int64_t sb, sc, sy, sx;
  int H, W;
};

struct BfpArgs {
  BfpMap in[FRH_MAX_LEVELS];      // forward: the input levels; backward: the upstream gradients
  float* out[FRH_MAX_LEVELS];     // NHWC contiguous: forward outputs / backward input gradients
  int64_t aoff[FRH_MAX_LEVELS];   // first element of level i's argmax map
  int row_off[FRH_MAX_LEVELS + 1];  // first (image, y) row of level i in the all-level launches
  int L, r, B, C;
  float div;                      // (float)(L - 1)
  float* refine;                  // [B, Hr, Wr, C]: the refine map / its scaled gradient
  int32_t* amax;                  // nullable in the forward
};

__device__ __forceinline__ int pool_start(int o, int in, int out) { return (int)(((uint32_t)o * (uint32_t)in) / (uint32_t)out); }
__device__ __forceinline__ int pool_end(int o, int in, int out) {
  return (int)(((uint32_t)(o + 1) * (uint32_t)in + (uint32_t)(out - 1)) / (uint32_t)out);
}
// windows o of an adaptive pool in -> out that contain input cell p: [first, last]
__device__ __forceinline__ int win_first(int p, int in, int out) { return (int)(((uint32_t)p * (uint32_t)out) / (uint32_t)in); }
__device__ __forceinline__ int win_last(int p, int in, int out) {
  const int o = (int)(((uint32_t)(p + 1) * (uint32_t)out - 1u) / (uint32_t)in);
  return o < out - 1 ? o : out - 1;
}
__device__ __forceinline__ int nearest_of(int dst, int in, int out) {
  const int s = (int)floorf((float)dst * ((float)in / (float)out));
  return s < in - 1 ? s : in - 1;
}
// destinations d in [0, out) whose nearest source is s: [*lo, *hi) (the rule is monotone in d)
__device__ __forceinline__ void nearest_preimage(int s, int in, int out, int* lo, int* hi) {
  int d = (int)(((uint32_t)s * (uint32_t)out) / (uint32_t)in);
  d = d < out ? d : out;
  while (d > 0 && nearest_of(d - 1, in, out) >= s) --d;
  while (d < out && nearest_of(d, in, out) < s) ++d;
  *lo = d;
  while (d < out && nearest_of(d, in, out) == s) ++d;
  *hi = d;
}

template <int V>
struct Vf {
  float v[V];
};
template <int V>
__device__ __forceinline__ Vf<V> ldv(const float* p) {
  Vf<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void stv(float* p, const Vf<V>& r) {
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else
    *p = r.v[0];
}
template <int V>
struct Vi {
  int32_t v[V];
};
template <int V>
__device__ __forceinline__ Vi<V> ldi(const int32_t* p) {
  Vi<V> r;
  if constexpr (V == 4) {
    const int4 t = *reinterpret_cast<const int4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void sti(int32_t* p, const Vi<V>& r) {
  if constexpr (V == 4)
    *reinterpret_cast<int4*>(p) = make_int4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else
    *p = r.v[0];
}

__device__ __forceinline__ const float* at(const BfpMap& m, int b, int c, int y, int x) {
  return m.p + (int64_t)b * m.sb + (int64_t)c * m.sc + (int64_t)y * m.sy + (int64_t)x * m.sx;
}
__device__ __forceinline__ int64_t nhwc(int b, int H, int W, int C, int y, int x, int c) {
  return (((int64_t)b * H + y) * W + x) * C + c;
}

// max over the window [y0, y1) x [x0, x1) of m at channels c..c+V-1, torch's CPU scan
template <int V>
__device__ __forceinline__ void window_max(const BfpMap& m, int b, int c, int y0, int y1, int x0, int x1, Vf<V>* best,
                                           Vi<V>* arg) {
#pragma unroll
  for (int k = 0; k < V; ++k) best->v[k] = -INFINITY, arg->v[k] = y0 * m.W + x0;
  for (int iy = y0; iy < y1; ++iy)
    for (int ix = x0; ix < x1; ++ix) {
      const Vf<V> val = ldv<V>(at(m, b, c, iy, ix));
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (val.v[k] > best->v[k] || isnan(val.v[k])) best->v[k] = val.v[k], arg->v[k] = iy * m.W + ix;
    }
}

// grid (x blocks, rows): row = (image, y) of the refine level
template <int V>
__global__ void __launch_bounds__(kBfpThreads) bfp_gather_kernel(BfpArgs a) {
  const int Hr = a.in[a.r].H, Wr = a.in[a.r].W, CV = a.C / V;
  for (int row = blockIdx.y; row < a.B * Hr; row += gridDim.y) {
    const int b = row / Hr, y = row - b * Hr;
    for (int q = blockIdx.x * kBfpThreads + threadIdx.x; q < Wr * CV; q += gridDim.x * kBfpThreads) {
      const int x = q / CV, c = (q - x * CV) * V;
      Vf<V> s;
#pragma unroll
      for (int k = 0; k < V; ++k) s.v[k] = 0.0f;
      for (int i = 0; i < a.L; ++i) {
        if (i == a.r) continue;
        const BfpMap& m = a.in[i];
        Vf<V> u;
        if (i < a.r) {
          Vi<V> arg;
          window_max<V>(m, b, c, pool_start(y, m.H, Hr), pool_end(y, m.H, Hr), pool_start(x, m.W, Wr),
                        pool_end(x, m.W, Wr), &u, &arg);
          if (a.amax) sti<V>(a.amax + a.aoff[i] + nhwc(b, Hr, Wr, a.C, y, x, c), arg);
        } else {
          u = ldv<V>(at(m, b, c, nearest_of(y, m.H, Hr), nearest_of(x, m.W, Wr)));
        }
#pragma unroll
        for (int k = 0; k < V; ++k) s.v[k] = s.v[k] + u.v[k];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) s.v[k] = s.v[k] / a.div;
      stv<V>(a.refine + nhwc(b, Hr, Wr, a.C, y, x, c), s);
    }
  }
}

// (level, image, y) of a row of the all-level launches; uniform per workgroup
__device__ __forceinline__ int row_level(const BfpArgs& a, int row, int* b, int* y) {
  int i = 0;
  while (i + 1 < a.L && row >= a.row_off[i + 1]) ++i;
  const int local = row - a.row_off[i];
  *b = local / a.in[i].H;
  *y = local - *b * a.in[i].H;
  return i;
}

// grid (x blocks, rows): row = (level, image, y) over every level
template <int V>
__global__ void __launch_bounds__(kBfpThreads) bfp_scatter_kernel(BfpArgs a) {
  const int Hr = a.in[a.r].H, Wr = a.in[a.r].W, CV = a.C / V;
  BfpMap ref{a.refine, (int64_t)Hr * Wr * a.C, 1, (int64_t)Wr * a.C, a.C, Hr, Wr};
  for (int row = blockIdx.y; row < a.row_off[a.L]; row += gridDim.y) {
    int b, y;
    const int i = row_level(a, row, &b, &y);
    const BfpMap& m = a.in[i];
    const int ys = i < a.r ? nearest_of(y, Hr, m.H) : pool_start(y, Hr, m.H), ye = pool_end(y, Hr, m.H);
    for (int q = blockIdx.x * kBfpThreads + threadIdx.x; q < m.W * CV; q += gridDim.x * kBfpThreads) {
      const int x = q / CV, c = (q - x * CV) * V;
      Vf<V> res;
      if (i < a.r) {
        res = ldv<V>(at(ref, b, c, ys, nearest_of(x, Wr, m.W)));
      } else if (i > a.r) {
        Vi<V> arg;
        window_max<V>(ref, b, c, ys, ye, pool_start(x, Wr, m.W), pool_end(x, Wr, m.W), &res, &arg);
        if (a.amax) sti<V>(a.amax + a.aoff[i] + nhwc(b, m.H, m.W, a.C, y, x, c), arg);
      } else {
        res = ldv<V>(at(ref, b, c, y, x));
      }
      const Vf<V> f = ldv<V>(at(m, b, c, y, x));
#pragma unroll
      for (int k = 0; k < V; ++k) res.v[k] = f.v[k] + res.v[k];
      stv<V>(a.out[i] + nhwc(b, m.H, m.W, a.C, y, x, c), res);
    }
  }
}

// backward launch 1: the gradient of the level sum, per refine cell (a.in = upstream gradients)
template <int V>
__global__ void __launch_bounds__(kBfpThreads) bfp_bwd_refine_kernel(BfpArgs a) {
  const int Hr = a.in[a.r].H, Wr = a.in[a.r].W, CV = a.C / V;
  for (int row = blockIdx.y; row < a.B * Hr; row += gridDim.y) {
    const int b = row / Hr, y = row - b * Hr;
    for (int q = blockIdx.x * kBfpThreads + threadIdx.x; q < Wr * CV; q += gridDim.x * kBfpThreads) {
      const int x = q / CV, c = (q - x * CV) * V;
      const int cell = y * Wr + x;
      Vf<V> g = ldv<V>(at(a.in[a.r], b, c, y, x));
      for (int i = 0; i < a.L; ++i) {
        if (i == a.r) continue;
        const BfpMap& m = a.in[i];
        if (i < a.r) {  // out[i] = .. + refine[nearest]: the cells this one is the source of
          int y0, y1, x0, x1;
          nearest_preimage(y, Hr, m.H, &y0, &y1);
          nearest_preimage(x, Wr, m.W, &x0, &x1);
          for (int dy = y0; dy < y1; ++dy)
            for (int dx = x0; dx < x1; ++dx) {
              const Vf<V> t = ldv<V>(at(m, b, c, dy, dx));
#pragma unroll
              for (int k = 0; k < V; ++k) g.v[k] += t.v[k];
            }
        } else {  // out[i] = .. + max over a refine window: the windows that chose this cell
          const int o0 = win_first(y, Hr, m.H), o1 = win_last(y, Hr, m.H);
          const int p0 = win_first(x, Wr, m.W), p1 = win_last(x, Wr, m.W);
          for (int oy = o0; oy <= o1; ++oy)
            for (int ox = p0; ox <= p1; ++ox) {
              const Vi<V> am = ldi<V>(a.amax + a.aoff[i] + nhwc(b, m.H, m.W, a.C, oy, ox, c));
              const Vf<V> t = ldv<V>(at(m, b, c, oy, ox));
#pragma unroll
              for (int k = 0; k < V; ++k) g.v[k] += am.v[k] == cell ? t.v[k] : 0.0f;
            }
        }
      }
#pragma unroll
      for (int k = 0; k < V; ++k) g.v[k] = g.v[k] / a.div;
      stv<V>(a.refine + nhwc(b, Hr, Wr, a.C, y, x, c), g);
    }
  }
}

// backward launch 2: the input gradients of every level but r (row_off skips level r)
template <int V>
__global__ void __launch_bounds__(kBfpThreads) bfp_bwd_levels_kernel(BfpArgs a) {
  const int Hr = a.in[a.r].H, Wr = a.in[a.r].W, CV = a.C / V;
  for (int row = blockIdx.y; row < a.row_off[a.L]; row += gridDim.y) {
    int b, y;
    const int i = row_level(a, row, &b, &y);
    const BfpMap& m = a.in[i];
    int y0, y1;  // finer: refine windows containing y [y0, y1]; coarser: refine rows with source y [y0, y1)
    if (i < a.r)
      y0 = win_first(y, m.H, Hr), y1 = win_last(y, m.H, Hr) + 1;
    else
      nearest_preimage(y, m.H, Hr, &y0, &y1);
    for (int q = blockIdx.x * kBfpThreads + threadIdx.x; q < m.W * CV; q += gridDim.x * kBfpThreads) {
      const int x = q / CV, c = (q - x * CV) * V;
      const int cell = y * m.W + x;
      Vf<V> g = ldv<V>(at(m, b, c, y, x));
      int x0, x1;
      if (i < a.r)
        x0 = win_first(x, m.W, Wr), x1 = win_last(x, m.W, Wr) + 1;
      else
        nearest_preimage(x, m.W, Wr, &x0, &x1);
      for (int ry = y0; ry < y1; ++ry)
        for (int rx = x0; rx < x1; ++rx) {
          const int64_t o = nhwc(b, Hr, Wr, a.C, ry, rx, c);
          const Vf<V> t = ldv<V>(a.refine + o);
          if (i < a.r) {
            const Vi<V> am = ldi<V>(a.amax + a.aoff[i] + o);
#pragma unroll
            for (int k = 0; k < V; ++k) g.v[k] += am.v[k] == cell ? t.v[k] : 0.0f;
          } else {
#pragma unroll
            for (int k = 0; k < V; ++k) g.v[k] += t.v[k];
          }
        }
      stv<V>(a.out[i] + nhwc(b, m.H, m.W, a.C, y, x, c), g);
    }
  }
}

// argmax maps: finer levels at the refine level's size, then the coarser levels at their own
int64_t bfp_argmax_layout(int L, int r, int B, int C, const int32_t* hw, int64_t* aoff) {
  const int64_t per_ref = (int64_t)B * hw[2 * r] * hw[2 * r + 1] * C;
  int64_t off = 0;
  for (int i = 0; i < L; ++i) {
    if (i == r) continue;
    if (aoff) aoff[i] = off;
    off += i < r ? per_ref : (int64_t)B * hw[2 * i] * hw[2 * i + 1] * C;
  }
  return off;
}

int32_t bfp_setup(const char* what, int32_t L, int32_t r, int32_t B, int32_t C, const void* const* maps,
                  const int32_t* hw, const int64_t* strides, void* const* outs, bool skip_r, const float* refine,
                  const int32_t* amax, int64_t amax_elems, BfpArgs* a, int* vec, int* max_w) {
  FRH_REQUIRE(L >= 2 && L <= FRH_MAX_LEVELS, "%s: num_levels must be in [2, %d]", what, FRH_MAX_LEVELS);
  FRH_REQUIRE(r >= 0 && r < L, "%s: refine_level out of range", what);
  FRH_REQUIRE(B >= 1 && C >= 1, "%s: bad batch / channels", what);
  FRH_REQUIRE(maps && hw && strides && outs && refine, "%s: null pointer argument", what);
  int v = C % 4 == 0 && (uintptr_t)refine % 16 == 0 && (uintptr_t)amax % 16 == 0;
  int64_t rows = 0;
  *max_w = 0;
  for (int i = 0; i < L; ++i) {
    const int H = hw[2 * i], W = hw[2 * i + 1];
    FRH_REQUIRE(H >= 1 && W >= 1 && H <= kBfpMaxSide && W <= kBfpMaxSide, "%s: level %d size out of range", what, i);
    FRH_REQUIRE(maps[i] && (outs[i] || (skip_r && i == r)), "%s: null level %d", what, i);
    const int64_t* s = strides + 4 * i;
    a->in[i] = BfpMap{static_cast<const float*>(maps[i]), s[0], s[1], s[2], s[3], H, W};
    a->out[i] = static_cast<float*>(outs[i]);
    v = v && s[1] == 1 && s[0] % 4 == 0 && s[2] % 4 == 0 && s[3] % 4 == 0 &&
        ((uintptr_t)maps[i] | (uintptr_t)outs[i]) % 16 == 0;
    a->row_off[i] = (int)rows;
    if (!(skip_r && i == r)) {
      rows += (int64_t)B * H;
      *max_w = std::max(*max_w, W);
    }
    FRH_REQUIRE(rows <= INT32_MAX && (int64_t)B * H * W * C <= ((int64_t)1 << 40), "%s: too many cells", what);
  }
  a->row_off[L] = (int)rows;
  const int64_t need = bfp_argmax_layout(L, r, B, C, hw, a->aoff);
  FRH_REQUIRE(!amax || amax_elems >= need, "%s: argmax buffer too small (%lld < %lld)", what, (long long)amax_elems,
              (long long)need);
  a->L = L, a->r = r, a->B = B, a->C = C;
  a->div = (float)(L - 1);
  a->refine = const_cast<float*>(refine);
  a->amax = const_cast<int32_t*>(amax);
  *vec = v;
  return FRH_OK;
}

dim3 bfp_grid(int width, int cv, int64_t rows) {
  const int64_t bx = ((int64_t)width * cv + kBfpThreads - 1) / kBfpThreads;
  return dim3((unsigned)std::min<int64_t>(std::max<int64_t>(bx, 1), 64), (unsigned)std::min<int64_t>(rows, 65535));
}

}  // namespace
}  // namespace frh

using namespace frh;

extern "C" size_t frh_bfp_argmax_elems(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                                        const int32_t* level_hw) {
  if (num_levels < 2 || num_levels > FRH_MAX_LEVELS || refine_level < 0 || refine_level >= num_levels || !level_hw)
    return 0;
  return (size_t)bfp_argmax_layout(num_levels, refine_level, batch, channels, level_hw, nullptr);
}

extern "C" int32_t frh_bfp_fwd(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                               const void* const* feats, const int32_t* level_hw, const int64_t* level_strides,
                               float* refine, void* const* outs, int32_t* argmax, int64_t argmax_elems, void* stream) {
  BfpArgs a;
  int vec, max_w;
  const int32_t st = bfp_setup("frh_bfp_fwd", num_levels, refine_level, batch, channels, feats, level_hw,
                               level_strides, outs, false, refine, argmax, argmax_elems, &a, &vec, &max_w);
  if (st != FRH_OK) return st;
  const int cv = vec ? channels / 4 : channels;
  const dim3 g1 = bfp_grid(level_hw[2 * refine_level + 1], cv, (int64_t)batch * level_hw[2 * refine_level]);
  const dim3 g2 = bfp_grid(max_w, cv, a.row_off[num_levels]);
  hipStream_t s = as_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(bfp_gather_kernel<4>, g1, dim3(kBfpThreads), 0, s, a);
    hipLaunchKernelGGL(bfp_scatter_kernel<4>, g2, dim3(kBfpThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(bfp_gather_kernel<1>, g1, dim3(kBfpThreads), 0, s, a);
    hipLaunchKernelGGL(bfp_scatter_kernel<1>, g2, dim3(kBfpThreads), 0, s, a);
  }
  return check_launch("frh_bfp_fwd");
}

extern "C" int32_t frh_bfp_bwd(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                               const void* const* grad_outs, const int32_t* level_hw, const int64_t* grad_strides,
                               const int32_t* argmax, int64_t argmax_elems, float* grad_refine,
                               void* const* grad_feats, void* stream) {
  BfpArgs a;
  int vec, max_w;
  FRH_REQUIRE(argmax, "frh_bfp_bwd: null argmax");
  const int32_t st = bfp_setup("frh_bfp_bwd", num_levels, refine_level, batch, channels, grad_outs, level_hw,
                               grad_strides, grad_feats, true, grad_refine, argmax, argmax_elems, &a, &vec, &max_w);
  if (st != FRH_OK) return st;
  const int cv = vec ? channels / 4 : channels;
  const dim3 g1 = bfp_grid(level_hw[2 * refine_level + 1], cv, (int64_t)batch * level_hw[2 * refine_level]);
  const dim3 g2 = bfp_grid(max_w, cv, a.row_off[num_levels]);
  hipStream_t s = as_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(bfp_bwd_refine_kernel<4>, g1, dim3(kBfpThreads), 0, s, a);
    hipLaunchKernelGGL(bfp_bwd_levels_kernel<4>, g2, dim3(kBfpThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(bfp_bwd_refine_kernel<1>, g1, dim3(kBfpThreads), 0, s, a);
    hipLaunchKernelGGL(bfp_bwd_levels_kernel<1>, g2, dim3(kBfpThreads), 0, s, a);
  }
  return check_launch("frh_bfp_bwd");
}
