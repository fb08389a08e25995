// TOOLS-ONLY: frh_conv3x3_nchw_bn_act with the kernel form chosen by the caller
// (tools/bench_conv3x3_nchw.py times every form per class to fill the product's table;
// tests/test_gpu_conv3x3_nchw.py and test_gpu_conv3x3_nchw_lds.py reach every form with it).
// Forms 0 .. kNwForms - 1 are the product's (conv3x3_nchw_kernels.h); the forms from kNwForms on
// are laboratory forms that lost at every class and are kept here to be measured again:
//   kNwForms + 0: U through LDS alone, NC = 2, TR = 4
//   kNwForms + 1: U through LDS and cin split in two, NC = 1, S = 2, TR = 2
//   kNwForms + 2: U through LDS alone, NC = 1, TR = 4
// U through LDS: the workgroup's TR waves of one cin range take TR consecutive 16-tile runs of
// the same NC channel blocks.  A chunk of 16 cin (four steps) is one LDS image [cin 16][quad 4]
// [cout 16 NC] of float4 (quad i = positions 4 i .. 4 i + 3), so a lane's A operands of a step
// are 4 NC ds_read_b128, 16 lanes reading 256 contiguous bytes and rows 256 or 512 bytes apart:
// conflict-free, as are the staging writes (8 lanes write 128 contiguous bytes;
// tools/lds_bank_sim.py --conv3x3-nchw).  Two ring stages, one barrier per chunk: while chunk c
// runs from one stage, chunk c + 1 goes global -> registers -> the other stage in two halves
// (loads ahead of steps 0 and 2, writes behind steps 1 and 3).  The patch is loaded two steps
// ahead.  The split, the masks and the epilogue are the product's.
#include "conv3x3_nchw_kernels.h"
#include "frcnn_tools.h"

namespace frh {

template <int NC, int S, int TR>
__global__ void __launch_bounds__(64 * S * TR, NC == 2 ? 1 : 2) conv3x3_nchw_lds_kernel(const Conv3x3NchwArgs a) {
  constexpr int NCO = 16 * NC;
  constexpr int kStage = 64 * NCO * 4;  // floats of one chunk's image
  constexpr int kRing = S * 2 * kStage;
  constexpr int kRed = S > 1 ? TR * (S - 1) * NCO * 64 : 0;
  constexpr int kLds = kRing > kRed ? kRing : kRed;
  static_assert(kLds > 0 && kLds * 4 <= 65536, "static LDS");
  __shared__ __attribute__((aligned(16))) float lds[kLds];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ks = wave % S, tr = wave / S;
  const int cbi = (int)blockIdx.x % a.cb;
  const int runs = a.total / a.cb;
  const int run = ((int)blockIdx.x / a.cb) * TR + tr;
  const bool live = run < runs;
  int rest = min(run, runs - 1);
  const int bxi = rest % a.bx;
  rest /= a.bx;
  const int byi = rest % a.by;
  const int64_t img = rest / a.by;

  const int q = lane >> 4, t = lane & 15;
  const int H = a.h, W = a.w, HW = H * W;
  const int c0 = (bxi * 16 + t) * 2;
  const bool ok_c = c0 < W, ok_l = c0 >= 1 && c0 - 1 < W, ok_r = c0 + 2 < W;
  const int cc = min(c0, W - 2), cl = min(max(c0 - 1, 0), W - 1), cr = min(c0 + 2, W - 1);
  uint32_t oc[4], ol[4], orr[4];
  bool rok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int iy = 2 * byi - 1 + r;
    rok[r] = iy >= 0 && iy < H;
    const int row = q * HW + min(max(iy, 0), H - 1) * W;
    oc[r] = (uint32_t)(row + cc) * 4u, ol[r] = (uint32_t)(row + cl) * 4u, orr[r] = (uint32_t)(row + cr) * 4u;
  }
  const char* xs = reinterpret_cast<const char*>(a.x + img * a.cin * HW);
  const int64_t xstep = (int64_t)16 * HW;

  // the wave's cin range in steps of 4: whole chunks of 16 cin, [s0, s1), possibly empty
  const int K4 = a.cin / 4;
  const int cpg = ((K4 + 3) / 4 + S - 1) / S;
  const int s0 = ks * cpg * 4;
  const int s1 = min(K4, s0 + cpg * 4);

  f32x4 acc[NC][16];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc)
#pragma unroll
    for (int p = 0; p < 16; ++p) acc[nc][p] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // the patch of step s (any step past the last loads the last: valid addresses, nobody reads it)
  auto load_patch = [&](NwPatch & P, int s) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t xp = uniform_rsrc(xs + min(s, K4 - 1) * xstep, xstep);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P.c[r] = nw_ld2(xp, oc[r]);
      P.l[r] = nw_ld1(xp, ol[r]);
      P.r[r] = nw_ld1(xp, orr[r]);
    }
  };
  // V = B^T d B of a landed patch, zero outside the plane
  auto transform = [&](const NwPatch& P, float* v) __attribute__((always_inline)) {
    float d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r][0] = rok[r] && ok_l ? P.l[r] : 0.0f;
      d[r][1] = rok[r] && ok_c ? P.c[r].x : 0.0f;
      d[r][2] = rok[r] && ok_c ? P.c[r].y : 0.0f;
      d[r][3] = rok[r] && ok_r ? P.r[r] : 0.0f;
    }
    float e[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      e[0][c] = d[0][c] - d[2][c];
      e[1][c] = d[1][c] + d[2][c];
      e[2][c] = d[2][c] - d[1][c];
      e[3][c] = d[1][c] - d[3][c];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i * 4 + 0] = e[i][0] - e[i][2];
      v[i * 4 + 1] = e[i][1] + e[i][2];
      v[i * 4 + 2] = e[i][2] - e[i][1];
      v[i * 4 + 3] = e[i][1] - e[i][3];
    }
  };
  auto mfmas = [&](const f32x4(&u)[NC][4], const float* v) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int nc = 0; nc < NC; ++nc)
        acc[nc][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[nc][p >> 2][p & 3], v[p], acc[nc][p], 0, 0, 0);
  };

  {
    // staging: thread j of the cin range's TR x 64 moves slots j, j + 64 TR, .. of each half
    constexpr int PH = NCO / (2 * TR);  // float4 per thread and half
    static_assert(PH >= 1 && PH * 2 * TR == NCO, "the chunk's halves divide among the threads");
    const int j = tr * 64 + lane;
    float* ring = lds + ks * 2 * kStage;
    f32x4 st[PH];
    // all of U; a row past cin lies past the descriptor's end and reads as zero
    const __amdgpu_buffer_rsrc_t ug = uniform_rsrc(a.u, (int64_t)a.cin * a.cout * 64);
    auto stage_load = [&](int chunk, int h) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < PH; ++m) {
        const int slot = h * 32 * NCO + m * TR * 64 + j;
        const int co = slot % NCO, i = (slot / NCO) % 4, ci = chunk * 16 + slot / (4 * NCO);
        st[m] = nw_ld4(ug, ci < a.cin ? (uint32_t)(((ci * a.cout + cbi * NCO + co) * 16 + i * 4) * 4) : 0x80000000u);
      }
    };
    auto stage_write = [&](int stg, int h) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < PH; ++m)
        *reinterpret_cast<f32x4*>(ring + stg * kStage + (h * 32 * NCO + m * TR * 64 + j) * 4) = st[m];
    };
    // step s = s0 + 4 ci + js from the landed patch `cur` and ring stage ci & 1; the patch of
    // step s + 2 into `nxt`; half `ldh` of chunk ci + 1 loaded ahead of the MFMAs, half `wrh`
    // written behind them (-1: neither)
    auto step = [&](const NwPatch& cur, NwPatch& nxt, int ci, int js, int ldh, int wrh) __attribute__((always_inline)) {
      const int s = s0 + 4 * ci + js;
      const bool on = s < s1, more = ci + 1 < cpg;
      f32x4 u[NC][4];
      float v[16];
      if (on) {
        const float* up = ring + (ci & 1) * kStage + (((4 * js + q) * 4) * NCO + t) * 4;
#pragma unroll
        for (int nc = 0; nc < NC; ++nc)
#pragma unroll
          for (int i = 0; i < 4; ++i) u[nc][i] = *reinterpret_cast<const f32x4*>(up + (i * NCO + nc * 16) * 4);
        transform(cur, v);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ldh >= 0 && more) stage_load(ks * cpg + ci + 1, ldh);
      load_patch(nxt, s + 2);
      __builtin_amdgcn_sched_barrier(0);
      if (on) mfmas(u, v);
      __builtin_amdgcn_sched_barrier(0);
      if (wrh >= 0 && more) stage_write((ci + 1) & 1, wrh);
    };

    NwPatch p0, p1, p2, p3;
    stage_load(ks * cpg, 0);
    stage_write(0, 0);
    stage_load(ks * cpg, 1);
    stage_write(0, 1);
    load_patch(p0, s0);
    load_patch(p1, s0 + 1);
    __syncthreads();
    for (int ci = 0; ci < cpg; ++ci) {
      step(p0, p2, ci, 0, 0, -1);
      step(p1, p3, ci, 1, -1, 0);
      step(p2, p0, ci, 2, 1, -1);
      step(p3, p1, ci, 3, -1, 1);
      __syncthreads();
    }
  }

  // Y = A^T M A of the wave's partial M: 16 NC values per lane (channel block, register i =
  // channel 4 q + i, then the 2 x 2 outputs)
  float o[NC][4][4];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t0[4], t1[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        t0[b] = (acc[nc][b][i] + acc[nc][4 + b][i]) + acc[nc][8 + b][i];
        t1[b] = (acc[nc][4 + b][i] - acc[nc][8 + b][i]) - acc[nc][12 + b][i];
      }
      o[nc][i][0] = (t0[0] + t0[1]) + t0[2];
      o[nc][i][1] = (t0[1] - t0[2]) - t0[3];
      o[nc][i][2] = (t1[0] + t1[1]) + t1[2];
      o[nc][i][3] = (t1[1] - t1[2]) - t1[3];
    }
  if constexpr (S > 1) {
    // the ring is free: every wave passed the barrier behind its last chunk
    float* red = lds + (tr * (S - 1) * NCO * 64 + lane);
    if (ks > 0) {
#pragma unroll
      for (int e = 0; e < NCO; ++e) red[((ks - 1) * NCO + e) * 64] = o[e / 16][(e / 4) % 4][e % 4];
    }
    __syncthreads();
    if (ks == 0) {
#pragma unroll
      for (int k = 1; k < S; ++k)
#pragma unroll
        for (int e = 0; e < NCO; ++e) o[e / 16][(e / 4) % 4][e % 4] += red[((k - 1) * NCO + e) * 64];
    }
  }
  if (ks != 0 || !live || c0 >= W) return;  // no barrier follows

  const bool bn = a.bn.mean != nullptr;
  const int oy = byi * 2;
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    const int co0 = cbi * NCO + nc * 16 + 4 * q;
    float bs[4] = {1.0f, 1.0f, 1.0f, 1.0f}, bb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bn) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bn_fold(a.bn, co0 + i, bs[i], bb[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float2 o0, o1;
      o0.x = bn_apply(o[nc][i][0], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o0.y = bn_apply(o[nc][i][1], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o1.x = bn_apply(o[nc][i][2], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      o1.y = bn_apply(o[nc][i][3], bn, &bs[i], &bb[i], false, nullptr, a.relu);
      float* yp = a.y + ((img * a.cout + co0 + i) * H + oy) * W + c0;
      *reinterpret_cast<float2*>(yp) = o0;
      if (oy + 1 < H) *reinterpret_cast<float2*>(yp + W) = o1;
    }
  }
}

}  // namespace frh

using namespace frh;

extern "C" int32_t frh_conv3x3_nchw_bn_act_form(int32_t form, const float* x, const float* w, const float* gamma,
                                                const float* beta, const float* mean, const float* var, float eps,
                                                float* y, float* workspace, int64_t n, int32_t cin, int32_t cout,
                                                int32_t h, int32_t wd, int32_t relu, void* stream) {
  const char* what = "frh_conv3x3_nchw_bn_act_form";
  FRH_REQUIRE(form >= 0 && form < kNwForms + 3, "form %d: 0 to %d", form, kNwForms + 2);
  if (form < kNwForms)
    return conv3x3_nchw_launch(what, form, x, w, y, {gamma, beta, mean, var, eps}, workspace, n, cin, cout, h, wd, relu,
                               stream);
  const int lab = form - kNwForms, NC = lab == 0 ? 2 : 1, S = lab == 1 ? 2 : 1, TR = lab == 1 ? 2 : 4;
  Conv3x3NchwArgs a;
  bool run = false;
  const int32_t st = conv3x3_nchw_prepare(1, NC, x, w, y, {gamma, beta, mean, var, eps}, workspace, n, cin, cout, h, wd,
                                          relu, a, run);
  if (st != FRH_OK || !run) return st;
  hipLaunchKernelGGL(conv3x3_nchw_weights_kernel, dim3((unsigned)(((int64_t)cin * cout + 255) / 256)), dim3(256), 0,
                     as_stream(stream), w, workspace, cin, cout);
  const int64_t runs = a.total / a.cb;
  const dim3 grid((unsigned)((runs + TR - 1) / TR * a.cb)), block((unsigned)(64 * S * TR));
  switch (lab) {
    case 0: hipLaunchKernelGGL((conv3x3_nchw_lds_kernel<2, 1, 4>), grid, block, 0, as_stream(stream), a); break;
    case 1: hipLaunchKernelGGL((conv3x3_nchw_lds_kernel<1, 2, 2>), grid, block, 0, as_stream(stream), a); break;
    default: hipLaunchKernelGGL((conv3x3_nchw_lds_kernel<1, 1, 4>), grid, block, 0, as_stream(stream), a); break;
  }
  return check_launch(what);
}
