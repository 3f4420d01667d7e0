// The attention gate network inside the softmax aggregation (fp32 build): FiberBundleConv(aggr="AttentionalAggregation"), conv.py:21-26,58-61,
// 138-139 with PyG's AttentionalAggregation(gate_nn = Linear + ReLU) and utils.softmax.  Per destination d, orientation o, channel c over the
// in-edges e of d (rows rowptr[d] .. rowptr[d+1] of the destination-sorted msg [E,16,64]):
//     pre_e = msg_e[o,:] . Wg[c,:] + bg[c]      gate_e = max(pre_e, 0)
//     alpha_e = exp(gate_e - m) / (sum_e' exp(gate_e' - m) + 1e-16),  m = max_e gate_e
//     x1[d,o,c] = sum_e alpha_e msg_e[o,c]
// Backward:  dgate_e = alpha_e dx1 (msg_e - x1),  dpre_e = dgate_e [pre_e > 0],  dmsg_e = alpha_e dx1 + dpre_e Wg  (the complete per-edge
// gradient),  dWg = sum_{e,o} dpre_e[o,:]^T msg_e[o,:],  dbg = sum_{e,o} dpre_e[o,:].
// Neither gate nor dgate ever exists in memory: one edge is ONE 16-row x 64 tile against the 64 x 64 weight, the 16-row-tile case of
// grl_tile16.h.  One wave per destination, four waves per workgroup, grid-stride over the destinations.  In the chain layout (lane = (row r,
// k-group g)) the f32x4 accumulator of n-tile nt holds pre[r][16 nt + 4 g + u] -- the SAME (row, channel) elements as the lane's four msg
// quads msg[r][16 nt + 4 g ..] -- so the softmax over a destination's edges is plain per-lane arithmetic: no cross-lane step, no atomics.
// The forward keeps a running maximum (online softmax: the sums are rescaled when the maximum moves) and leaves stat [n_dst,16,64,2] =
// (m, 1 / (den + 1e-16)) for the backward, which recomputes pre with the forward's device function (gate_pre) and forms
// alpha_e = exp(gate_e - m) * inv from it.
// Precision.  exp turns an ABSOLUTE error of pre into a RELATIVE error of alpha, so pre is the one product of this file that the usual
// split-bf16 triple (hi hi + lo hi + hi lo: ~2^-16 relative, and its dropped lo lo term is a coherent shrink of the product) does not
// serve: with gates of 50 .. 200 it left x1 2.0e-4 of its scale off (emulated in float64 and measured alike; four terms: 1.4e-4).  pre
// therefore splits both operands into THREE bf16 pieces, x = hi + lo + l2 exactly (l2 = the remainder of the existing lo), and sums six
// products, smallest first -- what is dropped is below 2^-24 of the product, the result is fp32-accurate (emulated: 2e-6 of x1's
// scale, the level of an fp32 GEMM).  Twelve MFMAs per 16 x 16 tile instead of six, beside ~30 exp per lane and edge.  dpre . Wg and
// dWg feed nothing non-linear and keep the triple.
#pragma once
#include "grl_tile16.h"
#include "grl_wimg.h"

#if !GRL_PREC
namespace {

constexpr int GATE_LD = WI_LD2;                 // image row length (80 bf16: the ds_read_b128 lane groups meet disjoint banks)
constexpr int GATE_PARTIAL = 64 * 64 + 64;      // one partial row per workgroup: [dWg 64x64 | dbg 64]

struct GateW {
  unsigned short Wh[64 * GATE_LD], Wl[64 * GATE_LD];   // image[n][32 s + 8 g + j] = Wg[n][32 s + 16 (j >> 2) + 4 g + (j & 3)]   (stage16)
  unsigned short W2[64 * GATE_LD];                     // the third piece, same layout (gate_stage_l2)
  float bg[64];
};
struct GateStage {
  unsigned short Ah[STG], Al[STG];   // dpre of the edge in progress, [row][channel]
  unsigned short Bh[STG], Bl[STG];   // its msg rows
};
struct GateBwdSmem {
  GateW w;
  unsigned short WTh[64 * GATE_LD], WTl[64 * GATE_LD];   // the image of Wg^T: dpre . Wg as a chain product
  GateStage st[4];
};

// third bf16 piece of x = hi + lo + l2 (hi, lo: split_pair's): what rounding x - hi to lo left behind, at most 8 significant bits -- exact
GRL_DEVINL float gate_rem(float x) {
  const float r = x - trunc_bf16(x);
  return r - (float)(__bf16)r;
}
GRL_DEVINL bf16x8 gate_split_l2(const float4& f0, const float4& f1) {
  u32x4 l;
  l[0] = pack_rn(gate_rem(f0.x), gate_rem(f0.y)); l[1] = pack_rn(gate_rem(f0.z), gate_rem(f0.w));
  l[2] = pack_rn(gate_rem(f1.x), gate_rem(f1.y)); l[3] = pack_rn(gate_rem(f1.z), gate_rem(f1.w));
  return __builtin_bit_cast(bf16x8, l);
}
// the image of Wg's third pieces, in stage16's layout
template <int NT>
GRL_DEVINL void gate_stage_l2(unsigned short* img, const float* __restrict__ W, int ld) {
  for (int idx = threadIdx.x; idx < 64 * 2 * 4; idx += NT) {
    const int g = idx & 3, s = (idx >> 2) & 1, n = idx >> 3;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W[n * 64 + 32 * s + 16 * (j >> 2) + 4 * g + (j & 3)];
    *reinterpret_cast<bf16x8*>(img + n * ld + 32 * s + 8 * g) =
        gate_split_l2(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
  }
}

// one fenced group (every operand fragment is loaded before the first MFMA, the accumulator is read behind the last: csrc/grl_common.h
// mma_wx_bf_fenced has the reason): acc(16 outputs of one n-tile x 16 rows) = init + sum over the two K-steps of W-tile . X, split-bf16
template <class Epi>
GRL_DEVINL void gate_group(const unsigned short* whi, const unsigned short* wlo, const bf16x8 (&xh)[2], const bf16x8 (&xl)[2], f32x4v acc,
                           Epi&& epi) {
  bf16x8 wh[2], wl[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    wh[s] = *reinterpret_cast<const bf16x8*>(whi + 32 * s);
    wl[s] = *reinterpret_cast<const bf16x8*>(wlo + 32 * s);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    acc = mfma16(wh[s], xh[s], acc);
    acc = mfma16(wl[s], xh[s], acc);
    acc = mfma16(wh[s], xl[s], acc);
  }
  epi(acc);
  __builtin_amdgcn_sched_barrier(0);
}

// the same with three pieces per operand and six products, smallest first (the header comment's "Precision")
template <class Epi>
GRL_DEVINL void gate_group6(const unsigned short* whi, const unsigned short* wlo, const unsigned short* wl2, const bf16x8 (&xh)[2],
                            const bf16x8 (&xl)[2], const bf16x8 (&x2)[2], f32x4v acc, Epi&& epi) {
  bf16x8 wh[2], wl[2], w2[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    wh[s] = *reinterpret_cast<const bf16x8*>(whi + 32 * s);
    wl[s] = *reinterpret_cast<const bf16x8*>(wlo + 32 * s);
    w2[s] = *reinterpret_cast<const bf16x8*>(wl2 + 32 * s);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    acc = mfma16(w2[s], xh[s], acc);
    acc = mfma16(wh[s], x2[s], acc);
    acc = mfma16(wl[s], xl[s], acc);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    acc = mfma16(wl[s], xh[s], acc);
    acc = mfma16(wh[s], xl[s], acc);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = mfma16(wh[s], xh[s], acc);
  epi(acc);
  __builtin_amdgcn_sched_barrier(0);
}

// this lane's four quads of row r of edge e: channels 16 nt + 4 g .. + 3
GRL_DEVINL void gate_load_rows(const float* __restrict__ t, size_t tile, int r, int g, float4 (&m)[4]) {
  const float* row = t + (tile * 16 + r) * 64 + 4 * g;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) m[nt] = *reinterpret_cast<const float4*>(row + 16 * nt);
}

// pre[nt] = bg + Wg msg^T for the lane's (row, channel quad) elements -- the ONE form both kernels use, so that the backward's gates are
// the forward's bits.  m: the fp32 quads mh / ml were split from
GRL_DEVINL void gate_pre(const GateW& w, const float4 (&m)[4], const bf16x8 (&mh)[2], const bf16x8 (&ml)[2], int r, int g,
                         float4 (&pre)[4]) {
  bf16x8 m2[2];
  m2[0] = gate_split_l2(m[0], m[1]);
  m2[1] = gate_split_l2(m[2], m[3]);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const float4 bq = *reinterpret_cast<const float4*>(w.bg + 16 * nt + 4 * g);
    const int off = (16 * nt + r) * GATE_LD + 8 * g;
    // (the bias joins last: one rounding at the sum's magnitude instead of twelve)
    gate_group6(w.Wh + off, w.Wl + off, w.W2 + off, mh, ml, m2, f32x4v{0.f, 0.f, 0.f, 0.f},
                [&](const f32x4v& acc) { pre[nt] = make_float4(acc[0] + bq.x, acc[1] + bq.y, acc[2] + bq.z, acc[3] + bq.w); });
  }
}

GRL_DEVINL void gate_online(float pre, float m, float& mx, float& den, float& num) {
  const float gt = fmaxf(pre, 0.f), mn = fmaxf(mx, gt);
  const float sc = expf(mx - mn), wgt = expf(gt - mn);   // (first edge: mx = -3e38, sc = 0 exactly)
  den = den * sc + wgt;
  num = num * sc + wgt * m;
  mx = mn;
}

__global__ __launch_bounds__(256) void gate_softmax_fwd_kernel(const float* __restrict__ msg, const int* __restrict__ rowptr, int n_dst,
                                                               float* __restrict__ x1, const float* __restrict__ Wg,
                                                               const float* __restrict__ bg, float* __restrict__ stat) {
  __shared__ __attribute__((aligned(16))) GateW w;
  stage16<64, 64, 256>(w.Wh, w.Wl, Wg, GATE_LD);
  gate_stage_l2<256>(w.W2, Wg, GATE_LD);
  if (threadIdx.x < 64) w.bg[threadIdx.x] = bg[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long long d = (long long)blockIdx.x * 4 + wave; d < n_dst; d += (long long)gridDim.x * 4) {
    const int e0 = rowptr[d], e1 = rowptr[d + 1];
    float4 mx[4], den[4], num[4], m[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      mx[nt] = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f);
      den[nt] = num[nt] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (e0 < e1) gate_load_rows(msg, (size_t)e0, r, g, m);
    for (int e = e0; e < e1; ++e) {
      float4 nx[4];
      if (e + 1 < e1) gate_load_rows(msg, (size_t)e + 1, r, g, nx);   // the next edge's rows travel under this edge's arithmetic
      bf16x8 mh[2], ml[2];
      split_pair(m[0], m[1], mh[0], ml[0]);
      split_pair(m[2], m[3], mh[1], ml[1]);
      float4 pre[4];
      gate_pre(w, m, mh, ml, r, g, pre);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        gate_online(pre[nt].x, m[nt].x, mx[nt].x, den[nt].x, num[nt].x);
        gate_online(pre[nt].y, m[nt].y, mx[nt].y, den[nt].y, num[nt].y);
        gate_online(pre[nt].z, m[nt].z, mx[nt].z, den[nt].z, num[nt].z);
        gate_online(pre[nt].w, m[nt].w, mx[nt].w, den[nt].w, num[nt].w);
      }
      if (e + 1 < e1) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) m[nt] = nx[nt];
      }
    }
    const bool any = e1 > e0;   // a destination without in-edges: x1 = 0 exactly, stat = (0, 0)
    float* xrow = x1 + ((size_t)d * 16 + r) * 64 + 4 * g;
    float* srow = stat + (((size_t)d * 16 + r) * 64 + 4 * g) * 2;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const float mv[4] = {mx[nt].x, mx[nt].y, mx[nt].z, mx[nt].w};
      const float dv[4] = {den[nt].x, den[nt].y, den[nt].z, den[nt].w};
      const float nv[4] = {num[nt].x, num[nt].y, num[nt].z, num[nt].w};
      float xo[4], so[8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xo[u] = any ? nv[u] / (dv[u] + 1e-16f) : 0.f;
        so[2 * u] = any ? mv[u] : 0.f;
        so[2 * u + 1] = any ? 1.f / (dv[u] + 1e-16f) : 0.f;
      }
      *reinterpret_cast<float4*>(xrow + 16 * nt) = make_float4(xo[0], xo[1], xo[2], xo[3]);
      *reinterpret_cast<float4*>(srow + 32 * nt) = make_float4(so[0], so[1], so[2], so[3]);
      *reinterpret_cast<float4*>(srow + 32 * nt + 4) = make_float4(so[4], so[5], so[6], so[7]);
    }
  }
}

// Same distribution of work.  Per edge: pre again (gate_pre), alpha from stat, dpre; dmsg = alpha dx1 + dpre . Wg as a second chain product
// against the image of Wg^T (the accumulator starts at alpha dx1); dWg += dpre^T msg contracted over the edge's 16 rows on the 32x32x16 form
// (both operands staged once in the wave's LDS images and read back transposed: grl_tile16.h tr_frag), accumulated over all the wave's
// edges in 64 registers per lane.  The four waves are summed through LDS in a fixed order; every workgroup writes its whole partial row.
__global__ __launch_bounds__(256, 1) void gate_softmax_bwd_kernel(const float* __restrict__ msg, const float* __restrict__ x1,
                                                                  const float* __restrict__ dx1, const int* __restrict__ rowptr, int n_dst,
                                                                  float* __restrict__ dmsg, const float* __restrict__ Wg,
                                                                  const float* __restrict__ bg, const float* __restrict__ stat,
                                                                  float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float gate_smem_raw[];
  GateBwdSmem& sm = *reinterpret_cast<GateBwdSmem*>(gate_smem_raw);
  stage16<64, 64, 256>(sm.w.Wh, sm.w.Wl, Wg, GATE_LD);
  gate_stage_l2<256>(sm.w.W2, Wg, GATE_LD);
  stage16<64, 64, 256, true>(sm.WTh, sm.WTl, Wg, GATE_LD);
  if (threadIdx.x < 64) sm.w.bg[threadIdx.x] = bg[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  GateStage& st = sm.st[wave];
  f32x16 acc[2][2];
#pragma unroll
  for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
    for (int b_ = 0; b_ < 2; ++b_) acc[a_][b_] = zero16();
  float db[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) db[i] = 0.f;

  for (long long d = (long long)blockIdx.x * 4 + wave; d < n_dst; d += (long long)gridDim.x * 4) {
    const int e0 = rowptr[d], e1 = rowptr[d + 1];
    if (e0 >= e1) continue;
    float4 xo[4], gd[4], m[4];
    float mxv[16], inv[16];
    gate_load_rows(x1, (size_t)d, r, g, xo);
    gate_load_rows(dx1, (size_t)d, r, g, gd);
    {
      const float* srow = stat + (((size_t)d * 16 + r) * 64 + 4 * g) * 2;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float4 a = *reinterpret_cast<const float4*>(srow + 32 * nt), b = *reinterpret_cast<const float4*>(srow + 32 * nt + 4);
        mxv[4 * nt] = a.x; inv[4 * nt] = a.y; mxv[4 * nt + 1] = a.z; inv[4 * nt + 1] = a.w;
        mxv[4 * nt + 2] = b.x; inv[4 * nt + 2] = b.y; mxv[4 * nt + 3] = b.z; inv[4 * nt + 3] = b.w;
      }
    }
    gate_load_rows(msg, (size_t)e0, r, g, m);
    for (int e = e0; e < e1; ++e) {
      float4 nx[4];
      if (e + 1 < e1) gate_load_rows(msg, (size_t)e + 1, r, g, nx);
      bf16x8 mh[2], ml[2];
      split_pair(m[0], m[1], mh[0], ml[0]);
      split_pair(m[2], m[3], mh[1], ml[1]);
      float4 pre[4];
      gate_pre(sm.w, m, mh, ml, r, g, pre);
      float4 ad[4], dp[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float pv[4] = {pre[nt].x, pre[nt].y, pre[nt].z, pre[nt].w};
        const float mv[4] = {m[nt].x, m[nt].y, m[nt].z, m[nt].w};
        const float xv[4] = {xo[nt].x, xo[nt].y, xo[nt].z, xo[nt].w};
        const float gv[4] = {gd[nt].x, gd[nt].y, gd[nt].z, gd[nt].w};
        float av[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float alpha = expf(fmaxf(pv[u], 0.f) - mxv[4 * nt + u]) * inv[4 * nt + u];
          av[u] = alpha * gv[u];
          dv[u] = pv[u] > 0.f ? av[u] * (mv[u] - xv[u]) : 0.f;
          db[4 * nt + u] += dv[u];
        }
        ad[nt] = make_float4(av[0], av[1], av[2], av[3]);
        dp[nt] = make_float4(dv[0], dv[1], dv[2], dv[3]);
      }
      bf16x8 dh[2], dl[2];
      split_pair(dp[0], dp[1], dh[0], dl[0]);
      split_pair(dp[2], dp[3], dh[1], dl[1]);
      // the operands of dWg, staged; the transposed reads are requested behind the second chain product
      stage_put<2>(st.Ah, st.Al, dh, dl, r, g);
      stage_put<2>(st.Bh, st.Bl, mh, ml, r, g);
      float* orow = dmsg + ((size_t)e * 16 + r) * 64 + 4 * g;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        gate_group(sm.WTh + (16 * nt + r) * GATE_LD + 8 * g, sm.WTl + (16 * nt + r) * GATE_LD + 8 * g, dh, dl,
                   f32x4v{ad[nt].x, ad[nt].y, ad[nt].z, ad[nt].w},
                   [&](const f32x4v& c) { *reinterpret_cast<float4*>(orow + 16 * nt) = v4(c); });
      bf16x8 fah[2], fal[2], fbh[2], fbl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fah[t] = tr_frag(st.Ah, t, lane);
        fal[t] = tr_frag(st.Al, t, lane);
        fbh[t] = tr_frag(st.Bh, t, lane);
        fbl[t] = tr_frag(st.Bl, t, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk) {
          acc[tn][tk] = mfma_bf(fah[tn], fbh[tk], acc[tn][tk]);
          acc[tn][tk] = mfma_bf(fal[tn], fbh[tk], acc[tn][tk]);
          acc[tn][tk] = mfma_bf(fah[tn], fbl[tk], acc[tn][tk]);
        }
      __builtin_amdgcn_sched_barrier(0);
      if (e + 1 < e1) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) m[nt] = nx[nt];
      }
    }
  }

  // ---- fold the four waves through LDS (images dead): 1 -> 0 and 3 -> 2, then 2 -> 0; fixed order, one partial row per workgroup
  constexpr int NACC = 4 * 16 + 16;
  float* fold = gate_smem_raw;
  static_assert(2 * NACC * 64 * sizeof(float) <= sizeof(GateBwdSmem), "the fold reuses the images' LDS");
  auto visit = [&](auto&& f) {
    int k = 0;
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
      for (int b_ = 0; b_ < 2; ++b_)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a_][b_][i] = f(acc[a_][b_][i], k++);
#pragma unroll
    for (int i = 0; i < 16; ++i) db[i] = f(db[i], k++);
  };
  __syncthreads();
  if (wave & 1) visit([&](float v_, int k) { fold[((wave >> 1) * NACC + k) * 64 + lane] = v_; return v_; });
  __syncthreads();
  if (!(wave & 1)) visit([&](float v_, int k) { return v_ + fold[((wave >> 1) * NACC + k) * 64 + lane]; });
  __syncthreads();
  if (wave == 2) visit([&](float v_, int k) { fold[k * 64 + lane] = v_; return v_; });
  __syncthreads();
  if (wave != 0) return;
  visit([&](float v_, int k) { return v_ + fold[k * 64 + lane]; });
  // 32x32 accumulator element rho of lane (column j = lane & 31, hh = lane >> 5): D[n = 8 (rho >> 2) + 4 hh + (rho & 3)][j]
  const int j = lane & 31, hh = lane >> 5;
  float* out = partial + (size_t)blockIdx.x * GATE_PARTIAL;
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int tk = 0; tk < 2; ++tk)
#pragma unroll
      for (int rho = 0; rho < 16; ++rho) {
        const int n = 32 * tn + (rho & 3) + 8 * (rho >> 2) + 4 * hh;
        out[n * 64 + 32 * tk + j] = acc[tn][tk][rho];
      }
  // dbg: this lane's sums of channels 16 nt + 4 g + u over its row -> over the 16 rows (the lanes that share g)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float x = db[i];
    x += __shfl_xor(x, 1, 64); x += __shfl_xor(x, 2, 64); x += __shfl_xor(x, 4, 64); x += __shfl_xor(x, 8, 64);
    if (r == 0) out[64 * 64 + 16 * (i >> 2) + 4 * g + (i & 3)] = x;
  }
}

int gate_softmax_fwd_launch(const float* msg, const int* rowptr, int n_dst, float* x1, const float* Wg, const float* bg, float* stat,
                            int n_blocks, hipStream_t stream) {
  hipLaunchKernelGGL(gate_softmax_fwd_kernel, dim3(n_blocks), dim3(256), 0, stream, msg, rowptr, n_dst, x1, Wg, bg, stat);
  GRL_CHECK_LAUNCH();
  return 0;
}
int gate_softmax_bwd_launch(const float* msg, const float* x1, const float* dx1, const int* rowptr, int n_dst, float* dmsg, const float* Wg,
                            const float* bg, const float* stat, float* partial, int n_blocks, hipStream_t stream) {
  GRL_ONCE(hipFuncSetAttribute((const void*)gate_softmax_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GateBwdSmem)));
  hipLaunchKernelGGL(gate_softmax_bwd_kernel, dim3(n_blocks), dim3(256), sizeof(GateBwdSmem), stream, msg, x1, dx1, rowptr, n_dst, dmsg, Wg,
                     bg, stat, partial);
  GRL_CHECK_LAUNCH();
  return 0;
}

}  // namespace
#endif   // !GRL_PREC
