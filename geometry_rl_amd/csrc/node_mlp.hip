// ConvNeXt node block of FiberBundleConv (reference conv.py:64-69,112; ponita.py:219-230):
//   out = x_dst + Linear(256,64)( GELU( Linear(64,256)( LayerNorm64(x2) ) ) )
// Rows are (node, orientation) pairs; each wave owns 32 rows (2 nodes) per step and keeps the whole chain in registers
// (see grl_common.h): LayerNorm by lane-pair shuffles, W3/W4 staged once per workgroup in LDS as MFMA A operands.
//
// Backward: ONE fused launch on 16-row chunks (node_mlp16.hip): dx2 and all six parameter gradients, nothing handed over through HBM.
#include "grl_common.h"
#include "grl_wimg.h"
#include <stdlib.h>

namespace {

constexpr int C = 64, O = 16, W = 256;
constexpr float LN_EPS = 1e-5f;
// split-bf16 weight images for the forward kernel: struct MlpSmemBf (grl_wimg.h, shared with the image producer)
constexpr int LB3 = WI_LB3;   // 72
constexpr int LB4 = WI_LB4;   // 264

GRL_DEVINL float pair_sum(float v) { return v + __shfl_xor(v, 32, 64); }

// loads this lane's 8 fragments of row `row` (64 floats)
GRL_DEVINL void load_row(const st_t* base, size_t row, int h, float4 (&f)[8]) {
  const st_t* p = base + row * C + 4 * h;
#pragma unroll
  for (int t = 0; t < 8; ++t) f[t] = ld4(p + 8 * t);
}
GRL_DEVINL void store_row(st_t* base, size_t row, int h, const float4 (&f)[8]) {
  st_t* p = base + row * C + 4 * h;
#pragma unroll
  for (int t = 0; t < 8; ++t) st4(p + 8 * t, f[t]);
}

GRL_DEVINL f32x16 bias_acc(const float* bias, int n0, int h) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b = *reinterpret_cast<const float4*>(bias + n0 + 8 * q + 4 * h);
    acc[4 * q] = b.x; acc[4 * q + 1] = b.y; acc[4 * q + 2] = b.z; acc[4 * q + 3] = b.w;
  }
  return acc;
}

GRL_DEVINL void mfma_fence(const f32x16& acc, float& sink) {
  // a compiler-visible VALU read of the accumulator: it cannot issue before the MFMA group that produced acc has finished
  sink += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, acc[0]), 0xE4, 0xF, 0xF, false));
}


// ------------------------------------------------------------------------------------------------ forward
// Both GEMMs run on the bf16 matrix pipe with split operands (grl_common.h): per 32-row tile 2 x 96 bf16 MFMAs of 32 cycles
// instead of 2 x 256 fp32 MFMAs of 64 cycles.
__global__ __launch_bounds__(512) void node_mlp_fwd_kernel(const st_t* __restrict__ x2, const st_t* __restrict__ x_dst,
                                                           const float* W3, const float* b3, const float* W4, const float* b4,
                                                           const float* gam, const float* bet, st_t* __restrict__ out,
                                                           int n_rows, int accumulate, const void* __restrict__ wimg) {
  extern __shared__ __attribute__((aligned(16))) float smem_raw[];
  MlpSmemBf& s = *reinterpret_cast<MlpSmemBf*>(smem_raw);
  if (wimg) {   // the whole struct, built once per forward pass by grl_weight_images (kind 2): a linear copy
    copy_image<512>(&s, wimg, (int)sizeof(MlpSmemBf));
  } else {
    stage_split<W, C, C, 512>(s.W3h, s.W3l, W3, LB3);
    stage_split<C, W, W, 512>(s.W4h, s.W4l, W4, LB4);
    for (int i = threadIdx.x; i < W; i += blockDim.x) s.b3s[i] = b3[i];
    for (int i = threadIdx.x; i < C; i += blockDim.x) { s.b4s[i] = b4[i]; s.gam[i] = gam[i]; s.bet[i] = bet[i]; }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int n_tiles = (n_rows + 31) >> 5;
  float sink = 0.f;
#if GRL_PREC
  // plain-bf16 build (184 registers of 256): the tile's x2 row arrives a tile ahead and its residual row is requested before the MLP
  // chain, both RAW (grl_common.h raw4_t) -- loaded where they were used, each cost the wave a full HBM round trip per tile (round 5:
  // 0.36 of the kernel's wave cycles in s_waitcnt).  The fp32 build has no registers left for it.
  raw4_t xr[8], rres[8];
  {
    const int tile0 = blockIdx.x * 8 + wave, row0 = tile0 * 32 + r;
    const size_t rr0 = (tile0 < n_tiles && row0 < n_rows) ? row0 : 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) xr[t] = ld4_raw(x2 + rr0 * C + 4 * h + 8 * t);
  }
#endif
  for (int tile = blockIdx.x * 8 + wave; tile < n_tiles; tile += gridDim.x * 8) {
    const int row = tile * 32 + r;
    const bool valid = row < n_rows;
    const size_t rr = valid ? row : 0;
    float4 x[8], xh[8], a[8];
    float rstd;
#if GRL_PREC
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = widen4(xr[t]);
    {
      const int tile_n = tile + gridDim.x * 8, row_n = tile_n * 32 + r;
      const size_t rn = (tile_n < n_tiles && row_n < n_rows) ? row_n : rr;   // (clamped: no branch around the loads)
#pragma unroll
      for (int t = 0; t < 8; ++t) rres[t] = ld4_raw(x_dst + rr * C + 4 * h + 8 * t);
#pragma unroll
      for (int t = 0; t < 8; ++t) xr[t] = ld4_raw(x2 + rn * C + 4 * h + 8 * t);
    }
#else
    load_row(x2, rr, h, x);
#endif
    {  // LayerNorm over the 64 channels of the row, split across the lane pair (l, l^32)
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) sum += (x[t].x + x[t].y) + (x[t].z + x[t].w);
      const float mean = pair_sum(sum) * (1.f / C);
      float sq = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        xh[t] = make_float4(x[t].x - mean, x[t].y - mean, x[t].z - mean, x[t].w - mean);
        sq += (xh[t].x * xh[t].x + xh[t].y * xh[t].y) + (xh[t].z * xh[t].z + xh[t].w * xh[t].w);
      }
      rstd = rsqrtf(pair_sum(sq) * (1.f / C) + LN_EPS);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float4 g = *reinterpret_cast<const float4*>(s.gam + 8 * t + 4 * h);
        const float4 b = *reinterpret_cast<const float4*>(s.bet + 8 * t + 4 * h);
        a[t] = make_float4(xh[t].x * rstd * g.x + b.x, xh[t].y * rstd * g.y + b.y, xh[t].z * rstd * g.z + b.z,
                           xh[t].w * rstd * g.w + b.w);
      }
    }
    bf16x8 ah[4], al[4];
    split_frags<64>(a, ah, al);
    f32x16 o0 = bias_acc(s.b4s, 0, h), o1 = bias_acc(s.b4s, 32, h);
    // Software pipeline over the eight 32-unit hidden tiles (round 2, DESIGN.md findings 18 / 20): one scheduling region holds the
    // GELU + split of tile nt (vector work), the z chain of tile nt + 1 and the two output chains of tile nt - 1 (24 MFMAs) -- three
    // independent streams of the SAME wave; every weight fragment is requested one region before its MFMAs, none between the MFMAs
    // of a chain.  (Before: each of the 24 fragment reads of an iteration sat directly in front of its MFMA.)
    struct F3 { bf16x8 h[4], l[4]; } f3;
    struct F4 { bf16x8 h[2][2], l[2][2]; } f4;
    auto load3 = [&](int nt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f3.h[u] = *reinterpret_cast<const bf16x8*>(s.W3h + (32 * nt + r) * LB3 + 8 * h + 16 * u);
        GRL_LO(f3.l[u] = *reinterpret_cast<const bf16x8*>(s.W3l + (32 * nt + r) * LB3 + 8 * h + 16 * u);)
      }
    };
    auto load4 = [&](int nt) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          f4.h[t2][u] = *reinterpret_cast<const bf16x8*>(s.W4h + (32 * t2 + r) * LB4 + 32 * nt + 8 * h + 16 * u);
          GRL_LO(f4.l[t2][u] = *reinterpret_cast<const bf16x8*>(s.W4l + (32 * t2 + r) * LB4 + 32 * nt + 8 * h + 16 * u);)
        }
    };
    auto zchain = [&](f32x16 acc) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = mfma_bf(f3.h[u], ah[u], acc);
        GRL_LO(acc = mfma_bf(f3.l[u], ah[u], acc);)
        GRL_LO(acc = mfma_bf(f3.h[u], al[u], acc);)
      }
      return acc;
    };
    load3(0);
    f32x16 acc = bias_acc(s.b3s, 0, h);
    __builtin_amdgcn_sched_barrier(0);
    acc = zchain(acc);
    mfma_fence(acc, sink);
    __builtin_amdgcn_sched_barrier(0);
    load3(1);
    bf16x8 ph[2], pl[2];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      f32x16 acc_next = acc;
      if (nt < 7) acc_next = zchain(bias_acc(s.b3s, 32 * (nt + 1), h));
      if (nt > 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          o0 = mfma_bf(f4.h[0][u], ph[u], o0);
          o1 = mfma_bf(f4.h[1][u], ph[u], o1);
          GRL_LO(o0 = mfma_bf(f4.l[0][u], ph[u], o0);)
          GRL_LO(o1 = mfma_bf(f4.l[1][u], ph[u], o1);)
          GRL_LO(o0 = mfma_bf(f4.h[0][u], pl[u], o0);)
          GRL_LO(o1 = mfma_bf(f4.h[1][u], pl[u], o1);)
        }
      }
      float4 hq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        hq[q] = gelu4(make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
      bf16x8 hh[2], hl[2];
      split_frags<32>(hq, hh, hl);
      // the fragment registers are re-loaded next: every MFMA that reads them must have finished, not merely issued (finding 3: with
      // two waves per SIMD an MFMA can sit queued behind the partner's) -- a vector read of each chain's accumulator
      mfma_fence(acc_next, sink);
      if (nt > 0) { mfma_fence(o0, sink); mfma_fence(o1, sink); }
      __builtin_amdgcn_sched_barrier(0);
      if (nt < 6) load3(nt + 2);
      load4(nt);
      ph[0] = hh[0]; ph[1] = hh[1];
      GRL_LO(pl[0] = hl[0]; pl[1] = hl[1];)
      acc = acc_next;
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      o0 = mfma_bf(f4.h[0][u], ph[u], o0);
      o1 = mfma_bf(f4.h[1][u], ph[u], o1);
      GRL_LO(o0 = mfma_bf(f4.l[0][u], ph[u], o0);)
      GRL_LO(o1 = mfma_bf(f4.l[1][u], ph[u], o1);)
      GRL_LO(o0 = mfma_bf(f4.h[0][u], pl[u], o0);)
      GRL_LO(o1 = mfma_bf(f4.h[1][u], pl[u], o1);)
    }
    float4 res[8], y[8];
#if GRL_PREC
#pragma unroll
    for (int t = 0; t < 8; ++t) res[t] = widen4(rres[t]);
#else
    load_row(x_dst, rr, h, res);
#endif
    if (accumulate) {
      load_row(out, rr, h, y);
#pragma unroll
      for (int t = 0; t < 8; ++t) res[t] = f4_add(res[t], y[t]);
    }
    acc_to_frag(o0, y[0], y[1], y[2], y[3]);
    acc_to_frag(o1, y[4], y[5], y[6], y[7]);
#pragma unroll
    for (int t = 0; t < 8; ++t) y[t] = f4_add(y[t], res[t]);
    if (valid) store_row(out, rr, h, y);
  }
  if (sink == 123456.789f) st1(out, sink);   // keeps the fences alive; never true
}

// partial slab per workgroup: [dW3 256x64 | db3 256 | dW4 64x256 | db4 64 | dgamma 64 | dbeta 64]
constexpr int MLP_PARTIAL = W * C + W + C * W + C + C + C;


int blocks_for(int n_rows, int rows_per_block, int cap) {
  const int b = (n_rows + rows_per_block - 1) / rows_per_block;
  return b < 1 ? 1 : (b < cap ? b : cap);
}

}  // namespace

extern "C" {

#if !GRL_PREC   // shape queries: shared by both precision builds of this file
int grl_node_mlp_partial_size() { return MLP_PARTIAL; }
int grl_node_mlp_bwd_blocks(int n_rows) { return blocks_for(n_rows, 32, 256); }
#else
int grl_node_mlp_bwd_blocks(int n_rows);
#endif

// rows = n_nodes*16.  out = (accumulate ? out : 0) + x_dst + MLP(LN(x2)).  grl_node_mlp_fwd_img: the same with an optional pre-split
// weight image of this forward pass (grl_weight_images kind 2; NULL = the kernel stages W3 / W4 itself)
int GRL_ENTRY(grl_node_mlp_fwd_img)(const st_t* x2, const st_t* x_dst, const float* W3, const float* b3, const float* W4, const float* b4,
                     const float* gamma, const float* beta, st_t* out, int n_rows, int accumulate, const void* wimg, hipStream_t stream) {
  if (n_rows <= 0) return 0;
  GRL_ONCE(hipFuncSetAttribute((const void*)node_mlp_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MlpSmemBf)));
  grl_prof_begin_replay("node_mlp_fwd_kernel", stream);
  hipLaunchKernelGGL(node_mlp_fwd_kernel, dim3(blocks_for(n_rows, 256, 256)), dim3(512), sizeof(MlpSmemBf), stream, x2, x_dst,
                     W3, b3, W4, b4, gamma, beta, out, n_rows, accumulate, wimg);
  grl_prof_end_replay(stream);
  GRL_CHECK_LAUNCH();
  return 0;
}
int GRL_ENTRY(grl_node_mlp_fwd)(const st_t* x2, const st_t* x_dst, const float* W3, const float* b3, const float* W4, const float* b4,
                     const float* gamma, const float* beta, st_t* out, int n_rows, int accumulate, hipStream_t stream) {
  return GRL_ENTRY(grl_node_mlp_fwd_img)(x2, x_dst, W3, b3, W4, b4, gamma, beta, out, n_rows, accumulate, nullptr, stream);
}

// partial [grl_node_mlp_bwd_blocks(n_rows) + 1][grl_node_mlp_partial_size()]: one gradient row per workgroup, and the LAST row is scratch
// (node_mlp16.hip) -- sum rows 0 .. blocks-1 only.  d x_dst is simply dout (residual), not produced here.
int GRL_ENTRY(grl_node_mlp_bwd16_launch)(const st_t* x2, const st_t* dout, const float* W3, const float* b3, const float* W4,
                                         const float* gamma, const float* beta, st_t* dx2, float* partial, int n_rows, int blocks,
                                         const void* wimg, hipStream_t stream);
int GRL_ENTRY(grl_node_mlp_bwd_img)(const st_t* x2, const st_t* dout, const float* W3, const float* b3, const float* W4, const float* b4,
                     const float* gamma, const float* beta, st_t* dx2, float* partial, int n_rows, const void* wimg, hipStream_t stream);
int GRL_ENTRY(grl_node_mlp_bwd)(const st_t* x2, const st_t* dout, const float* W3, const float* b3, const float* W4, const float* b4,
                     const float* gamma, const float* beta, st_t* dx2, float* partial, int n_rows, hipStream_t stream) {
  return GRL_ENTRY(grl_node_mlp_bwd_img)(x2, dout, W3, b3, W4, b4, gamma, beta, dx2, partial, n_rows, nullptr, stream);
}
// the same with an optional pre-split fragment image of this step's weights (grl_weight_images kind 3).  n_rows must be a multiple of 16
// (it is n_nodes * 16): the 16-row kernel returns -3 for any other count and launches nothing.
int GRL_ENTRY(grl_node_mlp_bwd_img)(const st_t* x2, const st_t* dout, const float* W3, const float* b3, const float* W4, const float* b4,
                     const float* gamma, const float* beta, st_t* dx2, float* partial, int n_rows, const void* wimg, hipStream_t stream) {
  (void)b4;
  if (n_rows <= 0) {   // no rows: zero gradients (the caller sums grl_node_mlp_bwd_blocks(n_rows) = 1 partial row)
    hipMemsetAsync(partial, 0, sizeof(float) * MLP_PARTIAL, stream);
    return 0;
  }
  grl_prof_begin_replay("node_mlp_bwd16_kernel", stream);
  const int rc = GRL_ENTRY(grl_node_mlp_bwd16_launch)(x2, dout, W3, b3, W4, gamma, beta, dx2, partial, n_rows, grl_node_mlp_bwd_blocks(n_rows), wimg, stream);
  grl_prof_end_replay(stream);
  return rc;
}

}  // extern "C"
