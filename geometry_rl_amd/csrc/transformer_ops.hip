// Transformer baseline actor (reference transformer_vanilla.py:29-36,87-92: torch's post-norm nn.TransformerEncoder, hidden 64, 2 layers,
// 2 heads, dim_feedforward 64, dropout 0, concat_global=False) and the post_fc Gaussian head, fp32 build only.  A library of
// its own, libgrl_transformer.so, declared in grl_transformer.h (geometry_rl_amd/hip.py transformer_call / transformer_query).
//
//   x_0 = u We^T + be                                                       [n,64] per sample, u [B,n,d_in]
//   layer l: [q|k|v] = x Win^T + bin;  head h = channels 32h .. 32h+31 of each third
//            s_h[i,j] = <q_h[i], k_h[j]> / sqrt(32);  p_h = softmax_j s_h;  o_h[i] = sum_j p_h[i,j] v_h[j]
//            y  = LayerNorm(x + [o_0|o_1] Wo^T + bo)       eps 1e-5, biased variance (norm1)
//            x' = LayerNorm(y + W2 relu(W1 y + b1) + b2)   (norm2)
//   hidden = x_2[m0 .. m0+G) Wf^T + bf                                      [B*G,64]
//
// One workgroup (8 waves) owns whole samples, a GROUP of S consecutive ones at a time (S n <= 256 rows; S = 1 until the batch has more
// samples than the 256 workgroups): group g = blockIdx.x, blockIdx.x + gridDim.x, ...  The row-wise phases run over all rows of the group
// (one weight load and one barrier per phase and group), attention stays inside each sample.  No [n,n] object exists outside LDS:
// the forward keeps per row and head the softmax maximum and sum, the backward recomputes the probabilities from them.  Every phase of a
// sample stages its rows from the saved activations into LDS, works, writes its result rows to global memory and ends with a workgroup
// barrier (which orders the workgroup's own global writes before its later reads).
//
// saved  [15][B*n][64]: x_0 | per layer: q, k, v interleaved as [B*n][192] (3 slots) | o | xhat1 | relu(W1 y + b1) | xhat2
//        (xhat = the normalised row BEFORE the affine map: y = xhat1 g1 + be1 is one fma, and a zero gamma loses nothing)
// stats  [2][B*n][6]:   1/std of norm1, of norm2, row maximum of head 0, 1, row sum of head 0, 1
// partial[blocks][54656 + 64 d_in]: per layer (25216 floats) [dWin 192x64 | dbin 192 | dWo 64x64 | dbo 64 | dg1 64 | dbe1 64 | dW1 64x64 |
//        db1 64 | dW2 64x64 | db2 64 | dg2 64 | dbe2 64], then [dWf 64x64 | dbf 64 | dbe 64 | dWe 64 x d_in].  A workgroup adds the
//        samples it owns into ITS row in sample order (the first one writes): no atomics, the same bits on every run.
//
// Products are plain fp32 fma chains (split into a few interleaved partial sums): a thread keeps one weight row (or column) of a 64x64 matrix in 64 registers and the activation rows
// are LDS broadcasts; the weight gradients are 8 accumulators per thread over the sample's rows.
#include "grl_common.h"

namespace {

constexpr int D = 64, HD = 32, NLAYER = 2, NMAX = 256, DIN_MAX = 64, AMAX = 16;
constexpr int NT = 512, NW = NT / 64;
constexpr int LDH = HD + 1;                 // row stride of the per-head Q / K / V / dO images: lane = row and lane = channel both hit 32 banks
constexpr int BLOCKS_MAX = 256;
constexpr int N_PARAMS = 2 + 12 * NLAYER + 2;
constexpr float SCALE = 0.17677669529663687f;   // 1 / sqrt(32)
constexpr float LN_EPS = 1e-5f;
// offsets inside one layer's slice of a partial row, and of the rest behind the layers
constexpr int P_WIN = 0, P_BIN = 12288, P_WO = 12480, P_BO = 16576, P_G1 = 16640, P_BE1 = 16704, P_W1 = 16768, P_B1 = 20864,
              P_W2 = 20928, P_B2 = 25024, P_G2 = 25088, P_BE2 = 25152, P_LAYER = 25216;
constexpr int P_WF = NLAYER * P_LAYER, P_BF = P_WF + 4096, P_BE = P_BF + 64, P_WE = P_BE + 64;
constexpr int WS_ROW = 5 * D;               // backward workspace per row: d(row) 64 | d(o) 64 | d[q|k|v] 192

struct LayerP {
  const float *Win, *bin, *Wo, *bo, *g1, *be1, *W1, *b1, *W2, *b2, *g2, *be2;
};
struct EncP {
  const float *We, *be;
  LayerP L[NLAYER];
  const float *Wf, *bf;
};

// samples per group: as many as fill 256 rows once every workgroup has one (a group shares every weight load and barrier of a phase)
int tf_group(int B, int n) {
  const int fit = NMAX / n, want = (B + BLOCKS_MAX - 1) / BLOCKS_MAX;
  const int S = want < fit ? want : fit;
  return S < 1 ? 1 : S;
}
int tf_blocks(int B, int n) {
  const int S = tf_group(B, n), g = (B + S - 1) / S;
  return g < 1 ? 1 : (g < BLOCKS_MAX ? g : BLOCKS_MAX);
}
size_t fwd_lds_bytes(int n) {   // n: the rows of a group
  const size_t a = (size_t)n * D, b = (size_t)3 * n * LDH + NW * NMAX;
  return sizeof(float) * (a > b ? a : b);
}
size_t bwd_lds_bytes(int n) {   // [two row images | four head images + three row arrays] + the per-wave p / ds rows (also the LayerNorm fold)
  return sizeof(float) * ((size_t)n * (4 * LDH + 3) + 2 * NW * NMAX);
}

GRL_DEVINL float wave_sum(float v) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
GRL_DEVINL float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
// LDS written by some lanes of a wave and read by others of the SAME wave: the LDS serves one wave's accesses in order; this keeps the
// compiler from moving them across
GRL_DEVINL void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
GRL_DEVINL float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// 4-byte loads: a parameter may sit at any float offset of a flat buffer and the numbers must not depend on it
GRL_DEVINL void load_w_row(float (&w)[D], const float* __restrict__ W, int j) {   // w[k] = W[j][k]
#pragma unroll
  for (int k = 0; k < D; ++k) w[k] = W[j * D + k];
}
GRL_DEVINL void load_w_col(float (&w)[D], const float* __restrict__ W, int j) {   // w[k] = W[k][j]
#pragma unroll
  for (int k = 0; k < D; ++k) w[k] = W[k * D + j];
}
// b + sum_k row[k] w[k] as four interleaved partial sums of 16 terms (k mod 4), folded pairwise: shorter rounding chains than one sum of
// 64, and four independent fma chains; ``row``: 64 floats in LDS, 16-byte aligned, the same for every lane (a broadcast)
GRL_DEVINL float dot_row(const float* row, const float (&w)[D], float b) {
  const float4* r4 = reinterpret_cast<const float4*>(row);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int k = 0; k < D / 4; ++k) {
    const float4 x = r4[k];
    s0 = fmaf(x.x, w[4 * k], s0);
    s1 = fmaf(x.y, w[4 * k + 1], s1);
    s2 = fmaf(x.z, w[4 * k + 2], s2);
    s3 = fmaf(x.w, w[4 * k + 3], s3);
  }
  return ((s0 + s1) + (s2 + s3)) + b;
}
// <r, row> over one head's 32 channels, the same way (four partial sums of 8): the forward and both backward passes form every logit with
// this one function, so the recomputed probabilities are the forward's bits
GRL_DEVINL float dot_head(const float (&r)[HD], const float* row) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int c = 0; c < HD; c += 4) {
    s0 = fmaf(r[c], row[c], s0);
    s1 = fmaf(r[c + 1], row[c + 1], s1);
    s2 = fmaf(r[c + 2], row[c + 2], s2);
    s3 = fmaf(r[c + 3], row[c + 3], s3);
  }
  return (s0 + s1) + (s2 + s3);
}
// sum_j a[j] b[j * ldb] over j = j0, j0 + 2, ... < n as two alternating partial sums
GRL_DEVINL float dot_strided(const float* a, const float* b, int ldb, int j0, int n) {
  float s0 = 0.f, s1 = 0.f;
  int j = j0;
  for (; j + 2 < n; j += 4) {
    s0 = fmaf(a[j], b[j * ldb], s0);
    s1 = fmaf(a[j + 2], b[(j + 2) * ldb], s1);
  }
  if (j < n) s0 = fmaf(a[j], b[j * ldb], s0);
  return s0 + s1;
}
// LayerNorm of the 64 values a wave holds (lane = channel): the normalised value and 1 / std
GRL_DEVINL void layer_norm(float z, float& xh, float& rstd) {
  const float mean = wave_sum(z) * (1.f / D);
  const float d = z - mean;
  const float var = wave_sum(d * d) * (1.f / D);
  rstd = 1.f / sqrtf(var + LN_EPS);
  xh = d * rstd;
}
// ... and its backward: dy the gradient of xh * gamma + beta -> the gradient of z
GRL_DEVINL float layer_norm_bwd(float dy, float gamma, float xh, float rstd) {
  const float g = dy * gamma;
  const float m1 = wave_sum(g) * (1.f / D);
  const float m2 = wave_sum(g * xh) * (1.f / D);
  return rstd * (g - m1 - xh * m2);
}
// part[j][k] (+)= sum_r G[r][j] X[r][k] for a 64 x 64 block: thread = (j, eight k).  ``first``: write, else add to what this workgroup wrote
GRL_DEVINL void dw_acc(float* part, const float* G, const float* X, int R, bool first, int tid) {
  const int j = tid >> 3, k0 = (tid & 7) * 8;
  float acc[2][8];   // even rows | odd rows: two shorter rounding chains, folded at the end
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = 0.f;
  auto row = [&](int r, float (&a8)[8]) {
    const float g = G[r * D + j];
    const float4 a = *reinterpret_cast<const float4*>(X + r * D + k0);
    const float4 b = *reinterpret_cast<const float4*>(X + r * D + k0 + 4);
    a8[0] = fmaf(g, a.x, a8[0]);
    a8[1] = fmaf(g, a.y, a8[1]);
    a8[2] = fmaf(g, a.z, a8[2]);
    a8[3] = fmaf(g, a.w, a8[3]);
    a8[4] = fmaf(g, b.x, a8[4]);
    a8[5] = fmaf(g, b.y, a8[5]);
    a8[6] = fmaf(g, b.z, a8[6]);
    a8[7] = fmaf(g, b.w, a8[7]);
  };
  int r = 0;
  for (; r + 1 < R; r += 2) {
    row(r, acc[0]);
    row(r + 1, acc[1]);
  }
  if (r < R) row(r, acc[0]);
  float* p = part + j * D + k0;
#pragma unroll
  for (int e = 0; e < 8; ++e) p[e] = first ? acc[0][e] + acc[1][e] : p[e] + (acc[0][e] + acc[1][e]);
}
GRL_DEVINL void db_acc(float* part, const float* G, int R, bool first, int tid) {   // part[j] (+)= sum_r G[r][j]
  if (tid < D) {   // eight interleaved partial sums (rows mod 8), folded pairwise: no rounding chain longer than R / 8 + 3
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    int r = 0;
    for (; r + 8 <= R; r += 8)
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += G[(r + e) * D + tid];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (r + e < R) a[e] += G[(r + e) * D + tid];
    const float t = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    part[tid] = first ? t : part[tid] + t;
  }
}
// the per-wave LayerNorm parameter sums, folded in wave order: part_g[j] (+)= sum_w red[w][j], part_b[j] (+)= sum_w red[w][64 + j]
GRL_DEVINL void ln_fold(float* part_g, float* part_b, const float* red, bool first, int tid) {
  if (tid < 2 * D) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) a += red[w * 2 * D + tid];
    float* p = tid < D ? part_g + tid : part_b + (tid - D);
    *p = first ? a : *p + a;
  }
}
// the input rows of a layer: x_0 as saved, or the previous layer's normalised rows under ITS norm2 affine map
GRL_DEVINL float layer_input(const float* x0, const float* xh_prev, const float* g_prev, const float* b_prev, long long idx, int j) {
  return xh_prev == nullptr ? x0[idx] : fmaf(xh_prev[idx], g_prev[j], b_prev[j]);
}
GRL_DEVINL float* saved_slot(float* saved, long long rows, int l, int slot) { return saved + rows * D * (1 + 7 * l + slot); }   // slots: qkv 0..2, o 3, xhat1 4, h 5, xhat2 6

// Q, K, V (and dO) of head hh of one sample as [n][33] LDS images
GRL_DEVINL void stage_head(float* Qs, float* Ks, float* Vs, const float* qkv_rows, int n, int hh, int tid) {
  for (int idx = tid; idx < n * HD; idx += NT) {
    const int r = idx >> 5, c = idx & 31;
    const float* q = qkv_rows + (long long)r * 3 * D + hh * HD + c;
    Qs[r * LDH + c] = q[0];
    Ks[r * LDH + c] = q[D];
    Vs[r * LDH + c] = q[2 * D];
  }
}

// ------------------------------------------------------------------------------------------------ encoder forward
__global__ __launch_bounds__(NT) void transformer_fwd_kernel(const float* __restrict__ u, EncP P, float* saved, float* stats,
                                                             float* __restrict__ hidden, int B, int n, int d_in, int m0, int G, int S) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long rows = (long long)B * n;
  const int RM = S * n;                              // rows of a full group of S samples (<= 256)
  float* x0 = saved;
  float* U = smem;                                   // [RM][64] row image
  float *Ks = smem, *Vs = smem + RM * LDH, *Qs = smem + 2 * RM * LDH, *Pw = smem + 3 * RM * LDH + w * NMAX;   // attention phase
  float wv[D];
  for (int grp = blockIdx.x; grp * S < B; grp += gridDim.x) {   // a group: S consecutive samples (the last one of the batch may hold fewer)
    const int s0 = grp * S, ns = B - s0 < S ? B - s0 : S, R = ns * n;
    const long long g0 = (long long)s0 * n;
    {   // embedding
      const float bj = P.be[lane];
#pragma unroll 1
      for (int i = w; i < R; i += NW) {
        const float* ur = u + (g0 + i) * d_in;
        float a = bj;
        for (int k = 0; k < d_in; ++k) a = fmaf(ur[k], P.We[lane * d_in + k], a);
        x0[(g0 + i) * D + lane] = a;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < NLAYER; ++l) {
      const LayerP& L = P.L[l];
      float* qkv = saved_slot(saved, rows, l, 0);
      float* o = saved_slot(saved, rows, l, 3);
      float* xh1 = saved_slot(saved, rows, l, 4);
      float* h = saved_slot(saved, rows, l, 5);
      float* xh2 = saved_slot(saved, rows, l, 6);
      float* st = stats + ((long long)l * rows + g0) * 6;
      const float* xhp = l == 0 ? nullptr : saved_slot(saved, rows, l - 1, 6);
      const float* gp = l == 0 ? nullptr : P.L[l - 1].g2;
      const float* bp = l == 0 ? nullptr : P.L[l - 1].be2;
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = layer_input(x0, xhp, gp, bp, g0 * D + idx, idx & 63);
      __syncthreads();
#pragma unroll 1
      for (int part = 0; part < 3; ++part) {   // [q | k | v] = x Win^T + bin
        load_w_row(wv, L.Win + part * D * D, lane);
        const float bj = L.bin[part * D + lane];
#pragma unroll 1
        for (int i = w; i < R; i += NW) qkv[(g0 + i) * 3 * D + part * D + lane] = dot_row(U + i * D, wv, bj);
      }
      __syncthreads();
#pragma unroll 1
      for (int hh = 0; hh < 2; ++hh) {
        stage_head(Qs, Ks, Vs, qkv + g0 * 3 * D, R, hh, tid);
        __syncthreads();
        const int c = lane & 31, half = lane >> 5;
#pragma unroll 1
        for (int i = w; i < R; i += NW) {   // one wave per query row
          const int jb = (i / n) * n;   // the first row of this row's sample inside the group
          const float ql = Qs[i * LDH + c];
          float q[HD];
#pragma unroll
          for (int cc = 0; cc < HD; ++cc) q[cc] = lane_value(ql, cc);
          float mx = -INFINITY;   // the row's scores, then its exp, live in this wave's LDS row (each lane its own entries)
#pragma unroll 1
          for (int t = 0; t * 64 < n; ++t) {
            const int j = t * 64 + lane;
            float sc = -INFINITY;
            if (j < n) {
              sc = dot_head(q, Ks + (jb + j) * LDH) * SCALE;
            }
            Pw[j] = sc;
            mx = fmaxf(mx, sc);
          }
          mx = wave_max(mx);
          float ps = 0.f;
#pragma unroll 1
          for (int t = 0; t * 64 < n; ++t) {
            const int j = t * 64 + lane;
            const float p = j < n ? expf(Pw[j] - mx) : 0.f;
            Pw[j] = p;
            ps += p;
          }
          ps = wave_sum(ps);
          wave_lds_sync();
          float a = dot_strided(Pw, Vs + jb * LDH + c, LDH, half, n);
          a += __shfl_xor(a, 32, 64);
          if (lane < HD) o[(g0 + i) * D + hh * HD + c] = a / ps;
          if (lane == 0) {
            st[i * 6 + 2 + hh] = mx;
            st[i * 6 + 4 + hh] = ps;
          }
          wave_lds_sync();
        }
        __syncthreads();
      }
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = o[g0 * D + idx];
      __syncthreads();
      {   // y = LayerNorm(x + o Wo^T + bo)
        load_w_row(wv, L.Wo, lane);
        const float bj = L.bo[lane];
#pragma unroll 1
        for (int i = w; i < R; i += NW) {
          const float a = dot_row(U + i * D, wv, bj);
          const float z = layer_input(x0, xhp, gp, bp, (g0 + i) * D + lane, lane) + a;
          float xh, rstd;
          layer_norm(z, xh, rstd);
          xh1[(g0 + i) * D + lane] = xh;
          if (lane == 0) st[i * 6] = rstd;
        }
      }
      __syncthreads();
      const float g1j = L.g1[lane], be1j = L.be1[lane];
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = fmaf(xh1[g0 * D + idx], L.g1[idx & 63], L.be1[idx & 63]);
      __syncthreads();
      {   // relu(W1 y + b1)
        load_w_row(wv, L.W1, lane);
        const float bj = L.b1[lane];
#pragma unroll 1
        for (int i = w; i < R; i += NW) {
          const float a = dot_row(U + i * D, wv, bj);
          h[(g0 + i) * D + lane] = a > 0.f ? a : 0.f;
        }
      }
      __syncthreads();
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = h[g0 * D + idx];
      __syncthreads();
      {   // x' = LayerNorm(y + W2 h + b2)
        load_w_row(wv, L.W2, lane);
        const float bj = L.b2[lane];
#pragma unroll 1
        for (int i = w; i < R; i += NW) {
          const float f = dot_row(U + i * D, wv, bj);
          const float z = fmaf(xh1[(g0 + i) * D + lane], g1j, be1j) + f;
          float xh, rstd;
          layer_norm(z, xh, rstd);
          xh2[(g0 + i) * D + lane] = xh;
          if (lane == 0) st[i * 6 + 1] = rstd;
        }
      }
      __syncthreads();
    }
    {   // hidden = x_2[m0 .. m0+G) Wf^T + bf
      const LayerP& L = P.L[NLAYER - 1];
      const float* xh2 = saved_slot(saved, rows, NLAYER - 1, 6);
      for (int idx = tid; idx < ns * G * D; idx += NT) {   // row sl * G + ii = token m0 + ii of the group's sample sl
        const int r = idx >> 6, sl = r / G;
        U[idx] = fmaf(xh2[(g0 + sl * n + m0 + (r - sl * G)) * D + (idx & 63)], L.g2[idx & 63], L.be2[idx & 63]);
      }
      __syncthreads();
      load_w_row(wv, P.Wf, lane);
      const float bj = P.bf[lane];
#pragma unroll 1
      for (int i = w; i < ns * G; i += NW) hidden[((long long)s0 * G + i) * D + lane] = dot_row(U + i * D, wv, bj);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ encoder backward
// ws [gridDim.x][S * n][320]: this workgroup's gradient rows (d row 64 | d o 64 | d[q|k|v] 192), rewritten for every group
__global__ __launch_bounds__(NT) void transformer_bwd_kernel(const float* __restrict__ u, EncP P, const float* __restrict__ saved,
                                                             const float* __restrict__ stats, const float* __restrict__ dhidden,
                                                             float* ws, float* partial, int psize, int B, int n, int d_in, int m0, int G, int S) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long rows = (long long)B * n;
  float* sv = const_cast<float*>(saved);   // (read only here; saved_slot is shared with the forward)
  const float* x0 = saved;
  const int RM = S * n;                              // rows of a full group of S samples (<= 256)
  float *U = smem, *Vb = smem + RM * D;              // two [RM][64] row images
  float *Qs = smem, *Ks = smem + RM * LDH, *Vs = smem + 2 * RM * LDH, *DOs = smem + 3 * RM * LDH;   // attention phase
  float *Ms = smem + 4 * RM * LDH, *Ss = Ms + RM, *Dl = Ss + RM;
  float* scratch = smem + RM * (4 * LDH + 3);
  float *Pw = scratch + w * NMAX, *Dw = scratch + NW * NMAX + w * NMAX;
  float* red = scratch;                              // [NW][128] LayerNorm parameter sums (not live beside Pw / Dw)
  float* part = partial + (size_t)blockIdx.x * psize;
  float* gA = ws + (size_t)blockIdx.x * RM * WS_ROW; // [RM][64]  gradient of the current layer boundary's rows
  float* gO = gA + (size_t)RM * D;                   // [RM][64]  gradient of o
  float* gQ = gO + (size_t)RM * D;                   // [RM][192] gradient of [q | k | v]
  float wv[D];
  for (int grp = blockIdx.x; grp * S < B; grp += gridDim.x) {
    const bool first = grp == (int)blockIdx.x;
    const int s0 = grp * S, ns = B - s0 < S ? B - s0 : S, R = ns * n;
    const long long g0 = (long long)s0 * n;
    {   // hidden = x_2[mask] Wf^T + bf
      const LayerP& L = P.L[NLAYER - 1];
      const float* xh2 = saved_slot(sv, rows, NLAYER - 1, 6);
      for (int idx = tid; idx < ns * G * D; idx += NT) {
        const int r = idx >> 6, sl = r / G;
        U[idx] = dhidden[(long long)s0 * G * D + idx];
        Vb[idx] = fmaf(xh2[(g0 + sl * n + m0 + (r - sl * G)) * D + (idx & 63)], L.g2[idx & 63], L.be2[idx & 63]);
      }
      __syncthreads();
      dw_acc(part + P_WF, U, Vb, ns * G, first, tid);
      db_acc(part + P_BF, U, ns * G, first, tid);
      load_w_col(wv, P.Wf, lane);
#pragma unroll 1
      for (int i = w; i < R; i += NW) {
        const int sl = i / n, il = i - sl * n;
        gA[i * D + lane] = (il >= m0 && il < m0 + G) ? dot_row(U + (sl * G + il - m0) * D, wv, 0.f) : 0.f;
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int l = NLAYER - 1; l >= 0; --l) {
      const LayerP& L = P.L[l];
      float* pl = part + l * P_LAYER;
      const float* qkv = saved_slot(sv, rows, l, 0);
      const float* o = saved_slot(sv, rows, l, 3);
      const float* xh1 = saved_slot(sv, rows, l, 4);
      const float* h = saved_slot(sv, rows, l, 5);
      const float* xh2 = saved_slot(sv, rows, l, 6);
      const float* st = stats + ((long long)l * rows + g0) * 6;
      const float* xhp = l == 0 ? nullptr : saved_slot(sv, rows, l - 1, 6);
      const float* gp = l == 0 ? nullptr : P.L[l - 1].g2;
      const float* bp = l == 0 ? nullptr : P.L[l - 1].be2;
      {   // norm2: U = d(y + f), Vb = h
        const float gj = L.g2[lane];
        float dgam = 0.f, dbet = 0.f;
#pragma unroll 1
        for (int i = w; i < R; i += NW) {
          const float dy = gA[i * D + lane], xh = xh2[(g0 + i) * D + lane];
          U[i * D + lane] = layer_norm_bwd(dy, gj, xh, st[i * 6 + 1]);
          Vb[i * D + lane] = h[(g0 + i) * D + lane];
          dgam = fmaf(dy, xh, dgam);
          dbet += dy;
        }
        red[w * 2 * D + lane] = dgam;
        red[w * 2 * D + D + lane] = dbet;
      }
      __syncthreads();
      ln_fold(pl + P_G2, pl + P_BE2, red, first, tid);
      dw_acc(pl + P_W2, U, Vb, R, first, tid);
      db_acc(pl + P_B2, U, R, first, tid);
      __syncthreads();
      load_w_col(wv, L.W2, lane);   // Vb = d(W1 y + b1) = (dz W2) where the unit is on (relu'(0) = 0)
#pragma unroll 1
      for (int i = w; i < R; i += NW) {
        const float a = dot_row(U + i * D, wv, 0.f);
        Vb[i * D + lane] = Vb[i * D + lane] > 0.f ? a : 0.f;
      }
      __syncthreads();
      load_w_col(wv, L.W1, lane);   // d y = dz + Vb W1
#pragma unroll 1
      for (int i = w; i < R; i += NW) gA[i * D + lane] = U[i * D + lane] + dot_row(Vb + i * D, wv, 0.f);
      __syncthreads();
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = fmaf(xh1[g0 * D + idx], L.g1[idx & 63], L.be1[idx & 63]);
      __syncthreads();
      dw_acc(pl + P_W1, Vb, U, R, first, tid);
      db_acc(pl + P_B1, Vb, R, first, tid);
      __syncthreads();
      {   // norm1: U = d(x + a) (kept in gA: it is the residual's share of d x), Vb = o
        const float gj = L.g1[lane];
        float dgam = 0.f, dbet = 0.f;
#pragma unroll 1
        for (int i = w; i < R; i += NW) {
          const float dy = gA[i * D + lane], xh = xh1[(g0 + i) * D + lane];
          const float dz = layer_norm_bwd(dy, gj, xh, st[i * 6]);
          U[i * D + lane] = dz;
          gA[i * D + lane] = dz;
          Vb[i * D + lane] = o[(g0 + i) * D + lane];
          dgam = fmaf(dy, xh, dgam);
          dbet += dy;
        }
        red[w * 2 * D + lane] = dgam;
        red[w * 2 * D + D + lane] = dbet;
      }
      __syncthreads();
      ln_fold(pl + P_G1, pl + P_BE1, red, first, tid);
      dw_acc(pl + P_WO, U, Vb, R, first, tid);
      db_acc(pl + P_BO, U, R, first, tid);
      load_w_col(wv, L.Wo, lane);
#pragma unroll 1
      for (int i = w; i < R; i += NW) gO[i * D + lane] = dot_row(U + i * D, wv, 0.f);
      __syncthreads();
#pragma unroll 1
      for (int hh = 0; hh < 2; ++hh) {
        stage_head(Qs, Ks, Vs, qkv + g0 * 3 * D, R, hh, tid);
        for (int idx = tid; idx < R * HD; idx += NT) DOs[(idx >> 5) * LDH + (idx & 31)] = gO[(idx >> 5) * D + hh * HD + (idx & 31)];
        for (int i = tid; i < R; i += NT) {
          Ms[i] = st[i * 6 + 2 + hh];
          Ss[i] = st[i * 6 + 4 + hh];
        }
        __syncthreads();
        const int c = lane & 31, half = lane >> 5;
#pragma unroll 1
        for (int i = w; i < R; i += NW) {   // one wave per query row: delta_i and d q_i
          const int jb = (i / n) * n;
          const float ql = Qs[i * LDH + c], dl = DOs[i * LDH + c];
          float q[HD], dO[HD];
#pragma unroll
          for (int cc = 0; cc < HD; ++cc) {
            q[cc] = lane_value(ql, cc);
            dO[cc] = lane_value(dl, cc);
          }
          const float mi = Ms[i], inv = 1.f / Ss[i];
          float acc = 0.f;   // p and d p of the row live in this wave's LDS rows (each lane its own entries)
#pragma unroll 1
          for (int t = 0; t * 64 < n; ++t) {
            const int j = t * 64 + lane;
            float pv = 0.f, dpv = 0.f;
            if (j < n) {
              pv = expf(dot_head(q, Ks + (jb + j) * LDH) * SCALE - mi) * inv;
              dpv = dot_head(dO, Vs + (jb + j) * LDH);
            }
            Pw[j] = pv;
            Dw[j] = dpv;
            acc = fmaf(pv, dpv, acc);
          }
          const float delta = wave_sum(acc);
#pragma unroll 1
          for (int t = 0; t * 64 < n; ++t) {
            const int j = t * 64 + lane;
            Dw[j] = Pw[j] * (Dw[j] - delta) * SCALE;
          }
          wave_lds_sync();
          float a = dot_strided(Dw, Ks + jb * LDH + c, LDH, half, n);
          a += __shfl_xor(a, 32, 64);
          if (lane < HD) gQ[i * 3 * D + hh * HD + c] = a;
          if (lane == 0) Dl[i] = delta;
          wave_lds_sync();
        }
        __syncthreads();
#pragma unroll 1
        for (int j = w; j < R; j += NW) {   // one wave per key row: d k_j and d v_j
          const int ib = (j / n) * n;
          const float kl = Ks[j * LDH + c], vl = Vs[j * LDH + c];
          float kk[HD], vv[HD];
#pragma unroll
          for (int cc = 0; cc < HD; ++cc) {
            kk[cc] = lane_value(kl, cc);
            vv[cc] = lane_value(vl, cc);
          }
#pragma unroll 1
          for (int t = 0; t * 64 < n; ++t) {
              const int il = t * 64 + lane, i = ib + il;
              float pv = 0.f, dsv = 0.f;
              if (il < n) {
                pv = expf(dot_head(kk, Qs + i * LDH) * SCALE - Ms[i]) * (1.f / Ss[i]);
                dsv = pv * (dot_head(vv, DOs + i * LDH) - Dl[i]) * SCALE;
              }
              Pw[il] = pv;
              Dw[il] = dsv;
            }
          wave_lds_sync();
          float dv = dot_strided(Pw, DOs + ib * LDH + c, LDH, half, n);
          float dk = dot_strided(Dw, Qs + ib * LDH + c, LDH, half, n);
          dv += __shfl_xor(dv, 32, 64);
          dk += __shfl_xor(dk, 32, 64);
          if (lane < HD) {
            gQ[j * 3 * D + D + hh * HD + c] = dk;
            gQ[j * 3 * D + 2 * D + hh * HD + c] = dv;
          }
          wave_lds_sync();
        }
        __syncthreads();
      }
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = layer_input(x0, xhp, gp, bp, g0 * D + idx, idx & 63);
#pragma unroll 1
      for (int part3 = 0; part3 < 3; ++part3) {   // d Win, d bin and d x += d[q|k|v] Win, one third at a time
        for (int idx = tid; idx < R * D; idx += NT) Vb[idx] = gQ[(idx >> 6) * 3 * D + part3 * D + (idx & 63)];
        __syncthreads();
        dw_acc(pl + P_WIN + part3 * D * D, Vb, U, R, first, tid);
        db_acc(pl + P_BIN + part3 * D, Vb, R, first, tid);
        load_w_col(wv, L.Win + part3 * D * D, lane);
#pragma unroll 1
        for (int i = w; i < R; i += NW) gA[i * D + lane] += dot_row(Vb + i * D, wv, 0.f);
        __syncthreads();
      }
    }
    {   // embedding: d We, d be
      for (int idx = tid; idx < R * D; idx += NT) U[idx] = gA[idx];
      __syncthreads();
      const int j = tid >> 3;
      for (int k = tid & 7; k < d_in; k += 8) {
        float a = 0.f;
        for (int r = 0; r < R; ++r) a = fmaf(U[r * D + j], u[(g0 + r) * d_in + k], a);
        float* p = part + P_WE + j * d_in + k;
        *p = first ? a : *p + a;
      }
      db_acc(part + P_BE, U, R, first, tid);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ post_fc head
// mean = hidden Wm^T + bm, pre = hidden Ws^T + bs, sigma = softplus(pre + shift) + min_std; A <= 16 outputs each (gnn_gaussian_policy_diag.py:65-83)
GRL_DEVINL float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch's threshold
GRL_DEVINL float sigmoid_f(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
constexpr int HEAD_PARTIAL = 2 * AMAX * D + 2 * AMAX;   // [dWm 16x64 | dWs 16x64 | dbm 16 | dbs 16], rows a >= A are zeros

int head_blocks(long long R) {
  long long b = (R + 63) / 64;
  if (b < 1) b = 1;
  return (int)(b < BLOCKS_MAX ? b : BLOCKS_MAX);
}

// thread = (row of eight, output of 32: 0..15 mean, 16..31 std)
__global__ __launch_bounds__(256) void postfc_head_fwd_kernel(const float* __restrict__ hidden, const float* __restrict__ Wm,
                                                              const float* __restrict__ bm, const float* __restrict__ Ws,
                                                              const float* __restrict__ bs, float shift, float min_std,
                                                              float* __restrict__ mean, float* __restrict__ sigma, float* __restrict__ pre,
                                                              long long R, int A) {
  const int a2 = threadIdx.x & 31, a = a2 & 15;
  const bool is_std = a2 >= 16;
  if (a >= A) return;
  const float* wrow = (is_std ? Ws : Wm) + a * D;
  const float b = (is_std ? bs : bm)[a];
  for (long long r = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); r < R; r += (long long)gridDim.x * 8) {
    const float* hr = hidden + r * D;
    float s = b;
#pragma unroll 8
    for (int k = 0; k < D; ++k) s = fmaf(hr[k], wrow[k], s);
    if (is_std) {
      pre[r * A + a] = s;
      sigma[r * A + a] = softplus_f(s + shift) + min_std;
    } else {
      mean[r * A + a] = s;
    }
  }
}

// d hidden[r][k] = sum_a dmean[r][a] Wm[a][k] + dsigma[r][a] sigmoid(pre + shift) Ws[a][k]: one wave per row, lane = k
__global__ __launch_bounds__(256) void postfc_head_bwd_dx_kernel(const float* __restrict__ Wm, const float* __restrict__ Ws,
                                                                 const float* __restrict__ pre, float shift, const float* __restrict__ dmean,
                                                                 const float* __restrict__ dsigma, float* __restrict__ dhidden, long long R,
                                                                 int A) {
  const int k = threadIdx.x & 63;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += (long long)gridDim.x * 4) {
    float s = 0.f;
    for (int a = 0; a < A; ++a) {
      s = fmaf(dmean[r * A + a], Wm[a * D + k], s);
      s = fmaf(dsigma[r * A + a] * sigmoid_f(pre[r * A + a] + shift), Ws[a * D + k], s);
    }
    dhidden[r * D + k] = s;
  }
}

// workgroup b sums the rows of ITS contiguous chunk in order: thread = (output of 32, eight k); every entry of its partial row is written
__global__ __launch_bounds__(256) void postfc_head_bwd_dw_kernel(const float* __restrict__ hidden, const float* __restrict__ pre, float shift,
                                                                 const float* __restrict__ dmean, const float* __restrict__ dsigma,
                                                                 float* __restrict__ partial, long long R, int A) {
  const int a2 = threadIdx.x >> 3, a = a2 & 15, k0 = (threadIdx.x & 7) * 8;
  const bool is_std = a2 >= 16;
  const long long chunk = (R + gridDim.x - 1) / gridDim.x;
  const long long r0 = (long long)blockIdx.x * chunk;
  const long long r1 = r0 + chunk < R ? r0 + chunk : R;
  float acc[8], ab = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (a < A)
    for (long long r = r0; r < r1; ++r) {
      const float g = is_std ? dsigma[r * A + a] * sigmoid_f(pre[r * A + a] + shift) : dmean[r * A + a];
      const float* hr = hidden + r * D + k0;
      ab += g;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(g, hr[e], acc[e]);
    }
  float* out = partial + (size_t)blockIdx.x * HEAD_PARTIAL;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[a2 * D + k0 + e] = acc[e];
  if ((threadIdx.x & 7) == 0) out[2 * AMAX * D + a2] = ab;
}

bool fill_params(EncP& P, const float* const* params) {
  for (int i = 0; i < N_PARAMS; ++i)
    if (params[i] == nullptr) return false;
  int k = 0;
  P.We = params[k++];
  P.be = params[k++];
  for (int l = 0; l < NLAYER; ++l) {
    LayerP& L = P.L[l];
    L.Win = params[k++]; L.bin = params[k++]; L.Wo = params[k++]; L.bo = params[k++]; L.g1 = params[k++]; L.be1 = params[k++];
    L.W1 = params[k++]; L.b1 = params[k++]; L.W2 = params[k++]; L.b2 = params[k++]; L.g2 = params[k++]; L.be2 = params[k++];
  }
  P.Wf = params[k++];
  P.bf = params[k++];
  return true;
}
bool shape_ok(int B, int n, int d_in, int m0, int G) {
  return B >= 0 && n >= 1 && n <= NMAX && d_in >= 1 && d_in <= DIN_MAX && m0 >= 0 && G >= 1 && m0 + G <= n;
}

}  // namespace

extern "C" {

int grl_transformer_blocks(int B, int n) { return n < 1 || n > NMAX ? -2 : tf_blocks(B, n); }
int grl_transformer_group_rows(int B, int n) { return n < 1 || n > NMAX ? -2 : tf_group(B, n) * n; }
int grl_transformer_partial_size(int d_in) { return d_in < 1 || d_in > DIN_MAX ? -2 : P_WE + D * d_in; }
int grl_transformer_ws_row(void) { return WS_ROW; }

int grl_transformer_fwd(const float* u, const float* const* params, float* saved, float* stats, float* hidden, int B, int n, int d_in, int m0,
                        int G, hipStream_t stream) {
  EncP P;
  if (!shape_ok(B, n, d_in, m0, G) || !fill_params(P, params)) return -2;
  if (B == 0) return 0;
  const int S = tf_group(B, n), lds = (int)fwd_lds_bytes(S * n);
  GRL_ONCE(hipFuncSetAttribute((const void*)transformer_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds_bytes(NMAX)));
  hipLaunchKernelGGL(transformer_fwd_kernel, dim3(tf_blocks(B, n)), dim3(NT), lds, stream, u, P, saved, stats, hidden, B, n, d_in, m0, G, S);
  GRL_CHECK_LAUNCH();
  return 0;
}

int grl_transformer_bwd(const float* u, const float* const* params, const float* saved, const float* stats, const float* dhidden, float* ws,
                        float* partial, int B, int n, int d_in, int m0, int G, hipStream_t stream) {
  EncP P;
  if (!shape_ok(B, n, d_in, m0, G) || B < 1 || !fill_params(P, params)) return -2;
  const int S = tf_group(B, n), lds = (int)bwd_lds_bytes(S * n);
  GRL_ONCE(hipFuncSetAttribute((const void*)transformer_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwd_lds_bytes(NMAX)));
  hipLaunchKernelGGL(transformer_bwd_kernel, dim3(tf_blocks(B, n)), dim3(NT), lds, stream, u, P, saved, stats, dhidden, ws, partial,
                     P_WE + D * d_in, B, n, d_in, m0, G, S);
  GRL_CHECK_LAUNCH();
  return 0;
}

int grl_postfc_head_partial_size(void) { return HEAD_PARTIAL; }
int grl_postfc_head_blocks(int n_rows) { return head_blocks(n_rows); }

int grl_postfc_head_fwd(const float* hidden, const float* Wm, const float* bm, const float* Ws, const float* bs, float shift, float min_std,
                        float* mean, float* sigma, float* pre, int n_rows, int A, hipStream_t stream) {
  if (n_rows < 0 || A < 1 || A > AMAX) return -2;
  if (n_rows == 0) return 0;
  const long long b = ((long long)n_rows + 7) / 8;
  hipLaunchKernelGGL(postfc_head_fwd_kernel, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, stream, hidden, Wm, bm, Ws, bs, shift,
                     min_std, mean, sigma, pre, (long long)n_rows, A);
  GRL_CHECK_LAUNCH();
  return 0;
}

int grl_postfc_head_bwd(const float* hidden, const float* Wm, const float* Ws, const float* pre, float shift, const float* dmean,
                        const float* dsigma, float* dhidden, float* partial, int n_rows, int A, hipStream_t stream) {
  if (n_rows < 0 || A < 1 || A > AMAX) return -2;
  if (n_rows > 0) {
    const long long b = ((long long)n_rows + 3) / 4;
    hipLaunchKernelGGL(postfc_head_bwd_dx_kernel, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, stream, Wm, Ws, pre, shift, dmean,
                       dsigma, dhidden, (long long)n_rows, A);
    GRL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(postfc_head_bwd_dw_kernel, dim3(head_blocks(n_rows)), dim3(256), 0, stream, hidden, pre, shift, dmean, dsigma, partial,
                     (long long)n_rows, A);
  GRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
