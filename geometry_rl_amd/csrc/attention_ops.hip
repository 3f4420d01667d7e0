// Key/query attention of the EMPN layer (reference ponita.py:21-24,126-161: SeparableFiberBundleConv(attention=True)), fp32 build only.
//
//   k = x Wk^T + bk, q = x Wq^T + bq                         [N,16,128]   (kq_project_*)
//   l[e,o]  = <k[src e,o,:], q[dst e,o,:]> / sqrt(128)                     (edge_logits_*)
//   M       = max over ALL (e,o) of l       -- ONE scalar per launch, part of the graph: the gradient flows through it
//   p[e,o]  = exp(l[e,o] - M),  S[d,o] = sum_{e->d} p[e,o]
//   a[e,o]  = p[e,o] / (S[dst e,o] + 1e-6)                                 (edge_attend_*)
//   x1[d,o,:] = sum_{e->d} a[e,o] msg[e,o,:]
//
// This is NOT the per-destination softmax of node_ops.hip (softmax_agg_*: per-segment maximum, 1e-16): the shift is global, so a
// destination whose logits sit far below the batch maximum has S comparable to the 1e-6 and its weights do not sum to 1.
// Backward, with da[e,o] = sum_c dx1[dst e,o,c] msg[e,o,c], A[d,o] = sum_{e->d} a, T[d,o] = sum_{e->d} a da:
//   dmsg[e,o,:] = a[e,o] dx1[dst e,o,:]
//   dl[e,o]     = a[e,o] (da[e,o] - T[dst e,o])              (holds with the 1e-6 as well)
//   dM          = - sum_{d,o} (1 - A[d,o]) T[d,o]            (zero for an exact softmax; here A < 1)
//   dl[argmax] += dM
// Ties of the maximum have measure zero; the LOWEST flat index (e * 16 + o, destination-sorted edge order) takes dM.
//
// Every launch is stream-ordered, reads nothing on the host and uses no atomics: per-row sums run over the CSR segments in index order,
// wave sums are xor butterflies, per-block partials are finished by one workgroup in block order -- two runs give the same bits.  Every
// row of every output is written (a node without edges gets exact zeros and never reads M).
#include "grl_common.h"

namespace {

constexpr int C = 64, O = 16, KD = 128, KQ = 2 * KD;
constexpr int KQ_PARTIAL = KQ * C + KQ;   // [dWk 128x64 | dWq 128x64 | dbk 128 | dbq 128]
constexpr int ROW_BLOCKS_MAX = 2048;      // workgroups (4 waves, one row per wave and iteration) of the row kernels
constexpr int KQ_BWD_BLOCKS_MAX = 512;
constexpr float INV_SQRT_KD = 0.08838834764831845f;   // 1 / sqrt(128)
constexpr float ATT_EPS = 1e-6f;

int row_blocks(long long rows) {
  long long b = (rows + 3) / 4;
  if (b < 1) b = 1;
  return (int)(b < ROW_BLOCKS_MAX ? b : ROW_BLOCKS_MAX);
}
int kq_bwd_blocks(long long rows) {
  long long b = (rows + 63) / 64;
  if (b < 1) b = 1;
  return (int)(b < KQ_BWD_BLOCKS_MAX ? b : KQ_BWD_BLOCKS_MAX);
}

GRL_DEVINL float wave_sum(float v) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ key / query projection
// Thread j of 256 owns output column j of [k | q] and keeps its weight row (64 floats) in registers; the row index is uniform over the
// workgroup, so the x operands are scalar loads.  Four rows per iteration.  Weights are read with 4-byte loads: a parameter may sit at
// any float offset of a flat buffer and the numbers must not depend on it.
__global__ __launch_bounds__(256) void kq_project_fwd_kernel(const float* __restrict__ x, const float* __restrict__ Wk,
                                                             const float* __restrict__ bk, const float* __restrict__ Wq,
                                                             const float* __restrict__ bq, float* __restrict__ k, float* __restrict__ q,
                                                             int n_rows) {
  const int j = threadIdx.x, jj = j & (KD - 1);
  const float* wrow = (j < KD ? Wk : Wq) + jj * C;
  float w[C];
#pragma unroll
  for (int c = 0; c < C; ++c) w[c] = wrow[c];
  const float b = (j < KD ? bk : bq)[jj];
  float* out = (j < KD ? k : q) + jj;
  for (long long r0 = (long long)blockIdx.x * 4; r0 < n_rows; r0 += (long long)gridDim.x * 4) {
    float acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long r = r0 + u < n_rows ? r0 + u : (long long)n_rows - 1;   // (a clamped duplicate: computed, not stored)
      const float* xr = x + r * C;
      float s = b;
#pragma unroll
      for (int c = 0; c < C; ++c) s = fmaf(xr[c], w[c], s);
      acc[u] = s;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r0 + u < n_rows) out[(r0 + u) * KD] = acc[u];
  }
}

// dx[r,c] = sum_j dk[r,j] Wk[j,c] + sum_j dq[r,j] Wq[j,c]: [Wk ; Wq] (256 x 64) in LDS as it lies in memory, one wave per row and
// iteration, lane = channel, the row's 256 gradients are wave-uniform (scalar) loads.  j runs 0 .. 255 in order.
__global__ __launch_bounds__(256) void kq_project_bwd_dx_kernel(const float* __restrict__ Wk, const float* __restrict__ Wq,
                                                                const float* __restrict__ dk, const float* __restrict__ dq,
                                                                float* __restrict__ dx, int n_rows) {
  __shared__ float W[KQ * C];
  for (int i = threadIdx.x; i < KD * C; i += 256) {
    W[i] = Wk[i];
    W[KD * C + i] = Wq[i];
  }
  __syncthreads();
  const int c = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long long r = (long long)blockIdx.x * 4 + wv; r < n_rows; r += (long long)gridDim.x * 4) {
    const float* gk = dk + r * KD;
    const float* gq = dq + r * KD;
    float s = 0.f;
#pragma unroll 8
    for (int j = 0; j < KD; ++j) s = fmaf(gk[j], W[j * C + c], s);
#pragma unroll 8
    for (int j = 0; j < KD; ++j) s = fmaf(gq[j], W[(KD + j) * C + c], s);
    dx[r * C + c] = s;
  }
}

// Weight gradients: thread j owns row j of [dWk ; dWq] (64 accumulators) and dbias[j]; workgroup b sums the rows of ITS contiguous
// chunk in order and writes its whole partial row (zeros for an empty chunk).
__global__ __launch_bounds__(256) void kq_project_bwd_dw_kernel(const float* __restrict__ x, const float* __restrict__ dk,
                                                                const float* __restrict__ dq, float* __restrict__ partial, int n_rows) {
  const int j = threadIdx.x, jj = j & (KD - 1);
  const float* g = (j < KD ? dk : dq) + jj;
  const long long chunk = ((long long)n_rows + gridDim.x - 1) / gridDim.x;
  const long long r0 = (long long)blockIdx.x * chunk;
  const long long r1 = r0 + chunk < n_rows ? r0 + chunk : (long long)n_rows;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  float ab = 0.f;
  for (long long r = r0; r < r1; ++r) {
    const float gj = g[r * KD];
    const float* xr = x + r * C;
    ab += gj;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(gj, xr[c], acc[c]);
  }
  float* out = partial + (size_t)blockIdx.x * KQ_PARTIAL;
#pragma unroll
  for (int c = 0; c < C; ++c) out[j * C + c] = acc[c];
  out[KQ * C + j] = ab;
}

// ------------------------------------------------------------------------------------------------ edge logits
// One wave per (e, o) row, lane = two of the 128 key channels.  Each wave keeps the (maximum, first flat index) of the rows it visits
// (rows ascend per wave, a strictly greater value replaces); the workgroup's four are merged in LDS and written as this block's partial.
GRL_DEVINL bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void edge_logits_fwd_kernel(const float* __restrict__ k, const float* __restrict__ q,
                                                              const int* __restrict__ e_src, const int* __restrict__ e_dst, int n_edges,
                                                              float* __restrict__ logit, float* __restrict__ pmax,
                                                              int* __restrict__ pidx) {
  __shared__ float smax[4];
  __shared__ int sidx[4];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long n_rows = (long long)n_edges * O;
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (long long row = (long long)blockIdx.x * 4 + wv; row < n_rows; row += (long long)gridDim.x * 4) {
    const int e = (int)(row >> 4), o = (int)(row & 15);
    const float2 kv = *reinterpret_cast<const float2*>(k + ((size_t)e_src[e] * O + o) * KD + 2 * lane);
    const float2 qv = *reinterpret_cast<const float2*>(q + ((size_t)e_dst[e] * O + o) * KD + 2 * lane);
    const float l = wave_sum(fmaf(kv.x, qv.x, kv.y * qv.y)) * INV_SQRT_KD;
    if (lane == 0) logit[row] = l;
    if (l > best) { best = l; besti = (int)row; }
  }
  if (lane == 0) { smax[wv] = best; sidx[wv] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float bv = smax[0];
    int bi = sidx[0];
    for (int w = 1; w < 4; ++w)
      if (better(smax[w], sidx[w], bv, bi)) { bv = smax[w]; bi = sidx[w]; }
    pmax[blockIdx.x] = bv;
    pidx[blockIdx.x] = bi;
  }
}
// the finish: block partials in block order -> M and the flat index of its first occurrence
__global__ __launch_bounds__(64) void edge_logits_max_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx, int n_blocks,
                                                             float* __restrict__ maxval, int* __restrict__ argmax) {
  if (threadIdx.x != 0) return;
  float bv = pmax[0];
  int bi = pidx[0];
  for (int b = 1; b < n_blocks; ++b)
    if (better(pmax[b], pidx[b], bv, bi)) { bv = pmax[b]; bi = pidx[b]; }
  maxval[0] = bv;
  argmax[0] = bi;
}

// dq[d,o,:] = 1/sqrt(128) sum_{e->d} dl[e,o] k[src e,o,:]   (destination-sorted rows rowptr_d[d] .. rowptr_d[d+1])
// dk[s,o,:] = 1/sqrt(128) sum_{i: source-sorted edges of s} dl[s2d[i],o] q[dst_s[i],o,:]
// rows 0 .. n_dst*16 of the launch are the dq rows, the n_src*16 behind them the dk rows; one wave per row, lane = two channels
__global__ __launch_bounds__(256) void edge_logits_bwd_kernel(const float* __restrict__ k, const float* __restrict__ q,
                                                              const float* __restrict__ dl, const int* __restrict__ rowptr_d,
                                                              const int* __restrict__ src_d, int n_dst, const int* __restrict__ rowptr_s,
                                                              const int* __restrict__ dst_s, const int* __restrict__ s2d, int n_src,
                                                              float* __restrict__ dk, float* __restrict__ dq) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long rows_q = (long long)n_dst * O, n_rows = rows_q + (long long)n_src * O;
  for (long long row = (long long)blockIdx.x * 4 + wv; row < n_rows; row += (long long)gridDim.x * 4) {
    float2 s = make_float2(0.f, 0.f);
    if (row < rows_q) {
      const int d = (int)(row >> 4), o = (int)(row & 15);
      const int e0 = rowptr_d[d], e1 = rowptr_d[d + 1];
      for (int e = e0; e < e1; ++e) {
        const float g = dl[(size_t)e * O + o];
        const float2 kv = *reinterpret_cast<const float2*>(k + ((size_t)src_d[e] * O + o) * KD + 2 * lane);
        s.x = fmaf(g, kv.x, s.x);
        s.y = fmaf(g, kv.y, s.y);
      }
      *reinterpret_cast<float2*>(dq + (size_t)row * KD + 2 * lane) = make_float2(s.x * INV_SQRT_KD, s.y * INV_SQRT_KD);
    } else {
      const long long rs = row - rows_q;
      const int n = (int)(rs >> 4), o = (int)(rs & 15);
      const int i0 = rowptr_s[n], i1 = rowptr_s[n + 1];
      for (int i = i0; i < i1; ++i) {
        const float g = dl[(size_t)s2d[i] * O + o];
        const float2 qv = *reinterpret_cast<const float2*>(q + ((size_t)dst_s[i] * O + o) * KD + 2 * lane);
        s.x = fmaf(g, qv.x, s.x);
        s.y = fmaf(g, qv.y, s.y);
      }
      *reinterpret_cast<float2*>(dk + (size_t)rs * KD + 2 * lane) = make_float2(s.x * INV_SQRT_KD, s.y * INV_SQRT_KD);
    }
  }
}

// ------------------------------------------------------------------------------------------------ attend and aggregate
// One wave per (d, o) row over the destination-sorted segment, lane = channel (as softmax_agg_* walks it).  M is read only by a row
// that has edges.  comp[d,o] = 1e-6 / (S + 1e-6) = 1 - A[d,o], kept for the backward: formed as 1 - sum a it would be a difference of
// two numbers near 1 wherever S is far above the 1e-6.
__global__ __launch_bounds__(256) void edge_attend_fwd_kernel(const float* __restrict__ logit, const float* __restrict__ maxval,
                                                              const float* __restrict__ msg, const int* __restrict__ rowptr, int n_dst,
                                                              float* __restrict__ a, float* __restrict__ comp,
                                                              float* __restrict__ x1) {
  const int c = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long n_rows = (long long)n_dst * O;
  for (long long row = (long long)blockIdx.x * 4 + wv; row < n_rows; row += (long long)gridDim.x * 4) {
    const int d = (int)(row >> 4), o = (int)(row & 15);
    const int e0 = rowptr[d], e1 = rowptr[d + 1];
    float num = 0.f, cmp = 1.f;
    if (e1 > e0) {
      const float M = maxval[0];
      float S = 0.f;
      for (int e = e0; e < e1; ++e) S += expf(logit[(size_t)e * O + o] - M);
      const float den = S + ATT_EPS;
      cmp = ATT_EPS / den;
      for (int e = e0; e < e1; ++e) {
        const size_t i = (size_t)e * O + o;
        const float w = expf(logit[i] - M) / den;
        if (c == 0) a[i] = w;
        num = fmaf(w, msg[i * C + c], num);
      }
    }
    if (c == 0) comp[row] = cmp;
    x1[(size_t)row * C + c] = num;
  }
}

// dmsg, dl (without the dM term) and this block's part of dM.  Pass 1 leaves da[e,o] in dl[e,o] (written and read back by lane 0 alone)
// and sums T; pass 2 turns it into a (da - T).
__global__ __launch_bounds__(256) void edge_attend_bwd_kernel(const float* __restrict__ a, const float* __restrict__ msg,
                                                              const float* __restrict__ comp, const float* __restrict__ dx1,
                                                              const int* __restrict__ rowptr, int n_dst, float* __restrict__ dmsg,
                                                              float* dl, float* __restrict__ pdm) {
  __shared__ float sdm[4];
  const int c = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long n_rows = (long long)n_dst * O;
  float dm = 0.f;
  for (long long row = (long long)blockIdx.x * 4 + wv; row < n_rows; row += (long long)gridDim.x * 4) {
    const int d = (int)(row >> 4), o = (int)(row & 15);
    const int e0 = rowptr[d], e1 = rowptr[d + 1];
    if (e1 <= e0) continue;
    const float g = dx1[(size_t)row * C + c];
    float T = 0.f;
    for (int e = e0; e < e1; ++e) {
      const size_t i = (size_t)e * O + o;
      const float w = a[i];
      const float da = wave_sum(g * msg[i * C + c]);
      dmsg[i * C + c] = w * g;
      if (c == 0) dl[i] = da;
      T = fmaf(w, da, T);
    }
    if (c == 0)
      for (int e = e0; e < e1; ++e) {
        const size_t i = (size_t)e * O + o;
        dl[i] = a[i] * (dl[i] - T);
      }
    dm -= comp[row] * T;
  }
  if (c == 0) sdm[wv] = dm;
  __syncthreads();
  if (threadIdx.x == 0) pdm[blockIdx.x] = ((sdm[0] + sdm[1]) + sdm[2]) + sdm[3];
}
// the finish: dM = the block partials in block order, added to dl at the stored argmax
// (an index outside the E * 16 rows -- logits that were all NaN leave none -- is not written to)
__global__ __launch_bounds__(64) void edge_attend_dm_kernel(const float* __restrict__ pdm, int n_blocks, const int* __restrict__ argmax,
                                                            const int* __restrict__ rowptr, int n_dst, float* __restrict__ dl) {
  if (threadIdx.x != 0) return;
  float s = 0.f;
  for (int b = 0; b < n_blocks; ++b) s += pdm[b];
  const long long i = argmax[0], n_rows = (long long)rowptr[n_dst] * O;
  if (i >= 0 && i < n_rows) dl[i] += s;
}

}  // namespace

extern "C" {

// workgroups of the row kernels for n_rows rows = the length of their per-block partial arrays (pmax / pidx / pdm)
int grl_attention_blocks(int n_rows) { return row_blocks(n_rows); }
int grl_kq_partial_size() { return KQ_PARTIAL; }
int grl_kq_bwd_blocks(int n_rows) { return kq_bwd_blocks(n_rows); }

int grl_kq_project_fwd(const float* x, const float* Wk, const float* bk, const float* Wq, const float* bq, float* k, float* q, int n_rows,
                       hipStream_t stream) {
  if (n_rows <= 0) return 0;
  const long long b = ((long long)n_rows + 3) / 4;
  hipLaunchKernelGGL(kq_project_fwd_kernel, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, stream, x, Wk, bk, Wq, bq, k, q, n_rows);
  GRL_CHECK_LAUNCH();
  return 0;
}

// partial: [grl_kq_bwd_blocks(n_rows)][grl_kq_partial_size()]; every row of it is written (n_rows = 0: one row of zeros)
int grl_kq_project_bwd(const float* x, const float* Wk, const float* Wq, const float* dk, const float* dq, float* dx, float* partial,
                       int n_rows, hipStream_t stream) {
  if (n_rows < 0) return -2;
  if (n_rows > 0) {
    hipLaunchKernelGGL(kq_project_bwd_dx_kernel, dim3(row_blocks(n_rows) < 1024 ? row_blocks(n_rows) : 1024), dim3(256), 0, stream, Wk, Wq,
                       dk, dq, dx, n_rows);
    GRL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(kq_project_bwd_dw_kernel, dim3(kq_bwd_blocks(n_rows)), dim3(256), 0, stream, x, dk, dq, partial, n_rows);
  GRL_CHECK_LAUNCH();
  return 0;
}

// logit [E,16] in destination-sorted edge order; pmax / pidx: [grl_attention_blocks(E * 16)] workspaces; maxval float[1], argmax int[1].
// n_edges must be positive (an empty maximum does not exist: the caller launches nothing that reads M)
int grl_edge_logits_fwd(const float* k, const float* q, const int* e_src, const int* e_dst, int n_edges, float* logit, float* pmax,
                        int* pidx, float* maxval, int* argmax, hipStream_t stream) {
  if (n_edges <= 0 || (long long)n_edges * O > 0x7fffffffLL) return -2;
  const int blocks = row_blocks((long long)n_edges * O);
  hipLaunchKernelGGL(edge_logits_fwd_kernel, dim3(blocks), dim3(256), 0, stream, k, q, e_src, e_dst, n_edges, logit, pmax, pidx);
  GRL_CHECK_LAUNCH();
  hipLaunchKernelGGL(edge_logits_max_kernel, dim3(1), dim3(64), 0, stream, pmax, pidx, blocks, maxval, argmax);
  GRL_CHECK_LAUNCH();
  return 0;
}

// dk [n_src,16,128], dq [n_dst,16,128]: every row written (zeros for a node without edges; dl is not read when there are no edges)
int grl_edge_logits_bwd(const float* k, const float* q, const float* dl, const int* rowptr_d, const int* src_d, int n_dst,
                        const int* rowptr_s, const int* dst_s, const int* s2d, int n_src, float* dk, float* dq, hipStream_t stream) {
  if (n_dst < 0 || n_src < 0) return -2;
  const long long rows = ((long long)n_dst + n_src) * O;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(edge_logits_bwd_kernel, dim3(row_blocks(rows)), dim3(256), 0, stream, k, q, dl, rowptr_d, src_d, n_dst, rowptr_s,
                     dst_s, s2d, n_src, dk, dq);
  GRL_CHECK_LAUNCH();
  return 0;
}

// a [E,16], comp [n_dst,16] (= 1 - sum of the row's weights), x1 [n_dst,16,64]; maxval is read only by rows that have edges
int grl_edge_attend_fwd(const float* logit, const float* maxval, const float* msg, const int* rowptr, int n_dst, float* a, float* comp,
                        float* x1, hipStream_t stream) {
  if (n_dst <= 0) return 0;
  hipLaunchKernelGGL(edge_attend_fwd_kernel, dim3(row_blocks((long long)n_dst * O)), dim3(256), 0, stream, logit, maxval, msg, rowptr,
                     n_dst, a, comp, x1);
  GRL_CHECK_LAUNCH();
  return 0;
}

// dmsg [E,16,64], dl [E,16] (with the dM term at argmax[0]); pdm: [grl_attention_blocks(n_dst * 16)] workspace.  Needs n_edges > 0.
int grl_edge_attend_bwd(const float* a, const float* msg, const float* comp, const float* dx1, const int* rowptr, int n_dst,
                        const int* argmax, float* dmsg, float* dl, float* pdm, hipStream_t stream) {
  if (n_dst <= 0) return -2;
  const int blocks = row_blocks((long long)n_dst * O);
  hipLaunchKernelGGL(edge_attend_bwd_kernel, dim3(blocks), dim3(256), 0, stream, a, msg, comp, dx1, rowptr, n_dst, dmsg, dl, pdm);
  GRL_CHECK_LAUNCH();
  hipLaunchKernelGGL(edge_attend_dm_kernel, dim3(1), dim3(64), 0, stream, pdm, blocks, argmax, rowptr, n_dst, dl);
  GRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
