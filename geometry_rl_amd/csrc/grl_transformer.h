/* grl_transformer.h -- C ABI of libgrl_transformer.so: the transformer baseline actor's encoder and the post_fc Gaussian head as gfx950
 * kernels (csrc/transformer_ops.hip), fp32 only.  A library of its own beside libgrl_hip.so, like libgrl_attention.so: the export list of
 * libgrl_hip.so is exactly include/grl_hip.h, which this addition leaves as it is (its ABI note 216 names it).  Conventions as in
 * include/grl_hip.h: device pointers borrowed for the call unless marked HOST, the caller allocates every output and workspace, launches
 * are asynchronous on `stream`, 0 = enqueued, -2 = unsupported shape, <= -1000 = -(1000 + hipError_t). */
#pragma once
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- transformer baseline actor: geometry_rl/modules/pyg_models/transformer_vanilla.py:29-36,87-92 (torch's post-norm
 *      nn.TransformerEncoder: hidden 64, 2 layers, 2 heads, dim_feedforward 64, dropout 0, concat_global=False, no mask) and the
 *      post_fc Gaussian head of gnn_gaussian_policy_diag.py:65-83.  fp32 only (csrc/transformer_ops.hip; include/grl_hip.h ABI 216).
 * u [B,n,d_in]; hidden [B*G,64] = fc_out of the encoder's rows m0 .. m0+G-1 of every sample.  1 <= n <= 256, 1 <= d_in <= 64,
 * 0 <= m0, 1 <= G, m0 + G <= n (anything else: -2, nothing launched).  One workgroup owns whole samples; no [n,n] object is ever in
 * global memory (the backward recomputes the attention weights from the saved per-row maximum and sum of each head).
 * params: HOST array of 28 device pointers: We [64,d_in], be, then per layer (2x) Win [192,64], bin, Wo [64,64], bo, norm1 weight, norm1
 *         bias, W1 [64,64], b1, W2 [64,64], b2, norm2 weight, norm2 bias, then Wf [64,64], bf (fc_out.lins.0).
 * saved  [15][B*n][64] floats, WRITTEN by the forward: x_0 | per layer [q|k|v] as [B*n][192] | o | xhat1 | relu(W1 y + b1) | xhat2
 * stats  [2][B*n][6] floats, WRITTEN: per layer and row 1/std of norm1, of norm2, the row maximum of head 0, 1, the row sum of head 0, 1
 * A workgroup takes its samples in groups of grl_transformer_group_rows(B, n) / n consecutive ones (1 until B exceeds the 256 workgroups,
 * then as many as keep a group within 256 rows): the row-wise stages run once per group, attention inside each sample.
 * backward: ws [grl_transformer_blocks(B, n)][grl_transformer_group_rows(B, n)][grl_transformer_ws_row()] workspace (fully written before
 *           it is read); partial [grl_transformer_blocks(B, n)][grl_transformer_partial_size(d_in)], every entry written: per layer (25216 floats)
 *           [dWin 12288 | dbin 192 | dWo 4096 | dbo 64 | dnorm1.weight 64 | dnorm1.bias 64 | dW1 4096 | db1 64 | dW2 4096 | db2 64 |
 *           dnorm2.weight 64 | dnorm2.bias 64], then [dWf 4096 | dbf 64 | dbe 64 | dWe 64 x d_in]; u gets no gradient.
 * No atomics, no host read: a workgroup sums ITS samples in order, the rows are folded in row order -- two runs give the same bits. */
int grl_transformer_blocks(int B, int n);
int grl_transformer_group_rows(int B, int n);
int grl_transformer_partial_size(int d_in);
int grl_transformer_ws_row(void);
int grl_transformer_fwd(const float* u, const float* const* params, float* saved, float* stats, float* hidden, int B, int n, int d_in, int m0,
                        int G, hipStream_t stream);
int grl_transformer_bwd(const float* u, const float* const* params, const float* saved, const float* stats, const float* dhidden, float* ws,
                        float* partial, int B, int n, int d_in, int m0, int G, hipStream_t stream);
/* mean [R,A] = hidden Wm^T + bm; pre [R,A] = hidden Ws^T + bs (WRITTEN: the backward reads it); sigma = softplus(pre + shift) + min_std
 * (torch's softplus, threshold 20); hidden [R,64], 1 <= A <= 16 (more: -2).  A state-independent std is Ws = 0, bs = the vector.
 * backward: dhidden [R,64] fully written; partial [grl_postfc_head_blocks(R)][grl_postfc_head_partial_size()] =
 * [dWm 16x64 | dWs 16x64 | dbm 16 | dbs 16], rows a >= A are zeros.  Two launches. */
int grl_postfc_head_partial_size(void);
int grl_postfc_head_blocks(int n_rows);
int grl_postfc_head_fwd(const float* hidden, const float* Wm, const float* bm, const float* Ws, const float* bs, float shift, float min_std,
                        float* mean, float* sigma, float* pre, int n_rows, int A, hipStream_t stream);
int grl_postfc_head_bwd(const float* hidden, const float* Wm, const float* Ws, const float* pre, float shift, const float* dmean,
                        const float* dsigma, float* dhidden, float* partial, int n_rows, int A, hipStream_t stream);

#ifdef __cplusplus
}
#endif
