/* grl_attention.h -- C ABI of libgrl_attention.so: the EMPN key/query attention kernels (attention_ops.hip), a library of its own beside
 * libgrl_hip.so (whose header, include/grl_hip.h, and export list stay as they are).  Conventions as in include/grl_hip.h: device pointers
 * borrowed for the call, the caller allocates every output and workspace, launches are asynchronous on `stream`, 0 = enqueued,
 * -2 = unsupported shape, <= -1000 = -(1000+hipError_t).  geometry_rl_amd/hip.py binds every declaration below (attention_call /
 * attention_query) with the binder of the main header; the exports of the library are exactly these names.
 *
 * ponita.py:21-24,126-161, SeparableFiberBundleConv(attention=True); fp32 only.
 * k = x Wk^T + bk, q = x Wq^T + bq ([n_rows = N*16, 128]); l[e,o] = <k[src e,o,:], q[dst e,o,:]> / sqrt(128);
 * M = max over ALL (e,o) of l (one scalar, NOT per destination, and the gradient flows through it); p = exp(l - M);
 * a[e,o] = p[e,o] / (sum_{e'->dst e} p[e',o] + 1e-6); x1[d,o,:] = sum_{e->d} a[e,o] msg[e,o,:].  Edge rows are in destination-sorted
 * order (the order of grl_edge_messages_fwd's msg).  No atomics, no host reads, fixed summation orders; every output row is written.
 * grl_kq_project_bwd: dx = dk Wk + dq Wq and partial [grl_kq_bwd_blocks(n_rows)][grl_kq_partial_size()] = [dWk | dWq | dbk | dbq].
 * grl_edge_logits_fwd: n_edges > 0; pmax / pidx are [grl_attention_blocks(n_edges * 16)] workspaces, maxval[0] = M, argmax[0] = the
 * lowest flat index e * 16 + o that attains it.  grl_edge_logits_bwd: dq from the destination-sorted rows, dk from the source-sorted view
 * (rowptr_s, dst_s, s2d); zeros for nodes without edges (dl is then not read).  grl_edge_attend_fwd: a [E,16], comp [n_dst,16] =
 * 1e-6 / (S + 1e-6) (one minus the row's weight sum), x1; rows without in-edges give exact zeros and do not read maxval.
 * grl_edge_attend_bwd (n_edges > 0): dmsg = a dx1[dst], dl = a (da - sum a' da') with da = <dx1[dst], msg>, and
 * dl[argmax[0]] += dM, dM = - sum_{d,o} comp[d,o] sum_{e->d} a da; pdm is a [grl_attention_blocks(n_dst * 16)] workspace. */
#pragma once
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

int grl_attention_blocks(int n_rows);
int grl_kq_partial_size(void);
int grl_kq_bwd_blocks(int n_rows);
int grl_kq_project_fwd(const float* x, const float* Wk, const float* bk, const float* Wq, const float* bq, float* k, float* q, int n_rows,
                       hipStream_t stream);
int grl_kq_project_bwd(const float* x, const float* Wk, const float* Wq, const float* dk, const float* dq, float* dx, float* partial,
                       int n_rows, hipStream_t stream);
int grl_edge_logits_fwd(const float* k, const float* q, const int* e_src, const int* e_dst, int n_edges, float* logit, float* pmax,
                        int* pidx, float* maxval, int* argmax, hipStream_t stream);
int grl_edge_logits_bwd(const float* k, const float* q, const float* dl, const int* rowptr_d, const int* src_d, int n_dst,
                        const int* rowptr_s, const int* dst_s, const int* s2d, int n_src, float* dk, float* dq, hipStream_t stream);
int grl_edge_attend_fwd(const float* logit, const float* maxval, const float* msg, const int* rowptr, int n_dst, float* a, float* comp,
                        float* x1, hipStream_t stream);
int grl_edge_attend_bwd(const float* a, const float* msg, const float* comp, const float* dx1, const int* rowptr, int n_dst,
                        const int* argmax, float* dmsg, float* dl, float* pdm, hipStream_t stream);

#ifdef __cplusplus
}
#endif
