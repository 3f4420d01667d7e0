"""Float64 restatement of the EMPN key / query attention layer -- PonitaGCN(attention=True), the ``attention`` key of
configs/algorithm/pyg_agent/model/ponita_gcn.yaml -- written from its formulas; a plain module like tests/ops_ref.py.  It is the
ground truth of tests/test_gpu_empn_attention_ops.py (per op) and, through tests/test_empn_attention_ref_cpu.py, is itself pinned to
the reference's own numbers: the fixtures tests/golden/tier2h_<case>_attention.npz / _attention_grad.npz (tools/make_golden.py
empn_attention) -- the first pin of PonitaGCN(attention=True), which tests/data_fixtures.py still lists as unpinned.

With x the layer input [N,16,64], (src, dst) the edges, Wk / Wq [128,64] and bk / bq [128]:

    msg[e,o,:] = x[src e,o,:] * kernel(kernel_basis)[e,o,:]
    k = x Wk^T + bk,  q = x Wq^T + bq                                [N,16,128]
    l[e,o]  = <k[src e,o,:], q[dst e,o,:]> / sqrt(128)
    M       = max over ALL (e,o) of l        -- one scalar for the whole batch, part of the graph (not detached)
    p[e,o]  = exp(l[e,o] - M)
    S[d,o]  = sum_{e -> d} p[e,o]
    a[e,o]  = p[e,o] / (S[dst e,o] + 1e-6)
    x_1[d,o,:] = sum_{e -> d} a[e,o] * msg[e,o,:]

then the layer goes on as without attention (fiber convolution, bias, LayerNorm, MLP, residual) and calibration rescales
``kernel.weight`` and ``fiber_kernel.weight`` by x.std() / x_1.std() and x_1.std() / x_2.std(); the key and query layers are never
rescaled.  Two things are unusual and ``VARIANTS`` holds the plausible misreadings of them: the maximum is global (a destination whose
logits sit far below it has S comparable to the 1e-6, so its weights do not sum to 1 and the 1e-6 matters), and the gradient flows
through M (d M = - sum_{d,o} (1 - sum_{e->d} a) (sum_{e->d} a da), added at the argmax).

``CASES`` is the per-op case table (homogeneous graphs, 16 orientations, 24 .. 96 nodes; each graph at logit spans of about +-1, +-3,
+-10 and +-20, produced by scaling k); ``BARS`` the per-op bars derived from it by the rule of tests/test_gpu_actor_ops.py: 8 x the
worst error of the fp32 torch CPU evaluation against the float64 one, rounded up to one digit (tests/test_empn_attention_ref_cpu.py
prints the table and checks the numbers; nothing is measured on the kernels)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import data_fixtures as dfx

KD, O, C = 128, 16, 64
VARIANTS = ("reference", "per_destination_max", "eps16", "detached_max")


# ------------------------------------------------------------------------------------------------ the two ops
def kq_project(x, wk, bk, wq, bq):
    return F.linear(x, wk, bk), F.linear(x, wq, bq)


def attention_weights(k, q, src, dst, n_dst, variant="reference"):
    """a [E,O] of the module docstring.  ``variant``: "reference", or one of the three misreadings -- "per_destination_max" (the shift of
    a segment softmax), "eps16" (PyG's 1e-16 in place of 1e-6), "detached_max" (M as a constant)."""
    assert variant in VARIANTS, variant
    l = (k[src] * q[dst]).sum(-1) / math.sqrt(KD)
    if variant == "per_destination_max":
        seg = torch.full((n_dst, l.shape[1]), -math.inf, dtype=l.dtype, device=l.device)
        seg = seg.scatter_reduce(0, dst[:, None].expand_as(l), l, "amax", include_self=True)
        shift = seg[dst]
    else:
        shift = l.max()
        if variant == "detached_max":
            shift = shift.detach()
    p = torch.exp(l - shift)
    S = torch.zeros(n_dst, l.shape[1], dtype=l.dtype, device=l.device).index_add(0, dst, p)
    return p / (S[dst] + (1e-16 if variant == "eps16" else 1e-6))


def edge_attention(k, q, msg, src, dst, n_dst, variant="reference"):
    """x_1 [n_dst,O,C]; msg rows in the order of (src, dst).  An empty edge set gives zeros (a safety rule: the reference would raise on
    the empty maximum)."""
    if src.numel() == 0:
        return torch.zeros(n_dst, msg.shape[1], msg.shape[2], dtype=msg.dtype, device=msg.device) + 0.0 * (k.sum() + q.sum() + msg.sum())
    a = attention_weights(k, q, src, dst, n_dst, variant)
    return torch.zeros(n_dst, msg.shape[1], msg.shape[2], dtype=msg.dtype, device=msg.device).index_add(0, dst, a[..., None] * msg)


# ------------------------------------------------------------------------------------------------ the layer and the EMPN forward
def attention_layer(x, kernel_basis, fiber_basis, edge_index, P, prefix, calibrate=False, variant="reference"):
    """One interaction layer with attention (the module docstring; the tail as oracle.equivariant.ponita_layer)."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    msg = x[src] * F.linear(kernel_basis, P[f"{prefix}.conv.kernel.weight"])
    k, q = kq_project(x, P[f"{prefix}.conv.key_transform.weight"], P[f"{prefix}.conv.key_transform.bias"],
                      P[f"{prefix}.conv.query_transform.weight"], P[f"{prefix}.conv.query_transform.bias"])
    x_1 = edge_attention(k, q, msg, src, dst, x.shape[0], variant)
    fk = F.linear(fiber_basis, P[f"{prefix}.conv.fiber_kernel.weight"])
    x_2 = torch.einsum("boc,poc->bpc", x_1, fk) / fk.shape[-2]
    if calibrate:   # the calibrating call still finishes with the old x_2; key / query are never rescaled
        with torch.no_grad():
            s_in, s_1, s_2 = x.std(), x_1.std(), x_2.std()
            P[f"{prefix}.conv.kernel.weight"] = P[f"{prefix}.conv.kernel.weight"] * s_in / s_1
            P[f"{prefix}.conv.fiber_kernel.weight"] = P[f"{prefix}.conv.fiber_kernel.weight"] * s_1 / s_2
    h = x_2 + P[f"{prefix}.conv.bias"]
    h = F.layer_norm(h, (h.shape[-1],), P[f"{prefix}.norm.weight"], P[f"{prefix}.norm.bias"], 1e-5)
    h = F.gelu(F.linear(h, P[f"{prefix}.linear_1.weight"], P[f"{prefix}.linear_1.bias"]))
    h = F.linear(h, P[f"{prefix}.linear_2.weight"], P[f"{prefix}.linear_2.bias"])
    return h + x


def empn_attention_forward(P, graph, scalar_dict, vector_dict, *, dim, output_dim, output_dim_vec, num_layers, batch_size, calibrate=False,
                           variant="reference"):
    """PonitaGCN(attention=True).one_step: the wrapper and the bases of oracle.equivariant (pinned by the attention-free fixtures), the
    layers of this module."""
    from oracle import equivariant as eq
    grid = P["ponita.ori_grid"]
    x, pos, ei = eq.empn_inputs(grid, graph, scalar_dict, vector_dict, dim, batch_size)
    kb = eq.basis_mlp(eq.spatial_invariants(grid, pos[ei[0]], pos[ei[1]]), P, "ponita.basis_fn")
    fb = eq.basis_mlp(eq.orientation_invariants(grid), P, "ponita.fiber_basis_fn")
    x = F.linear(x, P["ponita.x_embedder.weight"])
    for i in range(num_layers):
        x = attention_layer(x, kb, fb, ei, P, f"ponita.interaction_layers.{i}", calibrate, variant)
    return eq.empn_output(P, x, graph, dim=dim, output_dim=output_dim, output_dim_vec=output_dim_vec, batch_size=batch_size)


# ------------------------------------------------------------------------------------------------ the fixtures
ATTENTION_CASES = {"empn_rigid_g2_pad_attention": "rigid", "empn_rope_dim2_attention": "rope"}


class AttentionFixture(dfx.ModelFixture):
    """tier2h_<case>_attention.npz + tier2h_<case>_attention_grad.npz: the record layout of data_fixtures.ModelFixture (``model`` has one more
    entry, attention = 1)."""

    def __init__(self, golden_dir, case):
        dfx.Fixture.__init__(self, golden_dir, case, f"tier2h_{case}.npz", ATTENTION_CASES[case])
        pick = lambda p: {k[len(p):]: torch.as_tensor(v) for k, v in self.z.items() if k.startswith(p)}
        self.model = {k: int(v) for k, v in pick("model.").items()}
        assert self.model["empn"] == 1 and self.model["attention"] == 1
        self.init = pick("init.")
        self.changed = sorted(pick("cal."))
        assert self.changed == sorted(pick("cal64.")) and set(self.changed) <= set(self.init)
        self.cal = {**self.init, **pick("cal.")}
        self.cal64 = {**{k: (v.double() if v.dtype.is_floating_point else v) for k, v in self.init.items()}, **pick("cal64.")}
        g = np.load(os.path.join(golden_dir, f"tier2h_{case}_grad.npz"))
        self.grad = {k[len("grad."):]: torch.from_numpy(g[k]) for k in g.files}


# ------------------------------------------------------------------------------------------------ the per-op case table
SPANS = (1.0, 3.0, 10.0, 20.0)


def _graph(name):
    """(n_nodes, edge_index [2,E] int64, sorted by (destination, source), no duplicate edges)."""
    g = torch.Generator().manual_seed({"degrees": 11, "hub": 12, "half_block": 13, "self_loops": 14, "empty": 15}[name])
    pairs = set()
    if name == "degrees":        # in-degrees 0 .. 5; destinations 0, 7, 14, .. have no in-edge, sources 30 .. 39 no out-edge
        n = 40
        for d in range(n):
            deg = 0 if d % 7 == 0 else 1 + (d % 5)
            for s in torch.randperm(30, generator=g)[:deg].tolist():
                pairs.add((s, d))
    elif name == "hub":          # destination 5 has 70 in-edges, the others 0 .. 2
        n = 96
        for s in torch.randperm(n, generator=g)[:70].tolist():
            pairs.add((s, 5))
        for d in range(n):
            if d != 5:
                for s in torch.randperm(n, generator=g)[:d % 3].tolist():
                    pairs.add((s, d))
    elif name == "half_block":   # 26 nodes = 416 rows: the last 64-row block of the projection's backward is half full
        n = 26
        for d in range(n):
            for s in torch.randperm(n, generator=g)[:3].tolist():
                pairs.add((s, d))
    elif name == "self_loops":   # every node has its self-loop, every second one two more in-edges
        n = 24
        for d in range(n):
            pairs.add((d, d))
            if d % 2:
                for s in torch.randperm(n, generator=g)[:2].tolist():
                    pairs.add((s, d))
    else:
        n = 24
    e = sorted(pairs, key=lambda p: (p[1], p[0]))
    ei = torch.tensor(e, dtype=torch.int64).t().reshape(2, -1) if e else torch.zeros(2, 0, dtype=torch.int64)
    return n, ei


class AttentionCase:
    """EdgeAttention on one graph at one logit span: k is scaled so that max |l| = span."""

    def __init__(self, graph, span):
        self.name = f"edge_attention[{graph}, span +-{span:g}]"
        self.graph, self.span = graph, span
        self.n, self.ei = _graph(graph)
        g = torch.Generator().manual_seed(100 + int(span))
        E = self.ei.shape[1]
        k = torch.randn(self.n, O, KD, generator=g, dtype=torch.float64)
        q = torch.randn(self.n, O, KD, generator=g, dtype=torch.float64)
        if E:
            l = (k[self.ei[0]] * q[self.ei[1]]).sum(-1) / math.sqrt(KD)
            k = k * (span / float(l.abs().max()))
        self.k, self.q = k.float(), q.float()            # (float32-representable inputs: both evaluations read the same numbers)
        self.msg = torch.randn(E, O, C, generator=g, dtype=torch.float64).float()
        self.R = torch.randn(self.n, O, C, generator=g, dtype=torch.float64).float()

    def with_edges(self, ei):
        """The same inputs with the msg rows defined on ``ei`` (the device's own destination-sorted order of the same edge set)."""
        assert sorted(zip(*ei.tolist())) == sorted(zip(*self.ei.tolist()))
        key = {p: i for i, p in enumerate(zip(*self.ei.tolist()))}
        perm = torch.tensor([key[p] for p in zip(*ei.tolist())], dtype=torch.int64)
        self.msg, self.ei = self.msg[perm].contiguous(), ei.clone()
        return self

    def evaluate(self, dtype, device="cpu", variant="reference"):
        k, q, msg = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (self.k, self.q, self.msg))
        ei = self.ei.to(device)
        x1 = edge_attention(k, q, msg, ei[0], ei[1], self.n, variant)
        (x1 * self.R.to(device=device, dtype=dtype)).sum().backward()
        return {"x1": x1.detach()}, {"k": k.grad, "q": q.grad, "msg": msg.grad}


class ProjectCase:
    """KeyQueryProject on n nodes: Xavier-sized weights, non-zero biases."""

    def __init__(self, n):
        self.name = f"kq_project[{n} nodes]"
        self.n = n
        g = torch.Generator().manual_seed(200 + n)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
        self.x = r(n, O, C)
        self.w = [r(KD, C) * 0.18, r(KD) * 0.1, r(KD, C) * 0.18, r(KD) * 0.1]   # (xavier_uniform(128, 64): std 0.10)
        self.Rk, self.Rq = r(n, O, KD), r(n, O, KD)

    def evaluate(self, dtype, device="cpu"):
        x, wk, bk, wq, bq = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (self.x, *self.w))
        k, q = kq_project(x, wk, bk, wq, bq)
        ((k * self.Rk.to(device=device, dtype=dtype)).sum() + (q * self.Rq.to(device=device, dtype=dtype)).sum()).backward()
        return {"k": k.detach(), "q": q.detach()}, {"x": x.grad, "wk": wk.grad, "bk": bk.grad, "wq": wq.grad, "bq": bq.grad}


GRAPHS = ("degrees", "hub", "half_block", "self_loops", "empty")


def attention_cases():
    return [AttentionCase(gname, span) for gname in GRAPHS for span in (SPANS if gname != "empty" else SPANS[:1])]


def project_cases():
    return [ProjectCase(n) for n in (24, 26, 96)]


# Per-op bars (values, gradients) as fractions of the tensor's own scale: 8 x the worst fp32-vs-float64 error of the torch CPU evaluation of
# the cases above, rounded up to one digit (tests/test_empn_attention_ref_cpu.py::test_bar_table prints the table these come from).
BARS = {"kq_project": (4e-6, 5e-6), "edge_attention": (7e-6, 2e-5)}
