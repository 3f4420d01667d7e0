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

``attention_cases()`` / ``project_cases()`` are the per-op case table: homogeneous graphs, 16 orientations, 24 .. 96 nodes, each graph at
logit spans of about +-1, +-3, +-10 and +-20, produced by scaling k; then graphs large enough that the kernels' grid-stride loops go
round (``LARGE_GRAPHS``, ``PROJECT_NODES_LARGE``), two of them bipartite; then exact three-way ties of the global maximum (``TIES``).
``BARS`` are the per-op bars derived from the table by the rule of tests/test_gpu_actor_ops.py: 8 x the worst error of the fp32 torch
CPU evaluation against the float64 one, rounded up to one digit (tests/test_empn_attention_ref_cpu.py prints the table and checks the
numbers; nothing is measured on the kernels).

Ties.  The kernels give d M to the LOWEST flat index e * 16 + o (destination-sorted edge order) that attains the maximum; torch's
``l.max()`` splits it evenly over the tied elements.  A case that declares ties is therefore evaluated with M = l.flatten()[lowest tied
index] (``attention_parts``).  For exactly duplicated graphs the parameter gradients agree under either rule (symmetry); the per-node
d k and d q do not: on the tie cases, where d M is the largest entry of d l, an even split moves d k and d q by 0.67 of their scale (two
thirds of d M leave the lowest row) and the highest index by 1.0."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import data_fixtures as dfx

KD, O, C = 128, 16, 64
VARIANTS = ("reference", "per_destination_max", "eps16", "detached_max", "tie_highest_index", "tie_even_split")


# ------------------------------------------------------------------------------------------------ the two ops
def kq_project(x, wk, bk, wq, bq):
    return F.linear(x, wk, bk), F.linear(x, wq, bq)


def attention_parts(k, q, src, dst, n_dst, variant="reference", ties=None):
    """(l [E,O], a [E,O], S [n_dst,O]) of the module docstring.  ``variant``: "reference", or a misreading -- "per_destination_max" (the
    shift of a segment softmax), "eps16" (PyG's 1e-16 in place of 1e-6), "detached_max" (M as a constant), and for an exactly tied
    maximum "tie_highest_index" / "tie_even_split".  ``ties``: the flat rows e * 16 + o the caller DECLARES to attain the maximum
    (asserted: the tied set is ``l == l.max()`` in the evaluation dtype).  The kernels hand d M to the LOWEST of them, so the reference is
    M = l.flatten()[lowest]; torch's own ``l.max()`` splits the gradient evenly over the tied elements ("tie_even_split"), and
    "tie_highest_index" is the opposite choice.  The value of M is the same in all three.  Without declared ties nothing changes."""
    assert variant in VARIANTS, variant
    l = (k[src] * q[dst]).sum(-1) / math.sqrt(KD)
    if variant == "per_destination_max":
        seg = torch.full((n_dst, l.shape[1]), -math.inf, dtype=l.dtype, device=l.device)
        seg = seg.scatter_reduce(0, dst[:, None].expand_as(l), l, "amax", include_self=True)
        shift = seg[dst]
    else:
        shift = l.max()
        if ties is not None:
            tied = (l.detach().flatten() == shift.detach()).nonzero().flatten().tolist()
            assert tied == sorted(ties), (tied, sorted(ties))
            if variant != "tie_even_split":
                shift = l.flatten()[tied[-1] if variant == "tie_highest_index" else tied[0]]
        if variant == "detached_max":
            shift = shift.detach()
    p = torch.exp(l - shift)
    S = torch.zeros(n_dst, l.shape[1], dtype=l.dtype, device=l.device).index_add(0, dst, p)
    return l, p / (S[dst] + (1e-16 if variant == "eps16" else 1e-6)), S


def attention_weights(k, q, src, dst, n_dst, variant="reference", ties=None):
    """a [E,O] of the module docstring (``attention_parts``)."""
    return attention_parts(k, q, src, dst, n_dst, variant, ties)[1]


def edge_attention(k, q, msg, src, dst, n_dst, variant="reference", ties=None):
    """x_1 [n_dst,O,C]; msg rows in the order of (src, dst).  An empty edge set gives zeros (a safety rule: the reference would raise on
    the empty maximum)."""
    if src.numel() == 0:
        return torch.zeros(n_dst, msg.shape[1], msg.shape[2], dtype=msg.dtype, device=msg.device) + 0.0 * (k.sum() + q.sum() + msg.sum())
    a = attention_weights(k, q, src, dst, n_dst, variant, ties)
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
    return n, _edge_index(pairs)


def _edge_index(pairs):
    e = sorted(pairs, key=lambda p: (p[1], p[0]))
    return torch.tensor(e, dtype=torch.int64).t().reshape(2, -1) if e else torch.zeros(2, 0, dtype=torch.int64)


# The graphs above keep every wave of every row kernel at ONE row (at most 96 x 16 = 1536 rows against 2048 workgroups x 4 waves = 8192 rows
# per pass of the grid).  The large graphs are the smallest that go round the grid again:
LARGE_GRAPHS = ("many_rows", "wide_sources", "wide_destinations")
ROWS_PER_PASS = 8192   # csrc/attention_ops.hip: ROW_BLOCKS_MAX = 2048 workgroups of 4 waves, one row per wave and iteration


@functools.lru_cache(maxsize=None)
def _large_graph(name):
    """(n_src, n_dst, edge_index) of a large graph, in the style of ``_graph`` (built once: no caller writes into the edge index)."""
    g = torch.Generator().manual_seed({"many_rows": 1, "wide_sources": 2, "wide_destinations": 3}[name])
    pairs = set()
    if name == "many_rows":             # 600 nodes, in-degree d % 5 (0 .. 4): 1200 edges = 19200 logit rows (waves visit two and three
        n_src = n_dst = 600             # rows), 9600 destination rows; sources 560 .. 599 have no out-edge
        for d in range(n_dst):
            for s in torch.randperm(560, generator=g)[:d % 5].tolist():
                pairs.add((s, d))
    elif name == "wide_sources":        # bipartite, 700 -> 40: the logits backward's 640 d q rows end inside the first pass, so a wave
        n_src, n_dst = 700, 40          # takes a d q row on one iteration and a d k row on the next
        for d in range(n_dst):
            for s in torch.randperm(n_src, generator=g)[:20].tolist():
                pairs.add((s, d))
    else:                               # bipartite, 30 -> 600: the 9600 d q rows alone go round the grid, the d k rows start mid-grid
        n_src, n_dst = 30, 600
        for d in range(n_dst):
            for s in torch.randperm(n_src, generator=g)[:d % 4].tolist():
                pairs.add((s, d))
    return n_src, n_dst, _edge_index(pairs)


# Exact three-way ties of the global maximum on ``many_rows``: (edge position in destination-sorted order, orientation) -> flat row
# e * 16 + o.  With wg(r) = (r // 4) % 2048 and wave(r) = r % 4 the workgroup and wave that visit row r:
#   first_pass: rows 3, 8147, 8192.  The lowest is in the first pass; 8192 is workgroup 0's (wave 0, second iteration) like row 3 (wave 3),
#               so the merge of the four waves sees the HIGHER index first; 8147 is workgroup 2036's, so the finish over the block
#               partials meets workgroup 0 first and must still prefer 3 over 8147 -- and 8147 over 8192 had the wave merge gone wrong.
#   late:       rows 8994, 16387, 17186.  Every occurrence lies behind the first pass (a kernel that kept only first-iteration rows has
#               the wrong M); 8994 and 17186 are the SAME wave (workgroup 200, wave 2) on consecutive iterations, so the per-wave running
#               maximum must keep the earlier one; 16387 is workgroup 0's, so the finish meets the higher index first.
#   one_workgroup: rows 8193, 16386, 17605.  The two lowest are workgroup 0's, the LOWER index in the lower wave (1 and 2): a merge of
#               the waves in which the later of equals wins gets the other two placements right and this one wrong.
# tests/test_empn_attention_ref_cpu.py restates the three-stage reduction and shows that each stage decides one of these.
TIES = {"first_pass": ((0, 3), (509, 3), (512, 0)), "late": ((562, 2), (1024, 3), (1074, 2)),
        "one_workgroup": ((512, 1), (1024, 2), (1100, 5))}


class AttentionCase:
    """EdgeAttention on one graph at one logit span: k is scaled so that max |l| = span."""

    def __init__(self, graph, span, tie=None):
        self.name = f"edge_attention[{graph}, span +-{span:g}{', tie ' + tie if tie else ''}]"
        self.graph, self.span, self.tie = graph, span, tie
        if graph in LARGE_GRAPHS:
            self.n_src, self.n_dst, self.ei = _large_graph(graph)
            self.n = self.n_dst if self.n_src == self.n_dst else None
            self.bar = "edge_attention_large"
        else:
            self.n, self.ei = _graph(graph)
            self.n_src = self.n_dst = self.n
            self.bar = "edge_attention"
        g = torch.Generator().manual_seed(100 + int(span))
        E = self.ei.shape[1]
        k = torch.randn(self.n_src, O, KD, generator=g, dtype=torch.float64)
        q = torch.randn(self.n_dst, O, KD, generator=g, dtype=torch.float64)
        self.tie_edges = []   # ((source, destination), orientation) of the declared ties; ``ties``: their flat rows in the order of ``ei``
        if E:
            l = (k[self.ei[0]] * q[self.ei[1]]).sum(-1) / math.sqrt(KD)
            k = k * ((0.8 if tie else 1.0) * span / float(l.abs().max()))
        if tie:
            # one direction u, the same in the three key rows and the three query rows: the three logits are the SAME arithmetic on the
            # same numbers -- bit-equal in every evaluation -- and equal the span; everything else stays at 0.8 x span and below
            u = torch.randn(KD, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
            u = u / u.norm() * math.sqrt(span * math.sqrt(KD))
            ends = [int(self.ei[r, e]) for e, _ in TIES[tie] for r in (0, 1)]
            assert len(set(ends)) == 6, ("the tied edges must have six distinct end nodes", ends)
            for e, o in TIES[tie]:
                s, d = int(self.ei[0, e]), int(self.ei[1, e])
                k[s, o], q[d, o] = u, u
                self.tie_edges.append(((s, d), o))
        self.k, self.q = k.float(), q.float()            # (float32-representable inputs: both evaluations read the same numbers)
        self.msg = torch.randn(E, O, C, generator=g, dtype=torch.float64).float()
        self.R = torch.randn(self.n_dst, O, C, generator=g, dtype=torch.float64).float()

    @property
    def ties(self):
        """Flat rows e * 16 + o of the declared ties in the current edge order, ascending (None: the case declares none)."""
        if not self.tie_edges:
            return None
        pos = {p: i for i, p in enumerate(zip(*self.ei.tolist()))}
        return sorted(pos[p] * O + o for p, o in self.tie_edges)

    def with_edges(self, ei):
        """The same inputs with the msg rows defined on ``ei`` (the device's own destination-sorted order of the same edge set)."""
        assert sorted(zip(*ei.tolist())) == sorted(zip(*self.ei.tolist()))
        key = {p: i for i, p in enumerate(zip(*self.ei.tolist()))}
        perm = torch.tensor([key[p] for p in zip(*ei.tolist())], dtype=torch.int64)
        self.msg, self.ei = self.msg[perm].contiguous(), ei.clone()
        return self

    def parts(self, dtype=torch.float64):
        """(l, a, comp = 1e-6 / (S + 1e-6)) of the reference: what the forward kernels leave for the backward."""
        k, q = self.k.to(dtype), self.q.to(dtype)
        l, a, S = attention_parts(k, q, self.ei[0], self.ei[1], self.n_dst, "reference", self.ties)
        return l, a, 1e-6 / (S + 1e-6)

    def evaluate(self, dtype, device="cpu", variant="reference"):
        # (copies: ``.to`` of a float32 tensor to float32 is the tensor itself, and the case's own inputs must stay plain leaves)
        k, q, msg = (t.to(device=device, dtype=dtype, copy=True).requires_grad_(True) for t in (self.k, self.q, self.msg))
        ei = self.ei.to(device)
        x1 = edge_attention(k, q, msg, ei[0], ei[1], self.n_dst, variant, self.ties)
        (x1 * self.R.to(device=device, dtype=dtype)).sum().backward()
        return {"x1": x1.detach()}, {"k": k.grad, "q": q.grad, "msg": msg.grad}


class ProjectCase:
    """KeyQueryProject on n nodes: Xavier-sized weights, non-zero biases.  ``rows``: x is [rows, 64] instead -- a row count the op never
    passes (it has 16 rows per node) and the C ABI accepts."""
    bar = "kq_project"

    def __init__(self, n=None, rows=None):
        assert (n is None) != (rows is None)
        self.name = f"kq_project[{n} nodes]" if rows is None else f"kq_project[{rows} rows]"
        self.n, self.rows = n, rows if rows is not None else n * O
        lead = (n, O) if rows is None else (rows,)
        g = torch.Generator().manual_seed(200 + n if rows is None else 300 + rows)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
        self.x = r(*lead, C)
        self.w = [r(KD, C) * 0.18, r(KD) * 0.1, r(KD, C) * 0.18, r(KD) * 0.1]   # (xavier_uniform(128, 64): std 0.10)
        self.Rk, self.Rq = r(*lead, KD), r(*lead, KD)

    def evaluate(self, dtype, device="cpu"):
        x, wk, bk, wq, bq = (t.to(device=device, dtype=dtype, copy=True).requires_grad_(True) for t in (self.x, *self.w))
        k, q = kq_project(x, wk, bk, wq, bq)
        ((k * self.Rk.to(device=device, dtype=dtype)).sum() + (q * self.Rq.to(device=device, dtype=dtype)).sum()).backward()
        return {"k": k.detach(), "q": q.detach()}, {"x": x.grad, "wk": wk.grad, "bk": bk.grad, "wq": wq.grad, "bq": bq.grad}


GRAPHS = ("degrees", "hub", "half_block", "self_loops", "empty")


LARGE_SPANS = (1.0, 10.0)
TIE_SPANS = (10.0, 20.0)
PROJECT_NODES = (24, 26, 96)
# 257 nodes = 4112 rows: four workgroups above the 1024-workgroup cap of the projection's forward and input-gradient kernels (a partial
# second iteration).  2049 nodes = 32784 rows: the weight-gradient kernel's 512 workgroups get chunks of 65 rows, workgroup 504 holds 24
# and 505 .. 511 none (zero partial rows that the fold still sums).
PROJECT_NODES_LARGE = (257, 2049)
PROJECT_ROWS = (1, 3, 5, 4101)   # by direct call: not multiples of 4, the kernels' batch of rows


def kq_bwd_blocks(rows):
    """grl_kq_bwd_blocks restated (csrc/attention_ops.hip: at most 512 workgroups, 64 rows each below the cap)."""
    return min(max((rows + 63) // 64, 1), 512)


def attention_cases():
    """The original table, then the large graphs, then the tie cases."""
    cases = [AttentionCase(gname, span) for gname in GRAPHS for span in (SPANS if gname != "empty" else SPANS[:1])]
    cases += [AttentionCase(gname, span) for gname in LARGE_GRAPHS for span in LARGE_SPANS]
    return cases + [AttentionCase("many_rows", span, tie) for tie in TIES for span in TIE_SPANS]


def project_cases():
    return [ProjectCase(n) for n in PROJECT_NODES + PROJECT_NODES_LARGE]


def project_row_cases():
    return [ProjectCase(rows=r) for r in PROJECT_ROWS]


# Per-op bars (values, gradients) as fractions of the tensor's own scale: 8 x the worst fp32-vs-float64 error of the torch CPU evaluation of
# the cases above, rounded up to one digit (tests/test_empn_attention_ref_cpu.py::test_bar_table prints the table these come from).
# "edge_attention" holds the original five graphs, "edge_attention_large" the large graphs and the tie cases; "kq_project" every
# projection case, the row counts of the direct calls included.  The large group's gradient bar is three times the small one's because of
# torch's fp32 evaluation, not of the operation: at +-1 every S is far above the 1e-6, torch forms 1 - sum a as a difference of two
# numbers near 1, and d M sums that rounding noise over 9600 destination rows instead of 1536 before it lands on one element of d l
# (many_rows +-1: d k 6.3e-6).  The kernels store 1e-6 / (S + 1e-6) and do not have that error; the rule is kept all the same.
BARS = {"kq_project": (4e-6, 5e-6), "edge_attention": (7e-6, 2e-5), "edge_attention_large": (6e-6, 6e-5)}
