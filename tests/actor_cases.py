"""Inputs of the per-op tests of the fp32 actor and critic kernels: seeded fp32 CPU tensors, shared by tests/test_ops_ref_cpu.py (which
evaluates the float64 references on them in fp32 to derive the bars) and tests/test_gpu_actor_ops.py (which feeds them to the kernels).

A ``Case`` names its inputs, says which of them are differentiated, how the reference maps them to named outputs, and which upstream
gradient each output gets (None: the output is left out of the loss)."""
import numpy as np
import torch

import ops_ref
from oracle import equivariant as eq


class Case:
    def __init__(self, name, inputs, diff, ref, ups):
        self.name, self.inputs, self.diff, self.ref, self.ups = name, inputs, diff, ref, ups

    def evaluate(self, dtype=torch.float64, device="cpu"):
        """-> (outputs, gradients of sum_k <out_k, ups_k> for the ``diff`` inputs), both dicts by name, in ``dtype`` on ``device``."""
        conv = lambda t: t.to(device=device, dtype=dtype) if t.is_floating_point() else t.to(device)
        ts = {k: ([conv(u) for u in t] if isinstance(t, list) else conv(t)) for k, t in self.inputs.items()}
        leaves = {}
        for k in self.diff:   # "wf#2" names element 2 of the list input "wf"
            base, _, idx = k.partition("#")
            leaf = ts[base][int(idx)] if idx else ts[base]
            leaves[k] = leaf.requires_grad_(True)
        outs = self.ref(ts)
        loss = sum((outs[k] * conv(u)).sum() for k, u in self.ups.items() if u is not None)
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        return ({k: v.detach() for k, v in outs.items()},
                {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(leaves, grads)})


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


GRID_KINDS = ["3d", "upper", "2d"]


def grid_of(kind):
    """"3d" full sphere, "upper" hemisphere, "2d" circle -> grid [16, dim]."""
    return eq.make_grid(2, 16) if kind == "2d" else eq.make_grid(3, 16, kind == "upper")


def grid3_of(kind):
    g = grid_of(kind)
    return torch.nn.functional.pad(g, (0, 3 - g.shape[1])).contiguous()


def weights(g, shapes):
    return [torch.randn(*s, generator=g) * (1.0 / np.sqrt(s[-1])) for s in shapes]


# ------------------------------------------------------------------------------------------------ fiber convolution, lift
NODE_COUNTS = [1, 3, 4, 5, 77, 9001, 70001]   # around the kernels' batches of four; 70001: more than 16 nodes per wave of the lift kernels
LIFT_SPLITS = [(1, 7), (2, 1), (5, 3), (8, 0)]  # widest vector block, a single vector, S + V = 8 = the kernels' maximum, no vectors


def fiber_conv_case(n):
    g = gen(1, n)
    inputs = {"x1": torch.randn(n, 16, 64, generator=g), "fk": torch.randn(16, 16, 64, generator=g), "bias": torch.randn(64, generator=g)}
    ref = lambda t: {"x2": ops_ref.fiber_conv(t["x1"], t["fk"], t["bias"])}
    return Case(f"fiber_conv n={n}", inputs, ["x1", "fk", "bias"], ref, {"x2": torch.randn(n, 16, 64, generator=g)})


def lift_case(n, grid_kind, S=3, V=4, tag=0):
    """S = 3, V = 4 with one-hot scalars: the bench configs' features (node type one-hot, four vectors); otherwise random scalars."""
    g = gen(2, n, S, V, tag, GRID_KINDS.index(grid_kind))
    if (S, V) == (3, 4):
        scal = torch.zeros(n, 3)
        scal[:, (n + tag) % 3] = 1
    else:
        scal = torch.randn(n, S, generator=g)
    inputs = {"scal": scal, "vec": torch.randn(n, V, 3, generator=g), "grid": grid_of(grid_kind), "w": torch.randn(64, S + V, generator=g)}
    ref = lambda t: {"x": ops_ref.lift_encode(t["scal"], t["vec"], t["grid"], t["w"])}
    return Case(f"lift n={n} {grid_kind} S{S} V{V}", inputs, ["w"], ref, {"x": torch.randn(n, 16, 64, generator=g)})


# LiftEncodeMulti: (node counts per type, index of a type whose output is left out of the loss or None, S, V, grid)
LIFT_MULTI = [([77], None, 3, 4, "3d"), ([5, 130], None, 3, 4, "3d"), ([9001, 3, 77], None, 3, 4, "3d"), ([4, 301, 1, 77], None, 3, 4, "3d"),
              ([0, 77, 5], None, 3, 4, "3d"), ([77, 0, 5], None, 3, 4, "2d"), ([77, 5, 0], None, 3, 4, "3d"), ([130, 77, 301], 0, 3, 4, "3d"),
              ([130, 77, 301], 1, 3, 4, "2d"), ([130, 0, 301, 4], 3, 3, 4, "3d"), ([70001, 77], None, 3, 4, "2d")]
LIFT_MULTI += [([301, 5, 77], None, S, V, k) for S, V in LIFT_SPLITS for k in ("3d", "2d")]


# ------------------------------------------------------------------------------------------------ fiber basis + fiber kernels
def fiber_basis_case(grid_kind, n_conv, unused=None):
    """``unused``: index of a convolution whose fk gets no gradient (the NULL dfk pointer of the backward)."""
    g = gen(3, n_conv, GRID_KINDS.index(grid_kind), -1 if unused is None else unused)
    w1, b1, w2, b2 = weights(g, [(64, 3), (64,), (64, 64), (64,)])
    inputs = {"poly": ops_ref.fiber_poly(grid_of(grid_kind)), "w1": w1, "b1": b1, "w2": w2, "b2": b2,
              "wf": weights(g, [(64, 64)] * n_conv)}

    def ref(t):
        return {f"fk{i}": fk for i, fk in enumerate(ops_ref.fiber_kernels(t["poly"], t["w1"], t["b1"], t["w2"], t["b2"], t["wf"]))}
    ups = {f"fk{i}": (None if i == unused else torch.randn(16, 16, 64, generator=g)) for i in range(n_conv)}
    return Case(f"fiber_basis {grid_kind} n_conv={n_conv} unused={unused}", inputs,
                ["w1", "b1", "w2", "b2"] + [f"wf#{i}" for i in range(n_conv)], ref, ups)


# ------------------------------------------------------------------------------------------------ read-out
READOUT_COUNTS = [1, 3, 5, 130, 4099]   # fewer nodes than the backward's four waves, a partial last workgroup, more than the resident waves
INIT_STD, MIN_STD = 1.0, 1e-5


def readout_case(n, od, ov, grid_kind, with_dhidden=True, with_dmean=True, with_dsigma=True):
    g = gen(4, n, od, ov, GRID_KINDS.index(grid_kind), with_dhidden, with_dmean, with_dsigma)
    inputs = {"lat": torch.randn(n, 16, 64, generator=g), "grid": grid_of(grid_kind),
              "wd": torch.randn(od + ov, 64, generator=g) * 0.2, "bd": torch.randn(od + ov, generator=g),   # std 1: bd * sum_o g_o carries weight
              "ws": torch.randn(3 * ov, 64, generator=g) * 0.2, "bs": torch.randn(3 * ov, generator=g) * 0.1}

    def ref(t):
        mean, sigma, hidden = ops_ref.readout(t["lat"], t["grid"], t["wd"], t["bd"], t["ws"], t["bs"], INIT_STD, MIN_STD, od, ov)
        return {"mean": mean, "sigma": sigma, "hidden": hidden}
    ups = {"mean": torch.randn(n, ov, 3, generator=g) if with_dmean else None,
           "sigma": torch.randn(n, 3 * ov, generator=g) if with_dsigma else None,
           "hidden": torch.randn(n, 64, generator=g) if with_dhidden else None}
    return Case(f"readout n={n} od={od} ov={ov} {grid_kind} dh={with_dhidden} dm={with_dmean} ds={with_dsigma}", inputs,
                ["lat", "wd", "bd", "ws", "bs"], ref, ups)


# ------------------------------------------------------------------------------------------------ DeepSets critic
DEEPSETS_SHAPES = [(1, 3, 15), (7, 35, 15), (130, 241, 12), (1030, 9, 7), (3, 64, 16), (5, 67, 1), (9, 130, 13), (1100, 65, 3), (2, 257, 15),
                   (1, 1, 15), (1, 70, 15)]   # the last two: one sample, with one row and with 64+ rows (the four-rows-per-access kernels)


def deepsets_case(B, n, d, masks=None):
    from oracle import graph as ogr
    P = ogr.init_critic_params(d, seed=5)
    g = gen(5, B, n, d)
    inputs = {k: P[k].clone() for k in ops_ref.DEEPSETS_KEYS}
    inputs["x"] = torch.randn(B, n, d, generator=g)
    ref = lambda t: {"value": ops_ref.deepsets_value(t["x"], [t[k] for k in ops_ref.DEEPSETS_KEYS], masks)}
    return Case(f"deepsets B={B} n={n} d={d}", inputs, list(ops_ref.DEEPSETS_KEYS), ref, {"value": torch.randn(B, generator=g)})


FMA_FAMILIES = {
    "fiber_conv": lambda: [fiber_conv_case(n) for n in NODE_COUNTS],
    "lift": lambda: ([lift_case(n, k) for n in NODE_COUNTS for k in ("3d", "2d")]
                     + [lift_case(301, k, S, V) for S, V in LIFT_SPLITS for k in ("3d", "2d")]),
    "fiber_basis": lambda: [fiber_basis_case(k, n) for k in GRID_KINDS for n in (1, 2, 3, 4)] + [fiber_basis_case("3d", 3, 1)],
    "readout": lambda: [readout_case(n, o, o, k) for n in READOUT_COUNTS for o in (1, 2) for k in GRID_KINDS],
    "deepsets": lambda: [deepsets_case(*s) for s in DEEPSETS_SHAPES],
}


# ------------------------------------------------------------------------------------------------ node block inputs
LN_MEAN_OVER_SPREAD = 256.0   # rows m + s randn: the largest power of two m / s torch's own fp32 layer_norm handles (test_ops_ref_cpu.py)
NODE_MLP_FAMILIES = ["randn", "constant_rows", "offset_rows", "times_1e3", "times_1e-3"]


# 700 / 1601 nodes: several chunks per workgroup of the backward; 4112 = 257 x 16 and 4101: above the forward's 256 workgroups x 256 rows.
# The other input families at three sizes: below one chunk, several chunks, the grid-stride loop with a partial block.
NODE_MLP_CASES = [("randn", n) for n in (1, 7, 130, 700, 1601, 4112, 4101)] + [(f, n) for f in NODE_MLP_FAMILIES[1:] for n in (7, 700, 4101)]


def node_mlp_rows(family, n, g):
    """x2 [n,16,64] of the family (the LayerNorm input; the other tensors of the block stay randn)."""
    x = torch.randn(n, 16, 64, generator=g)
    if family == "constant_rows":   # every second row constant (variance 0: padded points carry identical latents); multiples of 1/4 up to
        #                             8, so that every partial sum of a row is exact in fp32 and the normalised row is exactly beta
        c = torch.randint(-32, 33, (n, 16, 1), generator=g).float() / 4
        rows = (torch.arange(n * 16).reshape(n, 16, 1) % 2) == 0
        x = torch.where(rows, c.expand(n, 16, 64), x)
    elif family == "offset_rows":   # mean far above the spread
        s = 0.5 + torch.rand(n, 16, 1, generator=g)
        sign = torch.randint(0, 2, (n, 16, 1), generator=g).float() * 2 - 1
        x = sign * s * LN_MEAN_OVER_SPREAD + s * x
    elif family == "times_1e3":
        x = x * 1e3
    elif family == "times_1e-3":
        x = x * 1e-3
    return x


def node_mlp_case(family, n, use_prev):
    g = gen(6, NODE_MLP_FAMILIES.index(family), n)
    x2 = node_mlp_rows(family, n, g)
    xd, prev = (torch.randn(n, 16, 64, generator=g) for _ in range(2))
    gam, bet = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    w3, b3, w4, b4 = weights(g, [(256, 64), (256,), (64, 256), (64,)])
    inputs = {"x2": x2, "x_dst": xd, "gamma": gam, "beta": bet, "w3": w3, "b3": b3, "w4": w4, "b4": b4}
    if use_prev:
        inputs["prev"] = prev
    ref = lambda t: {"out": ops_ref.node_mlp(t["x2"], t["x_dst"], t["gamma"], t["beta"], t["w3"], t["b3"], t["w4"], t["b4"], t.get("prev"))}
    return Case(f"node_mlp {family} n={n} prev={use_prev}", inputs, list(inputs), ref, {"out": torch.randn(n, 16, 64, generator=g)})


# ------------------------------------------------------------------------------------------------ edge graphs
def degree_graph(degs, n_src, g):
    """Destination d gets degs[d] in-edges from random sources; edge ids in no particular order."""
    degs = torch.as_tensor(degs, dtype=torch.long)
    dst = torch.repeat_interleave(torch.arange(degs.numel()), degs)
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])


# graphs of the few-tile 32-row forward (n_dst <= 1024) ...
EDGE32_GRAPHS = ["rand37", "bip50_9_upper", "one_edge_dim2", "rand300", "hub300", "empty_runs", "n1024", "self_loops", "dim2", "bipartite", "empty"]
# ... and of the 16-row forward
EDGE16_GRAPHS = ["star_in", "star_out", "sparse_sources", "chain_of_hubs", "rand1500_upper", "n1025", "above_grid_cap", "chunks", "empn_like",
                 "knn_like"]


def edge_graph(kind):
    """-> (edge_index [2,E], n_src, n_dst, dim, grid kind, pos_src [n_src,3], pos_dst [n_dst,3])."""
    g = gen(7, (EDGE32_GRAPHS + EDGE16_GRAPHS).index(kind))
    dim, gk = 3, "upper"
    rnd = lambda n_s, n_d, E: torch.stack([torch.randint(0, n_s, (E,), generator=g), torch.randint(0, n_d, (E,), generator=g)])
    if kind == "rand37":
        n_src = n_dst = 37
        ei, gk = rnd(37, 37, 150), "3d"
    elif kind == "bip50_9_upper":
        n_src, n_dst = 50, 9
        ei = rnd(50, 9, 211)
    elif kind == "one_edge_dim2":   # dim = 2 with exactly one edge
        n_src, n_dst, dim, gk = 21, 5, 2, "2d"
        ei = torch.tensor([[13], [4]])
    elif kind == "rand300":
        n_src = n_dst = 300
        ei, gk = rnd(300, 300, 900), "3d"
    elif kind == "hub300":          # a hub of 300 in-edges (more than four 64-edge batches) among destinations of degree 0 / 1; odd n_dst
        n_src, n_dst = 200, 301
        degs = torch.randint(0, 2, (n_dst,), generator=g)
        degs[5] = 300
        ei = degree_graph(degs, n_src, g)
    elif kind == "empty_runs":      # no in-edge: destinations 0..9, 100..149 (inside), 290..298 (end); odd n_dst (last tile half full)
        n_src, n_dst = 120, 299
        degs = torch.randint(1, 6, (n_dst,), generator=g)
        degs[:10] = 0
        degs[100:150] = 0
        degs[290:] = 0
        ei = degree_graph(degs, n_src, g)
    elif kind == "n1024":           # the largest destination count of the 32-row forward
        n_src, n_dst = 700, 1024
        ei = degree_graph(torch.randint(0, 4, (n_dst,), generator=g), n_src, g)
    elif kind == "n1025":           # ... and the smallest of the 16-row forward
        n_src, n_dst = 700, 1025
        ei = degree_graph(torch.randint(0, 4, (n_dst,), generator=g), n_src, g)
    elif kind == "self_loops":
        n_src = n_dst = 300
        ei = rnd(300, 300, 900)
        ei[0, :150] = ei[1, :150]
    elif kind == "dim2":            # dim = 2 with a few hundred edges
        n_src, n_dst, dim, gk = 200, 150, 2, "2d"
        ei = rnd(200, 150, 400)
    elif kind == "bipartite":
        n_src, n_dst, gk = 900, 40, "3d"
        ei = rnd(900, 40, 700)
    elif kind == "empty":
        n_src, n_dst = 40, 30
        ei = torch.zeros(2, 0, dtype=torch.long)
    elif kind == "star_in":
        n_src, n_dst = 400, 1100
        ei = torch.stack([torch.randint(0, n_src, (900,), generator=g), torch.cat([torch.full((300,), 3), torch.randperm(n_dst, generator=g)[:600]])])
    elif kind == "star_out":
        n_src, n_dst = 1500, 1200
        ei = torch.stack([torch.cat([torch.full((200,), 17), torch.randint(0, 40, (300,), generator=g) * 37]),
                          torch.cat([torch.randperm(n_dst, generator=g)[:200], torch.randint(0, n_dst, (300,), generator=g)])])
    elif kind == "sparse_sources":
        n_src = n_dst = 2900
        idx = torch.arange(0, 2900, 29)
        ei = torch.stack([idx[torch.randint(0, 100, (700,), generator=g)], idx[torch.randint(0, 100, (700,), generator=g)]])
    elif kind == "chain_of_hubs":
        n_src = n_dst = 1300
        ps_, pd_ = [], []
        for hub, deg in ((15, 70), (16, 130), (31, 65)):
            ps_ += [torch.full((deg,), hub), torch.randint(0, n_src, (deg,), generator=g)]
            pd_ += [torch.randint(0, n_dst, (deg,), generator=g), torch.full((deg,), hub)]
        ei = torch.stack([torch.cat(ps_), torch.cat(pd_)])
    elif kind == "rand1500_upper":
        n_src = n_dst = 1500
        ei = rnd(1500, 1500, 2500)
    elif kind == "above_grid_cap":  # more destinations than the 16-row forward's 3072 wave slots: its grid-stride loop over chunks
        n_src, n_dst = 2000, 3100
        ei = degree_graph(torch.randint(0, 4, (n_dst,), generator=g), n_src, g)
    elif kind == "chunks":          # several nodes per chunk, forward (24 576 or more destinations) and backward (8 192 or more sources)
        n_src = n_dst = 24700
        ei = degree_graph(torch.randint(1, 4, (n_dst,), generator=g), n_src, g)
    elif kind == "empn_like":       # a few high-degree nodes behind many low-degree ones (the merged EMPN graph): a forward partition
        n_src, n_dst = 3000, 4000
        degs = torch.ones(n_dst, dtype=torch.long)
        degs[3600:] = 17
        ei = degree_graph(degs, n_src, g)
    else:                           # knn_like: every destination has 8 in-edges, the out-degrees of the sources vary widely: a backward partition
        n_src, n_dst = 3000, 2500
        near = (torch.rand(n_dst * 8, generator=g) ** 3 * n_src).long().clamp_(max=n_src - 1)
        ei = torch.stack([near, torch.repeat_interleave(torch.arange(n_dst), 8)])
    pos_s, pos_d = torch.rand(n_src, 3, generator=g) * 2 - 1, torch.rand(n_dst, 3, generator=g) * 2 - 1
    if kind == "self_loops":        # coincident positions: rel = 0 on the self-loops and on 100 more edges
        pos_d = pos_s.clone()
        pos_d[ei[1, 150:250]] = pos_s[ei[0, 150:250]]
    return ei, n_src, n_dst, dim, gk, pos_s, pos_d


def edge_case(kind, with_dres):
    ei, n_src, n_dst, dim, gk, pos_s, pos_d = edge_graph(kind)
    g = gen(8, (EDGE32_GRAPHS + EDGE16_GRAPHS).index(kind))
    w1, b1, w2, b2, wk = weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])
    inputs = {"x_src": torch.randn(n_src, 16, 64, generator=g), "w1": w1, "b1": b1, "w2": w2, "b2": b2, "wk": wk,
              "pos_s": pos_s, "pos_d": pos_d, "grid": grid_of(gk), "src": ei[0], "dst": ei[1]}
    if with_dres:   # the residual gradient enters as a second, linear use of x_src: d x_src = the convolution's + dres
        inputs["dres"] = torch.randn(n_src, 16, 64, generator=g)

    def ref(t):
        x1 = ops_ref.edge_conv(t["x_src"], t["src"], t["dst"], n_dst, t["grid"], t["pos_s"], t["pos_d"], t["w1"], t["b1"], t["w2"], t["b2"],
                               t["wk"], dim)
        out = {"x1": x1}
        if with_dres:
            out["res"] = (t["x_src"] * t["dres"]).sum().reshape(1)
        return out
    ups = {"x1": torch.randn(n_dst, 16, 64, generator=g)}
    if with_dres:
        ups["res"] = torch.ones(1)
    c = Case(f"edge_conv {kind} dres={with_dres}", inputs, ["x_src", "w1", "b1", "w2", "b2", "wk"], ref, ups)
    c.meta = (ei, n_src, n_dst, dim, gk)
    return c
