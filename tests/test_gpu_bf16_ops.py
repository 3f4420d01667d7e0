"""Per-op parity of the plain-bf16 build of the actor kernels (entry points ``*_bf16``, csrc/grl_common.h GRL_PREC = 1) -- FiberConv,
LiftEncode, LiftEncodeMulti, NodeMLP, EdgeConv -- through the ``ops.*`` autograd functions with ``prec="_bf16"``, on the case table of the
fp32 suite (tests/actor_cases.py, tests/test_gpu_actor_ops.py), each against the float64 emulation of that build's rounding points
(tests/bf16_ref.py, pinned to the oracle by tests/test_bf16_ref_cpu.py); and the merged launches (grl_lift_fiber_basis_bwd, grl_step_head,
both builds) called directly with a role absent, against the stand-alone launches, bitwise.

Every latent-typed input and every upstream gradient is rounded to bf16 first and handed over as torch.bfloat16; the reference sees the same
values.  A stored tensor is compared with its unrounded reference value, allowing the half bf16 ulp of its one store rounding on top of
the bar (margin16); an fp32 weight gradient plainly (margin); each against the tensor's OWN scale.  Every margin is printed.

Bars, as fractions of the tensor's own scale: "bar (measured worst on the MI355X)".
* EdgeConv, NodeMLP (one bf16 MFMA per product) -- the project's bars of that chain (tests/test_gpu_attention_ops.py B16_VAL / B16_DX /
  B16_GRAD): EdgeConv values 4e-3 (8.6e-4), stored gradients 4e-3 (8.8e-4), weight gradients 3e-3 (2.1e-4);
  NodeMLP values 4e-3 (9.4e-4), stored gradients 4e-3 (1.1e-3), weight gradients 3e-3 (1.0e-3); the node
  block behind its convolution (x1 stored in between) values 4e-3 (1.6e-3), d x 4e-3 (1.1e-3), weight gradients 3e-3 (5.0e-4).
* FiberConv, LiftEncode, LiftEncodeMulti (fp32 multiply-adds on bf16-exact values, one store) -- the fp32 build's own bars
  (ops_ref.BARS): FiberConv values 9e-7 (2.9e-7), gradients 4e-6 (stored 8.5e-8, weights 1.4e-7);
  LiftEncode / LiftEncodeMulti values 2e-6 (3.5e-8), weight gradient 6e-6 (2.2e-7).
tests/test_bf16_ref_cpu.py evaluates the emulation of every case below in fp32 and in float64 and holds the difference -- what last-bit
differences alone do to the reference -- under HALF of each bar; the other half is the kernel's.

Bitwise findings of the same run: x1 and d x_src with and without a balanced partition are equal (empn_like, knn_like: as in the fp32 build,
the partition changes which wave owns a node, not the order of a node's sum); EdgeConv (both forward kernels) and NodeMLP with their parameters
at float offset 1 or 3 equal the aligned call; LiftEncodeMulti's forward equals the single-type launches; every slab, fk, saved tensor and
image byte of the merged launches equals the stand-alone launches'."""
import ctypes

import pytest
import torch

import actor_cases as ac
import bf16_ref as br
import ops_ref
from test_gpu_attention_ops import B16_DX, B16_GRAD, B16_VAL, margin, margin16
from test_gpu_actor_ops import bits_equal, dev, dleaf

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# family -> (stored values, stored gradients, fp32 weight gradients)
BARS = {"FiberConv": (ops_ref.BARS["fiber_conv"][0], ops_ref.BARS["fiber_conv"][1], ops_ref.BARS["fiber_conv"][1]),
        "LiftEncode": (ops_ref.BARS["lift"][0], ops_ref.BARS["lift"][1], ops_ref.BARS["lift"][1]),
        "NodeMLP": (B16_VAL, B16_DX, B16_GRAD), "EdgeConv": (B16_VAL, B16_DX, B16_GRAD), "NodeBlock": (B16_VAL, B16_DX, B16_GRAD)}

# ------------------------------------------------------------------------------------------------ the case tables
LIFT_CASES = [(n, k, 3, 4) for n in ac.NODE_COUNTS for k in ("3d", "2d")] + [(301, k, S, V) for S, V in ac.LIFT_SPLITS for k in ("3d", "2d")]
NODE_MLP_CASES = list(ac.NODE_MLP_CASES)
# the graph kinds the bf16 build had not seen (tests/test_gpu_attention_ops.py has star_in ... chunks)
EDGE_CASES = [(k, False) for k in ("rand37", "bip50_9_upper", "hub300", "empty_runs", "n1024", "n1025", "self_loops", "empty", "rand1500_upper",
                                   "above_grid_cap")] + [(k, True) for k in ("hub300", "empty_runs", "empty")]
PARTITION_CASES = [("empn_like", False, ("split_d", "split_s")), ("knn_like", True, ("split_s",))]
UNALIGNED_EDGE = {"EdgeConv32": "rand300", "EdgeConv16": "rand1500_upper"}
UNALIGNED_NODE_MLP = ("randn", 700, True)
NODE_BLOCK = (300, 900)


def reference_cases():
    """(family, case) of every case a test of this file compares with the emulation (tests/test_bf16_ref_cpu.py walks them)."""
    for n in ac.NODE_COUNTS:
        yield "FiberConv", br.fiber_conv_case(n)
    for n, k, S, V in LIFT_CASES:
        yield "LiftEncode", br.lift_case(n, k, S, V)
    for ns, left_out, S, V, k in ac.LIFT_MULTI:
        yield "LiftEncode", br.lift_multi_case(ns, left_out, S, V, k)
    assert UNALIGNED_NODE_MLP[:2] in NODE_MLP_CASES
    for fam, n in NODE_MLP_CASES:
        for use_prev in (False, True):
            yield "NodeMLP", br.node_mlp_case(fam, n, use_prev)
    edge = EDGE_CASES + [(k, d_) for k, d_, _ in PARTITION_CASES] + [(k, False) for k in UNALIGNED_EDGE.values()]
    for kind, with_dres in dict.fromkeys(edge):
        yield "EdgeConv", br.edge_case(kind, with_dres)
    yield "NodeBlock", br.conv_block_case(*NODE_BLOCK)


def tensor_kind(name, is_output):
    """0: a stored value, 1: a stored gradient (of a latent input), 2: an fp32 weight gradient -- the index into BARS[family]."""
    return 0 if is_output else (1 if name in br.LATENTS else 2)


MEASURED = {}   # family -> worst margins [values, stored gradients, weight gradients] of this run (printed after every test)


def lat(t):
    """A device leaf holding the (bf16-exact) latent ``t`` as torch.bfloat16."""
    return t.to(dev()).to(BF).requires_grad_(True)


def compare(family, case, outs, grads, rdev="cpu"):
    """Every output and gradient of the HIP side against the float64 emulation of ``case``."""
    print(f"{case.name} (reference on {rdev})")
    o64, g64 = case.evaluate(torch.float64, rdev)
    w = MEASURED.setdefault(family, [0.0, 0.0, 0.0])
    for k, v in outs.items():
        assert v.dtype == BF, (k, v.dtype)
        w[0] = max(w[0], margin16(k, v, o64[k], BARS[family][0]))
    for k, v in grads.items():
        if tensor_kind(k, False) == 1:
            assert v.dtype == BF, (k, v.dtype)
            w[1] = max(w[1], margin16("d " + k, v, g64[k], BARS[family][1]))
        else:
            assert v.dtype == torch.float32, (k, v.dtype)
            w[2] = max(w[2], margin("d " + k, v, g64[k], BARS[family][2]))
    print(f"  [{family}: worst so far values {w[0]:.2e}, stored gradients {w[1]:.2e}, weight gradients {w[2]:.2e}]")
    return o64, g64


# ------------------------------------------------------------------------------------------------ FiberConv, LiftEncode, LiftEncodeMulti
@pytest.mark.parametrize("n", ac.NODE_COUNTS)
def test_fiber_conv(n):
    """Around the batch of four and its element-wise tail (1, 3, 4, 5), several batches per workgroup (9001), 70001: the packed backward
    batch of the bf16 build against x2, d x1, d fk and d bias."""
    from geometry_rl_amd import ops
    d = dev()
    c = br.fiber_conv_case(n)
    L = {"x1": lat(c.inputs["x1"]), "fk": dleaf(c.inputs["fk"]), "bias": dleaf(c.inputs["bias"])}
    out = ops.FiberConv.apply(L["x1"], L["fk"], L["bias"], "_bf16")
    out.backward(c.ups["x2"].to(d).to(BF))
    compare("FiberConv", c, {"x2": out.detach()}, {k: v.grad for k, v in L.items()}, d if n > 5000 else "cpu")


def run_lift(c, kind):
    from geometry_rl_amd import ops
    d = dev()
    w = dleaf(c.inputs["w"])
    x = ops.LiftEncode.apply(c.inputs["scal"].to(d), c.inputs["vec"].to(d), ac.grid3_of(kind).to(d), w, "_bf16")
    x.backward(c.ups["x"].to(d).to(BF))
    return x.detach(), w.grad


@pytest.mark.parametrize("n,kind,S,V", LIFT_CASES)
def test_lift_encode(n, kind, S, V):
    """The backward walks four nodes per wave and iteration: 77 nodes are 20 waves and one burst with dead slots (slots past N re-read
    the iteration's first node with their input zeroed), 70001 five sweeps, the last partial; every scalar / vector split at 301."""
    c = br.lift_case(n, kind, S, V)
    x, dw = run_lift(c, kind)
    compare("LiftEncode", c, {"x": x}, {"w": dw}, dev() if n > 5000 else "cpu")


@pytest.mark.parametrize("ns,left_out,S,V,kind", ac.LIFT_MULTI)
def test_lift_encode_multi(ns, left_out, S, V, kind):
    """Several node types in one launch each way: 1..4 types, a type without nodes in first / middle / last position, one type's output
    left out of the loss (its dx is None), every S / V split, 2-d and 3-d grids.  Forward bitwise equal to the single-type launches."""
    from geometry_rl_amd import ops
    d = dev()
    c = br.lift_multi_case(ns, left_out, S, V, kind)
    w = dleaf(c.inputs["w"])
    g3 = ac.grid3_of(kind).to(d)
    sv = [c.inputs[f"{a}{i}"].to(d) for i in range(len(ns)) for a in ("scal", "vec")]
    xs = ops.LiftEncodeMulti.apply(g3, w, "_bf16", *sv)
    used = [i for i in range(len(ns)) if c.ups[f"x{i}"] is not None]
    torch.autograd.backward([xs[i] for i in used], [c.ups[f"x{i}"].to(d).to(BF) for i in used])
    compare("LiftEncode", c, {f"x{i}": x.detach() for i, x in enumerate(xs)}, {"w": w.grad}, d if max(ns) > 5000 else "cpu")
    for i, x in enumerate(xs):
        if ns[i] > 0:
            single = ops.LiftEncode.apply(sv[2 * i], sv[2 * i + 1], g3, w.detach(), "_bf16")
            assert torch.equal(x.detach(), single), f"type {i}: the multi-type forward equals the single-type launch bitwise"


# ------------------------------------------------------------------------------------------------ NodeMLP
def run_node_mlp(family, n, use_prev, off=0):
    from geometry_rl_amd import ops
    d = dev()
    c = br.node_mlp_case(family, n, use_prev)
    L = {k: (lat(v) if k in br.LATENTS else dleaf(v, off)) for k, v in c.inputs.items()}
    out = ops.NodeMLP.apply(L["x2"], L["x_dst"], L["gamma"], L["beta"], L["w3"], L["b3"], L["w4"], L["b4"], L.get("prev"), None, "_bf16")
    out.backward(c.ups["out"].to(d).to(BF))
    return c, out.detach(), {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("family,n", NODE_MLP_CASES)
def test_node_mlp(family, n):
    """The fp32 suite's table: several chunks per workgroup of the backward (700, 1601), above the forward's 256 workgroups x 256 rows
    (4112, 4101: the grid-stride loop with a partial block); randn rows, constant rows (variance 0), rows with a mean far above their
    spread, rows scaled by 1e3 and 1e-3; with and without prev."""
    for use_prev in (False, True):
        c, out, grads = run_node_mlp(family, n, use_prev)
        compare("NodeMLP", c, {"out": out}, grads)
        up = c.ups["out"].to(BF)
        assert torch.equal(grads["x_dst"].cpu(), up), "d x_dst is d out itself"
        if use_prev:
            assert torch.equal(grads["prev"].cpu(), up), "d prev is d out itself"


def test_node_block_hands_its_residual_gradient_to_the_edge_conv():
    """hepi._conv in the bf16 build: x feeds the convolution AND the residual of its own node block; NodeMLP.backward leaves d out in the
    shared dict and the edge backward adds it inside the d x_src kernel.  Reference: edge_conv(stored=True) into node_mlp, d x the sum of
    both branches."""
    from geometry_rl_amd import ops
    d = dev()
    c = br.conv_block_case(*NODE_BLOCK)
    ei, n = c.meta
    L = {k: (lat(c.inputs[k]) if k == "x" else dleaf(c.inputs[k])) for k in c.diff}
    es = ops.build_edge_set(ei.to(d), n, n)
    pos = c.inputs["pos"].to(d)
    res = {}
    x1 = ops.EdgeConv.apply(L["x"], pos, pos, ac.grid3_of("upper").to(d), *[L[f"e{i}"] for i in range(5)], es, 3, res, "_bf16")
    out = ops.NodeMLP.apply(x1, L["x"], *[L[f"m{i}"] for i in range(6)], None, res, "_bf16")
    out.backward(c.ups["out"].to(d).to(BF))
    assert res == {}, "the edge backward consumes the residual gradient"
    compare("NodeBlock", c, {"out": out.detach()}, {k: v.grad for k, v in L.items()})


# ------------------------------------------------------------------------------------------------ EdgeConv
def run_edge(kind, with_dres, off=0):
    from geometry_rl_amd import ops
    d = dev()
    c = br.edge_case(kind, with_dres)
    ei, n_src, n_dst, dim, gk = c.meta
    es = ops.build_edge_set(ei.to(d), n_src, n_dst)
    L = {"x_src": lat(c.inputs["x_src"])}
    L.update({k: dleaf(c.inputs[k], off) for k in ("w1", "b1", "w2", "b2", "wk")})
    res = {"dres": c.inputs["dres"].to(d).to(BF)} if with_dres else None
    x1 = ops.EdgeConv.apply(L["x_src"], c.inputs["pos_s"].to(d), c.inputs["pos_d"].to(d), ac.grid3_of(gk).to(d), L["w1"], L["b1"], L["w2"],
                            L["b2"], L["wk"], es, dim, res, "_bf16")
    x1.backward(c.ups["x1"].to(d).to(BF))
    assert res is None or "dres" not in res, "the backward consumes the residual gradient"
    return c, es, x1.detach(), {k: v.grad for k, v in L.items()}


def check_edge(kind, with_dres, off=0):
    from geometry_rl_amd import hip
    c, es, x1, grads = run_edge(kind, with_dres, off)
    ei, n_src, n_dst, dim, gk = c.meta
    want_kind = 1 if kind in ac.EDGE32_GRAPHS else 0   # ops.WIMG_EDGE32 / WIMG_EDGE16: which forward kernel the launch takes
    assert hip.query("grl_edge_fwd_image_kind", n_dst) == want_kind, (kind, n_dst)
    rdev = dev() if es.n_edges > 3000 else "cpu"    # the float64 reference of the large cases runs as torch float64 ops on the GPU
    compare("EdgeConv", c, {"x1": x1}, grads, rdev)
    deg_in = torch.bincount(ei[1], minlength=n_dst)
    deg_out = torch.bincount(ei[0], minlength=n_src)
    assert bool((x1.cpu()[deg_in == 0] == 0).all()), "destinations without in-edges must be exactly 0"
    lone = deg_out == 0
    want = c.inputs["dres"][lone].to(BF) if with_dres else torch.zeros(int(lone.sum()), 16, 64, dtype=BF)
    assert torch.equal(grads["x_src"].cpu()[lone], want), "sources without out-edges: d x_src is the residual gradient itself (or 0)"
    if es.n_edges == 0:
        for k in ("w1", "b1", "w2", "b2", "wk"):
            assert bool((grads[k] == 0).all()), f"d {k}: the empty edge set has exactly-zero weight gradients"
    return c, es, x1, grads


@pytest.mark.parametrize("kind,with_dres", EDGE_CASES)
def test_edge_conv(kind, with_dres):
    """The 32-row forward (n_dst <= 1024: hubs, runs of empty destinations, a half-full last tile, n_dst = 1024, self-loops / coincident
    positions, the empty edge set) and the 16-row forward (n_dst = 1025, more destinations than wave slots), each with the fused backward;
    the residual gradient on a hub, on runs of empty destinations and on the empty edge set."""
    from geometry_rl_amd import hip
    c, es, _, _ = check_edge(kind, with_dres)
    if kind == "above_grid_cap":
        n_dst = c.meta[2]
        assert n_dst > hip.query("grl_edge_fwd_slots", n_dst) > 0


@pytest.mark.parametrize("kind,with_dres,which", PARTITION_CASES, ids=[c[0] for c in PARTITION_CASES])
def test_edge_conv_with_and_without_partition(kind, with_dres, which):
    """Graphs for which build_edge_set builds the balanced partition (grl_edge_conv_{fwd,bwd}_balanced_bf16): with and without it within
    the bars; the forward output and d x_src bitwise equal between the two (the partition changes which wave owns a node, not the order
    in which a node's edges are summed)."""
    from geometry_rl_amd import ops
    saved = ops.SPLIT_FORWARD, ops.SPLIT_BACKWARD
    runs = {}
    try:
        for on in (True, False):
            ops.SPLIT_FORWARD = ops.SPLIT_BACKWARD = on
            print(f"partitions {'on' if on else 'off'}")
            c, es, x1, grads = check_edge(kind, with_dres)
            for w in which:
                assert getattr(es, w) is not None, f"{kind}: build_edge_set built no {w}"
            runs[on] = (x1, grads)
    finally:
        ops.SPLIT_FORWARD, ops.SPLIT_BACKWARD = saved
    same_x1, same_dx = torch.equal(runs[True][0], runs[False][0]), torch.equal(runs[True][1]["x_src"], runs[False][1]["x_src"])
    print(f"{kind}: with and without the partition bitwise equal: x1 {same_x1}, d x_src {same_dx}")
    assert same_x1, "x1 with and without the forward partition"
    assert same_dx, "d x_src with and without the backward partition"


# ------------------------------------------------------------------------------------------------ unaligned parameter views
# The ops whose results with every parameter a view at an odd float offset are bitwise equal to the aligned call (as measured on the
# MI355X); printed for all, asserted for these.
BITWISE_WHEN_UNALIGNED = {"EdgeConv32", "EdgeConv16", "NodeMLP"}


@pytest.mark.parametrize("op", ["EdgeConv32", "EdgeConv16", "NodeMLP"])
def test_unaligned_parameter_views(op):
    """PolicyUpdater hands every kernel views into one flat buffer: every parameter at float offset 1 or 3 (pointer not 16-byte aligned;
    ops.weight_images then builds no image of the node block's backward, and the kernels stage the weights themselves)."""
    outs, grads = [], []
    for off in (0, 1, 3):
        print(f"{op}: parameters at float offset {off}")
        if op in UNALIGNED_EDGE:
            c, es, x1, g = run_edge(UNALIGNED_EDGE[op], False, off)
            o = {"x1": x1}
            compare("EdgeConv", c, o, g)
        else:
            c, out, g = run_node_mlp(*UNALIGNED_NODE_MLP, off)
            o = {"out": out}
            compare("NodeMLP", c, o, g)
        outs.append([o[k] for k in sorted(o)])
        grads.append([g[k] for k in sorted(g)])
    same = all(bits_equal(outs[0], outs[i]) and bits_equal(grads[0], grads[i]) for i in (1, 2))
    print(f"{op}: unaligned parameter views bitwise equal to the aligned call: {same}")
    if op in BITWISE_WHEN_UNALIGNED:
        assert same, op


# ------------------------------------------------------------------------------------------------ merged launches, called directly
def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else 0) for t in ts])


def fiber_basis_forward(n_conv, unused=None):
    """-> (case, poly2, [W1, b1, W2, b2], [Wf], saved, fks) after grl_fiber_basis_fwd as its own launch."""
    from geometry_rl_amd import hip
    d = dev()
    c = ac.fiber_basis_case("3d", n_conv, unused)
    P = [c.inputs[k].to(d) for k in ("w1", "b1", "w2", "b2")]
    W = [w.to(d) for w in c.inputs["wf"]]
    poly2 = c.inputs["poly"].reshape(256, 3).contiguous().to(d)
    saved = torch.full((4, 256, 64), float("nan"), device=d)
    fks = [torch.full((16, 16, 64), float("nan"), device=d) for _ in W]
    hip.call("grl_fiber_basis_fwd", poly2, *P, ptrs(W), n_conv, saved, ptrs(fks))
    return c, poly2, P, W, saved, fks


# (node counts per type, index of a type that is skipped -- n_nodes[t] = 0 and a NULL dx -- or None, n_conv, index of a NULL dfk or None)
TAIL_CASES = {"lift_alone": ([77, 5], None, 0, None), "fiber_basis_alone": ([], None, 3, None), "both": ([77, 130], None, 3, None),
              "four_types": ([4, 301, 1, 77], None, 2, None), "skipped_first": ([77, 5, 130], 0, 3, None),
              "skipped_middle": ([77, 5, 130], 1, 3, None), "skipped_last": ([77, 5, 130], 2, 3, None), "null_dfk": ([77, 5], None, 3, 1)}


@pytest.mark.parametrize("prec", ["", "_bf16"], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_lift_fiber_basis_backward_merged_launch(name, prec):
    """grl_lift_fiber_basis_bwd[_bf16] with either role absent, four types, a skipped type in every position, a NULL dfk: both partial
    slabs (prefilled with NaN) bitwise those of grl_lift_encode_bwd_multi[_bf16] and grl_fiber_basis_bwd launched alone, no row left
    unwritten."""
    from geometry_rl_amd import hip
    d = dev()
    ns, skipped, n_conv, null_dfk = TAIL_CASES[name]
    T, S, V = len(ns), 3, 4
    st = hip.storage_dtype(prec)
    nan = lambda r, c_: torch.full((r, c_), float("nan"), device=d)
    if T:
        cases = [br.lift_case(n, "3d", S, V, tag=i) for i, n in enumerate(ns)]
        scal, vec = [c.inputs["scal"].to(d) for c in cases], [c.inputs["vec"].to(d) for c in cases]
        dxs = [None if i == skipped else c.ups["x"].to(d).to(st) for i, c in enumerate(cases)]
        n_eff = (ctypes.c_int * T)(*[0 if i == skipped else n for i, n in enumerate(ns)])
        lift_rows = hip.query("grl_lift_bwd_blocks_multi", T, n_eff)
        assert lift_rows > 0
        largs = lambda part: [T, ptrs(scal), ptrs(vec), ac.grid3_of("3d").to(d), ptrs(dxs), part, n_eff, S, V]
    else:
        lift_rows = 0
        largs = lambda part: [0, None, None, None, None, None, None, 0, 0]
    if n_conv:
        c, poly2, P, W, saved, _ = fiber_basis_forward(n_conv, null_dfk)
        dfk = [c.ups[f"fk{i}"].to(d) if c.ups[f"fk{i}"] is not None else None for i in range(n_conv)]
        assert (null_dfk is None) or dfk[null_dfk] is None
        fb_shape = (hip.query("grl_fiber_basis_blocks"), hip.query("grl_fiber_basis_partial_size", n_conv))
        fargs = lambda part: [poly2, P[2], ptrs(W), n_conv, saved, ptrs(dfk), part]
    else:
        fargs = lambda part: [None, None, None, 0, None, None, None]
    lift_alone = lift_merged = fb_alone = fb_merged = None
    if T:
        lift_alone, lift_merged = nan(lift_rows, 64 * (S + V)), nan(lift_rows, 64 * (S + V))
        hip.call("grl_lift_encode_bwd_multi" + prec, *largs(lift_alone))
    if n_conv:
        fb_alone, fb_merged = nan(*fb_shape), nan(*fb_shape)
        hip.call("grl_fiber_basis_bwd", *fargs(fb_alone))
    hip.call("grl_lift_fiber_basis_bwd" + prec, *largs(lift_merged), *fargs(fb_merged))
    torch.cuda.synchronize()
    for what, alone, merged in (("lift", lift_alone, lift_merged), ("fiber basis", fb_alone, fb_merged)):
        if alone is not None:
            assert bool(torch.isfinite(merged).all()), f"{what}: a row of the merged launch's slab was left unwritten"
            assert torch.equal(alone, merged), f"{what}: the merged launch's slab differs from the stand-alone launch's"


@pytest.mark.parametrize("prec", ["", "_bf16"], ids=["fp32", "bf16"])
@pytest.mark.parametrize("roles", ["fiber_basis_alone", "images_alone", "both"])
def test_step_head_without_the_feature_role(roles, prec):
    """grl_step_head[_bf16] with n_desc = 0 and a NULL bump: fk, saved and the image bytes bitwise those of grl_fiber_basis_fwd and
    grl_weight_images[_bf16] (outputs prefilled, so no byte is left unwritten by one launch only)."""
    from geometry_rl_amd import hip, ops
    d = dev()
    with_fiber, with_images = roles != "images_alone", roles != "fiber_basis_alone"
    fargs = [None, None, None, None, None, None, 0, None, None]
    if with_fiber:
        n_conv = 3
        _, poly2, P, W, saved_alone, fks_alone = fiber_basis_forward(n_conv)
        saved = torch.full_like(saved_alone, float("nan"))
        fks = [torch.full_like(f, float("nan")) for f in fks_alone]
        fargs = [poly2, *P, ptrs(W), n_conv, saved, ptrs(fks)]
    wargs = [0, None, None, None]
    if with_images:
        g = ac.gen(10)
        w1, b1, w2, b2, wk = [w.to(d) for w in ac.weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])]
        gamma, beta = (torch.rand(64, generator=g) + 0.5).to(d), (torch.randn(64, generator=g) * 0.1).to(d)
        w3, b3, w4, b4 = [w.to(d) for w in ac.weights(g, [(256, 64), (256,), (64, 256), (64,)])]
        grid3 = ac.grid3_of("upper").to(d)
        edge_src = [w1, b1, w2, b2, wk, grid3]
        jobs = [(ops.WIMG_EDGE16, edge_src), (ops.WIMG_EDGE32, edge_src), (ops.WIMG_MLP_FWD, [w3, b3, w4, b4, gamma, beta]),
                (ops.WIMG_MLP_BWD16, [w3, w4])]
        n_img = len(jobs)
        assert n_img <= hip.query("grl_wimg_max_jobs")
        kinds = (ctypes.c_int * n_img)(*[k for k, _ in jobs])
        srcs = (ctypes.c_void_p * (6 * n_img))(*[p for _, s in jobs for p in [t.data_ptr() for t in s] + [0] * (6 - len(s))])
        image = lambda: [torch.full((hip.query("grl_wimg_bytes", k),), 0xAB, dtype=torch.uint8, device=d) for k, _ in jobs]
        img_alone, img_head = image(), image()
        hip.call("grl_weight_images" + prec, n_img, kinds, srcs, ptrs(img_alone))
        wargs = [n_img, kinds, srcs, ptrs(img_head)]
    hip.call("grl_step_head" + prec, None, 0, None, *fargs, *wargs)
    torch.cuda.synchronize()
    if with_fiber:
        assert bool(torch.isfinite(saved).all()) and torch.equal(saved, saved_alone), "saved"
        for i, (a, b) in enumerate(zip(fks_alone, fks)):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b), f"fk {i}"
    if with_images:
        for (k, _), a, b in zip(jobs, img_alone, img_head):
            assert torch.equal(a, b), f"image of kind {k}"
            assert not bool((b == 0xAB).all()), f"image of kind {k} was not written"
