"""Per-op parity of the fp32 actor and critic kernels -- EdgeConv, NodeMLP, FiberConv, LiftEncode, LiftEncodeMulti, FiberKernels, Readout,
DeepSetsValue -- through the ``ops.*`` autograd functions the model uses, each against the float64 reference of the same operation
(tests/ops_ref.py, pinned to the oracle by tests/test_ops_ref_cpu.py) on the inputs of tests/actor_cases.py.  Every tensor (output, input
gradient, every weight gradient) is compared against its OWN scale (no max(1, .) floor; a reference that is exactly zero must be matched
exactly); every margin is printed.

Bars, as fractions of the tensor's own scale: "bar (measured worst on the MI355X)".
* EdgeConv, NodeMLP (split-bf16 MFMA products) -- the bars tests/test_gpu_attention_ops.py holds the same chain to:
  EdgeConv values 1e-4 (4.2e-5), gradients 2e-4 (5.3e-5); NodeMLP values 1e-4 (2.3e-5), gradients 2e-4 (3.6e-5).
* The plain fp32 FMA kernels: 8 x the worst error of the reference's own fp32 torch CPU evaluation against its float64 evaluation,
  rounded up to one digit, never above the old bar (ops_ref.BARS; tests/test_ops_ref_cpu.py prints the table and checks the numbers):
  FiberConv values 9e-7 (3.4e-7), gradients 4e-6 (5.2e-7); LiftEncode / LiftEncodeMulti 2e-6 (1.5e-7), 6e-6 (2.4e-7);
  FiberKernels 4e-6 (5.8e-7), 7e-6 (5.7e-7); Readout 5e-6 (8.2e-7), 2e-5 (9.9e-7); DeepSetsValue 1e-5 (7.6e-7), 4e-5 (6.2e-6).
Bitwise findings of the same run: the forward output and d x_src with and without a balanced partition are equal; every op's results
with its parameters at an odd float offset equal the aligned call's (EdgeConv both forward kernels, NodeMLP, FiberKernels, Readout,
DeepSetsValue); LiftEncodeMulti's forward equals the single-type launches; no ReLU branch of the critic differed from the float64
reference's own (up to 4.6 M pre-activations per case)."""
import types

import pytest
import torch

import actor_cases as ac
import ops_ref
from ops_ref import margin

pytestmark = pytest.mark.gpu

MEASURED = {}   # family -> [worst value margin, worst gradient margin] of this run (printed after every test)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def dleaf(t, off=0):
    """A device leaf holding ``t``; ``off`` > 0: a view at that float offset into a larger buffer (its pointer is 4 * off bytes past a
    16-byte boundary, as the parameter views into PolicyUpdater's flat buffer may be)."""
    d = dev()
    if off == 0:
        return t.clone().to(d).requires_grad_(True)
    buf = torch.zeros(t.numel() + 8, device=d)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t.to(d))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (off % 4)
    return v.requires_grad_(True)


def compare(family, case, outs, grads, bar_v, bar_g, rdev="cpu"):
    """Every output and gradient of the HIP side against the float64 reference of ``case``."""
    print(f"{case.name} (reference on {rdev})")
    o64, g64 = case.evaluate(torch.float64, rdev)
    w = MEASURED.setdefault(family, [0.0, 0.0])
    for k, v in outs.items():
        w[0] = max(w[0], margin(k, v, o64[k], bar_v))
    for k, v in grads.items():
        w[1] = max(w[1], margin("d " + k, v, g64[k], bar_g))
    print(f"  [{family}: worst so far values {w[0]:.2e}, gradients {w[1]:.2e}]")
    return o64, g64


def bits_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ EdgeConv (fp32)
def run_edge(kind, with_dres, off=0):
    from geometry_rl_amd import ops
    d = dev()
    c = ac.edge_case(kind, with_dres)
    ei, n_src, n_dst, dim, gk = c.meta
    es = ops.build_edge_set(ei.to(d), n_src, n_dst)
    L = {"x_src": dleaf(c.inputs["x_src"])}
    L.update({k: dleaf(c.inputs[k], off) for k in ("w1", "b1", "w2", "b2", "wk")})
    res = {"dres": c.inputs["dres"].to(d)} if with_dres else None
    x1 = ops.EdgeConv.apply(L["x_src"], c.inputs["pos_s"].to(d), c.inputs["pos_d"].to(d), ac.grid3_of(gk).to(d), L["w1"], L["b1"], L["w2"],
                            L["b2"], L["wk"], es, dim, res)
    x1.backward(c.ups["x1"].to(d))
    assert res is None or "dres" not in res, "the backward consumes the residual gradient"
    return c, es, x1.detach(), {k: v.grad for k, v in L.items()}


def check_edge(kind, with_dres, off=0):
    from geometry_rl_amd import hip
    c, es, x1, grads = run_edge(kind, with_dres, off)
    ei, n_src, n_dst, dim, gk = c.meta
    want_kind = 1 if kind in ac.EDGE32_GRAPHS else 0   # ops.WIMG_EDGE32 / WIMG_EDGE16: which forward kernel the launch takes
    assert hip.query("grl_edge_fwd_image_kind", n_dst) == want_kind, (kind, n_dst)
    rdev = dev() if es.n_edges > 3000 else "cpu"    # the float64 reference of the large cases runs as torch float64 ops on the GPU
    compare("EdgeConv", c, {"x1": x1}, grads, ops_ref.MFMA_VAL, ops_ref.MFMA_GRAD, rdev)
    deg_in = torch.bincount(ei[1], minlength=n_dst)
    deg_out = torch.bincount(ei[0], minlength=n_src)
    assert bool((x1.cpu()[deg_in == 0] == 0).all()), "destinations without in-edges must be exactly 0"
    lone = deg_out == 0
    want = c.inputs["dres"][lone] if with_dres else torch.zeros(int(lone.sum()), 16, 64)
    assert torch.equal(grads["x_src"].cpu()[lone], want), "sources without out-edges: d x_src is the residual gradient itself (or 0)"
    if es.n_edges == 0:
        for k in ("w1", "b1", "w2", "b2", "wk"):
            assert bool((grads[k] == 0).all()), f"d {k}: the empty edge set has exactly-zero weight gradients"
    return c, es, x1, grads


@pytest.mark.parametrize("kind", ac.EDGE32_GRAPHS)
def test_edge_conv_32_row_forward(kind):
    """The few-tile 32-row forward (n_dst <= 1024) and the fused backward: hubs, runs of empty destinations, a half-full last tile,
    n_dst = 1024, self-loops / coincident positions, 2-d grids, bipartite sets, the empty edge set."""
    check_edge(kind, with_dres=False)


@pytest.mark.parametrize("kind", ac.EDGE16_GRAPHS)
def test_edge_conv_16_row_forward(kind):
    """The 16-row forward: ragged graphs, n_dst = 1025, more destinations than wave slots (grid-stride loop), several nodes per chunk."""
    from geometry_rl_amd import hip
    c, es, _, _ = check_edge(kind, with_dres=False)
    ei, n_src, n_dst, dim, gk = c.meta
    if kind == "above_grid_cap":
        assert n_dst > hip.query("grl_edge_fwd_slots", n_dst) > 0
    if kind == "chunks":
        assert hip.query("grl_edge_fwd_chunk_nodes", n_dst) >= 2 and hip.query("grl_edge_bwd_chunk_nodes", n_src) >= 2


@pytest.mark.parametrize("kind", ["one_edge_dim2", "hub300", "empty_runs", "bipartite", "empty", "chain_of_hubs", "sparse_sources", "chunks"])
def test_edge_conv_residual_gradient(kind):
    """residual={"dres": R}: d x_src is the kernel's sum plus R (on sources without out-edges: R alone, bitwise)."""
    check_edge(kind, with_dres=True)


@pytest.mark.parametrize("kind,which", [("empn_like", "split_d"), ("empn_like", "split_s"), ("knn_like", "split_s")])
def test_edge_conv_with_and_without_partition(kind, which):
    """A graph for which build_edge_set builds the balanced partition: with and without it within the bars; the forward output and d x_src
    bitwise equal between the two (the partition changes which wave owns a node, not the order in which a node's edges are summed)."""
    from geometry_rl_amd import ops
    saved = ops.SPLIT_FORWARD, ops.SPLIT_BACKWARD
    runs = {}
    try:
        for on in (True, False):
            ops.SPLIT_FORWARD = ops.SPLIT_BACKWARD = on
            print(f"partitions {'on' if on else 'off'}")
            c, es, x1, grads = check_edge(kind, with_dres=(kind == "knn_like"))
            assert getattr(es, which) is not None, f"{kind}: build_edge_set built no {which}"
            runs[on] = (x1, grads)
    finally:
        ops.SPLIT_FORWARD, ops.SPLIT_BACKWARD = saved
    assert torch.equal(runs[True][0], runs[False][0]), "x1 with and without the forward partition"
    assert torch.equal(runs[True][1]["x_src"], runs[False][1]["x_src"]), "d x_src with and without the backward partition"


@pytest.mark.parametrize("n,E", [(300, 900), (1500, 4000)])   # the 32-row and the 16-row forward
def test_node_block_hands_its_residual_gradient_to_the_edge_conv(n, E):
    """hepi._conv: x feeds the convolution AND the residual of its own node block; NodeMLP.backward leaves d out in the shared dict and
    the edge backward adds it inside the d x_src kernel.  d x against the float64 sum of both branches."""
    from geometry_rl_amd import ops
    d = dev()
    g = ac.gen(9, n, E)
    ei = torch.stack([torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)])
    pos = torch.rand(n, 3, generator=g) * 2 - 1
    we = ac.weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])
    wm = [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1] + ac.weights(g, [(256, 64), (256,), (64, 256), (64,)])
    inputs = {"x": torch.randn(n, 16, 64, generator=g), "pos": pos, "grid": ac.grid_of("upper"), "src": ei[0], "dst": ei[1]}
    inputs.update({f"e{i}": w for i, w in enumerate(we)})
    inputs.update({f"m{i}": w for i, w in enumerate(wm)})

    def ref(t):
        x1 = ops_ref.edge_conv(t["x"], t["src"], t["dst"], n, t["grid"], t["pos"], t["pos"], *[t[f"e{i}"] for i in range(5)])
        return {"out": ops_ref.node_mlp(x1, t["x"], *[t[f"m{i}"] for i in range(6)])}
    c = ac.Case(f"conv + node block n={n} E={E}", inputs, ["x"] + [f"e{i}" for i in range(5)] + [f"m{i}" for i in range(6)], ref,
                {"out": torch.randn(n, 16, 64, generator=g)})
    L = {k: dleaf(inputs[k]) for k in c.diff}
    es = ops.build_edge_set(ei.to(d), n, n)
    res = {}
    x1 = ops.EdgeConv.apply(L["x"], pos.to(d), pos.to(d), ac.grid3_of("upper").to(d), *[L[f"e{i}"] for i in range(5)], es, 3, res)
    out = ops.NodeMLP.apply(x1, L["x"], *[L[f"m{i}"] for i in range(6)], None, res)
    out.backward(c.ups["out"].to(d))
    assert res == {}
    compare("EdgeConv", c, {"out": out.detach()}, {k: v.grad for k, v in L.items()}, ops_ref.MFMA_VAL, ops_ref.MFMA_GRAD, d)


# ------------------------------------------------------------------------------------------------ NodeMLP (fp32)
def run_node_mlp(family, n, use_prev, off=0):
    from geometry_rl_amd import ops
    d = dev()
    c = ac.node_mlp_case(family, n, use_prev)
    L = {k: dleaf(v, off if k not in ("x2", "x_dst", "prev") else 0) for k, v in c.inputs.items()}
    out = ops.NodeMLP.apply(L["x2"], L["x_dst"], L["gamma"], L["beta"], L["w3"], L["b3"], L["w4"], L["b4"], L.get("prev"))
    out.backward(c.ups["out"].to(d))
    return c, out.detach(), {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("family,n", ac.NODE_MLP_CASES)
def test_node_mlp(family, n):
    """randn rows, constant rows (variance 0), rows with a mean far above their spread, rows scaled by 1e3 and 1e-3; with and without prev."""
    for use_prev in (False, True):
        c, out, grads = run_node_mlp(family, n, use_prev)
        compare("NodeMLP", c, {"out": out}, grads, ops_ref.MFMA_VAL, ops_ref.MFMA_GRAD)
        up = c.ups["out"]
        assert torch.equal(grads["x_dst"].cpu(), up), "d x_dst is d out itself"
        if use_prev:
            assert torch.equal(grads["prev"].cpu(), up), "d prev is d out itself"


# ------------------------------------------------------------------------------------------------ FiberConv, LiftEncode, LiftEncodeMulti
@pytest.mark.parametrize("n", ac.NODE_COUNTS)
def test_fiber_conv(n):
    from geometry_rl_amd import ops
    d = dev()
    c = ac.fiber_conv_case(n)
    L = {k: dleaf(v) for k, v in c.inputs.items()}
    out = ops.FiberConv.apply(L["x1"], L["fk"], L["bias"])
    out.backward(c.ups["x2"].to(d))
    compare("FiberConv", c, {"x2": out.detach()}, {k: v.grad for k, v in L.items()}, *ops_ref.BARS["fiber_conv"], d if n > 5000 else "cpu")


def run_lift(c, kind):
    from geometry_rl_amd import ops
    d = dev()
    w = dleaf(c.inputs["w"])
    x = ops.LiftEncode.apply(c.inputs["scal"].to(d), c.inputs["vec"].to(d), ac.grid3_of(kind).to(d), w)
    x.backward(c.ups["x"].to(d))
    return x.detach(), w.grad


@pytest.mark.parametrize("kind", ["3d", "2d"])
@pytest.mark.parametrize("n", ac.NODE_COUNTS)
def test_lift_encode(n, kind):
    c = ac.lift_case(n, kind)
    x, dw = run_lift(c, kind)
    compare("LiftEncode", c, {"x": x}, {"w": dw}, *ops_ref.BARS["lift"], dev() if n > 5000 else "cpu")


@pytest.mark.parametrize("kind", ["3d", "2d"])
@pytest.mark.parametrize("S,V", ac.LIFT_SPLITS)
def test_lift_encode_feature_splits(S, V, kind):
    c = ac.lift_case(301, kind, S, V)
    x, dw = run_lift(c, kind)
    compare("LiftEncode", c, {"x": x}, {"w": dw}, *ops_ref.BARS["lift"])


@pytest.mark.parametrize("ns,left_out,S,V,kind", ac.LIFT_MULTI)
def test_lift_encode_multi(ns, left_out, S, V, kind):
    """Several node types in one launch each way: 1..4 types, a type without nodes in first / middle / last position, one type's output
    left out of the loss (its dx is None), every S / V split, 2-d and 3-d grids.  Forward bitwise equal to the single-type launches."""
    from geometry_rl_amd import ops
    d = dev()
    cases = [ac.lift_case(n, kind, S, V, tag=i) for i, n in enumerate(ns)]
    w0 = cases[0].inputs["w"]
    inputs = {"w": w0, "grid": ac.grid_of(kind)}
    for i, c in enumerate(cases):
        inputs[f"scal{i}"], inputs[f"vec{i}"] = c.inputs["scal"], c.inputs["vec"]
    ref = lambda t: {f"x{i}": ops_ref.lift_encode(t[f"scal{i}"], t[f"vec{i}"], t["grid"], t["w"]) for i in range(len(ns))}
    ups = {f"x{i}": (None if i == left_out else c.ups["x"]) for i, c in enumerate(cases)}
    c = ac.Case(f"lift multi {ns} left out {left_out} S{S} V{V} {kind}", inputs, ["w"], ref, ups)
    w = dleaf(w0)
    g3 = ac.grid3_of(kind).to(d)
    sv = [inputs[f"{a}{i}"].to(d) for i in range(len(ns)) for a in ("scal", "vec")]
    xs = ops.LiftEncodeMulti.apply(g3, w, "", *sv)
    loss = sum((x * ups[f"x{i}"].to(d)).sum() for i, x in enumerate(xs) if ups[f"x{i}"] is not None)
    loss.backward()
    compare("LiftEncode", c, {f"x{i}": x.detach() for i, x in enumerate(xs)}, {"w": w.grad}, *ops_ref.BARS["lift"],
            d if max(ns) > 5000 else "cpu")
    for i, x in enumerate(xs):
        if ns[i] > 0:
            single = ops.LiftEncode.apply(sv[2 * i], sv[2 * i + 1], g3, w.detach())
            assert torch.equal(x.detach(), single), f"type {i}: the multi-type forward equals the single-type launch bitwise"


# ------------------------------------------------------------------------------------------------ FiberKernels
def run_fiber_kernels(c, n_conv, off=0):
    """Through ops.fiber_kernels (at most four convolutions per launch: five or more take two launches)."""
    from geometry_rl_amd import ops
    d = dev()
    L = {k: dleaf(c.inputs[k], off) for k in ("w1", "b1", "w2", "b2")}
    wf = [dleaf(w, off) for w in c.inputs["wf"]]
    ns = types.SimpleNamespace
    basis_fn = [None, ns(weight=L["w1"], bias=L["b1"]), None, ns(weight=L["w2"], bias=L["b2"])]
    convs = [ns(fiber_kernel=ns(weight=w)) for w in wf]
    fks = ops.fiber_kernels(c.inputs["poly"].to(d), basis_fn, convs)
    outs = {f"fk{i}": fks[id(cv)] for i, cv in enumerate(convs)}
    loss = sum((outs[k] * u.to(d)).sum() for k, u in c.ups.items() if u is not None)
    loss.backward()
    grads = {k: v.grad for k, v in L.items()}
    grads.update({f"wf#{i}": w.grad for i, w in enumerate(wf)})
    return {k: v.detach() for k, v in outs.items()}, grads


@pytest.mark.parametrize("kind", ac.GRID_KINDS)
@pytest.mark.parametrize("n_conv,unused", [(1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None),
                                           (3, 1), (4, 0), (6, 5)])
def test_fiber_kernels(n_conv, unused, kind):
    """Fiber basis + fiber kernels, all seven kinds of leaf gradients (W1, b1, W2, b2, every Wf); one fk unused (a NULL dfk pointer)."""
    c = ac.fiber_basis_case(kind, n_conv, unused)
    outs, grads = run_fiber_kernels(c, n_conv)
    assert all(g is not None for g in grads.values())
    compare("FiberKernels", c, outs, grads, *ops_ref.BARS["fiber_basis"])


@pytest.mark.parametrize("off", [1, 2, 3])
def test_fiber_kernels_with_unaligned_weights_are_bitwise_the_aligned_call(off):
    """Every weight a view at float offset 1, 2, 3 into a larger buffer (fb_stage's scalar path): the staging differs, the arithmetic does
    not."""
    c = ac.fiber_basis_case("upper", 4, 2)
    o0, g0 = run_fiber_kernels(c, 4)
    o1, g1 = run_fiber_kernels(c, 4, off)
    compare("FiberKernels", c, o1, g1, *ops_ref.BARS["fiber_basis"])
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "d " + k


def test_fiber_basis_backward_with_a_null_gradient_pointer():
    """Through autograd an unused fk reaches the backward as a zero tensor (undefined gradients are materialised), so the kernel's NULL
    dfk branch is only reached by a direct call: the partial rows must be bitwise those of the call with a zero tensor in its place."""
    import ctypes
    from geometry_rl_amd import hip
    d = dev()
    c = ac.fiber_basis_case("3d", 3, 1)
    P = [c.inputs[k].to(d) for k in ("w1", "b1", "w2", "b2")]
    W = [w.to(d) for w in c.inputs["wf"]]
    poly2 = c.inputs["poly"].reshape(256, 3).contiguous().to(d)
    saved = torch.empty(4, 256, 64, device=d)
    fks = [torch.empty(16, 16, 64, device=d) for _ in W]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else 0) for t in ts])
    hip.call("grl_fiber_basis_fwd", poly2, *P, ptrs(W), 3, saved, ptrs(fks))
    ups = [c.ups[f"fk{i}"].to(d) if c.ups[f"fk{i}"] is not None else None for i in range(3)]
    assert ups[1] is None
    parts = []
    for dfk in (ups, [u if u is not None else torch.zeros(16, 16, 64, device=d) for u in ups]):
        partial = torch.full((hip.query("grl_fiber_basis_blocks"), hip.query("grl_fiber_basis_partial_size", 3)), float("nan"), device=d)
        hip.call("grl_fiber_basis_bwd", poly2, P[2], ptrs(W), 3, saved, ptrs(dfk), partial)
        parts.append(partial)
    torch.cuda.synchronize()
    assert torch.equal(parts[0], parts[1]) and bool(torch.isfinite(parts[0]).all())
    _, g64 = c.evaluate()
    tot = parts[0].double().sum(0).cpu()
    o = 3 * 4096
    for k, lo, ln in [("wf#0", 0, 4096), ("wf#1", 4096, 4096), ("wf#2", 8192, 4096), ("w2", o, 4096), ("b2", o + 4096, 64), ("w1", o + 4160, 192),
                      ("b1", o + 4352, 64)]:
        margin("d " + k, tot[lo:lo + ln].reshape(g64[k].shape), g64[k], ops_ref.BARS["fiber_basis"][1])


# ------------------------------------------------------------------------------------------------ Readout
def run_readout(c, od, ov, kind, off=0):
    from geometry_rl_amd import ops
    from oracle import trpl as otr
    d = dev()
    shift = float(otr.inverse_softplus(torch.tensor(ac.INIT_STD - ac.MIN_STD)))
    L = {k: dleaf(c.inputs[k], off if k != "lat" else 0) for k in c.diff}
    mean, sigma, hidden = ops.Readout.apply(L["lat"], ac.grid3_of(kind).to(d), L["wd"], L["bd"], L["ws"], L["bs"], shift, ac.MIN_STD, od, ov)
    outs = {"mean": mean, "sigma": sigma, "hidden": hidden}
    sum((outs[k] * u.to(d)).sum() for k, u in c.ups.items() if u is not None).backward()
    return {k: v.detach() for k, v in outs.items()}, {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("kind", ac.GRID_KINDS)
@pytest.mark.parametrize("od", [1, 2])
@pytest.mark.parametrize("n", ac.READOUT_COUNTS)
def test_readout(n, od, kind):
    """(od, ov) = (1, 1) (the default of the cloth and rope configs) and (2, 2); full sphere, upper hemisphere (sum_o g_o far from 0:
    the bd * sum_o g_o term of the kernel's regrouped sums carries weight) and the 2-d grid; d hidden given and None; d mean or d sigma
    None."""
    variants = [(True, True, True), (False, True, True)]
    if n in (5, 130):
        variants += [(True, False, True), (True, True, False)]
    for dh, dm, ds in variants:
        c = ac.readout_case(n, od, od, kind, dh, dm, ds)
        outs, grads = run_readout(c, od, od, kind)
        compare("Readout", c, outs, grads, *ops_ref.BARS["readout"])


def test_readout_refuses_unequal_output_widths():
    """od != ov pairs scalar j with vector j that does not exist: the entry point returns -2 and launches nothing."""
    from geometry_rl_amd import hip
    d = dev()
    n = 5
    lat, grid3 = torch.randn(n, 16, 64, device=d), ac.grid3_of("3d").to(d)
    wd, bd, ws, bs = torch.randn(3, 64, device=d), torch.randn(3, device=d), torch.randn(3, 64, device=d), torch.randn(3, device=d)
    mean, sigma, hidden = torch.full((n, 1, 3), 7.0, device=d), torch.full((n, 3), 7.0, device=d), torch.full((n, 64), 7.0, device=d)
    with pytest.raises(RuntimeError, match="grl_readout_fwd failed with status -2"):
        hip.call("grl_readout_fwd", lat, grid3, wd, bd, ws, bs, 0.5, 1e-5, mean, sigma, hidden, n, 2, 1)
    torch.cuda.synchronize()
    assert bool((mean == 7).all()) and bool((sigma == 7).all()) and bool((hidden == 7).all()), "nothing was launched"


# ------------------------------------------------------------------------------------------------ DeepSets critic
def run_deepsets(B, n, dd, off=0):
    """-> (case with the ReLU branches the kernels took, value, gradients).  The kernels decide a branch on their fp32 pre-activation
    (h - mean) / (sigma + eps) * gamma + beta > 0 with the fp64 slot statistics rounded to fp32 (csrc/critic_ops.hip ln_stat); the same
    expression on the stored h1 / u1 gives the branches, and the float64 reference differentiates THOSE (a pre-activation within rounding
    distance of 0 may sit on the other side in float64; one flipped row would move a weight gradient by ~1e-3 of its scale)."""
    from geometry_rl_amd import ops
    d = dev()
    c0 = ac.deepsets_case(B, n, dd)
    L = {k: dleaf(c0.inputs[k], off) for k in ops_ref.DEEPSETS_KEYS}
    val = ops.DeepSetsValue.apply(c0.inputs["x"].to(d), *[L[k] for k in ops_ref.DEEPSETS_KEYS], None)
    pipe = val.grad_fn.pipe
    masks = []
    for h, st, cnt, nk in ((pipe.h1, pipe.stats1, pipe.c1, "gnn.mlp_inner.norms.0"), (pipe.u1, pipe.stats2, pipe.c2, "gnn.mlp_outer.norms.0")):
        s = st.reshape(-1, 2).sum(0)
        m = s[0] / cnt
        sig = (s[1] / cnt - m * m).clamp_min(0).sqrt().float()
        pre = (h - m.float()) / (sig + 1e-5) * L[nk + ".weight"].detach() + L[nk + ".bias"].detach()
        masks.append((pre > 0).cpu())
    (val * c0.ups["value"].to(d)).sum().backward()
    c = ac.deepsets_case(B, n, dd, masks=tuple(masks))
    # how many branches the float64 reference itself would have taken differently
    _, p1, p2 = ops_ref.deepsets_value(c0.inputs["x"].double(), [c0.inputs[k].double() for k in ops_ref.DEEPSETS_KEYS], want_pre=True)
    flips = int(((p1 > 0) != masks[0]).sum() + ((p2 > 0) != masks[1]).sum())
    total = p1.numel() + p2.numel()
    print(f"deepsets B={B} n={n} d={dd}: ReLU branches that differ from the float64 reference's own: {flips} of {total}")
    assert flips <= max(1, 1e-5 * total), (flips, total)
    return c, val.detach(), {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("B,n,dd", ac.DEEPSETS_SHAPES)
def test_deepsets_critic(B, n, dd):
    """The six critic kernels over batch / set / feature sizes around their tiling, plus one sample with one row and with 64+ rows."""
    c, val, grads = run_deepsets(B, n, dd)
    compare("DeepSets", c, {"value": val}, grads, *ops_ref.BARS["deepsets"])


# ------------------------------------------------------------------------------------------------ unaligned parameter views
# The ops whose results with every parameter a view at an odd float offset are bitwise equal to the aligned call (their arithmetic does not
# depend on the staging path: all of them, as measured on the MI355X); printed for all, asserted for these.
BITWISE_WHEN_UNALIGNED = {"EdgeConv32", "EdgeConv16", "NodeMLP", "Readout", "DeepSets"}


@pytest.mark.parametrize("op", ["EdgeConv32", "EdgeConv16", "NodeMLP", "Readout", "DeepSets"])
def test_unaligned_parameter_views(op):
    """PolicyUpdater hands every kernel views into one flat buffer: every parameter at float offset 1 or 3 (pointer not 16-byte aligned)."""
    outs, grads = [], []
    for off in (0, 1, 3):
        if op.startswith("EdgeConv"):
            c, es, x1, g = run_edge("rand300" if op == "EdgeConv32" else "rand1500_upper", False, off)
            o, bars = {"x1": x1}, (ops_ref.MFMA_VAL, ops_ref.MFMA_GRAD)
        elif op == "NodeMLP":
            c, out, g = run_node_mlp("randn", 700, True, off)
            o, bars = {"out": out}, (ops_ref.MFMA_VAL, ops_ref.MFMA_GRAD)
        elif op == "Readout":
            c = ac.readout_case(130, 2, 2, "upper")
            o, g = run_readout(c, 2, 2, "upper", off)
            bars = ops_ref.BARS["readout"]
        else:
            c, val, g = run_deepsets(9, 130, 13, off)
            o, bars = {"value": val}, ops_ref.BARS["deepsets"]
        print(f"{op}: parameters at float offset {off}")
        compare("EdgeConv" if op.startswith("EdgeConv") else op, c, o, g, *bars)
        outs.append([o[k] for k in sorted(o)])
        grads.append([g[k] for k in sorted(g)])
    same = all(bits_equal(outs[0], outs[i]) and bits_equal(grads[0], grads[i]) for i in (1, 2))
    print(f"{op}: unaligned parameter views bitwise equal to the aligned call: {same}")
    if op in BITWISE_WHEN_UNALIGNED:
        assert same, op
