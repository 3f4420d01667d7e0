"""Every actor and critic kernel on poisoned, guarded buffers (tests/footprint.py), through the ``ops.*`` functions the model uses.

Each case runs three times from identical inputs: plain (the run the per-op suites hold against float64 -- test_gpu_actor_ops.py,
test_gpu_bf16_ops.py, test_gpu_attention_ops.py, test_gpu_ops.py), under ``Guarded(NAN)`` and under ``Guarded(HUGE)``.  In the guarded
runs every output and workspace the op takes from ``torch.empty`` / ``torch.empty_like`` is poisoned and sits between poisoned guards,
and every input, upstream gradient and index array is wrapped the same way.  Asserted: ``ledger.check`` of both guarded runs (no guard
word changed, no input changed, no result element still poisoned or not finite, the proxy was in the path) and that every result of
both guarded runs is BITWISE the plain run's -- no tolerance anywhere: the kernels are deterministic and the views keep the alignment of
a plain allocation.  The cases are those of tests/actor_cases.py and of the attention suite, at the smallest sizes that still have the
tails; the float64 comparisons stay where they are.  The pre-split weight images are byte buffers whose layout has holes on purpose (LDS
bank padding; no lo halves in the bf16 build): they are held to the layout's own count of never-written words and to "every other word
is the same in all three runs" (``fp.unwritten_words``), and what the kernels compute from them to the checks above.  Every case prints how many allocations were interposed and how many inputs wrapped."""
import contextlib
import types

import pytest
import torch

import actor_cases as ac
import footprint as fp

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PRECS = pytest.mark.parametrize("prec", ["", "_bf16"], ids=["fp32", "bf16"])


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def storage(prec):
    return BF if prec else torch.float32


def image_holes(bf16):
    """32-bit words of each weight image that its producer never writes, from the layouts of csrc/grl_wimg.h: the images ARE the kernels' LDS
    structs, whose rows are padded against bank conflicts (the operand loads never touch the padding), and the bf16 build has no lo halves
    ("fully written except for the lo halves in the bf16 build", csrc/weight_images.hip).  rows x (padded - used) bf16 elements / 2, hi
    and lo image each; bf16 build: the lo images in full, the padding of the hi ones."""
    def rows(n, ld, used, arrays):   # arrays = number of (hi, lo) pairs of [n, ld] images
        pad, full = n * (ld - used) // 2, n * ld // 2
        return arrays * (full + pad if bf16 else 2 * pad)
    return {"e16": rows(64, 40, 32, 1) + rows(64, 80, 64, 4),      # W1 | W2, Wk, Wk^T, W2^T
            "e32": rows(64, 24, 16, 1) + rows(64, 72, 64, 2),      # W1 | W2, Wk
            "mlp_f": rows(256, 72, 64, 1) + rows(64, 264, 256, 1),  # W3 | W4
            "mlp_b": 3 * 4 * 4 * 2 * 64 * 4 if bf16 else 0}        # per-lane fragments, no padding: the lo fragments (16 bytes each)


IMAGE_HOLES = {False: image_holes(False), True: image_holes(True)}


def three_runs(op, label, run):
    """``fp.three_runs`` with the weight images held to the layout's own hole counts of the op's build."""
    return fp.three_runs(op, label, run, image_holes=IMAGE_HOLES[op.endswith("_bf16")])


def leaf(w, t):
    return w(t).requires_grad_(True)


def grads_of(leaves):
    return {k: v.grad for k, v in leaves.items()}


@contextlib.contextmanager
def ops_switches(**kw):
    from geometry_rl_amd import ops
    saved = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def mlp_weights(g):
    """(gamma, beta, W3, b3, W4, b4) of a ConvNeXt block."""
    return [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1] + ac.weights(g, [(256, 64), (256,), (64, 256), (64,)])


def images_of(ops, wk, n_dst, mlp, grid3, basis, prec, with_backward=True):
    """ops.weight_images for one block, called like hepi does (inside the guarded block: the image buffer is interposed)."""
    (img,) = ops.weight_images([(wk, n_dst, tuple(mlp))], grid3, tuple(basis), prec, with_backward)
    assert img is not None
    return img


def image_results(img):
    return {m: getattr(img, m) for m in ("e16", "e32", "mlp_f", "mlp_b") if getattr(img, m) is not None}


# ------------------------------------------------------------------------------------------------ EdgeConv
EDGE_KINDS = ac.EDGE32_GRAPHS + ["star_in", "star_out", "sparse_sources", "chain_of_hubs", "n1025", "chunks", "empn_like"]


@PRECS
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_edge_conv(kind, prec):
    """grl_edge_conv_fwd_balanced / _bwd_balanced: with and without the residual gradient, the balanced partitions (where build_edge_set
    builds one) and the weight images.  bip50_9_upper (211 edges) and one_edge_dim2 have odd edge counts: the odd tail of the backward's
    two-edges-per-pass walk."""
    from geometry_rl_amd import hip, ops
    d, st = dev(), storage(prec)
    c = ac.edge_case(kind, True)
    ei, n_src, n_dst, dim, gk = c.meta
    I = {k: c.inputs[k].to(d) for k in ("x_src", "w1", "b1", "w2", "b2", "wk", "pos_s", "pos_d", "dres")}
    I["x_src"], I["dres"], up = I["x_src"].to(st), I["dres"].to(st), c.ups["x1"].to(d).to(st)
    ei_d, g3 = ei.to(d), ac.grid3_of(gk).to(d)
    mlp = [t.to(d) for t in mlp_weights(ac.gen(31))]
    probe = ops.build_edge_set(ei_d, n_src, n_dst)
    has_split = probe.split_s is not None or probe.split_d is not None
    if kind == "empn_like":
        assert probe.split_d is not None, "empn_like: build_edge_set built no forward partition"
    if kind == "chunks":
        assert hip.query("grl_edge_fwd_chunk_nodes", n_dst) >= 2 and hip.query("grl_edge_bwd_chunk_nodes", n_src) >= 2
    assert kind not in ("bip50_9_upper", "one_edge_dim2") or probe.n_edges % 2 == 1

    def run(w, with_dres, images):
        es = fp.guard_edge_set(ops.build_edge_set(ei_d, n_src, n_dst), w)
        L = {k: leaf(w, I[k]) for k in ("x_src", "w1", "b1", "w2", "b2", "wk")}
        grid3 = w(g3)
        img = images_of(ops, L["wk"], n_dst, [w(t) for t in mlp], grid3, [L[k] for k in ("w1", "b1", "w2", "b2")], prec) if images else None
        res = {"dres": w(I["dres"])} if with_dres else None
        x1 = ops.EdgeConv.apply(L["x_src"], w(I["pos_s"]), w(I["pos_d"]), grid3, L["w1"], L["b1"], L["w2"], L["b2"], L["wk"], es, dim, res,
                                prec, img)
        x1.backward(w(up))
        assert res is None or "dres" not in res, "the backward consumes the residual gradient"
        return {"x1": x1.detach(), "grads": grads_of(L), "images": image_results(img) if img else None}

    for split in ((True, False) if has_split else (True,)):
        with ops_switches(SPLIT_FORWARD=split, SPLIT_BACKWARD=split):
            for with_dres in (False, True):
                for images in (False, True):
                    three_runs("EdgeConv" + prec, f"{kind} dres={with_dres} split={split} images={images}",
                               lambda w: run(w, with_dres, images))


# ------------------------------------------------------------------------------------------------ EdgeMessages + SoftmaxAggregate
@PRECS
@pytest.mark.parametrize("kind", ["star_in", "star_out", "one_edge", "self_loops", "chunks", "empty"])
def test_edge_messages_and_softmax_aggregate(kind, prec):
    """Per-edge messages into the per-destination softmax, as FiberBundleConv(aggr="AttentionalAggregation") chains them; star_in,
    star_out and one_edge have destinations without in-edges (x1 rows that must be written as zeros)."""
    import torch.nn.functional as F
    import test_gpu_attention_ops as att
    from geometry_rl_amd import ops
    from oracle import equivariant as eq
    d, st = dev(), storage(prec)
    g = torch.Generator().manual_seed(att.MSG_CASES.index(kind) + 5)
    ei, n_src, n_dst, dim, upper, pos_s, pos_d = att.msg_case(kind, g)
    grid = eq.make_grid(dim, 16, upper)
    g3 = F.pad(grid, (0, 3 - grid.shape[1])).contiguous().to(d)
    E = ei.shape[1]
    x_src = torch.randn(n_src, 16, 64, generator=g).to(d).to(st)
    W = [t.to(d) for t in att.weights(g)]
    gate = F.relu(torch.randn(E, 16, 64, generator=g) * 2).to(d)
    up = torch.randn(n_dst, 16, 64, generator=g).to(d).to(st)
    R = torch.randn(n_src, 16, 64, generator=g).to(d).to(st)
    ei_d, ps, pd = ei.to(d), pos_s.to(d), pos_d.to(d)
    if kind in ("star_in", "star_out", "one_edge"):
        assert int((torch.bincount(ei[1], minlength=n_dst) == 0).sum()) > 0

    def run(w, with_dres):
        es = fp.guard_edge_set(ops.build_edge_set(ei_d, n_src, n_dst), w)
        L = {"x_src": leaf(w, x_src), "gate": leaf(w, gate)}
        L.update({k: leaf(w, t) for k, t in zip(("w1", "b1", "w2", "b2", "wk"), W)})
        res = {"dres": w(R)} if with_dres else None
        msg = ops.EdgeMessages.apply(L["x_src"], w(ps), w(pd), w(g3), L["w1"], L["b1"], L["w2"], L["b2"], L["wk"], es, dim, res, prec)
        msg.retain_grad()
        x1 = ops.SoftmaxAggregate.apply(L["gate"], msg, es, prec)
        x1.backward(w(up))
        assert res is None or "dres" not in res
        return {"msg": msg.detach(), "x1": x1.detach(), "dmsg": msg.grad, "grads": grads_of(L)}

    for with_dres in (False, True):
        three_runs("EdgeMessages+SoftmaxAggregate" + prec, f"{kind} dres={with_dres}", lambda w: run(w, with_dres))


# ------------------------------------------------------------------------------------------------ NodeMLP
@PRECS
@pytest.mark.parametrize("n", [1, 7, 130, 700, 1601])
def test_node_mlp(n, prec):
    """grl_node_mlp_fwd_img / _bwd_img with and without prev, with and without the weight images.  The partial slab has blocks + 1 rows
    (the last one scratch); at 700 and 1601 nodes grl_node_mlp_bwd_blocks is capped and one workgroup walks several chunks."""
    from geometry_rl_amd import hip, ops
    d, st = dev(), storage(prec)
    c = ac.node_mlp_case("randn", n, True)
    I = {k: v.to(d) for k, v in c.inputs.items()}
    for k in ("x2", "x_dst", "prev"):
        I[k] = I[k].to(st)
    up = c.ups["out"].to(d).to(st)
    ew = [t.to(d) for t in ac.weights(ac.gen(32), [(64, 14), (64,), (64, 64), (64,), (64, 64)])]
    g3 = ac.grid3_of("upper").to(d)
    if n >= 700:
        assert hip.query("grl_node_mlp_bwd_blocks", 16 * n) == hip.query("grl_node_mlp_bwd_blocks", 16 * 100000), "the cap"

    def run(w, use_prev, images):
        L = {k: leaf(w, I[k]) for k in I if k != "prev" or use_prev}
        mlp = [L[k] for k in ("gamma", "beta", "w3", "b3", "w4", "b4")]
        img = images_of(ops, w(ew[4]), n, mlp, w(g3), [w(t) for t in ew[:4]], prec) if images else None
        out = ops.NodeMLP.apply(L["x2"], L["x_dst"], *mlp, L.get("prev"), None, prec, img)
        out.backward(w(up))
        return {"out": out.detach(), "grads": grads_of(L), "images": image_results(img) if img else None}

    for use_prev in (False, True):
        for images in (False, True):
            three_runs("NodeMLP" + prec, f"n={n} prev={use_prev} images={images}", lambda w: run(w, use_prev, images))


# ------------------------------------------------------------------------------------------------ FiberConv
@PRECS
@pytest.mark.parametrize("n", [1, 3, 4, 5, 77])
def test_fiber_conv(n, prec):
    """grl_fiber_conv_fwd / _bwd and the _sig forward, whose lane signal flag_dst[0] = flag_src[0] lands in a guarded word."""
    from geometry_rl_amd import ops
    d, st = dev(), storage(prec)
    c = ac.fiber_conv_case(n)
    I = {"x1": c.inputs["x1"].to(d).to(st), "fk": c.inputs["fk"].to(d), "bias": c.inputs["bias"].to(d)}
    up = c.ups["x2"].to(d).to(st)
    seven = torch.tensor([7], dtype=torch.int32, device=d)

    def run(w, sig):
        L = {k: leaf(w, v) for k, v in I.items()}
        flag = None
        if sig:
            flag = w.out((1,), torch.int32, d)
            ops.PENDING_SIGNAL = (flag, w(seven))
        try:
            x2 = ops.FiberConv.apply(L["x1"], L["fk"], L["bias"], prec)
            assert ops.PENDING_SIGNAL is None, "the forward launch takes the pending signal"
        finally:
            ops.PENDING_SIGNAL = None
        x2.backward(w(up))
        if sig:
            assert int(flag[0]) == 7
        return {"x2": x2.detach(), "grads": grads_of(L), "flag": flag}

    for sig in (False, True):
        three_runs("FiberConv" + prec, f"n={n} sig={sig}", lambda w: run(w, sig))


# ------------------------------------------------------------------------------------------------ LiftEncode, LiftEncodeMulti
def lift_inputs(c, kind, st):
    d = dev()
    return {"scal": c.inputs["scal"].to(d), "vec": c.inputs["vec"].to(d), "grid3": ac.grid3_of(kind).to(d), "w": c.inputs["w"].to(d),
            "up": c.ups["x"].to(d).to(st)}


LIFT_CASES = [(n, k, 3, 4) for n in ac.NODE_COUNTS if n <= 9001 for k in ("3d", "2d")] + [(301, k, S, V) for S, V in ac.LIFT_SPLITS
                                                                                         for k in ("3d", "2d")]


@PRECS
@pytest.mark.parametrize("n,kind,S,V", LIFT_CASES)
def test_lift_encode(n, kind, S, V, prec):
    from geometry_rl_amd import ops
    I = lift_inputs(ac.lift_case(n, kind, S, V), kind, storage(prec))

    def run(w):
        wl = leaf(w, I["w"])
        x = ops.LiftEncode.apply(w(I["scal"]), w(I["vec"]), w(I["grid3"]), wl, prec)
        x.backward(w(I["up"]))
        return {"x": x.detach(), "dw": wl.grad}

    three_runs("LiftEncode" + prec, f"n={n} {kind} S{S} V{V}", run)


@PRECS
@pytest.mark.parametrize("ns,left_out,S,V,kind", [m for m in ac.LIFT_MULTI if max(m[0]) <= 9001])
def test_lift_encode_multi(ns, left_out, S, V, kind, prec):
    """1..4 node types per launch, a type without nodes in every position, a type whose output gets no gradient (dx None)."""
    from geometry_rl_amd import ops
    d, st = dev(), storage(prec)
    Is = [lift_inputs(ac.lift_case(n, kind, S, V, tag=i), kind, st) for i, n in enumerate(ns)]

    def run(w):
        wl = leaf(w, Is[0]["w"])
        sv = [w(I[a]) for I in Is for a in ("scal", "vec")]
        xs = ops.LiftEncodeMulti.apply(w(Is[0]["grid3"]), wl, prec, *sv)
        used = [i for i in range(len(ns)) if i != left_out]
        torch.autograd.backward([xs[i] for i in used], [w(Is[i]["up"]) for i in used])
        return {"xs": [x.detach() for x in xs], "dw": wl.grad}

    three_runs("LiftEncodeMulti" + prec, f"{ns} left out {left_out} S{S} V{V} {kind}", run)


# ------------------------------------------------------------------------------------------------ FiberKernels
@pytest.mark.parametrize("n_conv,unused", [(1, None), (2, None), (3, None), (4, None), (3, 1), (4, 0)])
def test_fiber_kernels(n_conv, unused):
    """Through ops.fiber_kernels.  ``unused``: through autograd that fk's gradient arrives as zeros; the backward is ALSO called directly
    with None in its place (the kernel's NULL dfk pointer), fresh gradients returned."""
    from geometry_rl_amd import ops
    d = dev()
    c = ac.fiber_basis_case("upper", n_conv, unused)
    I = {k: c.inputs[k].to(d) for k in ("poly", "w1", "b1", "w2", "b2")}
    wf0 = [t.to(d) for t in c.inputs["wf"]]
    ups = [c.ups[f"fk{i}"].to(d) if c.ups[f"fk{i}"] is not None else None for i in range(n_conv)]
    ns = types.SimpleNamespace

    def run(w, direct):
        L = {k: leaf(w, I[k]) for k in ("w1", "b1", "w2", "b2")}
        L.update({f"wf{i}": leaf(w, t) for i, t in enumerate(wf0)})
        basis_fn = [None, ns(weight=L["w1"], bias=L["b1"]), None, ns(weight=L["w2"], bias=L["b2"])]
        convs = [ns(fiber_kernel=ns(weight=L[f"wf{i}"])) for i in range(n_conv)]
        fks = ops.fiber_kernels(w(I["poly"]), basis_fn, convs)
        outs = [fks[id(cv)] for cv in convs]
        dfk = [w(u) if u is not None else None for u in ups]
        if direct:
            with torch.no_grad():
                got = ops.FiberKernels.backward(outs[0].grad_fn, *dfk)
            return {"fk": [o.detach() for o in outs], "grads": list(got)}
        used = [i for i in range(n_conv) if dfk[i] is not None]
        torch.autograd.backward([outs[i] for i in used], [dfk[i] for i in used])
        return {"fk": [o.detach() for o in outs], "grads": grads_of(L)}

    three_runs("FiberKernels", f"n_conv={n_conv} unused={unused}", lambda w: run(w, False))
    if unused is not None:
        three_runs("FiberKernels", f"n_conv={n_conv} unused={unused}, backward called with None", lambda w: run(w, True))


# ------------------------------------------------------------------------------------------------ Readout
@pytest.mark.parametrize("od", [1, 2])
@pytest.mark.parametrize("n", ac.READOUT_COUNTS)
def test_readout(n, od):
    from geometry_rl_amd import ops
    from oracle import trpl as otr
    d = dev()
    shift = float(otr.inverse_softplus(torch.tensor(ac.INIT_STD - ac.MIN_STD)))
    for kind in ("upper", "2d"):
        for with_dh in (True, False):
            c = ac.readout_case(n, od, od, kind, with_dh)
            I = {k: c.inputs[k].to(d) for k in c.diff}
            g3 = ac.grid3_of(kind).to(d)
            ups = {k: (u.to(d) if u is not None else None) for k, u in c.ups.items()}

            def run(w):
                L = {k: leaf(w, v) for k, v in I.items()}
                mean, sigma, hidden = ops.Readout.apply(L["lat"], w(g3), L["wd"], L["bd"], L["ws"], L["bs"], shift, ac.MIN_STD, od, od)
                outs = {"mean": mean, "sigma": sigma, "hidden": hidden}
                used = [k for k in outs if ups[k] is not None]
                torch.autograd.backward([outs[k] for k in used], [w(ups[k]) for k in used])
                return {"outs": {k: v.detach() for k, v in outs.items()}, "grads": grads_of(L)}

            three_runs("Readout", f"n={n} od={od} {kind} dhidden={with_dh}", run)


@pytest.mark.parametrize("poison", fp.POISONS)
def test_a_slab_row_no_workgroup_wrote_is_noticed(poison, monkeypatch):
    """That the guarded runs see what plain runs cannot, on the real kernels and inside the allocations: a host that sizes the read-out's
    partial slab one row larger than the kernel's grid (here: the query answers one more) makes the fold read a row no workgroup wrote.
    On a fresh ``torch.empty`` that row is very often zero; poisoned, it reaches every weight gradient and check (c) reports it."""
    from geometry_rl_amd import hip, ops
    from oracle import trpl as otr
    d = dev()
    shift = float(otr.inverse_softplus(torch.tensor(ac.INIT_STD - ac.MIN_STD)))
    c = ac.readout_case(130, 2, 2, "upper")
    real_query = hip.query
    monkeypatch.setattr(hip, "query", lambda name, *a: real_query(name, *a) + (1 if name == "grl_readout_blocks" else 0))
    with fp.Guarded(poison) as ledger:
        L = {k: leaf(ledger.guard, c.inputs[k].to(d)) for k in c.diff}
        outs = ops.Readout.apply(L["lat"], ledger.guard(ac.grid3_of("upper").to(d)), L["wd"], L["bd"], L["ws"], L["bs"], shift, ac.MIN_STD, 2, 2)
        torch.autograd.backward(list(outs), [ledger.guard(c.ups[k].to(d)) for k in ("mean", "sigma", "hidden")])
        torch.cuda.synchronize()
    ledger.check({"outs": [o.detach() for o in outs], "dlat": L["lat"].grad})   # what the kernels write themselves is sound
    with pytest.raises(AssertionError, match=r"\(c\) result wd "):
        ledger.check(grads_of(L))


# ------------------------------------------------------------------------------------------------ DeepSets critic
@pytest.mark.parametrize("B,n,dd", ac.DEEPSETS_SHAPES)
def test_deepsets_value(B, n, dd):
    """The six critic kernels: the four stat-slot arrays (fp64, per-workgroup, "written in full by the producing stage") and the three
    partial slabs are interposed; B = 1, n not a multiple of 64, d = 1 and 16 are in the table."""
    import ops_ref
    from geometry_rl_amd import ops
    d = dev()
    c = ac.deepsets_case(B, n, dd)
    I = {k: c.inputs[k].to(d) for k in ops_ref.DEEPSETS_KEYS}
    x, up = c.inputs["x"].to(d), c.ups["value"].to(d)

    def run(w):
        L = {k: leaf(w, v) for k, v in I.items()}
        val = ops.DeepSetsValue.apply(w(x), *[L[k] for k in ops_ref.DEEPSETS_KEYS], None)
        val.backward(w(up))
        return {"value": val.detach(), "grads": grads_of(L)}

    three_runs("DeepSetsValue", f"B={B} n={n} d={dd}", run)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("B,n,dd", [(1, 3, 15), (1, 70, 15), (5, 67, 1), (3, 64, 16), (7, 35, 15), (2, 257, 15)])
def test_deepsets_values_groups(B, n, dd, groups):
    import ops_ref
    from geometry_rl_amd import ops
    d = dev()
    c = ac.deepsets_case(B, n, dd)
    P = [c.inputs[k].to(d) for k in ops_ref.DEEPSETS_KEYS]
    x = torch.randn(groups * B, n, dd, generator=ac.gen(33, B, n, dd, groups)).to(d)

    def run(w):
        return {"value": ops.deepsets_values_groups(w(x), [w(t) for t in P], groups)}

    plain = three_runs("deepsets_values_groups", f"B={B} n={n} d={dd} groups={groups}", run)
    assert plain["value"].shape == (groups, B)


# ------------------------------------------------------------------------------------------------ weight images
@PRECS
@pytest.mark.parametrize("n_dst,with_backward", [(300, True), (300, False), (2000, True), (2000, False)])
def test_weight_images(n_dst, with_backward, prec):
    """ops.weight_images, sized by grl_wimg_bytes: 300 destinations take the 32-row forward image (with the backward all four kinds),
    2000 the 16-row one."""
    from geometry_rl_amd import hip, ops
    d = dev()
    g = ac.gen(34)
    ew = [t.to(d) for t in ac.weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])]
    mlp = [t.to(d) for t in mlp_weights(g)]
    g3 = ac.grid3_of("upper").to(d)
    kind = hip.query("grl_edge_fwd_image_kind", n_dst)
    want = {"mlp_f"} | ({"e32"} if kind == ops.WIMG_EDGE32 else set()) | ({"e16"} if with_backward or kind == ops.WIMG_EDGE16 else set()) \
        | ({"mlp_b"} if with_backward else set())

    def run(w):
        img = images_of(ops, w(ew[4]), n_dst, [w(t) for t in mlp], w(g3), [w(t) for t in ew[:4]], prec, with_backward)
        return {"images": image_results(img)}

    plain = three_runs("weight_images" + prec, f"n_dst={n_dst} with_backward={with_backward}", run)["images"]
    assert set(plain) == want, (set(plain), want)
    sizes = {"e16": 0, "e32": 1, "mlp_f": 2, "mlp_b": 3}
    for m, v in plain.items():
        assert v.numel() == hip.query("grl_wimg_bytes", sizes[m]), m


# ------------------------------------------------------------------------------------------------ the feature builder
def feature_case(name, B):
    from geometry_rl_amd import graph, synthetic as syn
    if name == "rigid_tiny":   # 1, 2, 3, 32, 5, 4 valid object points: padding dropped from the actor graph
        from oracle_cases import make_case
        _, spec, _, obs = make_case("rigid_tiny", B)
        return spec, obs
    assert name == "rope_var", name
    return graph.rope_spec(n_links=20, variable_length=True), syn.make_rope_obs(B, n_links=20, seed=6, variable_length=True)


@pytest.mark.parametrize("layout", ["per_type", "dense"])
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", ["rigid_tiny", "rope_var"])
def test_feature_builder(name, noise, layout):
    """HyperData.build_data at B = 12, padded (rigid_tiny) and variable-length (rope_var) samples, with and without training noise: the
    first call builds the topology (its kNN buffers are interposed too), the second is the cached path."""
    from geometry_rl_amd import graph
    d, B = dev(), 12
    spec, obs = feature_case(name, B)
    obs_d = [obs[k].to(d) for k in spec.in_features]
    dense = layout == "dense"

    def run(w):
        hd = graph.HyperData(spec, full_graph_obs=dense, dist_as_pos=True, output_mask_key=None if dense else "grippers",
                             concat_input_vector=dense, training_noise=noise, training_noise_std=0.01, noise_seed=0x1234_5678_9abc_def0)
        args = [w(t) if t.is_floating_point() else t for t in obs_d]
        res = []
        for _ in range(2):
            gb, out = hd.build_data(*args, train=True)
            edges = [[e.rowptr_d, e.src_d, e.dst_d, e.rowptr_s, e.src_s, e.dst_s] for e in gb.edges.values() if e is not None]
            res.append({"x": out, "edges": edges} if dense else {"pos": gb.pos_all, "vec": gb.vec_all, "edges": edges})
        return {"calls": res}

    three_runs("HyperData.build_data", f"{name} noise={noise} {layout}", run)


# ------------------------------------------------------------------------------------------------ one eager update
UPDATES = {"hepi_fp32": ("rigid_tiny", {}), "hepi_bf16": ("rigid_tiny", dict(precision="bf16")), "hepi_attention": ("rigid_attn", {}),
           "empn": ("empn_g2", {})}


@pytest.mark.parametrize("name", list(UPDATES))
def test_one_eager_update(name, monkeypatch):
    """loss(batch) and both backward passes with the deferred folds flushed, as PolicyUpdater issues them eagerly (the merged head launch,
    the merged lift / fiber-basis backward, the fold queue with poisoned slabs), at B = 12 from a fresh seeded agent: the flat gradient
    and the parameters after the step, bit for bit.  Attention runs on the HEPi actor (the EMPN actor has no attention form here)."""
    from geometry_rl_amd import agent, hip, synthetic as syn
    from oracle_cases import make_case
    d, B = dev(), 12
    case, extra = UPDATES[name]
    _, spec, kw, obs = make_case(case, B)
    cfg = agent.AgentConfig(**dict(kw, **extra))
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=B))
    dbatch = {k: v.to(d) for k, v in batch.items()}

    def run(w):
        torch.manual_seed(3)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=d)
        upd = agent.PolicyUpdater(loss)
        out = upd.step({k: (w(v) if v.is_floating_point() else v) for k, v in dbatch.items()})
        torch.cuda.synchronize()
        assert not upd.mode.startswith("graph")
        return {"gradient": upd.gflat.clone(), "parameters": upd.flat.clone(), "loc": out["loc"], "state_value": out["state_value"]}

    launched = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), real_call(entry, *a, **k))[1])
    plain = three_runs("eager update", name, run)
    assert bool(plain["gradient"].abs().max() > 0)
    names = sorted(set(launched))
    print(f"eager update {name}: entry points launched: {names}")
    # what this case is for: the merged head launch, the merged lift / fiber-basis backward, the queued folds (flushed by the fused tail, or,
    # with the attention gate, by the fold launch of its own)
    for want in (("grl_step_head",), ("grl_lift_fiber_basis_bwd",), ("grl_fold_adam_report", "grl_reduce_partials_multi_ow")):
        assert any(n.startswith(want) for n in names), (want, names)
