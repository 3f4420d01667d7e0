"""Pins tests/ops_ref.py, the float64 references tests/test_gpu_actor_ops.py holds the fp32 actor and critic kernels against, to the
oracle (values and gradients to 1e-12 in float64), derives the bars of the plain-FMA kernels from the error of the references' own fp32
evaluation (the table is printed), and checks that the inputs of tests/actor_cases.py are ones the reference alone handles."""
import torch
import torch.nn.functional as F

import actor_cases as ac
import ops_ref
from oracle import equivariant as eq
from oracle import graph as ogr
from oracle import trpl as otr


def close(name, a, b, tol=1e-12):
    err = float((a.detach() - b.detach()).abs().max())
    sc = max(1.0, float(b.detach().abs().max()))
    assert err <= tol * sc, (name, err, sc)


def test_margin_uses_the_own_scale_and_wants_exact_zeros():
    import pytest
    ref = torch.tensor([1e-6, -2e-6], dtype=torch.float64)
    assert ops_ref.margin("small", ref * (1 + 1e-5), ref, 2e-5) <= 1e-5 * (1 + 1e-9)
    with pytest.raises(AssertionError):
        ops_ref.margin("small", ref + 1e-7, ref, 1e-4)     # 5e-2 of its own scale: a max(1, .) floor would have let it pass
    assert ops_ref.margin("zero", torch.zeros(3), torch.zeros(3, dtype=torch.float64), 1e-4) == 0.0
    with pytest.raises(AssertionError):
        ops_ref.margin("zero", torch.full((3,), 1e-30), torch.zeros(3, dtype=torch.float64), 1e-4)
    assert ops_ref.round_up_1(2.01e-6) == 3e-6 and ops_ref.round_up_1(3e-6) == 3e-6 and ops_ref.round_up_1(9.5e-7) == 1e-6


def test_conv_block_chain_is_the_oracle():
    """edge_conv -> fiber_kernels -> fiber_conv -> node_mlp is the oracle's fiber_bundle_conv with its bases, for 3-d and 2-d grids."""
    for dim, upper in ((3, False), (3, True), (2, False)):
        g = torch.Generator().manual_seed(10 + dim + upper)
        n_src, n_dst, E = 23, 11, 57
        ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst - 1, (E,), generator=g)])
        grid = eq.make_grid(dim, 16, upper).double()
        pos_s, pos_d = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1 for n in (n_src, n_dst))
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) / s[-1] ** 0.5
        names = ["basis_fn.1.weight", "basis_fn.1.bias", "basis_fn.3.weight", "basis_fn.3.bias", "c.kernel.weight",
                 "fiber_basis_fn.1.weight", "fiber_basis_fn.1.bias", "fiber_basis_fn.3.weight", "fiber_basis_fn.3.bias", "c.fiber_kernel.weight",
                 "c.bias", "c.node_mlp.0.weight", "c.node_mlp.0.bias", "c.node_mlp.1.weight", "c.node_mlp.1.bias", "c.node_mlp.3.weight",
                 "c.node_mlp.3.bias"]
        shapes = [(64, 14), (64,), (64, 64), (64,), (64, 64), (64, 3), (64,), (64, 64), (64,), (64, 64), (64,), (64,), (64,), (256, 64), (256,),
                  (64, 256), (64,)]
        vals = [rnd(*s) for s in shapes] + [torch.randn(n_src, 16, 64, generator=g, dtype=torch.float64),
                                            torch.randn(n_dst, 16, 64, generator=g, dtype=torch.float64)]
        la = [t.clone().requires_grad_(True) for t in vals]
        lb = [t.clone().requires_grad_(True) for t in vals]
        # the oracle
        P = dict(zip(names, lb))
        xs, xd = lb[-2], lb[-1]
        kb = eq.basis_mlp(eq.spatial_invariants(grid, pos_s[ei[0]][:, :dim], pos_d[ei[1]][:, :dim]), P, "basis_fn")
        fb = eq.basis_mlp(eq.orientation_invariants(grid), P, "fiber_basis_fn")
        out_o, x1_o, x2_o = eq.fiber_bundle_conv(xs, xd, ei, kb, fb, P, "c", return_intermediates=True)
        # the references
        A = dict(zip(names, la))
        x1 = ops_ref.edge_conv(la[-2], ei[0], ei[1], n_dst, grid, pos_s, pos_d, *la[0:5], dim=dim)
        (fk,) = ops_ref.fiber_kernels(ops_ref.fiber_poly(grid), *la[5:9], [la[9]])
        close("fiber kernel", fk, F.linear(fb, lb[9]))
        x2 = ops_ref.fiber_conv(x1, fk, A["c.bias"])
        out = ops_ref.node_mlp(x2, la[-1], *la[11:17])
        close("x1", x1, x1_o)
        assert bool((x1[-1] == 0).all()), "a destination without in-edges"
        close("x2", x2, x2_o + lb[10])
        close("out", out, out_o)
        R = torch.randn(out.shape, generator=g, dtype=torch.float64)
        (out * R).sum().backward()
        (out_o * R).sum().backward()
        for n_, a, b in zip(names + ["x_src", "x_dst"], la, lb):
            close("grad " + n_, a.grad, b.grad)
        # prev: the sum over the edge types of a destination type (hetero_fiber_conv.py:63-64)
        close("prev", ops_ref.node_mlp(x2, la[-1], *la[11:17], prev=x1), out + x1)


def test_fiber_basis_reference_is_the_oracles_basis_mlp_and_fiber_kernel_linear():
    for kind in ac.GRID_KINDS:
        c = ac.fiber_basis_case(kind, 4)
        t = {k: ([u.double() for u in v] if isinstance(v, list) else v.double()) for k, v in c.inputs.items()}
        P = {"fiber_basis_fn.1.weight": t["w1"], "fiber_basis_fn.1.bias": t["b1"], "fiber_basis_fn.3.weight": t["w2"],
             "fiber_basis_fn.3.bias": t["b2"]}
        grid = ac.grid_of(kind).double()
        fb = eq.basis_mlp(eq.orientation_invariants(grid), P, "fiber_basis_fn")
        fks = ops_ref.fiber_kernels(ops_ref.fiber_poly(grid), t["w1"], t["b1"], t["w2"], t["b2"], t["wf"])
        for i in range(4):
            close(f"fk{i} {kind}", fks[i], F.linear(fb, t["wf"][i]))
        # the case's own polynomial features are the fp32 ones the model hands to the kernel (hepi.HEPi.fiber_poly)
        assert c.inputs["poly"].dtype == torch.float32 and c.inputs["poly"].shape == (16, 16, 3)
        close("poly", c.inputs["poly"].double(), ops_ref.fiber_poly(grid), 1e-6)


def test_lift_readout_and_critic_references_are_the_oracle():
    g = torch.Generator().manual_seed(3)
    for kind in ac.GRID_KINDS:
        grid = ac.grid_of(kind).double()
        dim = grid.shape[1]
        n, S, V = 19, 3, 4
        scal, vec = torch.randn(n, S, generator=g, dtype=torch.float64), torch.randn(n, V, 3, generator=g, dtype=torch.float64)
        w = torch.randn(64, S + V, generator=g, dtype=torch.float64)
        close("lift " + kind, ops_ref.lift_encode(scal, vec, grid, w), F.linear(eq.lift_features(scal, vec.reshape(n, -1), grid, dim), w))
        for od in (1, 2):
            c = ac.readout_case(7, od, od, kind)
            t = {k: v.double() for k, v in c.inputs.items()}
            outs, _ = c.evaluate()
            mean_o, hid_o = eq.readout(t["lat"], t["wd"], t["bd"], grid, dim, od, od)
            close("mean", outs["mean"].reshape(-1, 3), mean_o)
            close("hidden", outs["hidden"], hid_o)
            close("sigma", outs["sigma"], otr.std_head(hid_o, t["ws"], t["bs"], ac.INIT_STD, ac.MIN_STD, 7))
            if kind == "2d":
                assert bool((outs["mean"][..., 2] == 0).all())
    # no vectors at all: the scalars on every orientation
    close("lift V=0", ops_ref.lift_encode(scal, vec[:, :0], grid, w[:, :S]), F.linear(scal, w[:, :S])[:, None, :].expand(n, 16, 64))
    for B, n, d in ((1, 3, 15), (7, 35, 15), (1, 70, 4)):
        c = ac.deepsets_case(B, n, d)
        la = {k: v.double().requires_grad_(True) for k, v in c.inputs.items() if k != "x"}
        x = c.inputs["x"].double()
        ref = ogr.value_forward(la, x).reshape(B)
        R = c.ups["value"].double()
        (ref * R).sum().backward()
        outs, grads = c.evaluate()
        close("value", outs["value"], ref)
        for k in ops_ref.DEEPSETS_KEYS:
            close("critic grad " + k, grads[k], la[k].grad)
        # the ReLU branches handed in: the reference's own reproduce it
        _, p1, p2 = ops_ref.deepsets_value(x, [la[k].detach() for k in ops_ref.DEEPSETS_KEYS], want_pre=True)
        outs_m, grads_m = ac.deepsets_case(B, n, d, masks=(p1 > 0, p2 > 0)).evaluate()
        close("value (masks)", outs_m["value"], ref)
        for k in ops_ref.DEEPSETS_KEYS:
            close("critic grad (masks) " + k, grads_m[k], la[k].grad)


def test_bars_of_the_plain_fma_kernels_are_derived_from_the_references_own_fp32_error():
    """Per family: the worst error, relative to the tensor's own scale, of the fp32 torch CPU evaluation of the reference against its
    float64 evaluation on the same inputs.  The GPU bar is 8 x that (another summation order over the same number of fp32 terms), rounded
    up to one significant digit, and never above the bar tests/test_gpu_ops.py held the kernel to (ops_ref.OLD_BARS).  The worst fp32
    error depends on the CPU's summation order by a few per cent, hence ops_ref.BARS may sit within a factor 1.5 of the table's value."""
    print()
    print(f"{'family':12s} {'cases':>5s} {'worst fp32 value':>17s} {'worst fp32 grad':>16s} {'derived bars':>20s} {'ops_ref.BARS':>20s}")
    bad = []
    for fam, cases in ac.FMA_FAMILIES.items():
        worst_v, worst_g, where = 0.0, 0.0, ("", "")
        n_cases = 0
        for c in cases():
            o64, g64 = c.evaluate(torch.float64)
            o32, g32 = c.evaluate(torch.float32)
            n_cases += 1
            for k in o64:
                e = ops_ref.rel_err(o32[k], o64[k])
                if e > worst_v:
                    worst_v, where = e, (f"{c.name}: {k}", where[1])
            for k in g64:
                e = ops_ref.rel_err(g32[k], g64[k])
                if e > worst_g:
                    worst_g, where = e, (where[0], f"{c.name}: d {k}")
            del o64, g64, o32, g32
        old_v, old_g = ops_ref.OLD_BARS[fam]
        dv, dg = ops_ref.derived_bar(worst_v, old_v), ops_ref.derived_bar(worst_g, old_g)
        bv, bg = ops_ref.BARS[fam]
        print(f"{fam:12s} {n_cases:5d} {worst_v:17.2e} {worst_g:16.2e} {dv:9.0e} / {dg:8.0e} {bv:9.0e} / {bg:8.0e}   ({where[0]}; {where[1]})")
        assert bv <= old_v and bg <= old_g, (fam, "a bar above the old one")
        if not (dv / 1.5 <= bv <= dv * 1.5 and dg / 1.5 <= bg <= dg * 1.5):
            bad.append((fam, (dv, dg), (bv, bg)))
    assert not bad, bad


def test_node_block_inputs_are_ones_torchs_own_fp32_layer_norm_handles():
    """Rows m + s randn: ac.LN_MEAN_OVER_SPREAD is the largest power of two m / s for which torch's fp32 layer_norm stays within a quarter
    of the 1e-4 bar of the float64 result; every input family: the fp32 torch evaluation of the whole block within a quarter of the bars;
    constant rows: the normalised row is exactly beta."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(4096, 64, generator=g)
    gam, bet = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    ok = {}
    for k in range(0, 17):
        x = (2.0 ** k + z).float()
        r64 = F.layer_norm(x.double(), (64,), gam.double(), bet.double(), 1e-5)
        ok[k] = ops_ref.rel_err(F.layer_norm(x, (64,), gam, bet, 1e-5), r64)
        print(f"  m / s = 2^{k}: fp32 layer_norm off by {ok[k]:.2e} of the result's scale")
    largest = max(k for k in ok if all(ok[j] <= 0.25 * ops_ref.MFMA_VAL for j in range(k + 1)))
    assert 2.0 ** largest == ac.LN_MEAN_OVER_SPREAD, (largest, ok)
    for fam in ac.NODE_MLP_FAMILIES:
        c = ac.node_mlp_case(fam, 130, True)
        o64, g64 = c.evaluate(torch.float64)
        o32, g32 = c.evaluate(torch.float32)
        ev = ops_ref.rel_err(o32["out"], o64["out"])
        eg = max(ops_ref.rel_err(g32[k], g64[k]) for k in g64)
        print(f"  {fam}: fp32 torch block off by {ev:.2e} (value), {eg:.2e} (worst gradient)")
        assert ev <= 0.25 * ops_ref.MFMA_VAL and eg <= 0.25 * ops_ref.MFMA_GRAD, (fam, ev, eg)
    x = ac.node_mlp_rows("constant_rows", 7, torch.Generator().manual_seed(1))
    const = (x == x[..., :1]).all(-1)
    assert int(const.sum()) >= 7 * 8
    for dt in (torch.float32, torch.float64):
        h = F.layer_norm(x.to(dt), (64,), gam.to(dt), bet.to(dt), 1e-5)
        assert torch.equal(h[const], bet.to(dt).expand_as(h[const]))


def test_edge_graphs_have_the_features_their_names_promise():
    for kind in ac.EDGE32_GRAPHS + ac.EDGE16_GRAPHS:
        ei, n_src, n_dst, dim, gk, pos_s, pos_d = ac.edge_graph(kind)
        assert ei.shape[0] == 2 and (ei.numel() == 0 or (int(ei[0].max()) < n_src and int(ei[1].max()) < n_dst and int(ei.min()) >= 0)), kind
        assert (n_dst <= 1024) == (kind in ac.EDGE32_GRAPHS), kind
        deg = torch.bincount(ei[1], minlength=n_dst)
        if kind == "hub300":
            assert int(deg.max()) == 300 and int(deg[deg < 300].max()) == 1 and n_dst % 2 == 1
        if kind == "empty_runs":
            assert int(deg[:10].sum() + deg[100:150].sum() + deg[290:].sum()) == 0 and int(deg[10:100].min()) >= 1
        if kind == "self_loops":
            rel = pos_s[ei[0]] - pos_d[ei[1]]
            loops = int((ei[0] == ei[1]).sum())
            assert loops >= 150 and int((rel.abs().sum(-1) == 0).sum()) >= loops + 30
        if kind == "empty":
            assert ei.shape[1] == 0
