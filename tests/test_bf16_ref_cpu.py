"""Pins tests/bf16_ref.py, the float64 emulation of the plain-bf16 kernels that tests/test_gpu_attention_ops.py checks them against:
with its roundings switched off and the erf GELU it must BE the oracle's maths (values and gradients to 1e-12), the normal CDF of its GELU
approximant must stay within 1.4e-4 of Phi (csrc/grl_common.h), and with roundings on it must round where it says it does.  The last test
measures how far last-bit differences alone move the emulation on the cases of tests/test_gpu_bf16_ops.py (fp32 against float64
evaluation) and holds that under half of each bar of that file."""
import torch
import torch.nn.functional as F

import bf16_ref as br
import ops_ref
from oracle import equivariant as eq


def close(name, a, b, tol=1e-12):
    err = float((a.detach() - b.detach()).abs().max())
    sc = max(1.0, float(b.detach().abs().max()))
    assert err <= tol * sc, (name, err, sc)


def _edge_inputs(seed, n_src=23, n_dst=11, E=57, dim=3):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)
    grid = eq.make_grid(dim, 16).double()
    pos_s, pos_d = (torch.rand(n, dim, generator=g, dtype=torch.float64) * 2 - 1 for n in (n_src, n_dst))
    x = torch.randn(n_src, 16, 64, generator=g, dtype=torch.float64)
    W = [torch.randn(*s, generator=g, dtype=torch.float64) / s[-1] ** 0.5 for s in [(64, 14), (64,), (64, 64), (64,), (64, 64)]]
    return src, dst, n_dst, grid, pos_s, pos_d, x, W


def test_edge_ops_without_rounding_are_the_oracle():
    for dim in (3, 2):
        src, dst, n_dst, grid, pos_s, pos_d, x, W = _edge_inputs(dim, dim=dim)
        la = [t.clone().requires_grad_(True) for t in [x] + W]
        lb = [t.clone().requires_grad_(True) for t in [x] + W]
        P = {"b.1.weight": lb[1], "b.1.bias": lb[2], "b.3.weight": lb[3], "b.3.bias": lb[4]}
        kb = eq.basis_mlp(eq.spatial_invariants(grid, pos_s[src], pos_d[dst]), P, "b")
        msg_o = F.linear(kb, lb[5]) * lb[0][src]
        msg = br.edge_messages(la[0], src, grid, pos_s[src], pos_d[dst], *la[1:], rounding=False, logistic=False)
        close("msg", msg, msg_o)
        x1 = br.edge_conv(la[0], src, dst, n_dst, grid, pos_s[src], pos_d[dst], *la[1:], rounding=False, logistic=False)
        x1_o = eq.scatter_sum(msg_o, dst, n_dst)
        close("x1", x1, x1_o)
        R = torch.randn(x1.shape, dtype=torch.float64)
        (x1 * R).sum().backward()
        (x1_o * R).sum().backward()
        for a, b in zip(la, lb):
            close("grad", a.grad, b.grad)


def test_node_mlp_and_softmax_without_rounding_are_the_oracle():
    g = torch.Generator().manual_seed(4)
    n = 9
    ts = [torch.randn(n, 16, 64, generator=g, dtype=torch.float64) for _ in range(3)]
    ws = [torch.randn(*s, generator=g, dtype=torch.float64) / s[-1] ** 0.5 for s in [(64,), (64,), (256, 64), (256,), (64, 256), (64,)]]
    la = [t.clone().requires_grad_(True) for t in ts + ws]
    lb = [t.clone().requires_grad_(True) for t in ts + ws]
    x2, xd, pv, gm, bt, w3, b3, w4, b4 = lb
    ref = xd + F.linear(F.gelu(F.linear(F.layer_norm(x2, (64,), gm, bt, 1e-5), w3, b3)), w4, b4) + pv
    out = br.node_mlp(la[0], la[1], *la[3:], prev=la[2], rounding=False, logistic=False)
    close("node mlp", out, ref)
    R = torch.randn(out.shape, dtype=torch.float64)
    (out * R).sum().backward()
    (ref * R).sum().backward()
    for a, b in zip(la, lb):
        close("node mlp grad", a.grad, b.grad)

    # softmax aggregation with the gate given: PyG AttentionalAggregation once the gate network's output is fed in
    E, n_dst = 40, 13
    dst = torch.randint(0, n_dst - 2, (E,), generator=g)                 # the last two destinations have no in-edge
    msg = torch.randn(E, 16, 64, generator=g, dtype=torch.float64)
    wg, bgt = torch.randn(64, 64, generator=g, dtype=torch.float64) / 8, torch.randn(64, generator=g, dtype=torch.float64)
    ma, mb = msg.clone().requires_grad_(True), msg.clone().requires_grad_(True)
    ref = eq.attentional_aggregation(mb, dst, n_dst, wg, bgt)
    x1, alpha = br.softmax_aggregate(F.relu(F.linear(ma, wg, bgt)), ma, dst, n_dst)
    close("softmax aggregation", x1, ref)
    assert bool((x1[-2:] == 0).all())
    # the closed-form backward against autograd of the oracle: d msg (direct part) and d gate
    gate = F.relu(F.linear(msg, wg, bgt)).requires_grad_(True)
    m2 = msg.clone().requires_grad_(True)
    x1g, alpha = br.softmax_aggregate(gate, m2, dst, n_dst)
    dx1 = torch.randn(x1g.shape, generator=g, dtype=torch.float64)
    (x1g * dx1).sum().backward()
    dmsg, dgate, mag = br.softmax_aggregate_bwd(alpha.detach(), msg, x1g.detach(), dx1, dst)
    close("d msg", dmsg, m2.grad)
    close("d gate", dgate, gate.grad)
    assert bool((mag >= dgate.abs()).all())


def test_gelu_approximant():
    """The approximant's normal CDF sigma(1.5976 x + 0.07056 x^3) is within 1.4e-4 of Phi (1.415e-4 at |x| ~ 2.5); the GELU value, x times
    that CDF, within 3.9e-4 of the erf GELU (3.83e-4 at |x| ~ 2.8)."""
    x = torch.linspace(-12, 12, 2000001, dtype=torch.float64, requires_grad=True)
    y = br.gelu_logistic(x)
    xd = x.detach()
    cdf_err = float((torch.sigmoid(xd * (1.5976 + 0.07056 * xd * xd)) - 0.5 * (1 + torch.erf(xd / 2 ** 0.5))).abs().max())
    err = float((y.detach() - F.gelu(xd)).abs().max())
    assert cdf_err <= 1.42e-4 and err <= 3.9e-4, (cdf_err, err)
    (dy,) = torch.autograd.grad(y.sum(), x)
    # the kernels' derivative (gelu_logistic_both): s + s (1 - s) x (1.5976 + 3 0.07056 x^2), s = sigma(1.5976 x + 0.07056 x^3)
    s = torch.sigmoid(xd * (1.5976 + 0.07056 * xd * xd))
    close("gelu'", dy, s + s * (1 - s) * xd * (1.5976 + 3 * 0.07056 * xd * xd))


def test_rounding_points():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(5, 16, 64, generator=g, dtype=torch.float64)
    w = torch.randn(32, 64, generator=g, dtype=torch.float64)
    b = torch.randn(32, generator=g, dtype=torch.float64)
    xr, wr = br.bf16(x), br.bf16(w)
    assert torch.equal(br.bf16(xr), xr) and not torch.equal(xr, x)
    assert float(((xr - x).abs() - 0.5 * br.ulp16(x)).max()) <= 0
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = br.mm(xa, wa, ba)
    close("mm forward", y, xr @ wr.t() + b)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    close("mm dx", xa.grad, br.bf16(dy) @ wr)
    close("mm dW", wa.grad, br.bf16(dy).reshape(-1, 32).t() @ xr.reshape(-1, 64))
    close("mm db", ba.grad, dy.reshape(-1, 32).sum(0))
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    br.mm(xa, wa, ba, round_db=True).backward(dy)
    close("mm db (MFMA column)", ba.grad, br.bf16(dy).reshape(-1, 32).sum(0))
    s = x.clone().requires_grad_(True)
    out = br.store(s)
    assert torch.equal(out, xr)
    dout = torch.randn(x.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    assert torch.equal(s.grad, br.bf16(dout))


def test_fiber_conv_and_lift_without_rounding_are_the_oracle():
    g = torch.Generator().manual_seed(12)
    n = 9
    x1, fk, bias = (torch.randn(*s, generator=g, dtype=torch.float64) for s in [(n, 16, 64), (16, 16, 64), (64,)])
    la = [t.clone().requires_grad_(True) for t in (x1, fk, bias)]
    lb = [t.clone().requires_grad_(True) for t in (x1, fk, bias)]
    out, ref = br.fiber_conv(*la, rounding=False), ops_ref.fiber_conv(*lb)
    close("fiber conv", out, ref)
    R = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * R).sum().backward()
    (ref * R).sum().backward()
    for a, b in zip(la, lb):
        close("fiber conv grad", a.grad, b.grad)
    for dim, S, V in ((3, 3, 4), (2, 3, 4), (3, 8, 0), (2, 1, 7)):
        grid = eq.make_grid(dim, 16).double()
        scal, vec, w = (torch.randn(*s, generator=g, dtype=torch.float64) for s in [(n, S), (n, V, 3), (64, S + V)])
        wa, wb = w.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out, ref = br.lift_encode(scal, vec, grid, wa, rounding=False), ops_ref.lift_encode(scal, vec, grid, wb)
        close("lift", out, ref)
        (out * R).sum().backward()
        (ref * R).sum().backward()
        close("lift grad", wa.grad, wb.grad)


def test_fiber_conv_and_lift_round_only_their_store():
    g = torch.Generator().manual_seed(13)
    x1, fk, bias = br.bf16(torch.randn(5, 16, 64, generator=g, dtype=torch.float64)), torch.randn(16, 16, 64, generator=g, dtype=torch.float64), \
        torch.randn(64, generator=g, dtype=torch.float64)
    xa = x1.clone().requires_grad_(True)
    out = br.fiber_conv(xa, fk, bias)
    exact = ops_ref.fiber_conv(x1, fk, bias)
    assert torch.equal(out, br.bf16(exact)) and torch.equal(br.fiber_conv(x1, fk, bias, stored=False), exact)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    close("fiber conv dx1 (the gradient as read from bf16 memory)", xa.grad, torch.einsum("bpc,opc->boc", br.bf16(dout), fk) / 16)


def test_last_bit_sensitivity_of_the_emulation_stays_under_half_of_each_gpu_bar():
    """Every case tests/test_gpu_bf16_ops.py compares with the emulation, evaluated once in fp32 and once in float64 on the same
    bf16-rounded inputs: the worst difference per family and tensor kind as a fraction of the tensor's own scale -- the reference's own
    sensitivity to last-bit differences (rounding flips at bf16 boundaries) -- must stay under HALF of the bar the GPU test holds that
    tensor to, which leaves the kernel the other half."""
    from test_gpu_bf16_ops import BARS, reference_cases, tensor_kind
    kinds = ("values", "stored gradients", "weight gradients")
    worst = {}
    for fam, c in reference_cases():
        o64, g64 = c.evaluate(torch.float64)
        o32, g32 = c.evaluate(torch.float32)
        line = []
        for is_out, d32, d64 in ((True, o32, o64), (False, g32, g64)):
            for k in d64:
                if is_out and k == "res":   # (the scalar that carries the residual gradient into d x_src: not a tensor of the op)
                    continue
                e, kind = ops_ref.rel_err(d32[k], d64[k]), tensor_kind(k, is_out)
                line.append(f"{'' if is_out else 'd '}{k} {e:.2e}")
                w = worst.setdefault(fam, [(0.0, "")] * 3)
                if e >= w[kind][0]:
                    w[kind] = (e, f"{c.name}: {'' if is_out else 'd '}{k}")
        print(f"  {c.name}: " + ", ".join(line))
        del o64, g64, o32, g32
    print()
    bad = []
    for fam, w in worst.items():
        for kind in range(3):
            e, where = w[kind]
            print(f"{fam:10s} {kinds[kind]:17s} worst fp32 vs float64 {e:.2e}  half bar {0.5 * BARS[fam][kind]:.1e}   ({where})")
            if not e <= 0.5 * BARS[fam][kind]:
                bad.append((fam, kinds[kind], e, where))
    assert not bad, bad
