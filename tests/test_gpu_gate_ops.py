"""Per-op parity of ``ops.GatedSoftmaxAggregate`` (the attention gate network inside the softmax-aggregation launches, csrc/grl_gate.h;
grl_softmax_aggregate_fwd / _bwd with Wg) against float64: bf16_ref.softmax_aggregate / softmax_aggregate_bwd around F.linear + ReLU,
autograd for d Wg, d bg and the gate network's part of d msg.

The ReLU kink must not decide a comparison, so the inputs come from constructions whose pre-activations stay away from it (asserted on
the float64 reference, so that the HIP side's mask IS the reference's and no element is left out):

* ``dyadic``: msg = k/8, Wg = k/8, bg = odd/128 -- all bf16-exact, pre exact in fp32 (asserted: fp32 equals float64 element for element),
  |pre| >= 1/128 everywhere, about half the pre-activations active.  Only the softmax arithmetic differs from exact: x1 within 1e-5.
* ``far``: msg ~ N(0,1), Wg ~ N(0,1)/8, bg[c] = +-6 std(msg Wg[c]^T) (per channel) alternating by channel: half the channels always active (real-valued
  gates, the lo halves of the split products), half always zero (uniform alphas, exact ties in the maximum).
* ``large``: ``far`` with Wg and bg times 18: active pre-activations of 54 .. 162 in the bulk, up to about 200 -- exp overflows without
  the shift by the segment maximum.

Graphs: those of test_gpu_attention_ops.softmax_case -- destinations without in-edges (runs of them, nearly all of 2000), single in-edges,
degrees 2 .. 300 (a hub above 256), 5000 destinations (more than the 256 workgroups x 4 waves: the grid-stride loop).

Bars: the composition test's of the torch gate (test_gpu_attention_ops.test_messages_gate_softmax_composition): 1e-4 of its own scale for
x1, 2e-4 for every gradient; every margin is printed."""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as br
from oracle import equivariant as eq
from test_gpu_attention_ops import dev, margin, msg_reference, softmax_case, weights

pytestmark = pytest.mark.gpu

KINDS = ["empty_runs", "mostly_empty", "single", "degrees", "grid_stride"]
CONSTRUCTIONS = ["dyadic", "far", "large"]


def far_gate(msg, g, scale=1.0, heavy_tails=False):
    """Wg ~ N(0,1)/8, bg[c] = +-6 std(msg Wg[c]^T) (the channel's own standard deviation) alternating by channel, both times ``scale``.
    ``heavy_tails``: bg[c] = +-1.25 max|msg Wg[c]^T| instead -- real messages are products K_e x_src whose rows differ in scale, so
    msg Wg^T reaches far beyond six of its standard deviations (measured on the composition cases: min|pre| 1.4e-4 of max|pre| 18 with
    6 std); 1.25 max keeps min|pre| >= 0.25 max|z| and max|pre| <= 2.25 max|z|, the same "half always active, half always zero"."""
    wg = torch.randn(64, 64, generator=g) / 8
    z = F.linear(msg.double(), wg.double()).reshape(-1, 64)
    s = (1.25 / 6.0 * z.abs().amax(0) if heavy_tails else z.std(0)) if msg.numel() else torch.ones(64, dtype=torch.float64)
    bg = 6.0 * s * torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    return (wg * scale).float(), (bg * scale).float()


def gate_inputs(construction, E, g):
    """(msg [E,16,64], Wg [64,64], bg [64]) fp32."""
    if construction == "dyadic":
        msg = torch.randint(-8, 9, (E, 16, 64), generator=g).float() / 8
        wg = torch.randint(-4, 5, (64, 64), generator=g).float() / 8
        bg = (2 * torch.randint(-8, 8, (64,), generator=g) + 1).float() / 128
        return msg, wg, bg
    msg = torch.randn(E, 16, 64, generator=g)
    wg, bg = far_gate(msg, g, 18.0 if construction == "large" else 1.0)
    return msg, wg, bg


def gate_reference(msg, wg, bg, dx1, dst, n_dst):
    """float64: (x1, d msg complete, d Wg, d bg, pre, per channel the sum of |d pre| = the magnitude of d bg's terms)."""
    m = msg.double().requires_grad_(True)
    w, b = wg.double().requires_grad_(True), bg.double().requires_grad_(True)
    pre = F.linear(m, w, b)
    gate = F.relu(pre)
    x1, alpha = br.softmax_aggregate(gate.detach(), msg.double(), dst, n_dst)
    dmsg_direct, dgate, _ = br.softmax_aggregate_bwd(alpha, msg.double(), x1, dx1.double(), dst)
    if msg.numel():
        gate.backward(dgate)
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return x1, dmsg_direct + z(m), z(w), z(b), pre.detach(), (dgate * (pre.detach() > 0)).abs().sum((0, 1))


def check_away_from_kink(construction, msg, wg, bg, pre):
    if not pre.numel():
        return
    lo, hi = float(pre.abs().min()), float(pre.abs().max())
    print(f"  pre-activations: min|pre| {lo:.3e}, max|pre| {hi:.3e}, active {float((pre > 0).double().mean()):.2f}")
    if construction == "dyadic":
        assert lo > 0 and lo >= 1 / 128
        assert torch.equal(F.linear(msg, wg, bg).double(), pre), "dyadic: the pre-activations are exact in fp32"
    else:
        assert lo >= 1e-2 * hi, (lo, hi)
        if construction == "large":
            assert hi > 100, hi   # (exp overflows fp32 beyond 88.7 without the shift)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("construction", CONSTRUCTIONS)
def test_gated_softmax_aggregate(construction, kind):
    from geometry_rl_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(KINDS.index(kind) + 41)
    ei, n_dst, _ = softmax_case(kind, g)
    E = ei.shape[1]
    es = ops.build_edge_set(ei.to(d), 97, n_dst)
    msg, wg, bg = gate_inputs(construction, E, g)
    dx1 = torch.randn(n_dst, 16, 64, generator=g)
    dst = es.dst_d.long().cpu()
    x1_r, dmsg_r, dwg_r, dbg_r, pre_r, mag_b = gate_reference(msg, wg, bg, dx1, dst, n_dst)
    deg = (es.rowptr_d[1:] - es.rowptr_d[:-1]).cpu()
    print(f"gated softmax {construction} {kind}: E={E}, n_dst={n_dst}, max degree {int(deg.max())}, "
          f"workgroups {ops.GatedSoftmaxAggregate.blocks(n_dst)}")
    check_away_from_kink(construction, msg, wg, bg, pre_r)

    md, wd, bd = (t.to(d).requires_grad_(True) for t in (msg, wg, bg))
    x1 = ops.GatedSoftmaxAggregate.apply(md, wd, bd, es, "")
    assert x1.dtype == torch.float32 and x1.shape == (n_dst, 16, 64)
    x1.backward(dx1.to(d))
    x1c, dmc, dwc, dbc = x1.detach().cpu(), md.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()

    assert bool((x1c[deg == 0] == 0).all()), "destinations without in-edges must be exactly 0"
    one = torch.repeat_interleave(deg == 1, deg)                 # edges that are their destination's only in-edge
    if bool(one.any()):
        assert torch.equal(x1c[deg == 1], msg[one]), "a single in-edge: x1 must equal its message bitwise"
        assert torch.equal(dmc[one], dx1[deg == 1]), "a single in-edge: d msg must equal d x1 bitwise"
    if int(deg.max()) <= 1:
        assert bool((dwc == 0).all()) and bool((dbc == 0).all()), "single in-edges only: d Wg and d bg are exactly 0"
    margin("x1", x1c, x1_r, 1e-5 if construction == "dyadic" else 1e-4)
    margin("dmsg", dmc, dmsg_r, 2e-4)
    margin("d gate W", dwc, dwg_r, 2e-4)
    check_dbg(construction, dbc, dbg_r, mag_b)


def check_dbg(construction, got, ref, mag_b):
    """d bg within 2e-4 of its own scale -- where it has one.  In ``far`` / ``large`` a channel is active on every edge or on none, so
    d bg[c] = sum_e d gate_e[c], which the softmax makes exactly zero: the float64 reference itself is rounding noise (1e-14) there,
    and the tensor is held against the magnitude of its cancelling terms instead, max_c sum_{e,o} |d pre_e[o,c]| (as the d gate checks of
    test_gpu_attention_ops.run_softmax do)."""
    if construction == "dyadic":
        margin("d gate b", got, ref, 2e-4)
    else:
        margin("d gate b vs max_c sum|d pre|", got, ref, 2e-4, scale=float(mag_b.max()))


def test_entry_points_refuse_what_the_fused_form_does_not_build():
    """The _bf16 twins return -2 with Wg; the fp32 entries return -2 when gate / dgate come along with Wg."""
    from geometry_rl_amd import hip
    d = dev()
    n, E = 4, 4
    rowptr = torch.arange(n + 1, dtype=torch.int32, device=d)
    f32 = lambda *s: torch.zeros(*s, device=d)
    b16 = lambda *s: torch.zeros(*s, device=d, dtype=torch.bfloat16)
    wg, bg, stat, partial = f32(64, 64), f32(64), f32(n, 16, 64, 2), f32(1, 64 * 64 + 64)
    s = hip.stream_ptr()
    assert hip.query("grl_softmax_aggregate_fwd_bf16", None, b16(E, 16, 64), rowptr, n, b16(n, 16, 64), wg, bg, stat, 1, s) == -2
    assert hip.query("grl_softmax_aggregate_bwd_bf16", None, b16(E, 16, 64), b16(n, 16, 64), b16(n, 16, 64), rowptr, n, None, b16(E, 16, 64),
                     wg, bg, stat, partial, 1, s) == -2
    gate = f32(E, 16, 64)
    assert hip.query("grl_softmax_aggregate_fwd", gate, f32(E, 16, 64), rowptr, n, f32(n, 16, 64), wg, bg, stat, 1, s) == -2
    assert hip.query("grl_softmax_aggregate_bwd", None, f32(E, 16, 64), f32(n, 16, 64), f32(n, 16, 64), rowptr, n, gate, f32(E, 16, 64),
                     wg, bg, stat, partial, 1, s) == -2
    assert hip.query("grl_softmax_aggregate_fwd", None, f32(E, 16, 64), rowptr, n, f32(n, 16, 64), wg, bg, stat, 0, s) == -2
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,E", [(200, 700), (1500, 4500)])   # second: more than 256 workgroups x 4 waves of destinations
def test_messages_gated_softmax_composition(n, E):
    """EdgeMessages -> GatedSoftmaxAggregate as hepi._conv wires it with gate_kernels="hip", with the ``far`` gate built on the oracle's
    messages, against the float64 oracle."""
    from geometry_rl_amd import hepi, ops
    d = dev()
    g = torch.Generator().manual_seed(n)
    dst = torch.randint(0, n, (E,), generator=g)
    dst[:n] = torch.arange(n)
    ei = torch.stack([torch.randint(0, n, (E,), generator=g), dst])
    grid = eq.make_grid(3, 16, True)
    grid3 = F.pad(grid, (0, 3 - grid.shape[1]))
    pos = torch.rand(n, 3, generator=g) * 2 - 1
    x_src = torch.randn(n, 16, 64, generator=g)
    W = weights(g)
    R = torch.randn(n, 16, 64, generator=g)
    es = ops.build_edge_set(ei.to(d), n, n)
    src, dsts = es.src_d.long().cpu(), es.dst_d.long().cpu()
    msg_r, leaves = msg_reference(x_src, W, grid, pos, pos, src, dsts, 3, "", torch.device("cpu"))

    conv = hepi.FiberBundleConv(64, 64, 64, groups=64, aggr="AttentionalAggregation").to(d)
    conv.gate_kernels = "hip"
    lin = conv.aggr_module.gate_nn[0]
    wg0, bg0 = far_gate(msg_r.detach(), g, heavy_tails=True)
    with torch.no_grad():
        lin.weight.copy_(wg0)
        lin.bias.copy_(bg0)
    wg, bg = wg0.double().requires_grad_(True), bg0.double().requires_grad_(True)
    pre_r = F.linear(msg_r, wg, bg)
    pre_r.retain_grad()
    print(f"gated composition n={n} E={E}")
    check_away_from_kink("far", None, None, None, pre_r.detach())
    x1_r, _ = br.softmax_aggregate(F.relu(pre_r), msg_r, dsts, n)
    (x1_r * R.double()).sum().backward()

    dl = [x_src.to(d).requires_grad_(True)] + [w.to(d).requires_grad_(True) for w in W]
    msg = ops.EdgeMessages.apply(dl[0], pos.to(d), pos.to(d), grid3.to(d), *dl[1:], es, 3, None, "")
    x1 = ops.GatedSoftmaxAggregate.apply(msg, lin.weight, lin.bias, es, "")
    (x1 * R.to(d)).sum().backward()

    margin("x1", x1.cpu(), x1_r.detach(), 1e-4)
    for name, a, b in zip(["dx_src", "dW1", "db1", "dW2", "db2", "dWk"], dl, leaves):
        margin(name, a.grad.cpu(), b.grad, 2e-4)
    margin("d gate W", lin.weight.grad.cpu(), wg.grad, 2e-4)
    check_dbg("far", lin.bias.grad.cpu(), bg.grad, pre_r.grad.abs().sum((0, 1)))
