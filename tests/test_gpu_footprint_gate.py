"""``ops.GatedSoftmaxAggregate`` (csrc/grl_gate.h behind grl_softmax_aggregate_fwd / _bwd) on poisoned, guarded buffers
(tests/footprint.py), chained behind EdgeMessages as hepi._conv chains them with gate_kernels="hip".

x1, stat, dmsg and partial come from ``torch.empty``: under the guards every one of them must be written in full by the launches -- stat is
looked at directly (the forward's saved tensor), partial through the fold that sums all of its rows into d Wg / d bg (a row no workgroup
wrote leaves the poison there).  Plain, NaN-poisoned and huge-poisoned runs must agree bit for bit."""
import pytest
import torch

import footprint as fp
from test_gpu_footprint import dev, grads_of, leaf, three_runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["star_in", "star_out", "one_edge", "self_loops", "chunks", "empty"])
def test_edge_messages_and_gated_softmax_aggregate(kind):
    """star_in, star_out and one_edge have destinations without in-edges (x1 rows of zeros, stat rows of (0, 0)); chunks has 5000
    destinations (the grid-stride loop of the 256 workgroups); empty launches with no edge at all (partial rows of zeros)."""
    import torch.nn.functional as F
    import test_gpu_attention_ops as att
    from geometry_rl_amd import ops
    from oracle import equivariant as eq
    d = dev()
    g = torch.Generator().manual_seed(att.MSG_CASES.index(kind) + 5)
    ei, n_src, n_dst, dim, upper, pos_s, pos_d = att.msg_case(kind, g)
    grid = eq.make_grid(dim, 16, upper)
    g3 = F.pad(grid, (0, 3 - grid.shape[1])).contiguous().to(d)
    x_src = torch.randn(n_src, 16, 64, generator=g).to(d)
    W = [t.to(d) for t in att.weights(g)]
    wg = (torch.randn(64, 64, generator=g) / 8).to(d)
    bg = (torch.randn(64, generator=g) * 0.3).to(d)
    up = torch.randn(n_dst, 16, 64, generator=g).to(d)
    R = torch.randn(n_src, 16, 64, generator=g).to(d)
    ei_d, ps, pd = ei.to(d), pos_s.to(d), pos_d.to(d)
    if kind in ("star_in", "star_out", "one_edge"):
        assert int((torch.bincount(ei[1], minlength=n_dst) == 0).sum()) > 0

    def run(w, with_dres):
        es = fp.guard_edge_set(ops.build_edge_set(ei_d, n_src, n_dst), w)
        L = {"x_src": leaf(w, x_src), "wg": leaf(w, wg), "bg": leaf(w, bg)}
        L.update({k: leaf(w, t) for k, t in zip(("w1", "b1", "w2", "b2", "wk"), W)})
        res = {"dres": w(R)} if with_dres else None
        msg = ops.EdgeMessages.apply(L["x_src"], w(ps), w(pd), w(g3), L["w1"], L["b1"], L["w2"], L["b2"], L["wk"], es, dim, res, "")
        msg.retain_grad()
        x1 = ops.GatedSoftmaxAggregate.apply(msg, L["wg"], L["bg"], es, "")
        stat = x1.grad_fn.saved_tensors[2]
        assert stat.shape == (n_dst, 16, 64, 2)
        x1.backward(w(up))
        assert res is None or "dres" not in res
        return {"msg": msg.detach(), "x1": x1.detach(), "stat": stat, "dmsg": msg.grad, "grads": grads_of(L)}

    for with_dres in (False, True):
        three_runs("EdgeMessages+GatedSoftmaxAggregate", f"{kind} dres={with_dres}", lambda w: run(w, with_dres))
