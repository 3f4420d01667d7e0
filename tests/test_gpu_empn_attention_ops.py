"""Per-op parity of the EMPN key / query attention kernels (csrc/attention_ops.hip) through ``ops.KeyQueryProject`` and
``ops.EdgeAttention`` against the float64 restatement tests/empn_attention_ref.py (pinned to the reference's PonitaGCN(attention=True)
fixtures by tests/test_empn_attention_ref_cpu.py -- the pin tests/data_fixtures.py still lists as missing).  Every output and gradient is
compared on its own scale (``ops_ref.margin``); the bars are ``empn_attention_ref.BARS``: 8 x the worst fp32-vs-float64 error of the torch
CPU evaluation of the same cases (kq_project 4e-6 values / 5e-6 gradients, edge_attention 7e-6 / 2e-5), nothing measured on the kernels.
Measured worst on the MI355X: kq_project 3.5e-7 / 5.2e-7, edge_attention 5.2e-7 / 2.2e-6.

Cases: homogeneous graphs with 16 orientations and 24 .. 96 nodes -- in-degrees 0 .. 5 with destinations without in-edges and sources
without out-edges (exact zeros asserted), a hub destination with 70 in-edges, 26 nodes (the last 64-row block of the projection's
backward half full), self-loops, the empty edge set -- each at logit spans of about +-1, +-3, +-10 and +-20 (k scaled; from +-10 on
destinations have S near or below the 1e-6, where a per-destination maximum, a 1e-16 or a detached M miss the bars by orders of
magnitude).  The same calls with the parameters at an odd float offset and a second run must be bitwise equal to the first."""
import pytest
import torch

import empn_attention_ref as ar
from ops_ref import margin
from test_gpu_actor_ops import bits_equal, dev, dleaf

pytestmark = pytest.mark.gpu

MEASURED = {}


def _record(op, kind, m):
    w = MEASURED.setdefault(op, [0.0, 0.0])
    w[kind] = max(w[kind], m)


def _project(c, off=0):
    from geometry_rl_amd import ops
    x = dleaf(c.x)
    ws = [dleaf(w, off) for w in c.w]
    k, q = ops.KeyQueryProject.apply(x, *ws)
    ((k * c.Rk.to(dev())).sum() + (q * c.Rq.to(dev())).sum()).backward()
    torch.cuda.synchronize()
    return {"k": k.detach(), "q": q.detach()}, dict(zip(("x", "wk", "bk", "wq", "bq"), [x.grad] + [w.grad for w in ws]))


@pytest.mark.parametrize("case", ar.project_cases(), ids=lambda c: c.name)
def test_key_query_project(case):
    outs, grads = _project(case)
    o64, g64 = case.evaluate(torch.float64)
    bv, bg = ar.BARS["kq_project"]
    print(case.name)
    for k, v in outs.items():
        _record("kq_project", 0, margin(k, v, o64[k], bv))
    for k, v in grads.items():
        _record("kq_project", 1, margin("d " + k, v, g64[k], bg))
    print(f"  [kq_project: worst so far values {MEASURED['kq_project'][0]:.2e}, gradients {MEASURED['kq_project'][1]:.2e}]")
    again = _project(case)
    assert bits_equal(outs.values(), again[0].values()) and bits_equal(grads.values(), again[1].values()), "a second run differs"
    for off in (1, 3):
        odd = _project(case, off)
        assert bits_equal(outs.values(), odd[0].values()) and bits_equal(grads.values(), odd[1].values()), f"offset {off} differs"


def _attend(c, es):
    from geometry_rl_amd import ops
    k, q, msg = dleaf(c.k), dleaf(c.q), dleaf(c.msg)
    x1 = ops.EdgeAttention.apply(k, q, msg, es)
    (x1 * c.R.to(dev())).sum().backward()
    torch.cuda.synchronize()
    return {"x1": x1.detach()}, {"k": k.grad, "q": q.grad, "msg": msg.grad}


@pytest.mark.parametrize("case", ar.attention_cases(), ids=lambda c: c.name)
def test_edge_attention(case):
    from geometry_rl_amd import ops
    es = ops.build_edge_set(case.ei.to(dev()), case.n, case.n)
    case.with_edges(torch.stack([es.src_d.long(), es.dst_d.long()]).cpu())   # msg rows in the edge set's own destination-sorted order
    outs, grads = _attend(case, es)
    o64, g64 = case.evaluate(torch.float64)
    bv, bg = ar.BARS["edge_attention"]
    print(case.name)
    _record("edge_attention", 0, margin("x1", outs["x1"], o64["x1"], bv))
    for k, v in grads.items():
        _record("edge_attention", 1, margin("d " + k, v, g64[k], bg))
    print(f"  [edge_attention: worst so far values {MEASURED['edge_attention'][0]:.2e}, gradients {MEASURED['edge_attention'][1]:.2e}]")
    # exact zeros: a destination without in-edges (x1, d q), a source without out-edges (d k)
    no_in = torch.bincount(case.ei[1], minlength=case.n) == 0
    no_out = torch.bincount(case.ei[0], minlength=case.n) == 0
    if case.graph in ("degrees", "empty"):
        assert bool(no_in.any()) and bool(no_out.any())
    assert not bool(outs["x1"][no_in.to(dev())].abs().sum() > 0) and not bool(grads["q"][no_in.to(dev())].abs().sum() > 0)
    assert not bool(grads["k"][no_out.to(dev())].abs().sum() > 0)
    if case.graph == "empty":
        assert grads["msg"].numel() == 0 and not bool(grads["k"].abs().sum() > 0) and not bool(grads["q"].abs().sum() > 0)
    again = _attend(case, es)
    assert bits_equal(outs.values(), again[0].values()) and bits_equal(grads.values(), again[1].values()), "a second run differs"

