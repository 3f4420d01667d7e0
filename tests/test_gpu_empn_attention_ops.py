"""Per-op parity of the EMPN key / query attention kernels (csrc/attention_ops.hip) through ``ops.KeyQueryProject`` and
``ops.EdgeAttention`` against the float64 restatement tests/empn_attention_ref.py (pinned to the reference's PonitaGCN(attention=True)
fixtures by tests/test_empn_attention_ref_cpu.py -- the pin tests/data_fixtures.py still lists as missing).  Every output and gradient is
compared on its own scale (``ops_ref.margin``); the bars are ``empn_attention_ref.BARS``: 8 x the worst fp32-vs-float64 error of the torch
CPU evaluation of the same cases (kq_project 4e-6 values / 5e-6 gradients, edge_attention 7e-6 / 2e-5, edge_attention_large 6e-6 / 6e-5),
nothing measured on the kernels.  Measured worst on the MI355X, values / gradients as fractions of the tensor's own scale:

    kq_project            3.8e-7 (q, 2049 nodes)            / 7.9e-7 (d x, 4101 rows by direct call; through the op 7.0e-7)
    edge_attention        8.9e-7 (comp, half_block +-10)    / 2.2e-6 (d k, hub +-20)           x1 alone: 5.2e-7
    edge_attention_large  7.0e-7 (comp, wide_sources +-10)  / 1.3e-6 (d k, many_rows +-20 tie) x1 alone: 3.4e-7

(the value columns include logit, a and comp of the direct calls; logit is within 1.3e-7 everywhere).

Cases: homogeneous graphs with 16 orientations and 24 .. 96 nodes -- in-degrees 0 .. 5 with destinations without in-edges and sources
without out-edges (exact zeros asserted), a hub destination with 70 in-edges, 26 nodes (the last 64-row block of the projection's
backward half full), self-loops, the empty edge set -- each at logit spans of about +-1, +-3, +-10 and +-20 (k scaled; from +-10 on
destinations have S near or below the 1e-6, where a per-destination maximum, a 1e-16 or a detached M miss the bars by orders of
magnitude).  The same calls with the parameters at an odd float offset and a second run must be bitwise equal to the first.

At those sizes every wave of every row kernel visits one row.  The large cases (tests/empn_attention_ref.py; what each reaches is
asserted from the restated launch shapes by tests/test_empn_attention_ref_cpu.py) are the first to run:
  * 257 nodes (4112 rows): the second, partial iteration of kq_project_fwd and kq_project_bwd_dx (1024-workgroup cap);
  * 2049 nodes (32784 rows): kq_project_bwd_dw with a chunk of 65 rows, the 24-row workgroup 504 and the empty workgroups 505 .. 511,
    whose zero partial rows the fold sums;
  * many_rows (600 nodes, 1200 edges = 19200 logit rows, 9600 destination rows) at +-1 and +-10: the per-wave running (best, besti) of
    edge_logits_fwd over two and three rows, the loops of edge_attend_fwd / _bwd and the per-wave d M over two rows, the loop of
    edge_logits_bwd;
  * wide_sources (700 -> 40) and wide_destinations (30 -> 600): n_src != n_dst; in edge_logits_bwd a wave that takes a d q row on one
    iteration and a d k row on the next, and d k rows that start mid-grid;
  * exact three-way ties of the global maximum on many_rows at +-10 and +-20, three placements (``empn_attention_ref.TIES``): the
    lowest flat index e * 16 + o takes d M, and each stage of the maximum -- the wave's strict ">", the merge of a workgroup's waves, the
    finish over the workgroups -- decides the argmax on one of them; on ``late`` and ``one_workgroup`` no occurrence lies in the first
    grid pass.  The reference takes M at the lowest tied index (torch's ``l.max()`` would split d M evenly: d k and d q off by 0.67 of
    their scale; the highest index: 1.0).  The placements are asserted on the DEVICE's destination-sorted order;
  * by direct call: M, the argmax and every workgroup's partial (maximum, first index) as exact statements about the kernel's own
    logits; logit, a and comp against float64; grl_kq_project_fwd / _bwd at 1, 3, 5 and 4101 rows (the clamp of the forward's batch of
    four) on poisoned, guarded buffers; the calls that launch nothing."""
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
    bv, bg = ar.BARS[case.bar]
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


def _edge_set(case):
    """The device's edge set of the case, and the case's msg rows (and declared ties) in that edge set's own destination-sorted order.
    The DEVICE's order decides the flat index e * 16 + o, so the placements a tie case is built for are asserted on it."""
    from geometry_rl_amd import ops
    es = ops.build_edge_set(case.ei.to(dev()), case.n_src, case.n_dst)
    assert (es.n_src, es.n_dst, es.n_edges) == (case.n_src, case.n_dst, case.ei.shape[1])
    case.with_edges(torch.stack([es.src_d.long(), es.dst_d.long()]).cpu())
    if case.tie:
        src_d, dst_d = es.src_d.tolist(), es.dst_d.tolist()
        for ((s, d), o), (e, o_) in zip(case.tie_edges, ar.TIES[case.tie]):
            assert (src_d[e], dst_d[e], o) == (s, d, o_), (case.name, e)
        assert case.ties == sorted(e * 16 + o for e, o in ar.TIES[case.tie])
    return es


@pytest.mark.parametrize("case", ar.attention_cases(), ids=lambda c: c.name)
def test_edge_attention(case):
    es = _edge_set(case)
    outs, grads = _attend(case, es)
    o64, g64 = case.evaluate(torch.float64)
    bv, bg = ar.BARS[case.bar]
    print(case.name)
    _record(case.bar, 0, margin("x1", outs["x1"], o64["x1"], bv))
    for k, v in grads.items():
        _record(case.bar, 1, margin("d " + k, v, g64[k], bg))
    print(f"  [{case.bar}: worst so far values {MEASURED[case.bar][0]:.2e}, gradients {MEASURED[case.bar][1]:.2e}]")
    # exact zeros: a destination without in-edges (x1, d q), a source without out-edges (d k)
    no_in = torch.bincount(case.ei[1], minlength=case.n_dst) == 0
    no_out = torch.bincount(case.ei[0], minlength=case.n_src) == 0
    if case.graph in ("degrees", "empty", "many_rows"):
        assert bool(no_in.any()) and bool(no_out.any())
    if case.graph == "wide_sources":
        assert bool(no_out.any())
    if case.graph == "wide_destinations":
        assert bool(no_in.any())
    assert not bool(outs["x1"][no_in.to(dev())].abs().sum() > 0) and not bool(grads["q"][no_in.to(dev())].abs().sum() > 0)
    assert not bool(grads["k"][no_out.to(dev())].abs().sum() > 0)
    if case.graph == "empty":
        assert grads["msg"].numel() == 0 and not bool(grads["k"].abs().sum() > 0) and not bool(grads["q"].abs().sum() > 0)
    again = _attend(case, es)
    assert bits_equal(outs.values(), again[0].values()) and bits_equal(grads.values(), again[1].values()), "a second run differs"


# ------------------------------------------------------------------------------------------------ the entry points by direct call
def _bits(t):
    return t.contiguous().view(torch.int32)


def _block_partials(flat, nb):
    """(maximum, first flat index that holds it) of the rows each of the ``nb`` workgroups visits: row r belongs to workgroup
    (r // 4) % nb."""
    rows = torch.arange(flat.numel())
    block = (rows // 4) % nb
    pmax = torch.full((nb,), -float("inf")).scatter_reduce(0, block, flat, "amax")
    at_max = flat == pmax[block]
    return pmax, torch.full((nb,), 2 ** 31 - 1, dtype=torch.int64).scatter_reduce(0, block[at_max], rows[at_max], "amin")


@pytest.mark.parametrize("case", [c for c in ar.attention_cases() if c.ei.shape[1]], ids=lambda c: c.name)
def test_logits_maximum_and_weights_by_direct_call(case):
    """What the forward leaves for the backward -- logit, M, its argmax, a, comp -- read directly: grl_edge_logits_fwd and
    grl_edge_attend_fwd on workspaces sized by grl_attention_blocks.  M and the argmax are exact statements about the kernel's OWN logits
    (no bar): M is their maximum bit for bit, the argmax the first flat index that holds it, and every workgroup's partial is the maximum
    and the first index of the rows that workgroup visits."""
    from geometry_rl_amd import hip
    d = dev()
    es = _edge_set(case)
    E, n_dst = es.n_edges, case.n_dst
    k, q, msg = case.k.to(d), case.q.to(d), case.msg.to(d)
    nb = hip.query("grl_attention_blocks", E * 16)
    assert nb == min((E * 16 + 3) // 4, 2048)
    nan = float("nan")
    logit, maxval = torch.full((E, 16), nan, device=d), torch.full((1,), nan, device=d)
    pmax, pidx = torch.full((nb,), nan, device=d), torch.full((nb,), -1, device=d, dtype=torch.int32)
    argmax = torch.full((1,), -1, device=d, dtype=torch.int32)
    hip.call("grl_edge_logits_fwd", k, q, es.src_d, es.dst_d, E, logit, pmax, pidx, maxval, argmax)
    a, comp = torch.full((E, 16), nan, device=d), torch.full((n_dst, 16), nan, device=d)
    x1 = torch.full((n_dst, 16, 64), nan, device=d)
    hip.call("grl_edge_attend_fwd", logit, maxval, msg, es.rowptr_d, n_dst, a, comp, x1)
    torch.cuda.synchronize()
    for name, t in (("logit", logit), ("pmax", pmax), ("maxval", maxval), ("a", a), ("comp", comp), ("x1", x1)):
        assert not bool(torch.isnan(t).any()), f"{name}: an element nobody wrote"
    flat = logit.flatten()
    assert torch.equal(_bits(maxval), _bits(flat.max().reshape(1))), "M is not the maximum of the kernel's own logits"
    first = int((flat == maxval).nonzero()[0])
    assert int(argmax) == first, (int(argmax), first)
    # per workgroup: rows 4 b + w (+ 4 nb per iteration) belong to workgroup b
    want_max, want_idx = _block_partials(flat.cpu(), nb)
    assert torch.equal(_bits(pmax.cpu()), _bits(want_max)), "a workgroup's partial maximum"
    assert torch.equal(pidx.cpu().long(), want_idx), "a workgroup's partial argmax is not the first index of its maximum"
    l64, a64, comp64 = case.parts()
    bv = ar.BARS[case.bar][0]
    print(case.name)
    _record(case.bar, 0, margin("logit", logit, l64, bv))
    _record(case.bar, 0, margin("a", a, a64, bv))
    _record(case.bar, 0, margin("comp", comp, comp64, bv))
    if case.tie:
        r0, r1, r2 = case.ties
        got = _bits(flat[[r0, r1, r2]]).tolist()
        assert got[0] == got[1] == got[2], "the kernel's logits are not bit-equal at the declared ties"
        assert int((flat == maxval).sum()) == 3 and first == r0 == int(argmax)


@pytest.mark.parametrize("case", ar.project_row_cases(), ids=lambda c: c.name)
def test_projection_by_direct_call(case):
    """grl_kq_project_fwd / _bwd at row counts that are no multiple of 4 (the op passes 16 per node; the C ABI takes any): the clamp of
    the forward's batch of four rows, and at 4101 rows the second iteration of both row kernels.  Plain, under the NaN poison and under
    the huge-finite poison (tests/footprint.py): every element of k, q, dx and the partial rows is written, nothing around them."""
    import footprint as fp
    from geometry_rl_amd import hip
    d, n = dev(), case.rows
    blocks, psize = hip.query("grl_kq_bwd_blocks", n), hip.query("grl_kq_partial_size")
    assert blocks == ar.kq_bwd_blocks(n) and psize == 2 * 128 * 64 + 2 * 128
    x, ws, Rk, Rq = case.x.to(d), [t.to(d) for t in case.w], case.Rk.to(d), case.Rq.to(d)

    def run(w):
        gx, (wk, bk, wq, bq) = w(x), [w(t) for t in ws]
        k, q = w.out((n, 128), torch.float32, d), w.out((n, 128), torch.float32, d)
        hip.call("grl_kq_project_fwd", gx, wk, bk, wq, bq, k, q, n)
        dx, partial = w.out((n, 64), torch.float32, d), w.out((blocks, psize), torch.float32, d)
        hip.call("grl_kq_project_bwd", gx, wk, wq, w(Rk), w(Rq), dx, partial, n)
        return {"k": k, "q": q, "dx": dx, "partial": partial}

    res = fp.three_runs("kq_project direct", f"{n} rows", run, direct=True)
    o64, g64 = case.evaluate(torch.float64)
    bv, bg = ar.BARS[case.bar]
    print(case.name)
    for name in ("k", "q"):
        _record("kq_project", 0, margin(name, res[name], o64[name], bv))
    fold = res["partial"].double().sum(0)   # (the fold's sum over the workgroups' rows, here in float64)
    got = {"x": res["dx"], "wk": fold[:8192].view(128, 64), "wq": fold[8192:16384].view(128, 64), "bk": fold[16384:16512], "bq": fold[16512:]}
    for name, v in got.items():
        _record("kq_project", 1, margin("d " + name, v, g64[name], bg))


def test_calls_that_launch_nothing():
    """Host-side refusals and the empty projection backward, on valid small buffers."""
    from geometry_rl_amd import hip
    d = dev()
    f = lambda *s: torch.zeros(*s, device=d)
    i = lambda *s: torch.zeros(*s, device=d, dtype=torch.int32)
    status = lambda name, *args: hip.query(name, *args, hip.stream_ptr())
    before = [f(1, 16), f(1), i(1), f(1), i(1)]
    assert status("grl_edge_logits_fwd", f(2, 16, 128), f(2, 16, 128), i(1), i(1), 0, *before) == -2
    assert status("grl_edge_attend_bwd", f(1, 16), f(1, 16, 64), f(1, 16), f(1, 16, 64), i(2), 0, i(1), f(1, 16, 64), f(1, 16), f(1)) == -2
    psize = hip.query("grl_kq_partial_size")
    assert hip.query("grl_kq_bwd_blocks", 0) == 1
    partial = torch.full((1, psize), float("nan"), device=d)
    dx = torch.full((1, 64), float("nan"), device=d)
    assert status("grl_kq_project_bwd", f(1, 64), f(128, 64), f(128, 64), f(1, 128), f(1, 128), dx, partial, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(partial), torch.zeros_like(_bits(partial))), "n_rows = 0 must leave one partial row of zeros"
    assert bool(torch.isnan(dx).all())   # (no row: dx is not touched)
    assert all(not bool(t.abs().sum() > 0) for t in before)
