"""tests/empn_attention_ref.py -- the float64 restatement of the EMPN key / query attention layer -- against the REFERENCE's own numbers,
without a GPU.  This is the pin of PonitaGCN(attention=True) that tests/data_fixtures.py and oracle/equivariant.py still list as
missing: tests/golden/tier2h_<case>_attention.npz / _attention_grad.npz hold what the reference's PonitaGCN(attention=True) computed on
the two EMPN cases of tier2h (tools/make_golden.py empn_attention).

1. The restatement reproduces both fixtures -- first-call outputs, calibrated weights, post-calibration outputs, every parameter
   gradient -- in float32 against the fp32 records and in float64 against ``out64`` / ``cal64``, at the bars
   tests/test_oracle_golden.py applies to the attention-free EMPN cases (2e-6 values; 1e-5 + 1e-4 |ref| gradients; 1e-10 in float64).
2. The per-op bar table: every case of ``empn_attention_ref`` evaluated in torch fp32 on the CPU against float64; the worst error per op
   is printed and ``BARS`` must be 8 x that, rounded up to one digit (within the factor 1.5 the CPU's summation order may move it,
   as tests/test_ops_ref_cpu.py allows).  Measured here (fraction of the tensor's own scale):

       op              cases  worst fp32 value  worst fp32 gradient  bars (8 x, one digit)
       kq_project          3         3.81e-07             5.83e-07   4e-6 / 5e-6     (96 nodes: q; 24 nodes: d wk)
       edge_attention     17         7.88e-07             2.39e-06   7e-6 / 2e-5     (degrees +-20: x1; half_block +-20: d k)

   The three misreadings on the same table, float64 against float64: per-destination maximum and 1e-16 move x1 by 1.1 and the gradients
   by 1.5 of their scale (spans +-20), a detached M moves d k by 1.0 of its scale (values unchanged).

3. Each of the three misreadings of the layer -- a per-destination maximum, 1e-16 in place of 1e-6, a detached M -- misses those bars
   on the case table (float64 against float64: nothing but the formula differs), so a kernel that implements one of them cannot pass
   tests/test_gpu_empn_attention_ops.py."""
import pytest
import torch

import empn_attention_ref as ar
import ops_ref
from test_oracle_golden import close, oracle_spec

from oracle import graph as gr


def restated_model(fx, dtype=torch.float32):
    spec = oracle_spec(fx)
    split = gr.split_obs(spec, {k: a.to(dtype) for k, a in fx.obs.items()})
    topo = gr.build_topology(spec, split, full_graph_obs=False)
    graph, s, v = gr.build_features(spec, topo, split, dist_as_pos=True)
    graph["output_mask_key"] = "grippers"
    m = fx.model
    kw = dict(dim=m["dim"], output_dim=m["output_dim"], output_dim_vec=m["output_dim_vec"], num_layers=2, batch_size=fx.B)
    return graph, s, v, lambda P, g, s_, v_, calibrate=False: ar.empn_attention_forward(P, g, s_, v_, calibrate=calibrate, **kw)


@pytest.mark.parametrize("case", list(ar.ATTENTION_CASES))
def test_restatement_reproduces_the_reference_fixture(golden_dir, case):
    fx = ar.AttentionFixture(golden_dir, case)
    graph, s, v, forward = restated_model(fx)
    z = fx.z
    assert any("key_transform.weight" in k for k in fx.init) and any("query_transform.bias" in k for k in fx.grad)

    P = {k: val.clone() for k, val in fx.init.items()}
    out0, hid0 = forward(P, graph, s, v, calibrate=True)
    close(out0, z["out_first_call"], 2e-6)
    close(hid0, z["hidden_first_call"], 2e-6)
    for k, val in fx.cal.items():
        if val.dtype.is_floating_point:
            close(P[k], val, 2e-6)
            assert torch.equal(P[k], fx.init[k]) == (k not in fx.changed), k   # the key and query layers are never rescaled
    assert any("kernel.weight" in k for k in fx.changed) and not any("key_transform" in k or "query_transform" in k for k in fx.changed)

    P64 = {k: (val.double() if val.dtype.is_floating_point else val.clone()) for k, val in fx.init.items()}
    g64, s64, v64, _ = restated_model(fx, torch.float64)
    forward(P64, g64, s64, v64, calibrate=True)
    for k in fx.changed:
        if fx.cal64[k].dtype.is_floating_point:
            close(P64[k], fx.cal64[k], 1e-10, 1e-10)
    out64, hid64 = forward({k: val.clone() for k, val in fx.cal64.items()}, g64, s64, v64)
    close(out64, z["out64"], 1e-10, 1e-10)
    close(hid64, z["hidden64"], 1e-10, 1e-10)

    P = {k: val.clone().requires_grad_(val.dtype.is_floating_point and "ori_grid" not in k) for k, val in fx.cal.items()}
    out, hid = forward(P, graph, s, v)
    close(out, z["out"], 2e-6)
    close(hid, z["hidden"], 2e-6)
    ((out * z["R_out"]).sum() + (hid * z["R_hidden"]).sum()).backward()
    for k, val in fx.grad.items():
        close(P[k].grad, val, 1e-5, 1e-4)
    assert len(fx.grad) >= 28
    for k, p in P.items():
        if p.requires_grad and k not in fx.grad:
            assert p.grad is None or not bool(p.grad.abs().sum() > 0), k


def _worst(cases, variant=None):
    """(worst value error, worst gradient error, where) of the cases: fp32 against float64, or (``variant``) the float64 evaluation of a
    misreading against the float64 reference."""
    wv, wg, where = 0.0, 0.0, ["", ""]
    for c in cases:
        o64, g64 = c.evaluate(torch.float64)
        o, g = c.evaluate(torch.float64, variant=variant) if variant else c.evaluate(torch.float32)
        for k in o64:
            e = ops_ref.rel_err(o[k], o64[k])
            if e > wv:
                wv, where[0] = e, f"{c.name}: {k}"
        for k in g64:
            e = ops_ref.rel_err(g[k], g64[k])
            if e > wg:
                wg, where[1] = e, f"{c.name}: d {k}"
    return wv, wg, where


def test_bar_table():
    print(f"{'op':16s} {'cases':>5s} {'worst fp32 value':>17s} {'worst fp32 grad':>16s} {'derived bars':>20s} {'BARS':>20s}")
    for op, cases in (("kq_project", ar.project_cases()), ("edge_attention", ar.attention_cases())):
        wv, wg, where = _worst(cases)
        dv, dg = ops_ref.round_up_1(8 * wv), ops_ref.round_up_1(8 * wg)
        bv, bg = ar.BARS[op]
        print(f"{op:16s} {len(cases):5d} {wv:17.2e} {wg:16.2e} {dv:9.0e} / {dg:8.0e} {bv:9.0e} / {bg:8.0e}   ({where[0]}; {where[1]})")
        assert dv / 1.5 <= bv <= dv * 1.5 and dg / 1.5 <= bg <= dg * 1.5, (op, (dv, dg), (bv, bg))


def test_case_table_covers_what_it_is_for():
    cases = ar.attention_cases()
    by = {c.graph: c for c in cases if c.span == 1.0}
    assert set(by) == set(ar.GRAPHS) and {c.span for c in cases} == set(ar.SPANS)
    assert all(24 <= c.n <= 96 for c in cases)
    deg = lambda c, row: torch.bincount(c.ei[row], minlength=c.n)
    d = by["degrees"]
    assert sorted(set(deg(d, 1).tolist())) == [0, 1, 2, 3, 4, 5] and int((deg(d, 0) == 0).sum()) >= 10
    assert int(deg(by["hub"], 1).max()) == 70
    assert (by["half_block"].n * 16) % 64 == 32
    s = by["self_loops"]
    assert int((s.ei[0] == s.ei[1]).sum()) == s.n
    assert by["empty"].ei.shape[1] == 0
    # at +-10 destinations with S within a decade of the 1e-6 appear in every graph (0.5 % .. 19 % of the rows); at +-20 a fifth to four
    # fifths of the rows have S BELOW 1e-6 (a property of the inputs, computed in float64)
    for c in cases:
        if c.ei.shape[1] and c.span >= 10:
            l = (c.k.double()[c.ei[0]] * c.q.double()[c.ei[1]]).sum(-1) / 128 ** 0.5
            assert abs(float(l.abs().max()) - c.span) < 1e-5 * c.span
            S = torch.zeros(c.n, 16, dtype=torch.float64).index_add(0, c.ei[1], torch.exp(l - l.max()))
            has = deg(c, 1) > 0
            assert float((S[has] < 1e-5).double().mean()) > 0, c.name
            if c.span >= 20:
                assert float((S[has] < 1e-6).double().mean()) > 0.2, c.name


@pytest.mark.parametrize("variant", [v for v in ar.VARIANTS if v != "reference"])
def test_a_misreading_of_the_layer_misses_the_bars(variant):
    wv, wg, where = _worst(ar.attention_cases(), variant)
    bv, bg = ar.BARS["edge_attention"]
    print(f"{variant}: values off by {wv:.2e} ({where[0]}), gradients by {wg:.2e} ({where[1]}); bars {bv:.0e} / {bg:.0e}")
    assert wg > 10 * bg, (variant, wg)
    if variant != "detached_max":   # (a detached M leaves the values alone: only the gradients tell)
        assert wv > 10 * bv, (variant, wv)
    else:
        assert wv == 0.0


def test_empty_edge_set_gives_zeros_and_zero_gradients():
    c = next(c for c in ar.attention_cases() if c.graph == "empty")
    o, g = c.evaluate(torch.float64)
    assert not bool(o["x1"].abs().sum() > 0) and g["msg"].numel() == 0
    assert not bool(g["k"].abs().sum() > 0) and not bool(g["q"].abs().sum() > 0)
