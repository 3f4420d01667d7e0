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

       op                    cases  worst fp32 value  worst fp32 gradient  bars (8 x, one digit)
       kq_project                9         4.15e-07             5.83e-07   4e-6 / 5e-6     (2049 nodes: k; 24 nodes: d wk)
       edge_attention           17         7.88e-07             2.39e-06   7e-6 / 2e-5     (degrees +-20: x1; half_block +-20: d k)
       edge_attention_large     12         6.27e-07             6.27e-06   6e-6 / 6e-5     (many_rows +-20 tie: x1; many_rows +-1: d k)

   kq_project holds the five node counts and the four row counts of the direct calls; edge_attention the original five graphs, whose
   bars are as the first table gave them; edge_attention_large the graphs that go round the kernels' grids and the tie cases (why its
   gradient bar is three times the small one: the comment at ``BARS``).
   The three misreadings on the original table, float64 against float64: per-destination maximum and 1e-16 move x1 by 1.1 and the
   gradients by 1.5 of their scale (spans +-20), a detached M moves d k by 1.0 of its scale (values unchanged).

3. Each of the three misreadings of the layer -- a per-destination maximum, 1e-16 in place of 1e-6, a detached M -- misses those bars
   on the case table (float64 against float64: nothing but the formula differs), so a kernel that implements one of them cannot pass
   tests/test_gpu_empn_attention_ops.py.  The same for the tie rule: d M at the highest tied index, or split evenly as torch's
   ``l.max()`` does, moves d k and d q by 1.0 and 0.67 of their scale on every tie case (values unchanged); for bitwise duplicated
   graphs the parameter gradients cannot tell and d x can.

4. The case table is what it is for: the large cases reach every loop, cap and chunk boundary of the launch shapes restated here, and
   each of the three stages of the kernels' maximum (per wave, across a workgroup's waves, across workgroups) decides the argmax on one
   of the tie placements."""
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
    groups = {}
    for c in ar.project_cases() + ar.project_row_cases() + ar.attention_cases():
        groups.setdefault(c.bar, []).append(c)
    assert list(groups) == list(ar.BARS)
    assert ar.BARS["kq_project"] == (4e-6, 5e-6) and ar.BARS["edge_attention"] == (7e-6, 2e-5)   # (the bars the first table gave: kept)
    print(f"{'op':20s} {'cases':>5s} {'worst fp32 value':>17s} {'worst fp32 grad':>16s} {'derived bars':>20s} {'BARS':>20s}")
    for op, cases in groups.items():
        wv, wg, where = _worst(cases)
        dv, dg = ops_ref.round_up_1(8 * wv), ops_ref.round_up_1(8 * wg)
        bv, bg = ar.BARS[op]
        print(f"{op:20s} {len(cases):5d} {wv:17.2e} {wg:16.2e} {dv:9.0e} / {dg:8.0e} {bv:9.0e} / {bg:8.0e}   ({where[0]}; {where[1]})")
        assert dv / 1.5 <= bv <= dv * 1.5 and dg / 1.5 <= bg <= dg * 1.5, (op, (dv, dg), (bv, bg))


def test_case_table_covers_what_it_is_for():
    every = ar.attention_cases()
    cases = [c for c in every if c.graph in ar.GRAPHS]   # the original five graphs: one row per wave everywhere
    by = {c.graph: c for c in cases if c.span == 1.0}
    assert set(by) == set(ar.GRAPHS) and {c.span for c in cases} == set(ar.SPANS)
    assert all(24 <= c.n <= 96 and c.n_src == c.n_dst == c.n and c.bar == "edge_attention" and c.ties is None for c in cases)
    assert all(max(c.ei.shape[1], c.n) * 16 <= ar.ROWS_PER_PASS and ar.kq_bwd_blocks(c.n * 16) == (c.n * 16 + 63) // 64 for c in cases)
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
    _large_cases_cover_the_loops([c for c in every if c.graph not in ar.GRAPHS])
    _project_cases_cover_the_caps()


def _large_cases_cover_the_loops(cases):
    """The large graphs and the tie cases, against the launch shapes of csrc/attention_ops.hip restated here: row kernels have at most
    2048 workgroups of 4 waves, one row per wave and iteration, so a grid pass is ``P`` = 8192 rows; wave w of workgroup b visits the
    rows 4 b + w, 4 b + w + P, ..."""
    P = ar.ROWS_PER_PASS
    assert P == 2048 * 4
    wg, wave = (lambda r: (r // 4) % 2048), (lambda r: r % 4)
    plain = [c for c in cases if not c.tie]
    assert {(c.graph, c.span) for c in plain} == {(g, s) for g in ar.LARGE_GRAPHS for s in ar.LARGE_SPANS} and {1.0, 10.0} <= set(ar.LARGE_SPANS)
    assert all(c.bar == "edge_attention_large" for c in cases)
    for c in cases:
        E = c.ei.shape[1]
        pairs = list(zip(*c.ei.tolist()))
        assert pairs == sorted(set(pairs), key=lambda p: (p[1], p[0])), c.name   # deduplicated, sorted by (destination, source)
        assert c.k.shape == (c.n_src, 16, 128) and c.q.shape == (c.n_dst, 16, 128) and c.msg.shape == (E, 16, 64)
        assert int(c.ei[0].max()) < c.n_src and int(c.ei[1].max()) < c.n_dst
        l = (c.k.double()[c.ei[0]] * c.q.double()[c.ei[1]]).sum(-1) / 128 ** 0.5
        assert abs(float(l.abs().max()) - c.span) < 1e-5 * c.span, c.name
        assert E * 16 > P, c.name                           # edge_logits_fwd: the per-wave running (best, besti) sees a second row
        rows_q, rows = c.n_dst * 16, (c.n_dst + c.n_src) * 16
        assert rows > P, c.name                             # edge_logits_bwd loops
        if c.graph == "many_rows":
            in_deg, out_deg = torch.bincount(c.ei[1], minlength=c.n_dst), torch.bincount(c.ei[0], minlength=c.n_src)
            assert c.n_src == c.n_dst == c.n and 550 <= c.n <= 650 and sorted(set(in_deg.tolist())) == [0, 1, 2, 3, 4]
            assert int((in_deg == 0).sum()) > 0 and int((out_deg == 0).sum()) > 0
            assert E * 16 > 2 * P and (E * 16) % P != 0     # waves visit two AND three logit rows
            assert rows_q > P and rows_q % P != 0           # edge_attend_fwd / _bwd loop; the last pass is partial
        elif c.graph == "wide_sources":                     # a wave takes a d q row on one iteration and a d k row on the next
            assert c.n_src >= 10 * c.n_dst and 0 < rows_q < P < rows and c.n is None
            assert int((torch.bincount(c.ei[0], minlength=c.n_src) == 0).sum()) > 0
        else:                                               # the d q rows alone go round the grid; the d k rows start mid-grid
            assert c.graph == "wide_destinations" and c.n_dst >= 10 * c.n_src and c.n is None
            assert rows_q > P and rows_q % P != 0 and rows_q % 4 == 0
            assert int((torch.bincount(c.ei[1], minlength=c.n_dst) == 0).sum()) > 0
    ties = [c for c in cases if c.tie]
    assert {(c.tie, c.span) for c in ties} == {(t, s) for t in ar.TIES for s in ar.TIE_SPANS} and {10.0, 20.0} <= set(ar.TIE_SPANS)
    for c in ties:
        assert c.graph == "many_rows"
        r0, r1, r2 = c.ties
        assert [r0, r1, r2] == sorted(e * 16 + o for e, o in ar.TIES[c.tie]) and r0 < r1 < r2 < c.ei.shape[1] * 16
        ends = [n for (s, d), _ in c.tie_edges for n in (s, d)]
        assert len(set(ends)) == 6
        # the three rows are bit-equal and alone at the top, in float64 and in float32; everything else is at 0.8 x span or below
        for dtype in (torch.float64, torch.float32):
            l = ((c.k.to(dtype)[c.ei[0]] * c.q.to(dtype)[c.ei[1]]).sum(-1) / 128 ** 0.5).flatten()
            assert (l == l.max()).nonzero().flatten().tolist() == [r0, r1, r2], (c.name, dtype)
            rest = l.clone()
            rest[[r0, r1, r2]] = 0
            assert float(rest.abs().max()) <= 0.8 * c.span * (1 + 1e-5), c.name
        if c.tie == "first_pass":
            assert (r0, r1, r2) == (3, 8147, 8192)
            assert wg(r1) > wg(r2) and r2 >= P              # the finish over the block partials meets the higher index first
            assert wg(r2) == wg(r0) and wave(r2) < wave(r0)   # ... and so does the merge of workgroup 0's four waves
        elif c.tie == "late":
            assert (r0, r1, r2) == (8994, 16387, 17186)
            assert r0 >= P                                  # no occurrence in the first pass
            assert (wg(r2), wave(r2)) == (wg(r0), wave(r0)) and r2 == r0 + P   # one wave meets it twice, on consecutive iterations
            assert wg(r1) < wg(r0)                          # the finish meets the higher index first
        else:
            assert c.tie == "one_workgroup" and (r0, r1, r2) == (8193, 16386, 17605)
            assert wg(r0) == wg(r1) and wave(r0) < wave(r1) and wg(r2) > wg(r0)   # the wave merge meets the LOWER index first


def _argmax_as_the_kernels_reduce(l, wave_keeps=">", waves_merge="index", blocks_merge="index", passes=None):
    """(M, argmax) of the flat logits ``l`` through the three stages of edge_logits_fwd / edge_logits_max, restated: each wave's running
    best over its rows 4 b + w + 8192 i (``wave_keeps``: ">" strictly greater replaces, ">=" the later of equals replaces), the
    workgroup's four waves merged in wave order and the block partials merged in block order (``*_merge``: "index" greater value or equal
    value and lower index replaces, ">" greater only, ">=" greater or equal).  ``passes``: rows of that many grid passes only."""
    nb, n = min((len(l) + 3) // 4, 2048), len(l) if passes is None else min(len(l), passes * 8192)

    def replaces(rule, v, i, bv, bi):
        return v > bv or (v == bv and (rule == ">=" or (rule == "index" and i < bi)))
    partial = []
    for b in range(nb):
        per_wave = []
        for w in range(4):
            best, besti = -float("inf"), 2 ** 31 - 1
            for r in range(4 * b + w, n, 4 * nb):
                if replaces(wave_keeps, l[r], r, best, besti):
                    best, besti = l[r], r
            per_wave.append((best, besti))
        bv, bi = per_wave[0]
        for v, i in per_wave[1:]:
            if replaces(waves_merge, v, i, bv, bi):
                bv, bi = v, i
        partial.append((bv, bi))
    bv, bi = partial[0]
    for v, i in partial[1:]:
        if replaces(blocks_merge, v, i, bv, bi):
            bv, bi = v, i
    return bv, bi


def test_each_stage_of_the_maximum_is_told_by_a_tie_placement():
    """The tie placements are there so that EVERY stage of the kernels' three-stage maximum decides the answer somewhere: the restated
    reduction gives the lowest tied row on both placements, and with any one stage taking equals the other way (or looking at the first
    grid pass only) it gives another row -- or another M -- on at least one of them.  A kernel with that mistake hands d M to that row,
    which is the ``tie_highest_index``-like miss of test_a_misreading_of_the_layer_misses_the_bars: d k and d q off by their whole scale."""
    cases = {c.tie: c for c in ar.attention_cases() if c.tie and c.span == 10.0}
    assert set(cases) == set(ar.TIES)
    logits = {t: c.parts(torch.float32)[0].flatten().tolist() for t, c in cases.items()}
    for t, c in cases.items():
        assert _argmax_as_the_kernels_reduce(logits[t]) == (max(logits[t]), c.ties[0]), t
    wrong = {"wave keeps the later of equals": dict(wave_keeps=">="), "waves merged without the index": dict(waves_merge=">"),
             "waves merged, later wins": dict(waves_merge=">="), "blocks merged without the index": dict(blocks_merge=">"),
             "blocks merged, later wins": dict(blocks_merge=">="), "first grid pass only": dict(passes=1)}
    for what, kw in wrong.items():
        told = [t for t, c in cases.items() if _argmax_as_the_kernels_reduce(logits[t], **kw) != (max(logits[t]), c.ties[0])]
        print(f"{what}: told by {told}")
        assert told, what


def _project_cases_cover_the_caps():
    """Launch shapes of the projection kernels, restated: forward and input gradient have min(ceil(rows / 4), 1024) workgroups of 4
    rows; the weight gradient has ``ar.kq_bwd_blocks(rows)`` workgroups, workgroup b the rows b * chunk .. (b + 1) * chunk with
    chunk = ceil(rows / workgroups)."""
    assert [c.n for c in ar.project_cases()] == list(ar.PROJECT_NODES + ar.PROJECT_NODES_LARGE) and ar.PROJECT_NODES == (24, 26, 96)
    assert [ar.kq_bwd_blocks(r) for r in (0, 1, 64, 65, 32768, 32769, 10 ** 8)] == [1, 1, 1, 2, 512, 512, 512]
    n_loop, n_chunk = ar.PROJECT_NODES_LARGE

    def chunks(rows):
        b = ar.kq_bwd_blocks(rows)
        chunk = (rows + b - 1) // b
        return chunk, [max(0, min(rows, (i + 1) * chunk) - i * chunk) for i in range(b)]
    for n in ar.PROJECT_NODES:                  # the original cases: no loop, chunks of at most 64 rows, none empty
        chunk, held = chunks(n * 16)
        assert (n * 16 + 3) // 4 <= 1024 and chunk <= 64 and min(held) > 0
    rows = n_loop * 16                          # 257 nodes
    assert (rows + 3) // 4 == 1024 + 4          # four workgroups go round again: a partial second iteration
    rows = n_chunk * 16                         # 2049 nodes
    chunk, held = chunks(rows)
    assert len(held) == 512 and chunk == 65 and sum(held) == rows
    assert held[:504] == [65] * 504 and held[504] == 24 and held[505:] == [0] * 7   # a short chunk, then seven empty ones
    for r in ar.PROJECT_ROWS:                   # the direct calls: the batch of four is never full at the end
        assert r % 4 != 0
    assert max(ar.PROJECT_ROWS) > 4096 and [c.rows for c in ar.project_row_cases()] == list(ar.PROJECT_ROWS)


@pytest.mark.parametrize("variant", [v for v in ar.VARIANTS if v != "reference"])
def test_a_misreading_of_the_layer_misses_the_bars(variant):
    if variant.startswith("tie_"):
        # the two other tie rules, on EACH tie case: d M at the highest tied index or split evenly (torch's l.max()) instead of at the
        # lowest.  The values cannot tell; d k and d q miss the bar by four orders of magnitude (measured: 0.67 of their scale for the
        # even split, 1.0 for the highest index, at both spans and both placements).  Without a declared tie they change nothing.
        bv, bg = ar.BARS["edge_attention_large"]
        tie_cases = [c for c in ar.attention_cases() if c.tie]
        assert len(tie_cases) == len(ar.TIES) * len(ar.TIE_SPANS)
        for c in tie_cases:
            o64, g64 = c.evaluate(torch.float64)
            o, g = c.evaluate(torch.float64, variant=variant)
            ek, eq = ops_ref.rel_err(g["k"], g64["k"]), ops_ref.rel_err(g["q"], g64["q"])
            print(f"{variant} on {c.name}: d k off by {ek:.2e}, d q by {eq:.2e} of their scale; bars {bv:.0e} / {bg:.0e}")
            assert torch.equal(o["x1"], o64["x1"]) and torch.equal(g["msg"], g64["msg"])   # (the values and d msg cannot tell)
            assert ek > 10 * bg and eq > 10 * bg, (variant, c.name, ek, eq)
        plain = next(c for c in ar.attention_cases() if c.graph == "many_rows" and not c.tie)
        assert _worst([plain], variant)[:2] == (0.0, 0.0)
        return
    cases = [c for c in ar.attention_cases() if c.bar == "edge_attention"]
    wv, wg, where = _worst(cases, variant)
    bv, bg = ar.BARS["edge_attention"]
    print(f"{variant}: values off by {wv:.2e} ({where[0]}), gradients by {wg:.2e} ({where[1]}); bars {bv:.0e} / {bg:.0e}")
    assert wg > 10 * bg, (variant, wg)
    if variant != "detached_max":   # (a detached M leaves the values alone: only the gradients tell)
        assert wv > 10 * bv, (variant, wv)
    else:
        assert wv == 0.0


def test_duplicated_graphs_hide_the_tie_rule_from_the_parameters_only():
    """Two bitwise-equal graphs in one batch (environments reset to the same state) tie the maximum exactly.  By symmetry the parameter
    gradients are the same whichever tied element takes d M; the per-node d x is not."""
    c = next(c for c in ar.attention_cases() if c.graph == "degrees" and c.span == 10.0)
    p = ar.ProjectCase(c.n)
    n, E = c.n, c.ei.shape[1]
    ei = torch.cat([c.ei, c.ei + n], 1)   # (still sorted by destination, then source)
    w = [t.double() * s for t, s in zip(p.w, (6.0, 1.0, 6.0, 1.0))]   # (logits of a span near +-10: M matters)
    msg, R = c.msg.double().repeat(2, 1, 1), c.R.double().repeat(2, 1, 1)
    grads = {}
    for variant in ("reference", "tie_highest_index", "tie_even_split"):
        x = p.x.double().repeat(2, 1, 1).requires_grad_(True)
        ws = [t.clone().requires_grad_(True) for t in w]
        k, q = ar.kq_project(x, *ws)
        l = (k[ei[0]] * q[ei[1]]).sum(-1).detach().flatten()
        top = int(l.argmax()) % (E * 16)
        assert float(l.abs().max()) > 5
        x1 = ar.edge_attention(k, q, msg, ei[0], ei[1], 2 * n, variant, ties=[top, top + E * 16])
        (x1 * R).sum().backward()
        grads[variant] = [x.grad] + [t.grad for t in ws]
    for variant in ("tie_highest_index", "tie_even_split"):
        dx, *dw = grads[variant]
        dx0, *dw0 = grads["reference"]
        for a, b in zip(dw, dw0):
            assert ops_ref.rel_err(a, b) < 1e-12, variant
        print(f"{variant}: d x differs by {ops_ref.rel_err(dx, dx0):.2e} of its scale, the four parameter gradients by < 1e-12")
        assert ops_ref.rel_err(dx, dx0) > 10 * ar.BARS["edge_attention"][1], variant


def test_empty_edge_set_gives_zeros_and_zero_gradients():
    c = next(c for c in ar.attention_cases() if c.graph == "empty")
    o, g = c.evaluate(torch.float64)
    assert not bool(o["x1"].abs().sum() > 0) and g["msg"].numel() == 0
    assert not bool(g["k"].abs().sum() > 0) and not bool(g["q"].abs().sum() > 0)
