"""Pins tests/fold_ref.py, the float64 restatements tests/test_gpu_fold_ops.py checks the gradient fold and the critic lane's value loss
against: fold64 must be numpy's float64 column sums, a plain fp32 torch.sum of every case must land inside fold_allowance (the reference
passes its own bar), the integer cases must be exact in fp32 in any summation order, and value_loss64 must be the hand-written clipped
l2 loss and its gradient on rows of every branch."""
import numpy as np
import pytest
import torch

import fold_ref as fr

CASES = fr.all_cases()


def _init(case, key):
    return case.init(key, torch.Generator().manual_seed(5))


@pytest.mark.parametrize("pair", CASES, ids=[p[0].name for p in CASES])
def test_fold64_is_numpy(pair):
    for case in pair:
        for key, (ln, _) in case.dst.items():
            slabs, starts = case.feeds(key)
            init = _init(case, key)
            want = sum(s.numpy().astype(np.float64)[:, st:st + ln].sum(0) for s, st in zip(slabs, starts))
            assert np.array_equal(case.ref(key).numpy(), want + np.zeros(ln)), (case.name, key)
            assert np.array_equal(case.ref(key, init).numpy(), want + init.numpy().astype(np.float64)), (case.name, key)


@pytest.mark.parametrize("pair", CASES, ids=[p[0].name for p in CASES])
def test_fp32_sum_is_inside_the_allowance(pair):
    """torch's fp32 sum (some order of its own) of each destination's terms, with and without a prior destination."""
    worst = 0.0
    for case in pair:
        for key, (ln, _) in case.dst.items():
            slabs, starts = case.feeds(key)
            init = _init(case, key)
            got = torch.zeros(ln)
            for s, st in zip(slabs, starts):
                got = got + s[:, st:st + ln].sum(0)
            worst = max(worst, fr.ratio(got, case.ref(key), case.allow(key)), fr.ratio(got + init, case.ref(key, init), case.allow(key, init)))
            if case.kind == "int":
                assert torch.equal(got.double(), case.ref(key)), (case.name, key)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("pair", CASES, ids=[p[0].name for p in CASES])
def test_integer_cases_are_exact_in_any_order(pair):
    """sum |terms| (with the prior destination) < 2^24 per column bounds every partial sum of every order: all are exact fp32 integers."""
    case = pair[0]
    assert case.kind == "int" and pair[1].kind == "gauss"
    for key, (ln, _) in case.dst.items():
        slabs, starts = case.feeds(key)
        for s in slabs:
            assert torch.equal(s, s.round()) and float(s.abs().max() if s.numel() else 0) <= 8
        init = _init(case, key)
        assert torch.equal(init, init.round()) and (init != 0).all()
        mag = sum(s[:, st:st + ln].double().abs().sum(0) for s, st in zip(slabs, starts)) + init.double().abs()
        assert float(mag.max()) < 2.0 ** 24, (case.name, key)


def test_cases_cover_the_shapes():
    """The sweep holds every length at aligned, odd and even-but-unaligned starts in both row strides, float4-eligible destinations and
    the misaligned one; the Gaussian cases hold a slab at 1e3 and one at 1e-5; segment lengths in one slab differ by more than 64."""
    for r in fr.ROWS:
        c = fr.sweep(r, "int")
        assert len(c.segs) <= 64 and all(s.shape[0] == r for s in c.slabs)
        vec = {k for k in c.dst if c.float4_rule(k)}
        assert vec == {f"s0+4x{n}" for n in (4, 64, 128, 132)}
        assert c.dst["mis1"] == (64, 1) and not c.float4_rule("mis1")
        assert {st % 2 for _, st, _, _ in c.segs} == {0, 1} and {s.shape[1] % 4 for s in c.slabs} == {0, 3}
    scales = [float(s.std()) for r in fr.ROWS[-6:] for s in fr.sweep(r, "gauss").slabs]
    assert min(scales) < 1e-4 and max(scales) > 1e2
    sh = fr.shared("gauss")
    assert sh.float4_rule("a") and not sh.float4_rule("b") and not sh.float4_rule("c")
    assert [s.shape[0] for s in sh.feeds("a")[0]] == [40, 7, 0, 300]
    assert len(fr.limit(64, "int").dst) == 64 and len(fr.limit(65, "int").dst) == 65


def _by_hand(V, Vo, R, clip, coef, inv_batch):
    """The clipped l2 value loss row by row in Python floats: max of the two losses; the gradient of the larger one (the clipped
    one's is that of the unclipped value inside the range, bounds included, and 0 outside), the mean of the two on a tie."""
    dv, terms = [], []
    for v, vo, r in zip(V.double().tolist(), Vo.double().tolist(), R.double().tolist()):
        l1, g1 = (v - r) ** 2, 2 * (v - r)
        l, g = l1, g1
        if clip:
            vc = vo + min(max(v - vo, -clip), clip)
            l2, g2 = (vc - r) ** 2, (2 * (vc - r) if -clip <= v - vo <= clip else 0.0)
            if l2 > l1:
                l, g = l2, g2
            elif l2 == l1:
                g = 0.5 * (g1 + g2)
        dv.append(g * coef * inv_batch)
        terms.append(l * coef)
    return torch.tensor(dv, dtype=torch.float64), terms


@pytest.mark.parametrize("clip", [0.0, 0.25, 1e6])
def test_value_loss64_is_the_formula(clip):
    for coef in (0.5, 1.0):
        V, Vo, R, names = fr.value_case(300, clip, 3)
        assert names[-1] == "tie outside" and len(names) == 11
        for inv in (1.0 / 300, 1.0 / 600):
            dv, total, mean = fr.value_loss64(V, Vo, R, clip, coef, inv)
            hdv, terms = _by_hand(V, Vo, R, clip, coef, inv)
            assert float((dv - hdv).abs().max()) <= 4 * 2.0 ** -53 * float(hdv.abs().max())
            assert ((dv - hdv).abs() <= 4 * 2.0 ** -53 * hdv.abs()).all()
            assert abs(total - sum(terms)) <= 300 * 2.0 ** -53 * sum(abs(t) for t in terms)
            assert mean == total * inv
            a_dv, a_sum, a_mean = fr.value_loss_allowances(V, Vo, R, clip, coef, inv)
            assert (a_dv > 0).all() and a_sum > 0 and a_mean == a_sum * inv


def test_value_rows_take_their_branches():
    """Each named row is what its name says, in exact arithmetic on exact fp32 values -- and the tie halves the gradient."""
    for clip in (0.25, 1e6):
        rows = {n: (vo, v, r) for n, vo, v, r in fr.value_rows(clip)}
        for n, (vo, v, r) in rows.items():
            for x in (vo, v, r):
                assert float(torch.tensor(x, dtype=torch.float64).float()) == x, (n, x)
            vc = vo + min(max(v - vo, -clip), clip)
            l1, l2 = (v - r) ** 2, (vc - r) ** 2
            if "larger" in n:
                assert l2 > l1 and abs(v - vo) > clip
            if "smaller" in n:
                assert l2 < l1 and abs(v - vo) > clip
            if n.startswith("on "):
                assert abs(v - vo) == clip
            if n == "inside":
                assert abs(v - vo) < clip
            if n == "tie outside":
                assert l1 == l2 and abs(v - vo) > clip and vc != v
        vo, v, r = rows["tie outside"]
        t = lambda x: torch.tensor([x], dtype=torch.float32)
        dv, _, _ = fr.value_loss64(t(v), t(vo), t(r), clip, 1.0, 1.0)
        assert float(dv) == v - r                              # half of 2 (V - R)
        vo, v, r = rows["above, clipped loss larger"]
        assert float(fr.value_loss64(t(v), t(vo), t(r), clip, 1.0, 1.0)[0]) == 0.0
