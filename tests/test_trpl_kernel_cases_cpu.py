"""The cases of tests/test_gpu_trpl_kernel.py through the float64 oracle only (no GPU): every per-frame regime of trpl_cases.REGIMES
occurs in every full workgroup of every case and does what it is meant to (the oracle's projection moves the parts it should and leaves
the others), the value and PPO clip regimes are populated, and every reference value is finite.  This keeps the GPU test's coverage
from drifting when the generator is edited."""
import pytest
import torch

import trpl_cases as tc


def _check_regimes(c, d, ref):
    B, A = c.B, c.A
    reg = tc.regimes_of(B, c.shift)
    mb, cb = tc.bounds(c.proj)
    mp, cp = ref["parts"]
    loc, sig = d["loc"].double(), d["sigma"].double()
    S, So, mo = sig ** 2, d["batch"]["var"].double(), d["batch"]["loc"].double()
    mm, cm = ref["mean_moved"], ref["cov_moved"]
    joint = c.proj == 4
    for f, r in enumerate(reg):
        ctx = (c.name, f, r, float(mp[f]), float(cp[f]))
        if r == "equal":
            assert torch.equal(loc[f], mo[f]) and torch.equal(S[f], So[f]), ctx
            assert float(mp[f]) == 0.0 and float(cp[f]) == 0.0 and not mm[f] and not cm[f], ctx
        elif r == "inside":
            assert (float(mp[f] + cp[f]) < 0.7 * mb) if joint else (mp[f] < 0.5 * mb and cp[f] < 0.5 * cb), ctx
            assert not mm[f] and not cm[f], ctx
        elif r == "mean_only":
            assert mp[f] > 2 * mb and cp[f] < 0.5 * cb and mm[f], ctx
            assert joint or not cm[f], ctx
        elif r == "cov_only":
            assert mp[f] < 0.5 * mb and cp[f] > 2 * cb and cm[f], ctx
            assert joint or not mm[f], ctx
        elif r == "both":
            assert mp[f] > 2 * mb and cp[f] > 2 * cb and mm[f] and cm[f], ctx
        elif r == "large":
            ratio = S[f] / So[f]
            assert float(ratio.max()) > 25.0 and mm[f] and cm[f], ctx
            assert A < 2 or float(ratio.min()) < 1 / 25.0, ctx
        elif r == "cov_split":
            assert cp[f] > 2 * cb and cm[f], ctx
            if A >= 2:
                eq = S[f] == So[f]
                assert bool(eq.any()) and not bool(eq.all()), ctx
        elif r == "min_std":
            assert float(d["sigma"][f, 0]) in (float(torch.tensor(1e-5)), float(torch.tensor(1e-3))) and float(So[f, 0]) == 1.0, ctx
            assert cm[f], ctx
    # every regime in every full workgroup
    for w in range(B // tc.TRPL_FPB):
        assert set(reg[w * tc.TRPL_FPB:(w + 1) * tc.TRPL_FPB]) == set(tc.REGIMES), (c.name, w)
    if reg.count("min_std") >= 2:
        assert {float(x) for x in d["sigma"][[f for f, r in enumerate(reg) if r == "min_std"], 0]} == {
            float(torch.tensor(1e-5)), float(torch.tensor(1e-3))}


def _check_values(c, d):
    if not c.value:
        return
    V, Vo, R = d["value"].double(), d["batch"]["state_value"].double(), d["batch"]["value_target"].double()
    for f in range(c.B):
        r = tc.VREGIMES[f % len(tc.VREGIMES)]
        v, vo, r_ = float(V[f]), float(Vo[f]), float(R[f])
        dlt, l1 = v - vo, (v - r_) * (v - r_)
        if c.clip_value > 0 and r != "on_edge":
            vc = vo + max(min(dlt, c.clip_value), -c.clip_value)
            l2 = (vc - r_) * (vc - r_)
            want = {"inside_clip": abs(dlt) < c.clip_value and l2 == l1, "clip_wins_above": dlt > c.clip_value and l2 > l1,
                    "clip_wins_below": dlt < -c.clip_value and l2 > l1, "unclipped_wins": abs(dlt) > c.clip_value and l2 < l1}[r]
            assert want, (c.name, f, r)
        if r == "on_edge":
            assert abs(dlt) == tc.CLIP_EDGE, (c.name, f)


def _finite(ref):
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()), k
        elif isinstance(v, tuple):
            assert all(bool(torch.isfinite(t).all()) for t in v), k


ALL = tc.lane_cases() + tc.batch_cases() + tc.option_cases()


@pytest.mark.parametrize("c", ALL, ids=[c.name for c in ALL])
def test_case_hits_its_regimes(c):
    d = tc.make_case(c)
    ref = tc.reference(c, d)
    _finite(ref)
    _check_regimes(c, d, ref)
    _check_values(c, d)
    assert tc.adv_error_bound(c, d) >= 0.0


@pytest.mark.parametrize("A", tc.A_SWEEP)
@pytest.mark.parametrize("proj", (0, 1, 2))
def test_target_reference_is_finite(A, proj):
    c = tc.Case(B=37, A=A, proj=proj)
    r = tc.target_reference(c, tc.make_case(c))
    assert all(bool(torch.isfinite(r[k]).all()) for k in ("maxes", "dloc", "dsigma"))
    assert all(v == v and abs(v) < float("inf") for v in r["sums"].values())


@pytest.mark.parametrize("B,A", tc.PPO_GRID)
def test_ppo_case_hits_both_sides_of_both_clip_bounds(B, A):
    d = tc.make_ppo_case(B, A)
    ref = tc.ppo_reference(d, ent_coef=0.015625, critic_coef=0.5, clip_value=0.2)
    for k in ("sums", "dloc", "dsigma", "dvalue", "lw"):
        assert bool(torch.isfinite(ref[k]).all()), k
    lo, hi = tc.ppo_bounds()
    lw, a = ref["lw"], ref["adv_n"]
    assert bool(((lw - lo).abs() > 0.04).all() and ((lw - hi).abs() > 0.04).all())
    if B >= 14:
        for side in ((lw > hi) & (a > 0), (lw < lo) & (a < 0), (lw > hi) & (a < 0), (lw < lo) & (a > 0), (lw > lo) & (lw < hi)):
            assert int(side.sum()) >= 1


def test_adv_error_bound_grows_with_the_offset():
    """The one-pass variance bound: below one fp32 ulp of a' at mean / spread = 1e3, several at 1e4; zero without normalisation."""
    c3, c4 = tc.Case(B=37, A=5, adv_kind="offset3"), tc.Case(B=37, A=5, adv_kind="offset4")
    b3, b4 = tc.adv_error_bound(c3, tc.make_case(c3)), tc.adv_error_bound(c4, tc.make_case(c4))
    assert b3 < 3 * tc.U32 < b4 < 300 * tc.U32, (b3, b4)
    c0 = tc.Case(B=37, A=5, adv_mode="none")
    assert tc.adv_error_bound(c0, tc.make_case(c0)) == 0.0
