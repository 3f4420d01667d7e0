"""The behaviour-cloning modes of the fused loss kernel (trpl_lanes_kernel<L, 8 | 9>, head_ops.hip; ops.bc_fwd_bwd) per op against the
float64 restatement tests/bc_ref.py on the same fp32 inputs, by the comparisons of tests/trpl_cases.py: ``close`` for the fp32 tensors,
RTOL64 / ATOL64 x B for the fp64 sums, the count exact, ``maxes_close``, ``report_close``.
Axes: lane width and padding (A over A_SWEEP at B = 37: L = 4, 8, 16 with 0 .. 15 padding lanes), batch and fold edges (B = 1, one
exactly full workgroup, a second workgroup of one frame, a fold over more than 256 slots), and inside every case the nine pairs of
sigma in {1e-3, 1, 1e3} and |a - mu| in {0, 1e-4, 10} (bc_ref.make_case: the NLL's cancellation)."""
import ctypes

import pytest
import torch

import bc_ref
import trpl_cases as tc
from geometry_rl_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("mse", "nll")
# grl_trpl_fwd_bwd's arguments behind cfg9 and action_dim (include/grl_hip.h), and the ones a behaviour-cloning launch hands over
TRPL_ARGS = ("mean", "sigma", "action", "old_mean", "old_var", "old_logp", "advantage", "value", "old_value", "value_target", "dmean", "dsigma",
             "dvalue", "proj_mean", "proj_var", "adv_stats", "sums", "maxes", "slots", "batch")
BC_GIVEN = {"mean", "sigma", "action", "dmean", "dsigma", "sums", "maxes", "slots", "batch"}


def _check(B, A, mode):
    d = bc_ref.make_case(B, A)
    ref = bc_ref.bc_reference(d["loc"], d["sigma"], d["action"], mode)
    loc, sigma, action = (d[k].to(DEV) for k in ("loc", "sigma", "action"))
    print(f"{mode} B={B} A={A}")
    sums, maxes, dloc, dsigma = ops.bc_fwd_bwd(loc, sigma, action, mode=mode, global_batch=B)
    fold, maxes_d, dloc_d, dsigma_d = ops.bc_fwd_bwd(loc, sigma, action, mode=mode, global_batch=B, defer_fold=True)
    tc.sums_close("sums", sums, ref["sums"], B)
    for col in (1, 7, 9):
        assert float(sums[col]) == 0.0, col
    tc.maxes_close("maxes", maxes, ref["maxes"])
    tc.close("dloc", dloc, ref["dloc"])
    tc.close("dsigma", dsigma, ref["dsigma"])
    if mode == "mse":   # written as exact zeros: an output like any other
        assert torch.equal(dsigma.view(torch.int32), torch.zeros_like(dsigma, dtype=torch.int32))
    # the deferred fold is bitwise the direct one; grl_trpl_report on its slots likewise
    sums_r = torch.empty(12, device=DEV, dtype=torch.float64)
    maxes_r = torch.empty(2, device=DEV, dtype=torch.int32)
    out_r = torch.empty(14, device=DEV, dtype=torch.float32)
    out_v = torch.empty(14, device=DEV, dtype=torch.float32)
    hip.call("grl_trpl_report", fold.slots, B, sums_r, maxes_r, 0.0, out_r)
    hip.call("grl_trpl_loss_values", sums, maxes, 0.0, out_v)
    sums_f, maxes_f = fold()
    for a_, b_ in ((sums_f, sums), (maxes_f, maxes), (sums_r, sums), (maxes_r, maxes), (dloc_d, dloc), (dsigma_d, dsigma), (out_r, out_v)):
        assert torch.equal(a_, b_)
    tc.report_close("loss_values", out_v, ref["report"], 0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("A", tc.A_SWEEP)
def test_lane_widths_and_padding(A, mode):
    _check(37, A, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", (1, 16, 17, 4097))
def test_batch_and_fold_edges(B, mode):
    _check(B, 6, mode)


@pytest.mark.parametrize("mode", MODES)
def test_a_shard_scales_the_gradients_by_the_global_batch(mode):
    B, G = 37, 3 * 37 + 1
    d = bc_ref.make_case(B, 5)
    ref = bc_ref.bc_reference(d["loc"], d["sigma"], d["action"], mode, G)
    sums, maxes, dloc, dsigma = ops.bc_fwd_bwd(*(d[k].to(DEV) for k in ("loc", "sigma", "action")), mode=mode, global_batch=G)
    tc.sums_close("sums", sums, ref["sums"], B)
    tc.close("dloc", dloc, ref["dloc"])
    tc.close("dsigma", dsigma, ref["dsigma"])


@pytest.mark.parametrize("mode", MODES)
def test_every_unused_pointer_is_null(mode, monkeypatch):
    """ops.bc_fwd_bwd hands grl_trpl_fwd_bwd NULL for the old distribution, the old log-prob, the advantage, the value columns, dvalue, the
    projection outputs and the advantage statistics -- and the launch with them runs (the comparisons above are made on such launches)."""
    seen = []
    real = hip.call

    def spy(name, *args, **kw):
        if name == "grl_trpl_fwd_bwd":
            seen.append(dict(zip(TRPL_ARGS, args[2:])))
        return real(name, *args, **kw)
    monkeypatch.setattr(hip, "call", spy)
    d = bc_ref.make_case(5, 3)
    ops.bc_fwd_bwd(*(d[k].to(DEV) for k in ("loc", "sigma", "action")), mode=mode, global_batch=5)
    assert len(seen) == 1 and len(seen[0]) == len(TRPL_ARGS)
    assert {k for k, v in seen[0].items() if v is not None} == BC_GIVEN


def _raw(mode, A=3, entry="grl_trpl_fwd_bwd", trail=(), **given):
    """A raw call of the entry point in a BC mode, buffers sized for 17 columns; ``given``: RL arguments handed over non-NULL."""
    B, W = 5, 17
    f = lambda *s: torch.ones(*s, device=DEV)
    a = {"mean": f(B, W), "sigma": f(B, W), "action": f(B, W), "dmean": torch.full((B, W), 7.0, device=DEV),
         "dsigma": torch.full((B, W), 7.0, device=DEV), "sums": torch.full((12,), 7.0, device=DEV, dtype=torch.float64),
         "maxes": torch.full((2,), 7, device=DEV, dtype=torch.int32),
         "slots": torch.full((hip.query("grl_trpl_slot_doubles", B),), 7.0, device=DEV, dtype=torch.float64), "batch": B}
    a.update(given)
    cfg = (ctypes.c_double * 10)(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / B, float(B), float(mode), 0.0)
    outs = {k: a[k] for k in ("dmean", "dsigma", "sums", "maxes", "slots")}
    try:
        hip.call(entry, cfg, A, *[a.get(k) for k in TRPL_ARGS], *trail)
    finally:
        torch.cuda.synchronize()
    return outs


def _untouched(outs):
    return all(bool((v == 7).all()) for v in outs.values())


@pytest.mark.parametrize("mode", (8, 9))
def test_refusals_happen_before_the_launch(mode):
    """The entropy-stage entry point has no BC instance (-3), A = 17 is refused (-2), and a BC mode takes no RL column (-3); the raw call
    itself is sound (it runs and writes every output)."""
    beta = torch.zeros(1, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="status -3"):
        _raw(mode, entry="grl_trpl_fwd_bwd_ent", trail=(0, beta))
    with pytest.raises(RuntimeError, match="status -2"):
        _raw(mode, A=17)
    for k in ("old_mean", "old_logp", "advantage", "adv_stats"):
        extra = torch.ones(5, 17, device=DEV, dtype=torch.float64 if k == "adv_stats" else torch.float32)
        with pytest.raises(RuntimeError, match="status -3"):
            _raw(mode, **{k: extra})
    outs = _raw(mode)
    dm, ds = outs["dmean"].reshape(-1), outs["dsigma"].reshape(-1)   # 5 frames x 3 columns, contiguous: the first 15 floats, nothing behind them
    assert not bool((dm[:15] == 7).any()) and not bool((ds[:15] == 7).any()) and not bool((outs["sums"] == 7).any())
    assert bool((dm[15:] == 7).all()) and bool((ds[15:] == 7).all())


@pytest.mark.parametrize("mode", (8, 9))
def test_a_refused_call_writes_nothing(mode):
    """The outputs of a refused call keep their sentinels (they are handed in, so they outlive the raise)."""
    B, W = 5, 17
    for kw in (dict(A=17), dict(entry="grl_trpl_fwd_bwd_ent", trail=(0, torch.zeros(1, device=DEV, dtype=torch.float64))),
               dict(advantage=torch.ones(B, device=DEV))):
        outs = {"dmean": torch.full((B, W), 7.0, device=DEV), "dsigma": torch.full((B, W), 7.0, device=DEV),
                "sums": torch.full((12,), 7.0, device=DEV, dtype=torch.float64), "maxes": torch.full((2,), 7, device=DEV, dtype=torch.int32),
                "slots": torch.full((hip.query("grl_trpl_slot_doubles", B),), 7.0, device=DEV, dtype=torch.float64)}
        with pytest.raises(RuntimeError):
            _raw(mode, **kw, **outs)
        assert _untouched(outs), kw


def test_ops_refuses_an_unknown_mode_and_foreign_shapes():
    d = {k: v.to(DEV) for k, v in bc_ref.make_case(5, 3).items()}
    with pytest.raises(ValueError):
        ops.bc_fwd_bwd(d["loc"], d["sigma"], d["action"], mode="huber", global_batch=5)
    with pytest.raises(ValueError):
        ops.bc_fwd_bwd(d["loc"], d["sigma"], d["action"][:, :2].contiguous(), mode="mse", global_batch=5)
