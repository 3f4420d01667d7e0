"""The fused TRPL / PPO loss kernel (trpl_lanes_kernel<L, PROJ>, head_ops.hip) and the rollout sampler (gaussian_sample_kernel) per op,
against float64 references on the same fp32 inputs (tests/trpl_cases.py: the oracle's TRPL loss, tests/ppo_ref.py, tests/w2nc_ref.py),
at fp32 output resolution:
  * fp64 sums: 1e-9 relative, plus 1e-11 per frame absolute; the count exact;
  * fp32 tensors: 4 fp32 ulp relative per element, plus 1e-6 of the largest |ref| of the element's frame (1-D tensors: of the tensor),
    plus 1e-10 of the tensor's largest |ref| (fp64 cancellation, see trpl_cases.CANCEL);
  * where the advantages are normalised, plus trpl_cases.adv_error_bound (the one-pass variance s1 - n m^2) times the output's
    sensitivity to the normalised advantages.
Axes: lane width and padding (A = 1 .. 16 at B = 37, every projection), batch and fold edges (B = 1 .. 4097), the eight per-frame
regimes of trpl_cases.REGIMES inside every workgroup, the options (trust region / entropy off, no critic, clip 0 / 0.2 / 0.25 exactly on
the edge, advantage statistics in-kernel / grl_adv_stats / a data-parallel shard / none, constant, sub-floor and offset advantages),
grl_trpl_target_terms, the PPO mode, the report path (grl_trpl_report, grl_trpl_loss_values, the deferred fold bitwise equal to the
direct one), host-side rejection of A outside 1 .. 16, and the sampler with its cross-check through the loss kernel."""
import ctypes

import pytest
import torch

import trpl_cases as tc
from geometry_rl_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _launch(c, d, defer=False):
    db = {k: v.to(DEV) for k, v in d["batch"].items()}
    adv_stats = None
    if c.adv_mode == "kernel_stats":
        adv_stats = torch.empty(2, device=DEV, dtype=torch.float64)
        hip.call("grl_adv_stats", db["advantage"].contiguous(), adv_stats, c.B)
    elif c.adv_mode == "shard":   # the global batch's statistics, as the all-reduced grl_adv_stats of the data-parallel ranks
        a = d["adv_global"].double()
        adv_stats = torch.tensor([float(a.sum()), float((a * a).sum())], dtype=torch.float64, device=DEV)
    return ops.trpl_fwd_bwd(d["loc"].to(DEV), d["sigma"].to(DEV), db, d["value"].to(DEV) if c.value else None, mean_bound=tc.EPS,
                            cov_bound=tc.EPS_COV, trust_region_coeff=c.tr_coeff, entropy_coef=c.ent_coef, critic_coef=c.critic_coef,
                            clip_value=c.clip_value, global_batch=c.global_batch, adv_stats=adv_stats, want_projection=True,
                            proj_type=c.proj, defer_fold=defer, adv_local=c.adv_mode == "local")


def _check_case(c):
    d = tc.make_case(c)
    ref = tc.reference(c, d)
    kap = tc.adv_error_bound(c, d)
    print(f"{c.name}: adv bound {kap:.2e}")
    sums, maxes, dloc, dsigma, dvalue, pm, pv = _launch(c, d)
    fold, maxes_d, dloc_d, dsigma_d, dvalue_d, pm_d, pv_d = _launch(c, d, defer=True)
    tc.launch_close((sums, maxes, dloc, dsigma, dvalue, pm, pv), ref, c.B, kap, value=c.value)
    # the report path: the deferred launch's slots through grl_trpl_report, the direct sums through grl_trpl_loss_values
    sums_r = torch.empty(12, device=DEV, dtype=torch.float64)
    maxes_r = torch.empty(2, device=DEV, dtype=torch.int32)
    out_r = torch.empty(14, device=DEV, dtype=torch.float32)
    out_v = torch.empty(14, device=DEV, dtype=torch.float32)
    hip.call("grl_trpl_report", fold.slots, c.B, sums_r, maxes_r, float(c.ent_coef), out_r)
    hip.call("grl_trpl_loss_values", sums, maxes, float(c.ent_coef), out_v)
    sums_f, maxes_f = fold()
    for a_, b_ in ((sums_r, sums), (maxes_r, maxes), (sums_f, sums), (maxes_f, maxes), (dloc_d, dloc), (dsigma_d, dsigma), (pm_d, pm),
                   (pv_d, pv)):
        assert torch.equal(a_, b_)
    if c.value:
        assert torch.equal(dvalue_d, dvalue)
    kap_obj = kap * float(ref["sens_sums"][0]) / c.B
    tc.report_close("report", out_r, ref["report"], kap_obj)
    tc.report_close("loss_values", out_v, ref["report"], kap_obj)


@pytest.mark.parametrize("c", tc.lane_cases(), ids=lambda c: c.name)
def test_lane_widths_and_padding(c):
    _check_case(c)


@pytest.mark.parametrize("c", tc.batch_cases(), ids=lambda c: c.name)
def test_batch_and_fold_edges(c):
    _check_case(c)


@pytest.mark.parametrize("c", tc.option_cases(), ids=lambda c: c.name)
def test_options(c):
    _check_case(c)


@pytest.mark.parametrize("proj", (0, 1, 2))
@pytest.mark.parametrize("A", tc.A_SWEEP)
def test_target_terms(A, proj):
    c = tc.Case(B=37, A=A, proj=proj)
    d = tc.make_case(c)
    ref = tc.target_reference(c, d)
    sums, maxes, dloc, dsigma = ops.trpl_target_terms(d["loc"].to(DEV), d["sigma"].to(DEV), d["batch"]["loc"].to(DEV),
                                                      d["batch"]["var"].to(DEV), mean_bound=tc.EPS, cov_bound=tc.EPS_COV,
                                                      trust_region_coeff=c.tr_coeff, global_batch=c.B, proj_type=proj)
    s = sums.cpu()
    assert float(s[10]) == c.B
    for k, want in ref["sums"].items():
        allowed = tc.RTOL64 * abs(want) + tc.ATOL64 * c.B
        assert abs(float(s[k]) - want) <= allowed, (k, float(s[k]), want)
    tc.maxes_close("maxes", maxes, ref["maxes"])
    tc.close("dloc", dloc, ref["dloc"])
    tc.close("dsigma", dsigma, ref["dsigma"])


@pytest.mark.parametrize("B,A", tc.PPO_GRID)
def test_ppo_mode(B, A):
    d = tc.make_ppo_case(B, A)
    kw = dict(ent_coef=0.015625, critic_coef=0.5, clip_value=0.2)
    ref = tc.ppo_reference(d, **kw)
    ce = torch.tensor(tc.PPO_EPS, dtype=torch.float32, device=DEV)
    db = {k: v.to(DEV) for k, v in d["batch"].items()}
    sums, maxes, dloc, dsigma, dvalue = ops.ppo_fwd_bwd(d["loc"].to(DEV), d["sigma"].to(DEV), db, d["value"].to(DEV), clip_epsilon=ce,
                                                        entropy_coef=kw["ent_coef"], critic_coef=kw["critic_coef"],
                                                        clip_value=kw["clip_value"], global_batch=B, adv_stats=None, adv_local=True)
    print(f"PPO B={B} A={A}")
    tc.sums_close("sums", sums, ref["sums"], B)
    for col in (1, 6, 7, 9, 11):
        assert float(sums[col]) == 0.0, col
    assert maxes.cpu().tolist() == [0, 0]
    tc.close("dloc", dloc, ref["dloc"])
    tc.close("dsigma", dsigma, ref["dsigma"])
    tc.close("dvalue", dvalue, ref["dvalue"])
    lo, hi = tc.ppo_bounds()
    lw, a = ref["lw"], ref["adv_n"]
    zero = ((lw > hi) & (a > 0)) | ((lw < lo) & (a < 0))   # the clipped side wins: no objective gradient, and loc has no entropy term
    assert bool((dloc.cpu()[zero] == 0).all())


@pytest.mark.parametrize("A", [0, 17])
def test_host_rejects_action_widths_outside_1_to_16(A):
    """A = 0 and A = 17 make every entry point of the kernel return an error before anything is launched: the outputs keep their
    sentinels.  (The buffers are sized for 17 columns, so nothing could be written out of bounds either way.)"""
    B, W = 5, 17
    f = lambda *s: torch.ones(*s, device=DEV)
    loc, sigma, act, om, ov = f(B, W), f(B, W), f(B, W), f(B, W), f(B, W)
    logp, adv = f(B), f(B)
    outs = {"dloc": torch.full((B, W), 7.0, device=DEV), "dsigma": torch.full((B, W), 7.0, device=DEV),
            "sums": torch.full((12,), 7.0, device=DEV, dtype=torch.float64), "maxes": torch.full((2,), 7, device=DEV, dtype=torch.int32),
            "slots": torch.full((hip.query("grl_trpl_slot_doubles", B),), 7.0, device=DEV, dtype=torch.float64)}
    o = outs
    cfg = (ctypes.c_double * 10)(tc.EPS, tc.EPS_COV, 1.0, 0.0, 0.0, 0.0, 1.0 / B, float(B), 0.0, 1.0)
    with pytest.raises(RuntimeError):
        hip.call("grl_trpl_fwd_bwd", cfg, A, loc, sigma, act, om, ov, logp, adv, None, None, None, o["dloc"], o["dsigma"], None, None,
                 None, None, o["sums"], o["maxes"], o["slots"], B)
    cfg6 = (ctypes.c_double * 6)(0.0, 0.0, 0.0, 1.0 / B, float(B), 1.0)
    ce = torch.tensor(0.2, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        hip.call("grl_ppo_fwd_bwd", cfg6, ce, A, loc, sigma, act, logp, adv, None, None, None, o["dloc"], o["dsigma"], None, None,
                 o["sums"], o["maxes"], o["slots"], B)
    with pytest.raises(RuntimeError):
        hip.call("grl_trpl_target_terms", cfg, A, loc, sigma, om, ov, o["dloc"], o["dsigma"], o["sums"], o["maxes"], o["slots"],
                 torch.zeros(B, device=DEV), B)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 7).all()), k


# ------------------------------------------------------------------------------------------------------------- sampler
def _sample(loc, sigma, eps):
    B, A = loc.shape
    action, var = torch.empty_like(loc), torch.empty_like(loc)
    logp = torch.empty(B, device=DEV, dtype=torch.float32)
    hip.call("grl_gaussian_sample", loc.contiguous(), sigma.contiguous(), eps.contiguous(), action, logp, var, B, A)
    return action, var, logp


@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("A", [1, 3, 16])
def test_gaussian_sample(A, B):
    g = torch.Generator().manual_seed(70 + A + B)
    loc = torch.randn(B, A, generator=g)
    sigma = torch.rand(B, A, generator=g) * 1.7 + 0.3
    eps = torch.randn(B, A, generator=g)
    action, var, logp = _sample(loc.to(DEV), sigma.to(DEV), eps.to(DEV))
    a_ref, v_ref, lp_ref, bound = tc.sample_reference(loc, sigma, eps, action.cpu())
    ea = (action.cpu().double() - a_ref).abs()
    ev = (var.cpu().double() - v_ref).abs()
    el = (logp.cpu().double() - lp_ref).abs()
    print(f"A={A} B={B}: action {float((ea / a_ref.abs()).max()):.2e} rel, var {float((ev / v_ref).max()):.2e} rel, "
          f"logp {float(el.max()):.2e} (bound {float(bound.min()):.2e} .. {float(bound.max()):.2e})")
    assert bool((ea <= 2 * tc.U32 * a_ref.abs() + 1e-30).all())
    assert bool((ev <= 2 * tc.U32 * v_ref).all())
    assert bool((el <= bound).all())


def test_sample_then_loss_with_p_equal_q():
    """Sample a batch, then run the loss on it with p == q (sigma^2 exact in fp32): every log-ratio is 0 up to the fp32 rounding of the
    sampler's log-prob, so sum_w and sum_w2 equal B within that rounding, the constraints are 0 and the reported ESS is 1."""
    B, A = 257, 7
    g = torch.Generator().manual_seed(3)
    loc = torch.randn(B, A, generator=g)
    sigma = (torch.randint(64, 192, (B, A), generator=g).float() / 128.0)
    eps = torch.randn(B, A, generator=g)
    action, var, logp = _sample(loc.to(DEV), sigma.to(DEV), eps.to(DEV))
    assert torch.equal(var.cpu().double(), sigma.double() ** 2)
    _, _, lp_ref, bound = tc.sample_reference(loc, sigma, eps, action.cpu())
    batch = {"action": action, "loc": loc.to(DEV), "var": var, "sample_log_prob": logp, "advantage": torch.randn(B, generator=g).to(DEV)}
    fold, _, dloc, dsigma, _, pm, pv = ops.trpl_fwd_bwd(loc.to(DEV), sigma.to(DEV), batch, None, mean_bound=tc.EPS, cov_bound=tc.EPS_COV,
                                                        trust_region_coeff=1.5, entropy_coef=0.0, critic_coef=0.0, clip_value=0.0,
                                                        global_batch=B, adv_stats=None, want_projection=True, proj_type=0, defer_fold=True,
                                                        adv_local=True)
    sums = torch.empty(12, device=DEV, dtype=torch.float64)
    maxes = torch.empty(2, device=DEV, dtype=torch.int32)
    out = torch.empty(14, device=DEV, dtype=torch.float32)
    hip.call("grl_trpl_report", fold.slots, B, sums, maxes, 0.0, out)
    s = sums.cpu()
    b = bound.double() + 1e-13
    tol_w, tol_w2 = float((b.exp() - 1).sum()), float(((2 * b).exp() - 1).sum())
    print(f"sum_w - B {float(s[4]) - B:.3e} (allowed {tol_w:.3e}), sum_w2 - B {float(s[5]) - B:.3e} (allowed {tol_w2:.3e}), "
          f"ESS {float(out[4])!r}")
    assert abs(float(s[4]) - B) <= tol_w and abs(float(s[5]) - B) <= tol_w2
    # constraints 0: the mean part exactly, the KL covariance part up to fp64 rounding (eta = 0 gives v = 1 / (1 / t), not t bitwise)
    assert float(s[6]) == 0.0 and abs(float(s[7])) <= 1e-12 * B and abs(float(s[11])) <= 1e-12 * B
    assert maxes.cpu().view(torch.float32).abs().max() <= 1e-12
    assert torch.equal(pm.cpu(), loc)
    tc.close("proj_S", pv, var.cpu())
    assert abs(float(out[4]) - 1.0) <= 2 * tc.U32
