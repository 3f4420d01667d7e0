"""The non-commuting Wasserstein projection (proj_type "w2_non_com", kernel code 4) on the GPU:
  (a) the kernel against the reference layer's own numbers (tier2f fixture): projection, trust-region loss and gradient, metrics;
  (b) the ten Newton-Schulz steps, not an exact square root, on the fixture's unconverged frame;
  (c) the whole fused loss (objective, entropy, trust region, critic) and its gradients against the float64 restatement
      (tests/w2nc_ref.py through the oracle's TRPL loss) on random batches at A = 3, 6, 12, 16;
  (d) five updates against the oracle with the restatement registered, rigid HEPi and two-agent EMPN;
  (e) recorded programs against the step-by-step loop (lanes, one stream, run_minibatches);
  (f) two data-parallel ranks against one rank; two runs bitwise identical."""
import pytest
import torch

import oracle_cases as oc
import trpl_cases as tc
import w2nc_ref
from oracle import trpl as otr
from geometry_rl_amd import synthetic as syn
from oracle_cases import M_TOL, V_TOL
from updater_cases import (DEV, assert_ranks_match, assert_two_runs_bitwise_identical, dp_ref, graph_modes_are_recorded, make_rollout,
                           moments_and_params_after, run_loop_and_launches, run_step_modes, run_two_ranks)

pytestmark = pytest.mark.gpu
EPS, EPS_COV = 0.05, 0.0025


@pytest.fixture
def registered(monkeypatch):
    monkeypatch.setitem(otr.PROJECTIONS, "w2_non_com", (w2nc_ref.projection, otr.wasserstein_value))


def _fixture(golden_dir, grp):
    return tc.projection_fixture(golden_dir, "tier2f_projection_w2_non_com.npz", grp)


# ------------------------------------------------------------------------------------------------------------- (a), (b) fixture
@pytest.mark.parametrize("grp", ["a6", "a3", "a12"])
def test_kernel_matches_the_reference_fixture(golden_dir, grp):
    from geometry_rl_amd import ops
    from geometry_rl_amd.trpl import WassersteinProjectionLayerNonCommuting
    z = _fixture(golden_dir, grp)
    B, A = z["mean"].shape
    layer = WassersteinProjectionLayerNonCommuting(mean_bound=z["mean_bound"], cov_bound=z["cov_bound"], trust_region_coeff=z["coeff"])
    mean, S = z["mean"].float().to(DEV), z["S"].float().to(DEV)
    q = (z["mean_o"].float().to(DEV), z["S_o"].float().to(DEV))
    pm, pS = layer(None, (mean, S.diag_embed()), (q[0], q[1].diag_embed()))
    assert pS.dim() == 3
    tc.rel_close("proj_mean", pm, z["proj_mean"], 1e-5)
    tc.rel_close("proj_S", pS.diagonal(dim1=-2, dim2=-1), z["proj_S"], 1e-5, floor=0.0)
    # the same launch through ops directly (proj_type=4, want_projection=True): proj_var is the projected "std" diagonal
    batch = {"action": mean, "loc": q[0], "var": q[1], "sample_log_prob": torch.zeros(B, device=DEV), "advantage": torch.zeros(B, device=DEV)}
    out = ops.trpl_fwd_bwd(mean, S.sqrt(), batch, None, mean_bound=z["mean_bound"], cov_bound=z["cov_bound"], trust_region_coeff=z["coeff"],
                           entropy_coef=0.0, critic_coef=0.0, clip_value=0.0, global_batch=B, adv_stats=None, want_projection=True, proj_type=4)
    assert torch.equal(out[5], pm) and torch.equal(out[6], pS.diagonal(dim1=-2, dim2=-1))
    # boundary methods: trust-region loss (value and gradient w.r.t. mean and S), metrics of (p, proj_p), trust_region_value
    m_g = mean.clone().requires_grad_(True)
    S_g = S.clone().requires_grad_(True)
    p_g = (m_g, S_g.diag_embed())
    tr = layer.get_trust_region_loss(None, p_g, (pm, pS))
    tr.backward()
    tc.rel_close("tr_loss", tr, z["tr_loss"], 1e-5)
    tc.rel_close("tr_grad_mean", m_g.grad, z["tr_grad_mean"], 2e-5, floor=0.0)
    tc.rel_close("tr_grad_S", S_g.grad, z["tr_grad_S"], 2e-5, floor=0.0)
    mt = layer.compute_metrics(None, (mean, S.diag_embed()), (pm, pS), step=0)
    for k in ("kl", "constraint", "mean_constraint", "cov_constraint", "mean_constraint_max", "cov_constraint_max", "entropy", "entropy_diff"):
        tc.rel_close("metric." + k, mt[k], z["metric." + k], 2e-5)
    vm, vc = layer.trust_region_value(None, (mean, S.diag_embed()), (q[0], q[1].diag_embed()))
    tc.rel_close("value_mean", vm, z["value_mean"], 1e-5)
    tc.rel_close("value_cov", vc, z["value_cov"], 1e-5)


def test_kernel_runs_the_ten_steps_not_an_exact_square_root(golden_dir):
    from geometry_rl_amd.trpl import WassersteinProjectionLayerNonCommuting
    z = _fixture(golden_dir, "a6")
    layer = WassersteinProjectionLayerNonCommuting(mean_bound=z["mean_bound"], cov_bound=z["cov_bound"], trust_region_coeff=z["coeff"])
    _, pS = layer(None, (z["mean"].float().to(DEV), z["S"].float().to(DEV)), (z["mean_o"].float().to(DEV), z["S_o"].float().to(DEV)))
    p64, q64 = (z["mean"], z["S"]), (z["mean_o"], z["S_o"])
    _, exact = w2nc_ref.projection(p64, q64, z["mean_bound"], z["cov_bound"], sqrt_fn=torch.sqrt)
    low = 1.0 - pS.cpu().double() / exact
    print("kernel below the exact square root: x/n = 1e-3:", float(low[3, 0]), " 1e-4:", float(low[4, 0]))
    assert abs(float(low[3, 0]) - 0.0243) < 1e-3 and abs(float(low[4, 0]) - 0.4706) < 2e-3
    assert abs(float(pS[3, 0]) / float(z["proj_S"][3, 0]) - 1.0) < 1e-5 and abs(float(pS[4, 0]) / float(z["proj_S"][4, 0]) - 1.0) < 1e-5


# ------------------------------------------------------------------------------------------------------------- (c) vs restatement
def _random_case(B, A, seed):
    """Frames on both sides of the bound: far outside, just outside (mp + cp in (eps + eps_cov, 1.2 (eps + eps_cov))), inside, in the
    band (eps, eps + eps_cov] that a bound on eps alone would project, and outside with one dimension of tiny x_i / n."""
    g = torch.Generator().manual_seed(seed)
    loc = torch.randn(B, A, generator=g, dtype=torch.float64)
    sigma = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    S = sigma ** 2
    old = loc + 0.4 * torch.randn(B, A, generator=g, dtype=torch.float64)
    S_o = S * (1 + 0.3 * torch.randn(B, A, generator=g, dtype=torch.float64)).abs().clamp_min(0.3)
    u = torch.randn(B, A, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    kind = torch.arange(B) % 6
    for b in range(B):
        k = int(kind[b])
        if k == 1:   # just outside: mean part only, 1.1 (eps + eps_cov)
            S_o[b] = S[b]
            old[b] = loc[b] + u[b] * S_o[b] * (1.1 * (EPS + EPS_COV)) ** 0.5
        elif k == 2:   # inside: small steps with distinct ratios
            S_o[b] = S[b] * (1 + 0.01 * u[b])
            old[b] = loc[b] + 0.05 * u[b] * S_o[b]
        elif k == 3:   # in the band (eps, eps + eps_cov]
            S_o[b] = S[b]
            old[b] = loc[b] + u[b] * S_o[b] * (EPS + 0.5 * EPS_COV) ** 0.5
        elif k == 4:   # an unconverged dimension: its old "std" small
            S_o[b, 0] = S_o[b, 0] * 0.02
    sigma, S_o, old, loc = sigma.float(), S_o.float(), old.float(), loc.float()
    var_f = S_o.double()
    action = (old.double() + var_f.sqrt() * torch.randn(B, A, generator=g, dtype=torch.float64)).float()
    logp = otr.mvn_diag_log_prob(action.double(), old.double(), var_f).float() + 0.1 * torch.randn(B, generator=g).float()
    batch = {"action": action, "loc": old, "var": S_o, "sample_log_prob": logp, "advantage": torch.randn(B, generator=g).float(),
             "state_value": torch.randn(B, generator=g).float(), "value_target": torch.randn(B, generator=g).float()}
    value = (batch["state_value"] + 0.3 * torch.randn(B, generator=g)).float()
    return loc, sigma, value, batch, kind


@pytest.mark.parametrize("A", [3, 6, 12, 16])
def test_kernel_matches_the_restatement(registered, A):
    from geometry_rl_amd import ops
    B = 6 * 11 + 5   # not a multiple of the 16 frames per workgroup
    loc, sigma, value, batch, kind = _random_case(B, A, seed=100 + A)
    kw = dict(mean_bound=EPS, cov_bound=EPS_COV, trust_region_coeff=1.7, entropy_coef=0.01, critic_coef=0.5, clip_value=0.2)
    loc_r = loc.double().requires_grad_(True)
    sig_r = sigma.double().requires_grad_(True)
    val_r = value.double().requires_grad_(True)
    bd = {k: v.double() for k, v in batch.items()}
    ref = otr.trpl_loss(loc_r, sig_r ** 2, bd, val_r, proj_type="w2_non_com", **kw)
    d_loc, d_sig = torch.autograd.grad(ref["loss_objective"] + ref["loss_entropy"] + ref["loss_trust_region"], [loc_r, sig_r])
    (d_val,) = torch.autograd.grad(ref["loss_critic"], [val_r])
    # the cases are where they are meant to be
    mp, cp = w2nc_ref.value((loc.double(), sigma.double() ** 2), (bd["loc"], bd["var"]))
    tot = mp + cp
    assert bool((tot[kind == 2] < EPS).all()) and bool((tot[kind == 1] > EPS + EPS_COV).all())
    assert bool(((tot[kind == 3] > EPS) & (tot[kind == 3] <= EPS + EPS_COV)).all())
    r = w2nc_ref.x_over_n((loc.double(), sigma.double() ** 2), (bd["loc"], bd["var"]), EPS, EPS_COV)
    assert float(r[kind == 4].min(-1).values.max()) < 2e-3
    db = {k: v.to(DEV) for k, v in batch.items()}
    sums, maxes, dloc, dsigma, dvalue, pm, pv = ops.trpl_fwd_bwd(loc.to(DEV), sigma.to(DEV), db, value.to(DEV), global_batch=B, adv_stats=None,
                                                                 want_projection=True, proj_type=4, adv_local=True, **kw)
    tc.rel_close("proj_mean", pm, ref["proj_mean"], 1e-5)
    tc.rel_close("proj_S", pv, ref["proj_S"], 1e-5, floor=0.0)
    s = sums.cpu()
    n = float(s[10])
    assert n == B
    mx = maxes.cpu().view(torch.float32)
    got = {"loss_objective": s[0] / n, "loss_trust_region": s[1] / n, "loss_critic": s[3] / n, "ESS": s[4] ** 2 / s[5] / n, "kl": s[11] / n,
           "mean_constraint": s[6] / n, "cov_constraint": s[7] / n, "entropy": s[8] / n, "entropy_diff": s[9] / n,
           "mean_constraint_max": mx[0], "cov_constraint_max": mx[1]}
    for k, v in got.items():
        want = float(ref[k])
        assert abs(float(v) - want) <= 1e-5 * max(1.0, abs(want)), (k, float(v), want)
    tc.rel_close("dloc", dloc, d_loc, 1e-5, floor=0.0)
    tc.rel_close("dsigma", dsigma, d_sig, 1e-5, floor=0.0)
    tc.rel_close("dvalue", dvalue, d_val, 1e-5, floor=0.0)
    # per frame, so that one kind of frame cannot hide behind the largest gradient of another
    for k in range(6):
        sel = kind == k
        tc.rel_close(f"dsigma[kind {k}]", dsigma.cpu()[sel], d_sig[sel], 2e-5, floor=0.0)
        tc.rel_close(f"dloc[kind {k}]", dloc.cpu()[sel], d_loc[sel], 2e-5, floor=0.0)


# ------------------------------------------------------------------------------------------------------------- (d) vs oracle
@pytest.mark.parametrize("name,B,K", [("rigid_g1", 64, 5), ("empn_g2", 32, 5)])
def test_five_updates_match_the_oracle(registered, name, B, K):
    from geometry_rl_amd import agent
    oc.cap_oracle_threads()
    kw = dict(proj_type="w2_non_com", trust_region_coeff=2.0)
    pair = oc.build_pair(name, B, seed=21, o_kw=kw, d_kw=kw)
    spec, cfg, loss = pair.spec, pair.cfg, pair.loss
    assert pair.proj.proj_code == 4
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batches = []
    for i in range(K):
        b = dict(oc.obs_of(name, B, 30 + i))
        b.update(syn.make_ppo_fields(B, A, seed=40 + i))
        batches.append(b)
    oc.adopt_calibration(pair, batches[0])
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=True)

    def per_step(i, out, ref):
        assert float(ref["kl"]) > 0.0   # frames were projected
        for k in ("loss_objective", "loss_trust_region", "loss_critic", "kl", "constraint", "mean_constraint", "cov_constraint", "entropy"):
            e = abs(float(out[k]) - float(ref[k]))
            assert e <= 1e-4 * max(1.0, abs(float(ref[k]))), (i, k, e)
    g_scale = oc.run_updates(pair, batches, upd, per_step)
    assert upd.mode.startswith("graph") and upd._program is not None
    bad, _ = moments_and_params_after(upd, pair.actor, pair.critic, pair.oracle, cfg, g_scale, K, M_TOL, V_TOL)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- (e) programs
KEYS = ("loss_objective", "loss_trust_region", "loss_critic", "kl", "constraint", "entropy", "ESS")


@pytest.mark.parametrize("form", ["unrolled"])
def test_run_minibatches_equals_the_step_loop(form):
    N, T = 8, 10
    res = run_loop_and_launches(lambda: make_rollout(N, T, seed=33, proj_type="w2_non_com"), form, N=N, T=T, ppo_epochs=2, driver_seed=9,
                                unroll=4, keys=KEYS)
    for a, b in zip(res["loop"][:3], res["launches"][:3]):
        assert torch.equal(a, b), (a - b).abs().max().item()
    for k in KEYS:
        assert torch.equal(res["loop"][3][-1][k], res["launches"][3][-1][k]), k


def test_recorded_programs_equal_the_eager_loop():
    res = run_step_modes(lambda: make_rollout(8, 2, seed=41, proj_type="w2_non_com"), ("eager", "graph", "one_stream", "one_stream_eager"), 4,
                         KEYS, lambda mode: dict(use_graph=mode in ("graph", "one_stream"), overlap_critic=not mode.startswith("one_stream")),
                         per_mode=graph_modes_are_recorded)
    for a, b in (("eager", "graph"), ("one_stream_eager", "one_stream")):
        for x, y in zip(res[a][:3], res[b][:3]):
            assert torch.equal(x, y), (a, b, (x - y).abs().max().item())
        for oa, ob in zip(res[a][3], res[b][3]):
            for kk in KEYS:
                assert torch.equal(oa[kk], ob[kk]), (a, b, kk)
    assert (res["graph"][0] - res["one_stream"][0]).abs().max().item() <= 1e-6


def test_two_runs_are_bitwise_identical():
    assert_two_runs_bitwise_identical(KEYS, proj_type="w2_non_com")


# ------------------------------------------------------------------------------------------------------------- (f) data parallel
def test_two_ranks_match_single_rank():
    world = 2
    ref_losses, ref_flat, ret = run_two_ranks(dp_ref(16, cfg_kw=dict(proj_type="w2_non_com")), world, use_graph=True, dp_use_graph=True,
                                              n_steps=3, keys=KEYS, updater_kw=dict(clip_grad_norm=False))
    assert_ranks_match(ref_losses, ref_flat, ret, world, 1e-5, 2e-6)
