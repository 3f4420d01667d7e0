"""The behaviour-cloning update (geometry_rl_amd.bc: BCLoss, BCUpdater) against the CPU oracle on identical, oracle-calibrated parameters
and inputs.  The oracle side is composed here from the oracle's actor (``pair.oracle.actor_forward``), the objective with autograd --
``nn.MSELoss`` of the mean, or ``-Independent(Normal(loc, std), 1).log_prob(action).mean()`` -- and ``torch.optim.Adam(actor leaves,
lr=5e-4)`` with torch's defaults (behavior_cloning.py:96-101,113-123).  Rules of tests/test_gpu_step.py and test_gpu_multistep_oracle.py:
values to 1e-4 (oracle_cases.TOL), every gradient tensor to 2e-4 of its own largest reference entry, the parameters after Adam's first step
to what that implies (parity_util, with THIS optimizer's lr = 5e-4 and eps = 1e-8), the moments after three updates to M_TOL / V_TOL."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import oracle_cases as oc
from geometry_rl_amd import synthetic as syn
from oracle_cases import M_TOL, V_TOL, check
from parity_util import adam_first_step_bound, adam_first_step_bound_elem, grad_error, grad_scales, param_excess
from updater_cases import merge_grad_scales, moments_and_params_after

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LR, EPS = 5e-4, 1e-8   # behavior_cloning.py:96-99: torch.optim.Adam(lr=5e-4), default eps


def oracle_objective(oracle, batch, objective):
    """-> the oracle's values of BCLoss's keys (``loss_bc`` carries the graph), loc and var."""
    from torch.distributions import Independent, Normal
    b = {k: v.to(oracle.dtype) if v.is_floating_point() else v for k, v in batch.items()}
    loc, var = oracle.actor_forward({k: b[k] for k in oracle.spec.in_features})
    dist = Independent(Normal(loc, var.sqrt()), 1)
    mse = torch.nn.MSELoss()(loc, b["action"])
    nll = -dist.log_prob(b["action"]).mean()
    return {"loss_bc": mse if objective == "mse" else nll, "mse": mse.detach(), "nll": nll.detach(), "entropy": dist.entropy().mean().detach(),
            "max_sq_err": ((loc - b["action"]) ** 2).sum(-1).max().detach(), "loc": loc.detach(), "var": var.detach()}


def oracle_update(oracle, optim, batch, objective, clip, max_norm):
    """One update of the oracle's actor: backward, optional clip_grad_norm_, Adam -> (values, {"actor": gradients before clipping, "critic": {}})"""
    out = oracle_objective(oracle, batch, objective)
    out["loss_bc"].backward()
    grads = {"actor": {k: v.grad.clone() for k, v in oracle.actor.items() if v.grad is not None}, "critic": {}}
    if clip:
        torch.nn.utils.clip_grad_norm_(oracle._actor_leaves(), max_norm)
    optim.step()
    optim.zero_grad()
    return {k: v.detach() for k, v in out.items()}, grads


def _batch(name, B, spec, cfg, obs, seed):
    A = spec.num_actuators * cfg.output_dim_vec * 3
    b = dict(obs)
    b["action"] = syn.make_ppo_fields(B, A, seed=seed)["action"]
    return b


@pytest.mark.parametrize("objective", ["mse", "nll"])
@pytest.mark.parametrize("name,B", [("rigid_tiny", 6), ("cloth", 4), ("empn_g2", 4), ("rope", 4)])
def test_one_update(name, B, objective):
    from geometry_rl_amd import bc
    oc.cap_oracle_threads()
    o_spec, spec, kw, obs = oc.make_case(name, B)
    pair = oc.build_pair((o_spec, spec, kw), seed=11)
    cfg, oracle, actor = pair.cfg, pair.oracle, pair.actor
    batch = _batch(name, B, spec, cfg, obs, seed=B)
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    oc.adopt_calibration(pair, batch)   # both sides continue from bit-identical, oracle-calibrated weights
    optim = torch.optim.Adam(oracle._actor_leaves(), lr=LR)
    loss = bc.BCLoss(actor, objective=objective)
    upd = bc.BCUpdater(loss, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=False)
    assert (upd.lr, upd.eps, upd.betas) == (LR, EPS, (0.9, 0.999))
    before = {k: p.detach().clone() for k, p in actor.named_parameters()}
    ref, ref_grads = oracle_update(oracle, optim, batch, objective, cfg.clip_grad_norm, cfg.max_grad_norm)

    # --- the eager loss module: values and, through autograd, the gradients (the parameters are untouched so far)
    upd.gflat.zero_()
    out = loss(dbatch)
    out["loss_bc"].backward()
    check("loc", out["loc"], ref["loc"])
    check("var", out["sigma"] ** 2, ref["var"])
    for k in loss.out_keys:
        check(k, out[k], ref[k])
    bad, scales = oc.gradients_off_scale(actor, pair.critic, ref_grads, nets=("actor",))
    assert not bad, bad
    std_head = [k for k, _ in actor.named_parameters() if k.startswith("_pre_std.")]
    assert std_head
    if objective == "mse":   # the std takes no part: torch hands the oracle no gradient, the kernel writes zeros
        for k, p in actor.named_parameters():
            if k in std_head:
                assert k not in ref_grads["actor"] and not bool(p.grad.any()), k

    # --- the real step from the same starting point
    rep = upd.step(dbatch)
    for k in loss.out_keys:
        check("step " + k, rep[k], ref[k])
    wrong = []
    for k, p in actor.named_parameters():
        p_ref = oracle.actor[k]
        if cfg.clip_grad_norm or k not in ref_grads["actor"]:
            allowed = adam_first_step_bound(LR, EPS, scales["actor"].get(k, 0.0), clip=cfg.clip_grad_norm, p_ref=p_ref)
        else:
            allowed = adam_first_step_bound_elem(LR, EPS, ref_grads["actor"][k], scales["actor"][k], p_ref=p_ref)
        e, x = grad_error(p, p_ref), param_excess(p, p_ref, allowed)
        print(f"param {k}: err {e:.3e} = {x:.2f} of allowed")
        if not (np.isfinite(x) and x <= 1.0):
            wrong.append((k, e, x))
    assert not wrong, wrong
    if objective == "mse":   # Adam on a zero gradient with zero moments moves nothing: bitwise unchanged, as the parameter torch skipped
        for k, p in actor.named_parameters():
            if k in std_head:
                assert torch.equal(p.detach(), before[k]) and torch.equal(oracle.actor[k].detach(), before[k].cpu()), k


def test_three_updates_nll_cloth():
    """Moments after three updates on three minibatches (from the second on the update depends on the RATIO of accumulated gradients); the
    third step is the recorded one.  The demonstrations are ONE expert's: the calibrated initial policy's own mean shifted by 0.5 in every
    dimension, so consecutive minibatches pull the same way, as recorded demonstrations do -- the moments then accumulate and their scale
    is the gradients' (independent random targets per minibatch would make the three gradients cancel in exp_avg, whose own largest entry is
    what M_TOL is a fraction of).  Every step's gradient error is printed as a fraction of its tensor's scale."""
    from geometry_rl_amd import bc
    oc.cap_oracle_threads()
    name, B, K = "cloth", 4, 3
    pair = oc.build_pair(name, B, seed=21)
    spec, cfg, oracle = pair.spec, pair.cfg, pair.oracle
    batches = [_batch(name, B, spec, cfg, oc.obs_of(name, B, 30 + i), seed=40 + i) for i in range(K)]
    oc.adopt_calibration(pair, batches[0])
    with torch.no_grad():
        for b in batches:
            b["action"] = (oracle.actor_forward({k: b[k] for k in pair.o_spec.in_features})[0] + 0.5).float()
    oracle.actor_optim = torch.optim.Adam(oracle._actor_leaves(), lr=LR)   # (moments_and_params_after reads the optimizer from the oracle)
    upd = bc.BCUpdater(bc.BCLoss(pair.actor, objective="nll"), use_graph=True)
    g_scale = None
    for i, b in enumerate(batches):
        ref, ref_grads = oracle_update(oracle, oracle.actor_optim, b, "nll", False, 1.0)
        out = upd.step({k: v.to(DEV) for k, v in b.items()})
        g_scale = merge_grad_scales(g_scale, ref_grads)
        sc = grad_scales(ref_grads["actor"])   # (overwrite mode, nothing clipped: the flat gradient still holds this step's)
        frac = max(grad_error(p.grad, ref_grads["actor"][k]) / sc[k] for k, p in pair.actor.named_parameters() if k in ref_grads["actor"])
        print(f"update {i}: worst gradient error {frac:.2e} of its tensor's scale")
        for k in ("loss_bc", "mse", "nll"):   # the trajectories stay together step by step
            e = abs(float(out[k]) - float(ref[k]))
            assert e <= 1e-4 * max(1.0, abs(float(ref[k]))), (i, k, e)
    assert upd.mode == "graph" and B in upd._programs
    bad, worst = moments_and_params_after(upd, pair.actor, pair.critic, oracle, replace(pair.o_cfg, lr=LR), g_scale, K, M_TOL, V_TOL)
    # (its parameter rule is written for the RL loop's eps = 1e-5; the moments are what is asserted here)
    assert worst["exp_avg"] <= M_TOL and worst["exp_avg_sq"] <= V_TOL and np.isfinite(worst["exp_avg"] + worst["exp_avg_sq"]), (worst, bad)
