"""The clipped PPO objective (geometry_rl_amd.ppo.ClipPPOLoss2, grl_ppo_fwd_bwd) on the GPU:
  (a) the kernel against the float64 restatement (tests/ppo_ref.py), frames on both sides of both bounds with both advantage signs;
  (b) five consecutive PolicyUpdater updates against the PPO oracle (clip_grad_norm, objective/default.yaml), recorded from the third on;
  (c) the recorded programs against the step-by-step loop (lanes, one stream, run_minibatches in its multi-step forms);
  (d) an annealed clip epsilon written in place takes effect at the next replay without recording again;
  (e) two data-parallel ranks against one rank on the whole batch;
  (f) the reference loop protocol (loss_module(td), two backward passes, two Adam steps) against PolicyUpdater.step."""
import math

import pytest
import torch

import oracle_cases as oc
from geometry_rl_amd import synthetic as syn
from oracle_cases import M_TOL, V_TOL
from ppo_ref import PPOOracleAgent, ppo_loss
from updater_cases import (DEV, assert_ranks_match, dp_ref, make_rollout, moments_and_params_after, run_loop_and_launches, run_step_modes,
                           run_two_ranks)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- (a) kernel
@pytest.mark.parametrize("A", [6, 12])
def test_kernel_matches_the_restatement(A):
    from geometry_rl_amd import ops
    eps = 0.2
    lo, hi = math.log1p(-eps), math.log1p(eps)
    g = torch.Generator().manual_seed(11 + A)
    regions = torch.tensor([lo - 0.6, lo - 0.05, 0.5 * lo, 0.0, 0.5 * hi, hi + 0.05, hi + 0.6], dtype=torch.float64)
    B = 7 * 12 + 5   # not a multiple of the 16 frames per workgroup
    lw_t = regions.repeat(13)[:B] + 0.01 * (torch.rand(B, generator=g, dtype=torch.float64) - 0.5)   # >= 0.04 from either bound
    loc = torch.randn(B, A, generator=g).float()
    sigma = (torch.rand(B, A, generator=g) + 0.4).float()
    action = (loc.double() + sigma.double() * torch.randn(B, A, generator=g, dtype=torch.float64)).float()
    var = sigma.double() ** 2
    from oracle import trpl as otr
    logp = (otr.mvn_diag_log_prob(action.double(), loc.double(), var) - lw_t).float()
    adv = torch.randn(B, generator=g).float()
    batch = {"action": action, "sample_log_prob": logp, "advantage": adv, "state_value": torch.randn(B, generator=g).float(),
             "value_target": torch.randn(B, generator=g).float()}
    value = (batch["state_value"] + 0.4 * torch.randn(B, generator=g)).float()
    ent_coef, critic_coef, clip_value = 0.01, 0.5, 0.2
    # reference (float64 autograd on the float32 inputs)
    loc_r = loc.double().requires_grad_(True)
    sig_r = sigma.double().requires_grad_(True)
    val_r = value.double().requires_grad_(True)
    bd = {k: v.double() for k, v in batch.items()}
    ref = ppo_loss(loc_r, sig_r ** 2, bd, val_r, clip_epsilon=eps, entropy_coef=ent_coef, critic_coef=critic_coef, clip_value=clip_value)
    d_loc, d_sig = torch.autograd.grad(ref["loss_objective"] + ref["loss_entropy"], [loc_r, sig_r])
    (d_val,) = torch.autograd.grad(ref["loss_critic"], [val_r])
    lw = ref["lw"]
    assert bool(((lw - lo).abs() > 0.03).all() and ((lw - hi).abs() > 0.03).all())
    a_n = (adv.double() - adv.double().mean()) / adv.double().std()
    for side in ((lw > hi) & (a_n > 0), (lw < lo) & (a_n < 0), (lw > hi) & (a_n < 0), (lw < lo) & (a_n > 0), (lw > lo) & (lw < hi)):
        assert int(side.sum()) >= 3   # every region is populated
    # kernel
    ce = torch.tensor(eps, dtype=torch.float32, device=DEV)
    db = {k: v.to(DEV) for k, v in batch.items()}
    sums, maxes, dloc, dsigma, dvalue = ops.ppo_fwd_bwd(loc.to(DEV), sigma.to(DEV), db, value.to(DEV), clip_epsilon=ce, entropy_coef=ent_coef,
                                                        critic_coef=critic_coef, clip_value=clip_value, global_batch=B, adv_stats=None,
                                                        adv_local=True)
    s = sums.cpu()
    n = float(s[10])
    assert n == B
    got = {"loss_objective": float(s[0]) / n, "entropy": float(s[2]) / n, "entropy_col8": float(s[8]) / n,
           "loss_critic": float(s[3]) / n, "ESS": float(s[4] ** 2 / s[5]) / n}
    want = {"loss_objective": float(ref["loss_objective"]), "entropy": float(ref["entropy"]), "entropy_col8": float(ref["entropy"]),
            "loss_critic": float(ref["loss_critic"]), "ESS": float(ref["ESS"])}
    for k in got:
        assert abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, got[k], want[k])
    for col in (1, 6, 7, 9, 11):   # trust-region / KL columns stay zero
        assert float(s[col]) == 0.0, col
    for name, a, b in (("dloc", dloc, d_loc), ("dsigma", dsigma, d_sig), ("dvalue", dvalue, d_val)):
        a = a.cpu().double()
        err = float((a - b).abs().max())
        scale = float(b.abs().max())
        print(f"A={A} {name}: max err {err:.3e} of scale {scale:.3e}")
        assert err <= 1e-5 * scale, (name, err, scale)
    zero = ((lw > hi) & (a_n > 0)) | ((lw < lo) & (a_n < 0))
    assert bool((dloc.cpu()[zero] == 0).all())   # the clipped side wins: no objective gradient (and loc has no entropy term)
    assert bool((dloc.cpu()[~zero].abs().sum(-1) > 0).all())


# ------------------------------------------------------------------------------------------------------------- (b) vs oracle
PPO_KW = dict(algorithm="ppo", clip_epsilon=0.2, critic_coef=1.0, clip_value=0.2, clip_grad_norm=True, max_grad_norm=1.0)   # objective/default.yaml


@pytest.mark.parametrize("name,B,K", [("rigid_g1", 64, 5), ("cloth", 16, 5), ("empn_g2", 32, 5)])
def test_five_updates_match_the_ppo_oracle(name, B, K):
    from geometry_rl_amd import agent
    oc.cap_oracle_threads()
    pair = oc.build_pair(name, B, seed=21, o_kw=dict(critic_coef=1.0, clip_value=0.2, clip_grad_norm=True), d_kw=PPO_KW,
                         oracle_cls=PPOOracleAgent)
    spec, cfg, loss = pair.spec, pair.cfg, pair.loss
    assert pair.proj is None
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batches = []
    for i in range(K):
        b = dict(oc.obs_of(name, B, 30 + i))
        b.update(syn.make_ppo_fields(B, A, seed=40 + i))
        batches.append(b)
    oc.adopt_calibration(pair, batches[0])
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=True)
    clipped_frac = []

    def per_step(i, out, ref):
        assert set(out) >= {"loss_objective", "loss_critic", "ESS", "entropy", "loss_entropy"} and "kl" not in out
        lw = ref["lw"]
        clipped_frac.append(float(((lw > math.log1p(0.2)) | (lw < math.log1p(-0.2))).double().mean()))
        for k in ("loss_objective", "loss_critic", "loss_entropy", "entropy", "ESS"):
            e = abs(float(out[k]) - float(ref[k]))
            assert e <= 1e-4 * max(1.0, abs(float(ref[k]))), (i, k, e)
    g_scale = oc.run_updates(pair, batches, upd, per_step)
    print("fraction of frames outside the clip bounds per update:", clipped_frac)
    assert min(clipped_frac) > 0.0   # the clipped branch is exercised
    assert upd.mode.startswith("graph") and upd._program is not None
    bad, _ = moments_and_params_after(upd, pair.actor, pair.critic, pair.oracle, cfg, g_scale, K, M_TOL, V_TOL)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- (c), (d)
ROLLOUT_KW = dict(PPO_KW, clip_grad_norm=False)
KEYS = ("loss_objective", "loss_critic", "ESS", "entropy", "loss_entropy")


@pytest.mark.parametrize("form", ["unrolled", "per_step"])
def test_run_minibatches_equals_the_step_loop(form):
    N, T = 8, 10
    res = run_loop_and_launches(lambda: make_rollout(N, T, seed=33, **ROLLOUT_KW), form, N=N, T=T, ppo_epochs=2, driver_seed=9, unroll=4, keys=KEYS)
    for a, b in zip(res["loop"][:3], res["launches"][:3]):
        assert torch.equal(a, b), (a - b).abs().max().item()
    for k in KEYS:   # the last update's loss dict
        assert torch.equal(res["loop"][3][-1][k], res["launches"][3][-1][k]), k


def test_recorded_programs_equal_the_eager_loop():
    """Eager steps, the recorded lanes program and the one-stream program (overlap_critic=False) over the same four updates: the replayed
    lanes program is the eager loop's arithmetic; the one-stream program sums the advantage statistics in another launch (last bits)."""
    res = run_step_modes(lambda: make_rollout(8, 2, seed=41, **ROLLOUT_KW), ("eager", "graph", "one_stream", "one_stream_eager"), 4, KEYS,
                         lambda mode: dict(use_graph=mode in ("graph", "one_stream"), overlap_critic=not mode.startswith("one_stream")))
    for a, b in (("eager", "graph"), ("one_stream_eager", "one_stream")):
        for x, y in zip(res[a][:3], res[b][:3]):
            assert (x - y).abs().max().item() <= 1e-7, (a, b)
        for oa, ob in zip(res[a][3], res[b][3]):
            for kk in KEYS:
                assert abs(float(oa[kk]) - float(ob[kk])) <= 1e-6 * max(1.0, abs(float(oa[kk]))), (a, b, kk)
    assert (res["graph"][0] - res["one_stream"][0]).abs().max().item() <= 1e-6


def test_annealed_clip_epsilon_takes_effect_on_replay():
    from geometry_rl_amd import agent
    N, T = 8, 4
    res = {}
    for mode in ("graph", "eager", "graph_unannealed"):
        r = make_rollout(N, T, seed=51, **ROLLOUT_KW)
        loss = r.loss
        upd = agent.PolicyUpdater(loss, lr=r.cfg.lr, use_graph=mode != "eager")
        ptr = loss.clip_epsilon.data_ptr()
        prog = None
        outs = []
        for t in range(T):
            if t == 2:
                prog = upd._program
                assert (prog is not None) == (mode != "eager")
                if mode != "graph_unannealed":
                    loss.clip_epsilon.copy_(torch.tensor(0.1))   # train.py:272-274
            outs.append({k: v.clone() for k, v in upd.step({kk: v[:, t].contiguous() for kk, v in r.data.items()}).items() if k in KEYS})
        torch.cuda.synchronize()
        if mode == "graph":
            assert upd._program is prog and loss.clip_epsilon.data_ptr() == ptr   # replayed, not recorded again
        res[mode] = (upd.flat.detach().clone(), outs)
    assert (res["graph"][0] - res["eager"][0]).abs().max().item() <= 1e-7
    for oa, ob in zip(res["graph"][1], res["eager"][1]):
        for k in KEYS:
            assert abs(float(oa[k]) - float(ob[k])) <= 1e-6 * max(1.0, abs(float(ob[k]))), k
    # the write changed the update (epsilon was read): the unannealed replay differs from step 3 on
    assert not torch.equal(res["graph"][1][2]["loss_objective"], res["graph_unannealed"][1][2]["loss_objective"])


def test_replacing_the_clip_epsilon_buffer_records_again():
    from geometry_rl_amd import agent
    N, T = 8, 4
    r = make_rollout(N, T, seed=52, **ROLLOUT_KW)
    upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=True)
    for t in range(3):
        upd.step({kk: v[:, t].contiguous() for kk, v in r.data.items()})
    prog = upd._program
    assert prog is not None
    r.loss.clip_epsilon = torch.tensor(0.1, device=DEV)   # a new tensor, not an in-place write
    upd.step({kk: v[:, 3].contiguous() for kk, v in r.data.items()})
    assert upd._program is not prog


# ------------------------------------------------------------------------------------------------------------- (e) data parallel
def test_two_ranks_match_single_rank():
    world = 2
    ref_losses, ref_flat, ret = run_two_ranks(dp_ref(16, cfg_kw=PPO_KW), world, use_graph=True, dp_use_graph=True, n_steps=3, keys=KEYS,
                                              updater_kw=dict(clip_grad_norm=True))
    assert_ranks_match(ref_losses, ref_flat, ret, world, 1e-5, 2e-6)


# ------------------------------------------------------------------------------------------------------------- (f) reference loop
@pytest.mark.parametrize("model", ["hepi", "transformer"])
def test_reference_loop_protocol_matches_the_updater(model):
    """examples/torchrl/train.py:279-316 with algorithm=ppo on the loss module itself, against PolicyUpdater.step on a copy."""
    from geometry_rl_amd import agent, graph
    B = 32
    spec = graph.rigid_spec()
    kw = dict(model="transformer", output_dim=2, output_dim_vec=2) if model == "transformer" else \
        dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    cfg = agent.AgentConfig(**dict(kw, **PPO_KW))
    batch = dict(syn.make_rigid_obs(B, seed=61))
    batch.update(syn.make_ppo_fields(B, 6, seed=61))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    sides = []
    for _ in range(2):
        torch.manual_seed(5)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
        with torch.no_grad():
            actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)   # calibration (HEPi), identical on both sides
        sides.append((actor, critic, loss))
    # the reference loop
    actor, critic, loss = sides[0]
    a_par = [p for p in actor.parameters() if p.requires_grad]
    c_par = [p for p in critic.parameters() if p.requires_grad]
    a_opt = torch.optim.Adam(a_par, lr=cfg.lr, eps=1e-5)
    c_opt = torch.optim.Adam(c_par, lr=cfg.lr, eps=1e-5)
    ref = []
    for _ in range(2):
        out = loss(dict(batch))
        assert set(loss.out_keys) <= set(out.keys())
        ref.append({k: float(out[k].detach()) for k in KEYS})
        critic_loss = out["loss_critic"]
        actor_loss = out["loss_objective"]
        actor_loss += out["loss_entropy"]
        actor_loss.backward()
        critic_loss.backward()
        torch.nn.utils.clip_grad_norm_(a_par, cfg.max_grad_norm)
        torch.nn.utils.clip_grad_norm_(c_par, cfg.max_grad_norm)
        a_opt.step()
        c_opt.step()
        a_opt.zero_grad()
        c_opt.zero_grad()
    # the updater
    actor2, critic2, loss2 = sides[1]
    upd = agent.PolicyUpdater(loss2, lr=cfg.lr, clip_grad_norm=True, max_grad_norm=cfg.max_grad_norm)
    got = []
    for _ in range(2):
        o = upd.step(dict(batch))
        got.append({k: float(o[k]) for k in KEYS})
    for r, g_ in zip(ref, got):
        for k in KEYS:
            assert abs(r[k] - g_[k]) <= 1e-5 * max(1.0, abs(r[k])), (k, r[k], g_[k])
    worst = 0.0
    for (n1, p1), (n2, p2) in zip(list(actor.named_parameters()) + list(critic.named_parameters()),
                                  list(actor2.named_parameters()) + list(critic2.named_parameters())):
        assert n1 == n2
        worst = max(worst, float((p1.detach() - p2.detach()).abs().max()))
    print(f"{model}: max |param(reference loop) - param(updater)| = {worst:.3e}")
    assert worst <= 2e-5
