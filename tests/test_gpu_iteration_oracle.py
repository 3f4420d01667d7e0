"""TWO WHOLE TRAINING ITERATIONS on the device against the CPU oracle, stage by stage (the case and the reference: tests/iteration_ref.py;
that the comparison would notice a wiring mistake: tests/test_iteration_ref_cpu.py).  Reference semantics: examples/torchrl/train.py:114-140
(collector, sampler, GAE(shifted=True)) and :232-316 (the iteration: episode statistics, advantages, minibatch updates).

The chain -- raw observation -> ObservationNormalizer -> collector-side PolicyActor -> collect / RolloutBuffer -> RolloutDriver.compute_advantages
-> the sampler's minibatches -> gathers -> updates -- runs on ONE normaliser, PolicyActor, PolicyUpdater(use_graph=True), RolloutDriver(ppo_epochs=1)
and EpisodeStats for an iteration of T = 3 and one of T = 2 (five updates), HyperData.check_topology_always on.  Both sides start from identical
parameters; the HIP actor calibrates in its first collector call (where training calibrates), its calibrated kernels are compared with the
oracle's, then the oracle's are loaded and the first call is repeated.  Each stage's reference is evaluated on the HIP side's outputs of the
stage before it (copied to the CPU) and each stage is compared before it is handed on; nothing is re-synchronised inside the five updates.
The collector's eps is reproduced by a twin generator, the sampler's minibatches by a twin RolloutDriver.

Stage, bar, and the worst margin measured on an MI355X (fraction of the bar unless a unit is given):

  calibration   kernel.weight / fiber_kernel.weight within 1e-4 max(1, |ref|) (test_gpu_step.py)                              0.12
  a  normalised groups and next_last within 2e-5, raw clipped groups and infos exact, state rtol 1e-5 (test_gpu_transforms.py) 0.012; state 8e-7 relative
  b  loc, var within 1e-4 max(1, |ref|);                                                                                       0.014
     action against loc_hip + sigma_hip eps within 2 U |action| (one fused multiply-add; U = 2^-24), var_hip against sigma_hip^2 within 2 U var,
     and against loc_hip + sqrt(var_hip) eps (float64) within 2 U |action| + U/2 |sqrt(var_hip) eps| (sigma read back through the rounded var:
     the rollout keeps var, not sigma; sigma_hip is tapped from the policy's forward_diag);                                     0.47, 0.50, 0.51
     sample_log_prob against the float64 log-density at the kernel's action under the ORACLE's loc, var within
         (A + 4) U (q / 2 + sum |log sigma| + A / 2 log 2 pi) + 4 U q              [trpl_cases.sample_reference; q = sum z^2]
         + sum_i |z_i| / sigma_i  e_loc  +  sum_i |z_i^2 - 1| / (2 sigma_i^2)  e_var   [first order; e_loc, e_var = this stage's loc / var bars;
                                                                                       z, sigma the reference's]                 0.0032
  c  state_value (and the value of next_last) within 1e-4 max(1, |ref|);                                                       0.0039
     advantage, value_target within train_ops_ref.gae's allowance on the HIP values + (1 + gamma) / (1 - gamma lambda) x the value bar     0.00016
  d  episode_reward, step_count, EpisodeStats.sums: equal to stats_ref (test_gpu_stats_ops.py)                                  exact
  e  every update's 13 loss-dict entries within 1e-4 max(1, |ref|) (read from step_from in a second, otherwise identical chain whose
     buffers, parameters and moments equal the first chain's bitwise; RolloutDriver.run returns the last dict only);             0.0048
     after the fifth update exp_avg 5e-4, exp_avg_sq 1e-3 of scale, parameters 5 x the first-step bound (test_gpu_multistep_oracle.py)  0.13, 0.098, 0.052
  f  on-policy: the ORACLE's kl, mean_constraint, cov_constraint of the first update of each iteration <= 1e-4 (iteration 2: the collector
     must see the updated parameters and weight images), ESS within 1e-4 of 1 on both sides in both iterations.  (These reported values
     measure p against its own PROJECTION: they are exactly 0 wherever p lies inside the trust region of q.  What pins the collector of
     iteration 2 to the updated parameters numerically is stage b there: the oracle's loc / var come from ITS updated parameters.)   0 (exactly), 0.0048"""
import numpy as np
import pytest
import torch

import iteration_ref as ir
import train_ops_ref
from oracle_cases import LOSS_KEYS, M_TOL, TOL, V_TOL, cap_oracle_threads, check, load_params
from updater_cases import merge_grad_scales, moments_and_params_after

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, A = ir.N, ir.A
NORM_KEYS = ("norm_position_vectors", "norm_velocity_vectors", "scalars")
RAW_KEYS = ("position_vectors", "velocity_vectors", "infos")


class _Tap:
    """Stands where PolicyActor holds its policy and keeps the sigma of every forward_diag (the rollout keeps var = sigma^2 only)."""

    def __init__(self, policy):
        self.policy, self.sigmas = policy, []

    def forward_diag(self, *args, **kw):
        loc, sigma = self.policy.forward_diag(*args, **kw)
        self.sigmas.append(sigma.detach().clone())
        return loc, sigma


def _build(a_par, c_par):
    """A HIP agent from the oracle's initial parameters, calibrated by its own FIRST COLLECTOR CALL on the first normalised observation.
    -> (spec, cfg, actor, critic, loss, its calibrated kernels, that observation on the CPU)"""
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.rollout import PolicyActor
    from geometry_rl_amd.transforms import ObservationNormalizer
    spec, cfg = graph.rigid_spec(), agent.AgentConfig(**ir.KW)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    load_params(actor, a_par, DEV)
    load_params(critic, {"_network1." + k: v for k, v in c_par.items()}, DEV)
    actor.hyper_data.check_topology_always = True
    critic._network1.hyper_data.check_topology_always = True
    obs0 = ObservationNormalizer(device=DEV)(ir.SyntheticEnv(DEV).raw_obs(0))
    PolicyActor(actor, spec, use_graph=False, seed=ir.ACTOR_SEED)(obs0)
    own = {k: v.detach().cpu().clone() for k, v in actor.state_dict().items() if "kernel.weight" in k}
    return spec, cfg, actor, critic, loss, own, ir.cpu(obs0)


def _run(built, oracle_actor, via):
    """Both iterations from the oracle's calibrated weights.  ``via`` "run": RolloutDriver.run (the last loss dict of each iteration);
    "step_from": compute_advantages + step_from per minibatch (every loss dict).  -> (per-iteration records on the CPU, updater, actor, critic)"""
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import EpisodeStats, PolicyActor, RolloutDriver, collect
    from geometry_rl_amd.transforms import ObservationNormalizer
    spec, cfg, actor, critic, loss, _, _ = built
    actor.load_state_dict({k: v.detach().to(DEV) for k, v in oracle_actor.items()}, strict=False)
    actor._calib_checked = True
    norm, tap, stats, env = ObservationNormalizer(device=DEV), _Tap(actor), EpisodeStats(N, DEV), ir.SyntheticEnv(DEV)
    collector = PolicyActor(tap, spec, use_graph=False, seed=ir.ACTOR_SEED)     # (eager: a captured generator does not reproduce the eager draws)
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=True)
    drv = RolloutDriver(upd, spec, gamma=ir.GAMMA, lmbda=ir.LMBDA, ppo_epochs=1, seed=ir.DRIVER_SEED)
    keep = lambda o: {k: o[k].detach().clone() for k in LOSS_KEYS}
    raw, its = env.raw_obs(0), []
    for T in ir.T_ITERS:
        tap.sigmas = []
        buf, next_last = collect(env.step, raw, collector, T, normalizer=norm, episode_stats=stats)
        raw = env.raw_obs(env.t)
        rec = dict(T=T, sigma=torch.stack(tap.sigmas, dim=1).cpu(), next_last={k: v[:, 0].cpu() for k, v in next_last.items()},
                   norm_state={k: v.cpu().clone() for k, v in norm.state.items()}, sums=stats.sums.cpu().clone())
        with torch.no_grad():   # the value compute_advantages takes for the T+1 column (the same call, before the updates move the critic)
            rec["v_last"] = critic(*[next_last[k] for k in spec.in_features], train=False).reshape(N).cpu()
        if via == "run":
            losses = [keep(drv.run(buf, next_last))]
        else:
            drv.compute_advantages(buf, next_last)
            losses = [keep(upd.step_from(buf, idx)) for idx in drv.minibatches(buf)]
        torch.cuda.synchronize()
        rec.update(data=ir.cpu(buf.data), losses=[{k: v.cpu() for k, v in o.items()} for o in losses])
        its.append(rec)
    return its, upd, actor, critic


def _ratio(got, ref, allow):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / allow).max())


def test_two_iterations_match_the_oracle():
    cap_oracle_threads()
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)
        assert np.isfinite(r) and r <= 1.0, (name, r)

    o_spec, o_cfg, a_par, c_par, oracle = ir.make_oracle()
    env, st, ep = ir.SyntheticEnv(), ir.new_norm_state(), ir.new_episode_state()

    # ---- calibration: the HIP actor's own, in its first collector call, against the oracle's on the same (HIP-normalised, checked) observation
    side_a = _build(a_par, c_par)
    obs0 = side_a[6]
    ref0 = ir.ref_normalise(env.raw_obs(0), ir.new_norm_state())
    for k in NORM_KEYS:
        note("a normalised / 2e-5", _ratio(obs0[k], ref0[k], ir.NORM_TOL))
    with torch.no_grad():
        oracle.actor_forward({k: obs0[k] for k in o_spec.in_features}, calibrate=True)
    n_cal = 0
    for k, v in oracle.actor.items():
        if "kernel.weight" in k:
            check("calibrated " + k, side_a[5][k], v, 1e-4)
            note("calibration / 1e-4 max(1, |ref|)", _ratio(side_a[5][k], v.detach(), ir.tol_of(v.detach(), 1e-4)))
            n_cal += 1
    assert n_cal > 0

    # ---- the device side, twice: through RolloutDriver.run, and step by step for every update's loss dict
    run_a, upd, actor, critic = _run(side_a, oracle.actor, "run")
    print("PolicyUpdater.mode:", upd.mode, "| steps", upd.steps)
    assert upd.mode.startswith("graph") and upd.steps == 5
    run_b, upd_b, _, _ = _run(_build(a_par, c_par), oracle.actor, "step_from")
    for ra, rb in zip(run_a, run_b):   # otherwise identical: the same bits everywhere
        assert all(torch.equal(ra["data"][k], rb["data"][k]) for k in ra["data"]) and sorted(ra["data"]) == sorted(rb["data"])
        assert all(torch.equal(ra["losses"][-1][k], rb["losses"][-1][k]) for k in LOSS_KEYS)
    for x, y in ((upd.flat, upd_b.flat), (upd.exp_avg, upd_b.exp_avg), (upd.exp_avg_sq, upd_b.exp_avg_sq)):
        assert torch.equal(x, y)

    twin = torch.Generator(device=DEV).manual_seed(ir.ACTOR_SEED)          # PolicyActor(seed=)'s generator, drawn in the same order
    eps = [torch.randn((N, A), device=DEV, dtype=torch.float32, generator=twin).cpu() for _ in range(ir.STEPS)]
    idx_all = [[i.cpu() for i in idxs] for idxs in ir.sampler_indices(DEV)]
    g_scale, s0 = None, 0
    for it, (rec, rec_b) in enumerate(zip(run_a, run_b)):
        T, data = rec["T"], rec["data"]
        assert data["action"].shape == (N, T, A) and data["sample_log_prob"].shape[:2] == (N, T)
        frames = [{k: data[k][:, t] for k in o_spec.in_features} for t in range(T)]

        # ---- a: normalised + clipped groups in the buffer and next_last, the normaliser's state
        for t in range(T + 1):
            ref = ir.ref_normalise(env.raw_obs(s0 + t), st, update=t < T)
            got = frames[t] if t < T else rec["next_last"]
            for k in NORM_KEYS:
                note("a normalised / 2e-5", _ratio(got[k], ref[k], ir.NORM_TOL))
            for k in RAW_KEYS:
                assert torch.equal(got[k], ref[k]), (it, t, k)
        for k in st:
            ref_s, got_s = ir.norm_state_vector(st, k), rec["norm_state"][k]
            worst["a state (relative)"] = max(worst.get("a state (relative)", 0.0), float(((got_s - ref_s).abs() / ref_s.abs().clamp_min(1e-30)).max()))
            assert torch.allclose(got_s[:-1], ref_s[:-1], rtol=1e-5) and torch.allclose(got_s[-1:], ref_s[-1:]), (it, k)

        # ---- b: the collector's loc, var, action, sample_log_prob of every frame
        for t in range(T):
            loc_h, var_h, act_h, sig_h = data["loc"][:, t], data["var"][:, t], data["action"][:, t], rec["sigma"][:, t]
            c = ir.ref_collect_step(oracle, frames[t], eps[s0 + t], act_h, loc_in=loc_h, var_in=var_h)
            check(f"it{it} t{t} loc", loc_h, c["loc"])
            check(f"it{it} t{t} var", var_h, c["var"])
            e_loc, e_var = ir.tol_of(c["loc"]), ir.tol_of(c["var"])
            note("b loc, var / 1e-4 max(1, |ref|)", max(_ratio(loc_h, c["loc"], e_loc), _ratio(var_h, c["var"], e_var)))
            a_exact = loc_h.double() + sig_h.double() * eps[s0 + t].double()
            note("b action / 2 U |a|", _ratio(act_h, a_exact, 2 * ir.U32 * a_exact.abs() + 1e-30))
            note("b var / 2 U sigma^2", _ratio(var_h, sig_h.double() ** 2, 2 * ir.U32 * sig_h.double() ** 2))
            back = 0.5 * ir.U32 * (var_h.double().sqrt() * eps[s0 + t].double()).abs()
            note("b action (sqrt var) / bound", _ratio(act_h, c["action_ref"], 2 * ir.U32 * c["action_ref"].abs() + back + 1e-30))
            note("b sample_log_prob / allowance", _ratio(data["sample_log_prob"][:, t], c["logp"], ir.logp_allowance(c, e_loc, e_var)))

        # ---- c: the critic's values, the shifted GAE
        r, d, tm = (data[k].reshape(N, T) for k in ("reward", "done", "terminated"))
        for k, want in (("reward", env.reward), ("done", lambda s: env.done[:, s]), ("terminated", lambda s: env.term[:, s])):
            assert torch.equal(data[k].reshape(N, T), torch.stack([want(s0 + t) for t in range(T)], dim=1)), k
        V, sv, adv, tgt = ir.ref_advantages(oracle, frames, rec["next_last"], r, d, tm)
        V_h = torch.cat([data["state_value"].reshape(N, T), rec["v_last"].reshape(N, 1)], dim=1)
        check(f"it{it} state_value", data["state_value"].reshape(N, T), sv)
        check(f"it{it} value of next_last", rec["v_last"], V[:, T])
        e_val = ir.tol_of(V)
        note("c values / 1e-4 max(1, |ref|)", _ratio(V_h, V, e_val))
        _, _, ea, et = train_ops_ref.gae(r, d, tm, V_h, train_ops_ref.f32(ir.GAMMA), train_ops_ref.f32(ir.LMBDA))
        prop = ir.value_propagation(e_val)
        note("c advantage / allowance", _ratio(data["advantage"].reshape(N, T), adv, ea + prop))
        note("c value_target / allowance", _ratio(data["value_target"].reshape(N, T), tgt, et + prop))

        # ---- d: RewardSum / StepCounter with the state carried across the rollouts
        er, sc, sums = ir.ref_episode_stats(r, d, ep)
        assert np.array_equal(data["episode_reward"].reshape(N, T).numpy(), er) and np.array_equal(data["step_count"].reshape(N, T).numpy(), sc)
        assert rec["sums"].numpy().tolist() == sums.tolist(), (rec["sums"], sums)

        # ---- e, f: the updates, on the rows of the device's buffer
        for j, (ref, ref_grads) in enumerate(ir.ref_updates(oracle, data, idx_all[it])):
            g_scale = merge_grad_scales(g_scale, ref_grads)
            got = rec_b["losses"][j]
            for k in LOSS_KEYS:
                check(f"it{it} update {j} {k}", got[k], ref[k])
                note("e loss dict / 1e-4 max(1, |ref|)", _ratio(got[k].reshape(()), ref[k].reshape(()), ir.tol_of(ref[k])))
            if j == 0:   # on-policy: a condition on the reference (iteration 2: the collector must have seen the UPDATED parameters)
                for k in ("kl", "mean_constraint", "cov_constraint"):
                    note("f oracle kl, constraints / 1e-4", abs(float(ref[k])) / TOL)
                note("f |ESS - 1| / 1e-4", max(abs(float(ref["ESS"]) - 1.0), abs(float(got["ESS"]) - 1.0)) / TOL)
        assert len(rec_b["losses"]) == T and len(rec["losses"]) == 1
        s0 += T

    bad, w = moments_and_params_after(upd, actor, critic, oracle, o_cfg, g_scale, ir.STEPS, M_TOL, V_TOL)
    worst.update({"e exp_avg / 5e-4 of scale": w["exp_avg"] / M_TOL, "e exp_avg_sq / 1e-3 of scale": w["exp_avg_sq"] / V_TOL,
                  "e parameters / 5 x first-step bound": w["param"]})
    for name, r in worst.items():
        print(f"worst margin  {name}: {r:.3g}")
    assert not bad, bad


def test_graph_collector_equals_eager_collector_bitwise():
    """PolicyActor(deterministic=True) recorded into a hipGraph against the eager one over four calls (eager, record, replay, replay) on
    observations that change every call, each side through a normaliser of its own: loc, var, action, sample_log_prob equal bitwise.
    (deterministic: a captured generator does not reproduce the eager draw order.)"""
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.rollout import PolicyActor
    from geometry_rl_amd.transforms import ObservationNormalizer
    spec, cfg = graph.rigid_spec(), agent.AgentConfig(**ir.KW)
    torch.manual_seed(0)
    actor, _, _, _ = agent.build_agent(spec, cfg, device=DEV)
    env = ir.SyntheticEnv(DEV)
    sides = {name: (PolicyActor(actor, spec, use_graph=name == "graph", deterministic=True), ObservationNormalizer(device=DEV))
             for name in ("eager", "graph")}
    for call in range(4):
        outs = {}
        for name, (act, norm) in sides.items():   # (call 0: the eager side's pass calibrates the fresh policy, both then see the same weights)
            outs[name] = {k: v.clone() for k, v in act(norm(env.raw_obs(call))).items()}
        for k in ("loc", "var", "action", "sample_log_prob"):
            assert torch.equal(outs["eager"][k], outs["graph"][k]), (call, k, float((outs["eager"][k] - outs["graph"][k]).abs().max()))
        assert torch.equal(outs["graph"]["action"], outs["graph"]["loc"]) and bool(torch.isfinite(outs["graph"]["sample_log_prob"]).all())
    assert sides["graph"][0]._graph is not None and sides["eager"][0]._graph is None
