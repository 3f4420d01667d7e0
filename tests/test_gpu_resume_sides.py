"""Save and resume around the policy update, every comparison BITWISE (resume_cases.differences):
  * the collector side -- ``PolicyActor`` (stochastic, recorded), ``ObservationNormalizer`` and ``EpisodeStats`` inside ``collect`` over the
    iteration tests' synthetic environment: two rollouts uninterrupted against one rollout, save, fresh objects, restore, the second rollout;
  * behaviour cloning -- ``BehaviorCloner.fit(2)`` against ``fit(1)``, save, a fresh cloner and updater, restore, ``fit(1)``; ``release()``
    then hands over the same actor."""
import pytest
import torch

import iteration_ref as ir
import resume_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------- collector side
def _collector(torch_seed, actor_seed):
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.rollout import EpisodeStats, PolicyActor
    from geometry_rl_amd.transforms import ObservationNormalizer
    spec = graph.rigid_spec()
    torch.manual_seed(torch_seed)
    actor, critic, proj, loss = agent.build_agent(spec, agent.AgentConfig(**ir.KW), device=DEV)
    upd = agent.PolicyUpdater(loss)   # (its part of the state holds the policy: weights, calibration latches, the cached topology)
    return dict(spec=spec, actor=actor, updater=upd, collector=PolicyActor(actor, spec, use_graph=True, seed=actor_seed),
                normalizer=ObservationNormalizer(decay=ir.DECAY, eps=ir.EPS, low=ir.LOW, high=ir.HIGH, device=DEV),
                episodes=EpisodeStats(ir.N, DEV))


def _parts(o):
    return {k: o[k] for k in ("updater", "collector", "normalizer", "episodes")}


def _rollout(o, env, T):
    from geometry_rl_amd.rollout import collect
    buf, next_last = collect(env.step, env.raw_obs(env.t), o["collector"], T, normalizer=o["normalizer"], episode_stats=o["episodes"])
    torch.cuda.synchronize()
    return {"buffer": {k: v.clone() for k, v in buf.data.items()}, "next_last": {k: v.clone() for k, v in next_last.items()},
            "normaliser": {k: v.clone() for k, v in o["normalizer"].state.items()},
            "episodes": [o["episodes"].ret_state.clone(), o["episodes"].len_state.clone(), o["episodes"].sums.clone()]}


def test_collector_side_resumes_bit_for_bit(tmp_path):
    from geometry_rl_amd import checkpoint
    T1, T2 = ir.T_ITERS
    a, env_a = _collector(0, ir.ACTOR_SEED), ir.SyntheticEnv(device=DEV)
    _rollout(a, env_a, T1)
    want = _rollout(a, env_a, T2)
    assert a["collector"]._graph is not None, "the uninterrupted collector did not record its pass"

    b, env_b = _collector(0, ir.ACTOR_SEED), ir.SyntheticEnv(device=DEV)
    first = _rollout(b, env_b, T1)
    path = str(tmp_path / "state.pt")
    checkpoint.save(path, **_parts(b))
    c, env_c = _collector(1, ir.ACTOR_SEED + 40), ir.SyntheticEnv(device=DEV)
    env_c.t = env_b.t                                  # (the simulator's own state stays the caller's)
    checkpoint.restore(checkpoint.load(path), **_parts(c))
    assert c["collector"]._calls == T1 and c["collector"]._graph is None
    rc.assert_same({k: first[k] for k in ("normaliser", "episodes")},
                   {"normaliser": dict(c["normalizer"].state), "episodes": [c["episodes"].ret_state, c["episodes"].len_state, c["episodes"].sums]},
                   "restored collector side")
    got = _rollout(c, env_c, T2)
    rc.assert_same(want, got, "second rollout")
    assert float(want["episodes"][2][2]) > 0 and want["buffer"]["action"].shape[:2] == (ir.N, T2)
    assert rc.differences(first["normaliser"], want["normaliser"]), "the second rollout did not move the normaliser: the case shows nothing"


# ------------------------------------------------------------------------------------------------------------- behaviour cloning
BC_N, BC_T, BC_MB = 10, 4, 8    # 8 of 10 environments train, 2 are held out; 4 minibatches of 8 frames per epoch


def _demonstrations(spec, keys):
    from geometry_rl_amd import synthetic as syn
    from geometry_rl_amd.rollout import RolloutBuffer
    frames = []
    for t in range(BC_T):
        b = dict(syn.make_rigid_obs(BC_N, seed=70 + t))
        b["action"] = syn.make_ppo_fields(BC_N, 6, seed=70 + t)["action"]
        frames.append({k: b[k].to(DEV) for k in list(keys) + ["action"]})
    return RolloutBuffer({k: torch.stack([f[k] for f in frames], dim=1) for k in frames[0]})


def _cloner(torch_seed, cloner_seed):
    from geometry_rl_amd import agent, bc, graph
    spec = graph.rigid_spec()
    torch.manual_seed(torch_seed)
    actor, *_ = agent.build_agent(spec, agent.AgentConfig(training_noise=True, **ir.KW), device=DEV)
    loss = bc.BCLoss(actor, objective="nll")
    upd = bc.BCUpdater(loss, use_graph=True)
    cl = bc.BehaviorCloner(upd, spec, _demonstrations(spec, loss.in_features), mini_batch_size=BC_MB, seed=cloner_seed)
    return actor, upd, cl


def _bc_state(upd, cl):
    torch.cuda.synchronize()
    return {"flat": upd.flat.clone(), "exp_avg": upd.exp_avg.clone(), "exp_avg_sq": upd.exp_avg_sq.clone(), "steps": (upd.steps, int(upd.step_dev)),
            "noise": tuple(upd.loss_module.actor_network.hyper_data.noise_state()), "train_rows": cl.train_rows().clone(),
            "heldout_rows": cl.heldout_rows().clone(), "epochs": cl.epochs_done, "generator": cl.gen.get_state().clone()}


def test_behaviour_cloning_resumes_bit_for_bit(tmp_path):
    from geometry_rl_amd import checkpoint
    actor_a, upd_a, cl_a = _cloner(0, 5)
    hist_a = cl_a.fit(2)
    want = _bc_state(upd_a, cl_a)

    actor_b, upd_b, cl_b = _cloner(0, 5)
    hist_b = cl_b.fit(1)
    path = str(tmp_path / "bc.pt")
    checkpoint.save(path, updater=upd_b, cloner=cl_b)
    actor_c, upd_c, cl_c = _cloner(1, 23)
    assert not torch.equal(upd_c.flat, upd_b.flat)
    checkpoint.restore(checkpoint.load(path), updater=upd_c, cloner=cl_c)
    rc.assert_same(_bc_state(upd_b, cl_b), _bc_state(upd_c, cl_c), "restored cloner")
    hist_c = cl_c.fit(1)
    got = _bc_state(upd_c, cl_c)
    rc.assert_same(want, got, "cloning resumed")
    assert hist_a["loss"] == hist_b["loss"] + hist_c["loss"] and hist_a["train"] == hist_b["train"] + hist_c["train"], (hist_a["loss"], hist_b["loss"], hist_c["loss"])
    assert got["epochs"] == 2 and got["steps"] == (2 * BC_T, 2 * BC_T)
    upd_a.release()
    upd_c.release()
    sa, sc = actor_a.state_dict(), actor_c.state_dict()
    assert set(sa) == set(sc)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
