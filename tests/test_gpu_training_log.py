"""``PolicyUpdater(track_stats=True)`` and ``RolloutDriver.iteration_log``: the per-iteration read-out of a training run
(examples/torchrl/train.py:237-246, 318-333) kept on the device.  The means of ``stats_read()`` are compared with the values the same
sequence of updates reports step by step with tracking off; tracking must change nothing it observes (parameters and Adam moments
bitwise) and, switched off, nothing at all (the program outline)."""
import contextlib
import math

import pytest
import torch

import stats_ref
from updater_cases import DEV, STATS_FORMS as FORMS, STATS_N as N, STATS_T as T, assert_stats_means, dp_ref, make_rollout, run_stats_epoch, snapshot, spawn_dp

pytestmark = pytest.mark.gpu
TRPL_KEYS = ("loss_objective", "loss_critic", "loss_trust_region", "loss_entropy", "kl", "constraint", "mean_constraint", "mean_constraint_max",
             "cov_constraint", "cov_constraint_max", "entropy", "entropy_diff", "ESS")
PPO_KEYS = ("loss_objective", "loss_critic", "ESS", "entropy", "loss_entropy")


@pytest.mark.parametrize("form", list(FORMS))
def test_means_of_twelve_updates_and_the_update_is_unchanged(form):
    """stats_read() after 12 minibatches = the fp64 mean of the values the steps report (to 12 * 2^-53 * max |v| of math.fsum / 12), the
    count is 12, and parameters and both Adam moments are bitwise those of the run without tracking."""
    ref_upd, _, _, vals = run_stats_epoch(form, False, {}, TRPL_KEYS)
    assert len(vals) == T
    upd, _, _, _ = run_stats_epoch(form, True, {}, TRPL_KEYS)
    assert_stats_means(upd.stats_read(), vals, TRPL_KEYS)
    for a, b in zip(snapshot(upd, None)[:3], snapshot(ref_upd, None)[:3]):
        assert torch.equal(a, b), float((a - b).abs().max())
    again = upd.stats_read()          # reading does not disturb the sums; a reset empties them
    assert again["updates"] == T
    upd.stats_reset()
    assert upd.stats_read() == {"updates": 0}


def test_ppo_reports_its_own_keys():
    """The clipped PPO objective through the multi-step launches: the keys of ppo.report_dict plus loss_objective and loss_critic; and the
    iteration log carries ``train/clip_epsilon``."""
    from geometry_rl_amd.rollout import RolloutDriver
    _, _, _, vals = run_stats_epoch("launches", False, dict(algorithm="ppo"), PPO_KEYS)
    upd, r, buf, _ = run_stats_epoch("launches", True, dict(algorithm="ppo"), PPO_KEYS)
    assert_stats_means(upd.stats_read(), vals, PPO_KEYS)
    log = RolloutDriver(upd, r.spec, ppo_epochs=1).iteration_log(buf)
    assert log["train/clip_epsilon"] == float(r.loss.clip_epsilon) and log["train/lr"] == upd.lr
    assert {f"train/{k}" for k in PPO_KEYS} <= set(log)


def test_tracking_off_is_the_program_without_the_argument():
    from geometry_rl_amd import agent
    r = make_rollout(N, 1, 21)
    plain = agent.PolicyUpdater(r.loss, lr=r.cfg.lr)
    off = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, track_stats=False)
    for published in (True, False):
        assert off.program_outline(published) == plain.program_outline(published)
    assert off.stats_actor is None and off.stats_critic is None
    with pytest.raises(RuntimeError, match="track_stats=True"):
        off.stats_read()
    with pytest.raises(RuntimeError, match="track_stats=True"):
        off.stats_reset()


# ------------------------------------------------------------------------------------------------------------- two ranks on one GPU
DP_STEPS = 4   # eager, recorded, two replays


@contextlib.contextmanager
def _record_steps(case, upd, shard, rank, ret):
    """Around a rank's updates (updater_cases.dp_worker): every step's reported values are cloned as the step returns, and the rank leaves
    them and its ``stats_read()`` behind."""
    vals = []
    step = upd.step

    def recording_step(batch):
        out = step(batch)
        vals.append({k: out[k].detach().clone() for k in TRPL_KEYS})
        return out
    upd.step = recording_step
    yield None
    ret[f"stats{rank}"] = upd.stats_read()
    ret[f"values{rank}"] = [{k: float(v) for k, v in s.items()} for s in vals]


def test_two_ranks_read_identical_means():
    """Data parallel, recorded graph segments: the accumulate launches ride behind the lanes' tails, whose values are the GLOBAL ones -- both
    ranks read identical means, equal to the mean of the values their steps reported, and no collective is added."""
    ret = spawn_dp(dp_ref(16, cfg_kw={}), 2, use_graph=True, n_steps=DP_STEPS, keys=("loss_objective",),
                   updater_kw=dict(track_stats=True), extra=(__name__, "_record_steps"))
    assert ret["stats0"] == ret["stats1"], (ret["stats0"], ret["stats1"])
    for rank in range(2):
        means, vals = ret[f"stats{rank}"], ret[f"values{rank}"]
        assert means["updates"] == DP_STEPS and len(vals) == DP_STEPS
        for k in TRPL_KEYS:
            v = [s[k] for s in vals]
            assert abs(means[k] - math.fsum(v) / DP_STEPS) <= DP_STEPS * 2.0 ** -53 * max(abs(x) for x in v), (rank, k, means[k], v)


# ------------------------------------------------------------------------------------------------------------- one whole iteration
def _iteration(done_pattern):
    """collect (T = 6, synthetic environment, ``done_pattern(t)`` -> bool [N]) with the episode scan, RolloutDriver.run, iteration_log."""
    from geometry_rl_amd import agent, graph, synthetic as syn
    from geometry_rl_amd.rollout import EpisodeStats, PolicyActor, RolloutDriver, collect
    n_env, steps = 8, 6
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    state = {"t": 0}

    def raw_obs(t):
        o = syn.make_rigid_obs(n_env, seed=70 + t)
        return {k: o[k].to(DEV) for k in spec.in_features}

    def env_step(action):
        t = state["t"]
        state["t"] += 1
        g = torch.Generator().manual_seed(t)
        reward = torch.randint(-512, 513, (n_env,), generator=g).float() / 256
        return raw_obs(t + 1), reward.to(DEV), done_pattern(t).to(DEV), torch.zeros(n_env, dtype=torch.bool, device=DEV)

    es = EpisodeStats(n_env, DEV)
    buf, next_last = collect(env_step, raw_obs(0), PolicyActor(actor, spec, use_graph=False), steps, episode_stats=es)
    assert buf.data["episode_reward"].shape == (n_env, steps, 1) and buf.data["step_count"].shape == (n_env, steps, 1)
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, use_graph=True, track_stats=True)
    upd.stats_actor.fill_(3.0)      # (stale sums: run() resets them before its first update)
    upd.stats_critic.fill_(3.0)
    drv = RolloutDriver(upd, spec, ppo_epochs=2, seed=1)
    out = drv.run(buf, next_last)
    assert "loss_objective" in out   # (the return value is what it was: the last update's loss dict)
    return drv.iteration_log(buf, es), buf, upd, steps


def test_iteration_log_has_the_reference_keys_and_episode_statistics():
    """Episodes finish on a fixed pattern (environment i at every step t with (t + i) % 3 == 2): every ``train/...`` key the reference logs
    from the device (train.py:241-245, 322-326) is there, ``train/reward`` / ``train/episode_length`` equal the restatement on the
    buffer's reward / done, the explained variance equals the per-op wrapper's, the means are those of 2 x 6 updates."""
    from geometry_rl_amd.rollout import explained_variance
    log, buf, upd, steps = _iteration(lambda t: (torch.arange(8) + t) % 3 == 2)
    want = {f"train/{k}" for k in TRPL_KEYS} | {"train/explained_variance", "train/explained_variance_flat", "train/lr", "train/reward",
                                                 "train/episode_length"}
    assert set(log) == want, sorted(set(log) ^ want)
    assert all(isinstance(v, float) and math.isfinite(v) for v in log.values())
    n = buf.N
    reward, done = buf.data["reward"].reshape(n, steps).cpu().numpy(), buf.data["done"].reshape(n, steps).cpu().numpy()
    er, sc, _, _, sums = stats_ref.episode_scan(reward, done, [0.0] * n, [0] * n)
    assert sums[2] > 0
    assert log["train/reward"] == sums[0] / sums[2] and log["train/episode_length"] == sums[1] / sums[2]
    assert (buf.data["episode_reward"].reshape(n, steps).cpu().numpy() == er).all() and (buf.data["step_count"].reshape(n, steps).cpu().numpy() == sc).all()
    ev = explained_variance(buf.data["state_value"], buf.data["value_target"]).tolist()
    assert [log["train/explained_variance"], log["train/explained_variance_flat"]] == ev
    ref = stats_ref.explained_variance(buf.data["state_value"].reshape(n, steps).cpu().numpy(), buf.data["value_target"].reshape(n, steps).cpu().numpy())
    for a, b in zip(ev, ref):
        assert abs(a - b) <= 4 * 2.0 ** -23 * max(1.0, abs(b)), (a, b)
    assert log["train/lr"] == upd.lr and upd.stats_read()["updates"] == 2 * steps


def test_iteration_log_omits_episode_keys_when_no_episode_finished():
    log, _, _, _ = _iteration(lambda t: torch.zeros(8, dtype=torch.bool))
    assert "train/reward" not in log and "train/episode_length" not in log and "train/explained_variance" in log
