"""Host logic of ``PolicyUpdater(track_stats=)`` without a GPU: the argument allocates the running sums and changes no program outline, and
``stats_read()`` maps the sums to the loss module's key names and refuses sums whose lanes disagree."""
import pytest
import torch


def _updater(**kw):
    from geometry_rl_amd import agent, graph
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, **kw.pop("cfg_kw", {}))
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device="cpu")
    return agent.PolicyUpdater(loss, lr=cfg.lr, **kw)


def test_argument_changes_no_outline_and_allocates_only_when_on():
    plain, off, on = _updater(), _updater(track_stats=False), _updater(track_stats=True)
    for published in (True, False):
        assert off.program_outline(published) == plain.program_outline(published) == on.program_outline(published)
    assert plain.track_stats is False and plain.stats_actor is None and off.stats_critic is None
    assert on.stats_actor.shape == (15,) and on.stats_critic.shape == (2,) and on.stats_actor.dtype == on.stats_critic.dtype == torch.float64
    with pytest.raises(RuntimeError, match="track_stats=True"):
        plain.stats_read()


def test_stats_read_maps_sums_to_the_loss_keys():
    from geometry_rl_amd.trpl import report_dict
    upd = _updater(track_stats=True)
    assert upd.stats_read() == {"updates": 0}
    upd.stats_actor.copy_(torch.cat([torch.arange(14, dtype=torch.float64) * 4, torch.tensor([4.0], dtype=torch.float64)]))
    upd.stats_critic.copy_(torch.tensor([10.0, 4.0], dtype=torch.float64))
    means = upd.stats_read()
    _, mt = report_dict(torch.arange(14, dtype=torch.float64), upd.loss_module)   # (the means are 0 .. 13: slot i reads i)
    want = {k: float(v) for k, v in mt.items()}
    want["loss_objective"] = want.pop("loss_objective_value")
    assert means == dict(want, loss_critic=2.5, updates=4)
    assert len(means) == 14 and all(isinstance(v, float) for k, v in means.items() if k != "updates")
    upd.stats_critic[1] = 3.0
    with pytest.raises(RuntimeError, match="counted 4 updates, the critic's 3"):
        upd.stats_read()
    upd.stats_reset()
    assert upd.stats_read() == {"updates": 0}


def test_one_stream_report_carries_the_critic_loss():
    upd = _updater(track_stats=True, overlap_critic=False)
    upd._plan({}, {})   # (the closures are built, not called)
    upd.stats_actor.copy_(torch.cat([torch.arange(14, dtype=torch.float64) * 2, torch.tensor([2.0], dtype=torch.float64)]))
    means = upd.stats_read()
    assert means["updates"] == 2 and means["loss_critic"] == 1.0


def test_ppo_keys():
    upd = _updater(track_stats=True, cfg_kw=dict(algorithm="ppo"))
    upd.stats_actor[14] = 1.0
    upd.stats_critic[1] = 1.0
    assert set(upd.stats_read()) == {"updates", "loss_objective", "loss_critic", "ESS", "entropy", "loss_entropy"}
