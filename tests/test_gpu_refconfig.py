"""Every shipped reference task config, built by ``refconfig.build_from_config`` at a small observation layout (tests/refconfig_cases.py),
takes one policy update on the GPU -- and that update is the one the hand-written twin ``agent.build_agent(spec, to_agent_config(cfg, spec))``
takes from the same weights on the same minibatch.  Seven of the combinations had never been constructed: EMPN and the transformer on cloth,
the transformer with training noise, HEPi at ponita_dim=2 with two output vectors, EMPN at ponita_dim=2 with training noise, a data class
without knn_k, rope with clip_grad_norm.

Tolerances.  Config-built against twin: both sides issue the same launches on the same numbers, so they differ by the order of fp32 atomic
sums alone; the bars are the ones ``smoke()`` holds the HIP update to against the float64 oracle (tests/oracle_cases.py TOL = 1e-4 relative
on outputs, 2e-5 absolute on the parameters after one Adam step of lr 3e-4), which bound that from above.  HIP transformer kernels against
the stock torch encoder: two fp32 evaluations of one function, each held to TOL of float64 elsewhere, hence 2 * TOL of each other."""
import pytest
import torch

import refconfig_cases as rcase
from refconfig_cases import NAMES

from geometry_rl_amd import agent, refconfig, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 16   # one minibatch; the rigid rows hold 6 .. 12 valid object points
TOL = 1e-4
OUT_KEYS = {"trpl": ("loc", "state_value", "loss_objective", "loss_trust_region", "loss_entropy", "loss_critic", "kl"),
            "ppo": ("loc", "state_value", "loss_objective", "loss_entropy", "loss_critic"),
            "kl_ppo": ("loc", "state_value", "loss_objective", "loss_entropy", "loss_critic", "kl")}
_ATT = "algorithm/policy/pyg_agent/model=../../../pyg_agent/model/hepi_attention"


def _one_update(loss, ts, batch):
    upd = agent.PolicyUpdater(loss, **ts.updater_kwargs())
    out = upd.step(batch)
    torch.cuda.synchronize()
    return {k: v.detach().float().cpu() for k, v in out.items() if torch.is_tensor(v)}


def _params(*modules):
    return {f"{i}.{k}": p for i, m in enumerate(modules) for k, p in m.named_parameters()}


def _update_from_config(name, overrides=(), head_gain=1.0, **kw):
    """Build the config and its twin from one seed and one set of weights; run the config-built side's update and check it on its own.
    ``head_gain``: the orthogonal(0.01) heads of a post_fc actor leave loc ~ 0; a comparison that is to see the encoder scales them up."""
    torch.manual_seed(11)
    cfg, (actor, critic, projection, loss) = rcase.build(name, overrides, device=DEV, **kw)
    if head_gain != 1.0:
        with torch.no_grad():
            actor._mean.weight.mul_(head_gain)
            actor._pre_std.weight.mul_(head_gain)
    ts = refconfig.train_settings(cfg)
    keys = OUT_KEYS[cfg["algorithm"]["name"]]
    assert (projection is not None) == (cfg["algorithm"]["name"] == "trpl")
    cpu = dict(rcase.make_obs(name, B, seed=4))
    cpu.update(syn.make_ppo_fields(B, actor.action_dim, seed=4))
    batch = {k: v.to(DEV) for k, v in cpu.items()}
    spec = actor.hyper_data.spec
    torch.manual_seed(11)   # (the same initial seed: a noisy HyperData takes its generator's seed from it)
    t_actor, t_critic, _, t_loss = agent.build_agent(spec, refconfig.to_agent_config(cfg, spec), device=DEV)
    t_actor.load_state_dict(actor.state_dict())
    t_critic.load_state_dict(critic.state_dict())
    before = {k: p.detach().clone() for k, p in _params(actor, critic).items()}
    out = _one_update(loss, ts, batch)
    for k in keys:
        assert k in out and bool(torch.isfinite(out[k]).all()), k
    assert tuple(out["loc"].shape) == (B, actor.action_dim)
    after = _params(actor, critic)
    assert all(bool(torch.isfinite(p).all()) for p in after.values())
    moved = [k for k, p in after.items() if not torch.equal(p, before[k])]
    assert any(k.startswith("0.") for k in moved) and any(k.startswith("1.") for k in moved), moved   # both networks took their Adam step
    return keys, out, after, (t_actor, t_critic, t_loss), ts, batch


def _check_against_twin(name, overrides=(), **kw):
    keys, out, after, (t_actor, t_critic, t_loss), ts, batch = _update_from_config(name, overrides, **kw)
    ref = _one_update(t_loss, ts, batch)
    for k in keys:
        err = float((out[k].double() - ref[k].double()).abs().max())
        print(f"{name} {k}: |value| <= {float(ref[k].abs().max()):.3e}, config-built vs twin {err:.3e}")
        assert err <= TOL * max(1.0, float(ref[k].abs().max())), (k, err)
    twin_after = _params(t_actor, t_critic)
    for k, p in after.items():
        err = float((p.detach() - twin_after[k].detach()).abs().max())
        assert err <= 2e-5, (k, err)


@pytest.mark.parametrize("name", NAMES)
def test_task_config_takes_the_update_of_its_hand_written_twin(name):
    _check_against_twin(name)


@pytest.mark.parametrize("name,overrides", [
    ("rigid_insertion_multi_hepi", ["algorithm=ppo"]),
    ("rope_closing_hepi", ["algorithm=kl_ppo"]),
    ("rigid_insertion_two_agents_multi_hepi", [_ATT]),
    ("rigid_pushing_multi_empn", ["algorithm.policy.pyg_agent.model.attention=True"]),
    ("rigid_sliding_multi_hepi", ["algorithm.projection.entropy_schedule=linear", "algorithm.projection.target_entropy=-3.0"]),
], ids=["ppo", "kl_ppo", "hepi_attention", "empn_attention", "entropy_schedule"])
def test_overridden_config_takes_the_update_of_its_twin(name, overrides):
    _check_against_twin(name, overrides)


def test_transformer_config_runs_on_the_hip_kernels_when_asked():
    """``transformer_kernels="hip"`` is the caller's switch, not the config's: the twin (to_agent_config leaves the switch at "torch") is the
    same config on the stock torch encoder."""
    keys, out, _, (t_actor, _, t_loss), ts, batch = _update_from_config("cloth_hanging_multi_transformer", head_gain=30.0,
                                                                         transformer_kernels="hip")
    assert t_actor.gnn.kernels == "torch"
    ref = _one_update(t_loss, ts, batch)
    for k in keys:
        err = float((out[k].double() - ref[k].double()).abs().max())
        print(f"hip vs torch encoder {k}: |value| <= {float(ref[k].abs().max()):.3e}, difference {err:.3e}")
        assert err <= 2 * TOL * max(1.0, float(ref[k].abs().max())), (k, err)
