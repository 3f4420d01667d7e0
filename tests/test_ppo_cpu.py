"""The clipped PPO objective without a GPU: the float64 restatement (tests/ppo_ref.py) against the gradient rule of the contract, a
cross-pin to the pinned TRPL oracle, and the construction of geometry_rl_amd.ppo.ClipPPOLoss2 as the reference builder calls it
(examples/torchrl/builders/agent.py:53-64 with configs/algorithm/objective/default.yaml)."""
import math
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from oracle import trpl as otr
from ppo_ref import ppo_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.2
LO, HI = math.log1p(-EPS), math.log1p(EPS)


def _frames_with_log_weights(lw_target, A=6, seed=0):
    """Frames whose log weight under (loc, var) is exactly ``lw_target`` (float64): sample_log_prob is set from it."""
    g = torch.Generator().manual_seed(seed)
    B = lw_target.numel()
    loc = torch.randn(B, A, generator=g, dtype=torch.float64)
    var = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    action = loc + var.sqrt() * torch.randn(B, A, generator=g, dtype=torch.float64)
    logp = otr.mvn_diag_log_prob(action, loc, var) - lw_target
    return loc, var, {"action": action, "sample_log_prob": logp}


def test_gradient_is_zero_exactly_where_the_clipped_side_wins():
    # six regions: below / inside / above the bounds, each with a positive and a negative (normalised) advantage
    lw = torch.tensor([LO - 0.3, LO - 0.05, 0.0, 0.05, HI + 0.05, HI + 0.4] * 2, dtype=torch.float64)
    adv = torch.tensor([1.0] * 6 + [-1.0] * 6, dtype=torch.float64)
    loc, var, b = _frames_with_log_weights(lw)
    b["advantage"] = adv
    B = lw.numel()
    lw_leaf = lw.clone().requires_grad_(True)
    # d loss / d lw through the restatement: feed lw directly as a function of loc (a shift of the log-prob by lw_leaf - lw)
    out = ppo_loss(loc, var, b, None, clip_epsilon=EPS, entropy_coef=0.0, critic_coef=1.0, normalize_advantage=False)
    assert torch.allclose(out["lw"], lw, atol=1e-12)
    b2 = dict(b, sample_log_prob=b["sample_log_prob"] + lw - lw_leaf)   # lw(frame) == lw_leaf
    loss = ppo_loss(loc, var, b2, None, clip_epsilon=EPS, entropy_coef=0.0, critic_coef=1.0, normalize_advantage=False)["loss_objective"]
    (g,) = torch.autograd.grad(loss, lw_leaf)
    for k in range(B):
        clipped = (lw[k] > HI and adv[k] > 0) or (lw[k] < LO and adv[k] < 0)
        want = 0.0 if clipped else float(-adv[k] * lw[k].exp() / B)
        assert float(g[k]) == pytest.approx(want, abs=1e-15), (k, float(lw[k]), float(adv[k]))
    assert int((g == 0).sum()) == 4   # lw > hi with adv > 0 (2 frames), lw < lo with adv < 0 (2 frames)
    # value: -mean(min(r adv, clip(r) adv))
    r = lw.exp()
    rc = lw.clamp(LO, HI).exp()
    assert float(loss.detach()) == pytest.approx(float(-torch.minimum(r * adv, rc * adv).mean()), abs=1e-14)


def test_ppo_matches_trpl_oracle_when_neither_clips_nor_projects():
    """eps large (0.9: the bounds are log1p(-eps) = -2.3 and log1p(eps) = 0.64) and TRPL's bounds large: the projection is inactive
    (proj_p = p, trust-region loss 0) and nothing is clipped, so the two objectives, their entropies, critic losses, ESS and gradients
    agree."""
    g = torch.Generator().manual_seed(3)
    B, A = 40, 6
    loc0 = torch.randn(B, A, generator=g, dtype=torch.float64)
    var0 = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    lw = 0.1 * torch.randn(B, generator=g, dtype=torch.float64)   # well inside log1p(-0.9), log1p(0.9)
    _, _, b = _frames_with_log_weights(lw, A=A, seed=4)
    b.update(loc=loc0 + 0.01 * torch.randn(B, A, generator=g, dtype=torch.float64), var=var0,
             advantage=torch.randn(B, generator=g, dtype=torch.float64),
             state_value=torch.randn(B, generator=g, dtype=torch.float64), value_target=torch.randn(B, generator=g, dtype=torch.float64))
    loc_p, var_p = _frames_with_log_weights(lw, A=A, seed=4)[:2]
    value = torch.randn(B, generator=g, dtype=torch.float64)
    outs, grads = {}, {}
    for name in ("ppo", "trpl"):
        loc = loc_p.clone().requires_grad_(True)
        var = var_p.clone().requires_grad_(True)
        v = value.clone().requires_grad_(True)
        if name == "ppo":
            o = ppo_loss(loc, var, b, v, clip_epsilon=0.9, entropy_coef=0.01, critic_coef=0.5, clip_value=0.2)
            actor = o["loss_objective"] + o["loss_entropy"]
        else:
            o = otr.trpl_loss(loc, var, b, v, mean_bound=1e6, cov_bound=1e6, trust_region_coeff=1.0, entropy_coef=0.01, critic_coef=0.5,
                              clip_value=0.2)
            assert float(o["loss_trust_region"]) == pytest.approx(0.0, abs=1e-12)
            o["entropy"] = o["entropy_dist"]
            actor = o["loss_objective"] + o["loss_entropy"] + o["loss_trust_region"]
        ga = torch.autograd.grad(actor, [loc, var])
        gc = torch.autograd.grad(o["loss_critic"], [v])
        outs[name], grads[name] = o, ga + gc
    assert float(outs["ppo"]["lw"].abs().max()) < 0.6
    for k in ("loss_objective", "loss_entropy", "entropy", "loss_critic", "ESS"):
        assert float(outs["ppo"][k]) == pytest.approx(float(outs["trpl"][k]), rel=1e-12, abs=1e-12), k
    for a, b_ in zip(grads["ppo"], grads["trpl"]):
        assert torch.allclose(a, b_, rtol=1e-10, atol=1e-14)


class _Spec:
    in_features = ["scalars", "vectors"]


class _HD:
    spec = _Spec()


class _Actor(torch.nn.Module):
    hyper_data = _HD()

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward_diag(self, *a, **k):
        raise NotImplementedError


class _Critic(torch.nn.Module):
    _network1 = None


# examples/torchrl/builders/agent.py:53-64 with configs/algorithm/objective/default.yaml
REF_KW = dict(clip_epsilon=0.2, loss_critic_type="l2", entropy_coef=0.0, entropy_bonus=True, critic_coef=1.0, clip_value=0.2,
              normalize_advantage=True)


def test_construction_with_the_reference_builder_arguments():
    from geometry_rl_amd.ppo import ClipPPOLoss2
    loss = ClipPPOLoss2(actor_network=_Actor(), critic_network=_Critic(), **REF_KW)
    assert loss.out_keys == ["loss_objective", "entropy", "loss_entropy", "loss_critic", "ESS"]
    assert "clip_epsilon" in dict(loss.named_buffers())
    assert loss.clip_epsilon.dtype == torch.float32 and loss.clip_epsilon.dim() == 0
    assert float(loss.clip_epsilon) == pytest.approx(0.2)
    loss.clip_epsilon.copy_(0.2 * 0.5)   # train.py:272-274 anneal: in place
    assert float(loss.clip_epsilon) == pytest.approx(0.1)
    assert loss.in_features == ["scalars", "vectors"] and loss.algorithm == "ppo"
    no_bonus = ClipPPOLoss2(_Actor(), _Critic(), **dict(REF_KW, entropy_bonus=False))
    assert no_bonus.out_keys == ["loss_objective", "loss_critic", "ESS"]


@pytest.mark.parametrize("kind", ["smooth_l1", "l1", None])
def test_only_the_l2_critic_loss_is_built(kind):
    from geometry_rl_amd.ppo import ClipPPOLoss2
    kw = dict(REF_KW)
    if kind is None:
        kw.pop("loss_critic_type")   # the reference's default, smooth_l1
    else:
        kw["loss_critic_type"] = kind
    with pytest.raises(NotImplementedError):
        ClipPPOLoss2(_Actor(), _Critic(), **kw)


def test_build_agent_ppo_returns_no_projection():
    from geometry_rl_amd import agent, graph
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, algorithm="ppo", clip_epsilon=0.15)
    actor, critic, proj, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    from geometry_rl_amd.ppo import ClipPPOLoss2
    assert proj is None and isinstance(loss, ClipPPOLoss2)
    assert float(loss.clip_epsilon) == pytest.approx(0.15) and loss.actor_network is actor
    assert agent.AgentConfig().algorithm == "trpl" and agent.AgentConfig().clip_epsilon == 0.2
    with pytest.raises(ValueError):
        agent.build_agent(graph.rigid_spec(), agent.AgentConfig(algorithm="kl_ppo"), device="cpu")


def test_loss_module_branch_on_stub_packages():
    code = """
        import torch, tensordict, torchrl.objectives as tro
        from geometry_rl_amd import ppo, trpl
        assert ppo._LossBase is tro.LossModule and issubclass(ppo.ClipPPOLoss2, tro.LossModule)
        class Spec: in_features = ["a", "b"]
        class HD: spec = Spec()
        class Actor(torch.nn.Module):
            hyper_data = HD()
            def forward_diag(self, *a, **k): raise NotImplementedError
        class Critic(torch.nn.Module):
            _network1 = None
        loss = ppo.ClipPPOLoss2(actor_network=Actor(), critic_network=Critic(), clip_epsilon=0.2, loss_critic_type="l2", entropy_coef=0.0,
                                entropy_bonus=True, critic_coef=1.0, clip_value=0.2, normalize_advantage=True)
        assert isinstance(loss, tro.LossModule) and loss.out_keys[0] == "loss_objective"
        assert "clip_epsilon" in dict(loss.named_buffers())
        print("ok")
    """
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests", "stubs"), ROOT, env.get("PYTHONPATH", "")])
    p = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "ok" in p.stdout
