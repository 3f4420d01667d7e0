"""The adaptive KL-penalty PPO objective without a GPU: the closed-form KL of the restatement (tests/klpen_ref.py) against
torch.distributions (value AND direction), hand-computed values of the loss and its gradient, the beta rule at its thresholds, and the
construction of geometry_rl_amd.klpen.KLPENPPOLoss as the reference builder calls it (examples/torchrl/builders/agent.py:65-78 with
configs/algorithm/objective/kl_ppo.yaml)."""
import math

import pytest
import torch

from klpen_ref import adapt_beta, kl_old_new, klpen_loss, thresholds


def test_closed_form_kl_is_torchs_kl_of_old_against_new():
    from torch.distributions import MultivariateNormal, kl_divergence
    g = torch.Generator().manual_seed(0)
    B, A = 33, 6
    mo = torch.randn(B, A, generator=g, dtype=torch.float64)
    So = torch.rand(B, A, generator=g, dtype=torch.float64) * 2 + 0.25
    mean = mo + 0.3 * torch.randn(B, A, generator=g, dtype=torch.float64)
    S = So * torch.exp2(4 * torch.rand(B, A, generator=g, dtype=torch.float64) - 2)   # up to 4x either way
    got = kl_old_new(mo, So, mean, S)
    want = kl_divergence(MultivariateNormal(mo, torch.diag_embed(So)), MultivariateNormal(mean, torch.diag_embed(S)))
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)
    # the formula of the kernel's header, term by term
    form = 0.5 * (So / S + (mean - mo) ** 2 / S - 1 + S.log() - So.log()).sum(-1)
    assert torch.allclose(got, form, rtol=1e-12, atol=1e-13)
    # the direction is pinned: the reverse KL is a different number on these frames
    rev = kl_divergence(MultivariateNormal(mean, torch.diag_embed(S)), MultivariateNormal(mo, torch.diag_embed(So)))
    assert float((got - rev).abs().min()) > 1e-3


def test_kl_is_exactly_zero_where_new_equals_old():
    g = torch.Generator().manual_seed(1)
    for dtype in (torch.float64, torch.float32):
        mo = torch.randn(9, 12, generator=g, dtype=dtype)
        So = torch.rand(9, 12, generator=g, dtype=dtype) + 0.1
        assert bool((kl_old_new(mo, So, mo.clone(), So.clone()) == 0).all())


def test_hand_computed_two_frames():
    """A = 2, B = 2, no advantage normalisation, beta = 3:
      frame 0: new == old, action == mean, old log-prob == new log-prob  ->  lw = 0, kl_f = 0, term = -adv0
      frame 1: mo = (0, 0), So = (1, 1), mean = (1, 0), S = (1, 4), action = mean, sample_log_prob chosen so that lw = log 2
               kl_f = 1/2 [(1 + 1 - 1 + 0) + (1/4 + 0 - 1 + log 4)] = 1/2 [1/4 + log 4]"""
    beta = 3.0
    adv = torch.tensor([0.5, -2.0], dtype=torch.float64)
    mo = torch.tensor([[0.3, -0.2], [0.0, 0.0]], dtype=torch.float64)
    So = torch.tensor([[0.5, 2.0], [1.0, 1.0]], dtype=torch.float64)
    loc = torch.tensor([[0.3, -0.2], [1.0, 0.0]], dtype=torch.float64, requires_grad=True)
    var = torch.tensor([[0.5, 2.0], [1.0, 4.0]], dtype=torch.float64, requires_grad=True)
    action = loc.detach().clone()
    logp_new = -0.5 * (2 * math.log(2 * math.pi) + var.detach().log().sum(-1))
    batch = {"action": action, "loc": mo, "var": So, "advantage": adv, "value_target": torch.tensor([1.0, -1.0], dtype=torch.float64),
             "sample_log_prob": logp_new - torch.tensor([0.0, math.log(2.0)], dtype=torch.float64)}
    value = torch.tensor([1.5, 1.0], dtype=torch.float64, requires_grad=True)
    out = klpen_loss(loc, var, batch, value, beta, entropy_coef=0.0, critic_coef=0.5, normalize_advantage=False)
    kl1 = 0.5 * (0.25 + math.log(4.0))
    assert float(out["kl_f"][0]) == 0.0 and float(out["kl_f"][1]) == pytest.approx(kl1, abs=1e-15)
    assert float(out["kl"]) == pytest.approx(kl1 / 2, abs=1e-15)
    want = 0.5 * ((-1.0 * 0.5 + 0.0) + (-2.0 * -2.0 + beta * kl1))
    assert float(out["loss_objective"].detach()) == pytest.approx(want, abs=1e-14)
    assert float(out["loss_critic"].detach()) == pytest.approx(0.5 * 0.5 * (0.25 + 4.0), abs=1e-15)   # plain l2, nothing clipped
    d_loc, d_var = torch.autograd.grad(out["loss_objective"], [loc, var])
    # frame 0: action == mean -> d lw / d mean = 0; d lw / d S_i = -1 / (2 S_i); KL term's gradient 0 at new == old
    assert d_loc[0].tolist() == [0.0, 0.0]
    assert d_var[0].tolist() == pytest.approx([0.5 * 0.5 * 1.0 / (2 * 0.5), 0.5 * 0.5 * 1.0 / (2 * 2.0)], abs=1e-15)
    # frame 1: objective -e^lw adv = 4: d/dS_i = -4 * (-1 / (2 S_i)) ... times 1/B; KL: dKL/dmean = (mean - mo) / S, dKL/dS = (1/S - So/S^2 - d^2/S^2) / 2
    assert d_loc[1].tolist() == pytest.approx([0.5 * beta * 1.0 / 1.0, 0.0], abs=1e-15)
    o1 = [0.5 * (2.0 * -2.0) * (-1 / (2 * 1.0)) * -1, 0.5 * (2.0 * -2.0) * (-1 / (2 * 4.0)) * -1]   # 1/B * (-e^lw adv) * d lw / d S
    k1 = [0.5 * beta * 0.5 * (1.0 - 1.0 - 1.0), 0.5 * beta * 0.5 * (1 / 4.0 - 1 / 16.0)]
    assert d_var[1].tolist() == pytest.approx([o1[0] + k1[0], o1[1] + k1[1]], abs=1e-15)


def test_adapt_beta_branches_and_thresholds():
    dtarg = 0.01
    hi, lo = thresholds(dtarg)
    assert hi == float(torch.tensor(0.015).float()) and lo == float(torch.tensor(0.01 / 1.5).float())
    assert adapt_beta(1.0, 0.02, dtarg, 2.0, 0.5) == 2.0
    assert adapt_beta(1.0, 0.01, dtarg, 2.0, 0.5) == 1.0
    assert adapt_beta(1.0, 0.004, dtarg, 2.0, 0.5) == 0.5
    up = float(torch.nextafter(torch.tensor(hi), torch.tensor(1.0)))
    down = float(torch.nextafter(torch.tensor(lo), torch.tensor(0.0)))
    # strict inequalities: AT a threshold nothing changes, one float32 beyond it beta moves
    assert adapt_beta(3.0, hi, dtarg, 2.0, 0.5) == 3.0 and adapt_beta(3.0, up, dtarg, 2.0, 0.5) == 6.0
    assert adapt_beta(3.0, lo, dtarg, 2.0, 0.5) == 3.0 and adapt_beta(3.0, down, dtarg, 2.0, 0.5) == 1.5
    from geometry_rl_amd import ops
    assert ops.klpen_thresholds(dtarg) == (hi, lo)


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


# examples/torchrl/builders/agent.py:65-78 with configs/algorithm/objective/kl_ppo.yaml
REF_KW = dict(dtarg=0.01, loss_critic_type="l2", entropy_coef=0.0, entropy_bonus=True, critic_coef=1.0, normalize_advantage=True)


def test_construction_and_beta_travels_in_the_state_dict():
    from geometry_rl_amd import KLPENPPOLoss
    from geometry_rl_amd.klpen import KLPENPPOLoss as direct
    assert KLPENPPOLoss is direct
    loss = KLPENPPOLoss(actor_network=_Actor(), critic_network=_Critic(), **REF_KW)
    assert loss.algorithm == "kl_ppo" and loss.out_keys == ["loss_objective", "kl", "entropy", "loss_entropy", "loss_critic"]
    assert "ESS" not in loss.out_keys
    assert (loss.dtarg, loss.increment, loss.decrement, float(loss.beta)) == (0.01, 2.0, 0.5, 1.0)
    assert loss.beta.dtype == torch.float32 and loss.beta.dim() == 0 and "beta" in dict(loss.named_buffers())
    assert "beta" in loss.state_dict()
    loss.beta.fill_(8.0)
    other = KLPENPPOLoss(_Actor(), _Critic(), samples_mc_kl=7, **REF_KW)
    other.load_state_dict(loss.state_dict())
    assert float(other.beta) == 8.0
    assert KLPENPPOLoss(_Actor(), _Critic(), **dict(REF_KW, entropy_bonus=False)).out_keys == ["loss_objective", "kl", "loss_critic"]


@pytest.mark.parametrize("kind", ["smooth_l1", "l1", None])
def test_only_the_l2_critic_loss_is_built(kind):
    from geometry_rl_amd.klpen import KLPENPPOLoss
    kw = dict(REF_KW)
    if kind is None:
        kw.pop("loss_critic_type")   # torchrl's default, smooth_l1
    else:
        kw["loss_critic_type"] = kind
    with pytest.raises(NotImplementedError):
        KLPENPPOLoss(_Actor(), _Critic(), **kw)


def test_a_minibatch_without_the_old_distribution_is_refused_by_name():
    from geometry_rl_amd.klpen import KLPENPPOLoss
    loss = KLPENPPOLoss(_Actor(), _Critic(), **REF_KW)
    td = {"scalars": torch.zeros(2, 3), "vectors": torch.zeros(2, 3), "action": torch.zeros(2, 6), "sample_log_prob": torch.zeros(2),
          "advantage": torch.zeros(2), "value_target": torch.zeros(2)}
    with pytest.raises(ValueError, match="'loc' and 'var'"):
        loss(dict(td))
    with pytest.raises(ValueError, match="'loc' and 'var'"):
        loss(dict(td, loc=torch.zeros(2, 6)))
    with pytest.raises(NotImplementedError):   # with both keys the check passes (the stub actor is reached)
        loss(dict(td, loc=torch.zeros(2, 6), var=torch.ones(2, 6)))


def test_build_agent_kl_ppo():
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.klpen import KLPENPPOLoss
    kw = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, algorithm="kl_ppo")
    cfg = agent.AgentConfig(dtarg=0.01, kl_beta=0.5, kl_increment=1.5, kl_decrement=0.25, **kw)
    actor, critic, proj, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    assert proj is None and isinstance(loss, KLPENPPOLoss) and loss.actor_network is actor
    assert loss.clip_value is None
    assert (loss.dtarg, float(loss.beta), loss.increment, loss.decrement) == (0.01, 0.5, 1.5, 0.25)
    d = agent.AgentConfig()
    assert (d.dtarg, d.kl_beta, d.kl_increment, d.kl_decrement) == (None, 1.0, 2.0, 0.5)
    with pytest.raises(ValueError, match="dtarg"):
        agent.build_agent(graph.rigid_spec(), agent.AgentConfig(**kw), device="cpu")
