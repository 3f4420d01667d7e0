"""tests/bc_ref.py (the float64 restatement the behaviour-cloning kernel modes are tested against) held to torch's own ``nn.MSELoss`` and
``Independent(Normal(mu, sigma), 1).log_prob``, gradients by autograd, everything in float64 on the same inputs: 1e-12 relative."""
import pytest
import torch

import bc_ref
from trpl_cases import A_SWEEP

RTOL = 1e-12   # both sides are float64 evaluations of the same expressions on the same inputs
B = 37


def _eq(name, got, want):
    torch.testing.assert_close(got.double(), want.double(), rtol=RTOL, atol=0.0, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("A", A_SWEEP)
@pytest.mark.parametrize("global_batch", [None, 3 * B + 1])
def test_regression_is_mse_loss(A, global_batch):
    d = bc_ref.make_case(B, A)
    ref = bc_ref.bc_reference(d["loc"], d["sigma"], d["action"], "mse", global_batch)
    mu = d["loc"].double().requires_grad_(True)
    sg = d["sigma"].double().requires_grad_(True)
    loss = torch.nn.MSELoss()(mu, d["action"].double()) * (B / (global_batch or B))
    (g_mu,) = torch.autograd.grad(loss, [mu])
    _eq("loss", ref["loss"], loss.detach())
    _eq("dloc", ref["dloc"], g_mu)
    assert not bool(ref["dsigma"].any()) and ref["dsigma"].shape == sg.shape   # (the std takes no part: torch would hand out no gradient)
    _eq("mse", ref["report"][1], torch.nn.MSELoss()(mu, d["action"].double()).detach())
    _eq("se", ref["se"], ((mu - d["action"].double()) ** 2).sum(-1).detach())
    assert float(ref["maxes"][0]) == float(ref["se"].max()) and float(ref["sums"][10]) == B


@pytest.mark.parametrize("A", A_SWEEP)
@pytest.mark.parametrize("global_batch", [None, 3 * B + 1])
def test_nll_is_minus_log_prob(A, global_batch):
    from torch.distributions import Independent, MultivariateNormal, Normal
    d = bc_ref.make_case(B, A)
    ref = bc_ref.bc_reference(d["loc"], d["sigma"], d["action"], "nll", global_batch)
    mu = d["loc"].double().requires_grad_(True)
    sg = d["sigma"].double().requires_grad_(True)
    dist = Independent(Normal(mu, sg), 1)
    nll = -dist.log_prob(d["action"].double())
    loss = nll.sum() / (global_batch or B)
    g_mu, g_sg = torch.autograd.grad(loss, [mu, sg])
    _eq("nll", ref["nll"], nll.detach())
    _eq("loss", ref["loss"], loss.detach())
    _eq("dloc", ref["dloc"], g_mu)
    _eq("dsigma", ref["dsigma"], g_sg)
    _eq("entropy", ref["entropy"], dist.entropy().detach())
    # the issue's wording of the same density: MultivariateNormal(mu, diag(sigma^2)) (its Cholesky path costs a few more roundings)
    mvn = -MultivariateNormal(mu.detach(), covariance_matrix=(sg.detach() ** 2).diag_embed()).log_prob(d["action"].double())
    torch.testing.assert_close(ref["nll"], mvn, rtol=1e-9, atol=0.0)


def test_cases_hold_every_regime():
    """All nine (sigma, deviation) pairs occur in a case of 9 frames or more, the zero deviation bitwise."""
    d = bc_ref.make_case(B, 6)
    dev = (d["action"].double() - d["loc"].double()).abs()
    seen = set()
    for f in range(B):
        s = min(bc_ref.SIGMAS, key=lambda x: abs(float(d["sigma"][f, 0]) / x - 1.0))
        v = min(bc_ref.DEVIATIONS, key=lambda x: abs(float(dev[f, 0]) - x))
        assert 0.5 <= float(d["sigma"][f].min()) / s and float(d["sigma"][f].max()) / s < 1.5
        if v == 0.0:
            assert torch.equal(d["action"][f], d["loc"][f])
        seen.add((s, v))
    assert len(seen) == 9
