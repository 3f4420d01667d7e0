"""The non-commuting Wasserstein projection (proj_type "w2_non_com") off the GPU:
  * the float64 restatement (tests/w2nc_ref.py) against the reference layer's own outputs and gradients (tier2f fixture, reference code
    under the tier-2 stubs plus the symeig shim), unconverged Newton-Schulz frames included;
  * the frame inside the bound with equal ratios S / S_o, where the reference's autograd gives NaN: pass-through;
  * the restatement's autograd against central finite differences;
  * the factory and build_agent reach the fused kernel's code 4."""
import os

import numpy as np
import pytest
import torch

import w2nc_ref
from oracle import trpl as otr

GROUPS = ("a6", "a3", "a12")


def _load(golden_dir):
    z = np.load(os.path.join(golden_dir, "tier2f_projection_w2_non_com.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _close(name, got, want, tol, rows=None):
    got, want = got.detach().double(), want.double()
    if rows is not None:
        got, want = got[rows], want[rows]
    err = float((got - want).abs().max()) if got.numel() else 0.0
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    assert np.isfinite(err) and err <= tol * scale, (name, err, tol * scale)


@pytest.mark.parametrize("grp", GROUPS)
def test_restatement_matches_the_reference_layer(golden_dir, grp):
    z = {k[len(grp) + 1:]: v for k, v in _load(golden_dir).items() if k.startswith(grp + ".")}
    z0 = _load(golden_dir)
    eps, eps_cov, coeff = float(z0["mean_bound"]), float(z0["cov_bound"]), float(z0["coeff"])
    mean = z["mean"].clone().requires_grad_(True)
    S = z["S"].clone().requires_grad_(True)
    q = (z["mean_o"], z["S_o"])
    pm, pS = w2nc_ref.projection((mean, S), q, eps, eps_cov)
    _close("proj_mean", pm, z["proj_mean"], 1e-12)
    _close("proj_S", pS, z["proj_S"], 1e-12)
    gm, gS = torch.autograd.grad((pm * z["R1"]).sum() + (pS * z["R2"]).sum(), [mean, S])
    finite = torch.isfinite(z["grad_mean"]).all(-1) & torch.isfinite(z["grad_S"]).all(-1)
    assert int(finite.sum()) >= len(finite) - 1   # only the equal-ratio frame of group a6 is NaN in the reference
    _close("grad_mean", gm, z["grad_mean"], 1e-10, finite)
    _close("grad_S", gS, z["grad_S"], 1e-10, finite)
    # trust-region regression loss (base_projection_layer.py:292-327): coeff * mean(value(p, stopgrad(proj_p)))
    md, cd = w2nc_ref.value((mean, S), (pm.detach(), pS.detach()))
    tr = (md + cd).mean() * coeff
    _close("tr_loss", tr, z["tr_loss"], 1e-12)
    tgm, tgS = torch.autograd.grad(tr, [mean, S])
    _close("tr_grad_mean", tgm, z["tr_grad_mean"], 1e-10)
    _close("tr_grad_S", tgS, z["tr_grad_S"], 1e-10)
    # metrics of (p, proj_p) and trust_region_value(p, q)
    with torch.no_grad():
        p_, t_ = (z["mean"], z["S"]), (pm.detach(), pS.detach())
        km, kc = otr.gaussian_kl(p_, t_)
        m_, c_ = w2nc_ref.value(p_, t_)
        want = {"kl": (km + kc).mean(), "constraint": (m_ + c_).mean(), "mean_constraint": m_.mean(), "cov_constraint": c_.mean(),
                "mean_constraint_max": m_.max(), "cov_constraint_max": c_.max(), "entropy": otr.entropy_std(z["S"]).mean(),
                "entropy_diff": (otr.entropy_std(pS) - otr.entropy_std(z["S"])).mean()}
        for k, v in want.items():
            _close("metric." + k, v, z["metric." + k], 1e-12)
        vm, vc = w2nc_ref.value(p_, q)
        _close("value_mean", vm, z["value_mean"], 1e-12)
        _close("value_cov", vc, z["value_cov"], 1e-12)


def test_fixture_covers_both_sides_and_the_unconverged_frames(golden_dir):
    z = _load(golden_dir)
    eps, eps_cov = float(z["mean_bound"]), float(z["cov_bound"])
    for grp in GROUPS:
        tot = z[f"{grp}.value_mean"] + z[f"{grp}.value_cov"]
        assert bool((tot <= eps + eps_cov).any()) and bool((tot > 2 * (eps + eps_cov)).any()), grp
    r = z["a6.x_over_n"]
    assert abs(float(r[3].min()) / 1e-3 - 1) < 1e-3 and abs(float(r[4].min()) / 1e-4 - 1) < 1e-3
    # the ten steps are the reference's semantics: far from an exact square root on these two frames, and the reference agrees
    pm, pS = w2nc_ref.projection((z["a6.mean"], z["a6.S"]), (z["a6.mean_o"], z["a6.S_o"]), eps, eps_cov)
    _, pS_exact = w2nc_ref.projection((z["a6.mean"], z["a6.S"]), (z["a6.mean_o"], z["a6.S_o"]), eps, eps_cov, sqrt_fn=torch.sqrt)
    low = 1.0 - z["a6.proj_S"] / pS_exact
    assert 0.023 < float(low[3, 0]) < 0.026         # 2.4 % low at x / n = 1e-3 (scalar iteration from Y = 1e-3: 2.43 %)
    assert 0.45 < float(low[4, 0]) < 0.5            # 47 % low at 1e-4
    assert float(low[3, 1:].abs().max()) < 1e-6     # the other dimensions have converged


def test_equal_ratio_frame_inside_the_bound_passes_the_gradient_through(golden_dir):
    z = _load(golden_dir)
    S, S_o = z["a6.S"][2], z["a6.S_o"][2]
    assert bool((S / S_o == (S / S_o)[0]).all())                                   # one ratio in every dimension
    assert not bool(torch.isfinite(z["a6.grad_S"][2]).all())                      # the reference's autograd: NaN
    mean = z["a6.mean"].clone().requires_grad_(True)
    Sg = z["a6.S"].clone().requires_grad_(True)
    pm, pS = w2nc_ref.projection((mean, Sg), (z["a6.mean_o"], z["a6.S_o"]), float(z["mean_bound"]), float(z["cov_bound"]))
    assert torch.equal(pm[2], z["a6.mean"][2]) and torch.equal(pS[2], z["a6.S"][2])
    gm, gS = torch.autograd.grad((pm * z["a6.R1"]).sum() + (pS * z["a6.R2"]).sum(), [mean, Sg])
    assert torch.equal(gm[2], z["a6.R1"][2]) and torch.equal(gS[2], z["a6.R2"][2])


def test_restatement_gradient_matches_finite_differences():
    g = torch.Generator().manual_seed(7)
    B, A = 6, 5
    mean = torch.randn(B, A, generator=g, dtype=torch.float64)
    S = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    mean_o = mean + 0.3 * torch.randn(B, A, generator=g, dtype=torch.float64)
    S_o = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    S_o[1, 0] = 0.02                       # x_0 / n small: an unconverged dimension (the coupling through n matters)
    mean_o[2] = mean[2] + 1e-3
    S_o[2] = S[2] * (1 + 1e-3 * torch.arange(A, dtype=torch.float64))   # inside the bound
    R1, R2 = torch.randn(B, A, generator=g, dtype=torch.float64), torch.randn(B, A, generator=g, dtype=torch.float64)

    def f(m, s):
        pm, pS = w2nc_ref.projection((m, s), (mean_o, S_o), 0.05, 0.0025)
        return (pm * R1).sum() + (pS * R2).sum()

    m_ = mean.clone().requires_grad_(True)
    s_ = S.clone().requires_grad_(True)
    gm, gS = torch.autograd.grad(f(m_, s_), [m_, s_])
    h = 1e-6
    for which, x, gx in (("mean", mean, gm), ("S", S, gS)):
        fd = torch.empty_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.clone(), x.clone()
            xp[idx] += h
            xm[idx] -= h
            with torch.no_grad():
                fp = f(xp, S) if which == "mean" else f(mean, xp)
                fm = f(xm, S) if which == "mean" else f(mean, xm)
            fd[idx] = (fp - fm) / (2 * h)
        err = float((fd - gx).abs().max())
        print(which, "max |fd - autograd|", err)
        assert err <= 1e-6 * max(1.0, float(gx.abs().max())), (which, err)


def test_factory_and_kernel_code():
    from geometry_rl_amd import trpl
    kw = dict(action_dim=6, total_train_steps=1000, cpu=False, dtype=torch.float32, mean_bound=0.05, cov_bound=0.0005, trust_region_coeff=1.0,
              scale_prec=True, entropy_schedule=False, target_entropy=0.0, temperature=0.5, entropy_eq=False, entropy_first=False)
    layer = trpl.get_projection_layer(proj_type="w2_non_com", **kw)
    assert type(layer) is trpl.WassersteinProjectionLayerNonCommuting and layer.proj_code == 4 and layer.cov_bound == 0.0005
    assert isinstance(layer, trpl.KLProjectionLayer) and layer.entropy_schedule_type is None
    assert trpl.KLProjectionLayer(proj_type="w2_non_com", **kw).proj_code == 4
    for name in ("kl", "frob", "w2"):   # unchanged
        assert type(trpl.get_projection_layer(proj_type=name, **kw)).__name__ != "WassersteinProjectionLayerNonCommuting"
    for name in ("papi", "ppo"):
        with pytest.raises(NotImplementedError):
            trpl.get_projection_layer(name, **kw)
    with pytest.raises(NotImplementedError):
        trpl.get_projection_layer("w2_non_com", **dict(kw, scale_prec=False))
    with pytest.raises(NotImplementedError):
        trpl.get_projection_layer("w2_non_com", **dict(kw, mean_eq=True))
    # trust_region_value: the per-frame value, on matrices or diagonals
    g = torch.Generator().manual_seed(2)
    m, s, mo, so = torch.randn(4, 6, generator=g), torch.rand(4, 6, generator=g) + 0.5, torch.randn(4, 6, generator=g), torch.rand(4, 6, generator=g) + 0.5
    a = layer.trust_region_value(None, (m, s.diag_embed()), (mo, so.diag_embed()))
    b = otr.wasserstein_value((m, s), (mo, so))
    assert torch.allclose(a[0], b[0]) and torch.allclose(a[1], b[1])


def test_build_agent_reaches_code_4():
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.trpl import KLProjectionLayer, TRPLLoss
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, proj_type="w2_non_com")
    actor, critic, proj, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    assert isinstance(loss, TRPLLoss) and loss.projection is proj and type(proj) is KLProjectionLayer and proj.proj_code == 4
