"""The Euclidean (``scale_prec=False``) forms of the Frobenius and the commutative Wasserstein projection off the GPU:
  * the float64 restatements (tests/euclid_ref.py) against the reference layers' own outputs and gradients (tier2g fixtures: reference
    code under the tier-2 stubs, float64 on float32-representable inputs), at the tolerances of tests/test_w2nc_cpu.py;
  * the restatements' autograd against central finite differences (step and bar of that file);
  * the fixtures hold every activity state (mean bound active or not x covariance bound active or not) in every group, no part within a
    relative 1e-3 of its bound;
  * the factory and build_agent reach the fused kernel's codes 6 and 7, "kl" stays code 0 either way, the refusals stay."""
import os

import numpy as np
import pytest
import torch

import euclid_ref
from oracle import trpl as otr

GROUPS = ("a6", "a3", "a12")
NAMES = ("frob", "w2")


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"tier2g_projection_{name}_euclid.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _close(name, got, want, tol):
    got, want = got.detach().double(), want.double()
    err = float((got - want).abs().max()) if got.numel() else 0.0
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    assert np.isfinite(err) and err <= tol * scale, (name, err, tol * scale)


@pytest.mark.parametrize("grp", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_layer(golden_dir, name, grp):
    z0 = _load(golden_dir, name)
    z = {k[len(grp) + 1:]: v for k, v in z0.items() if k.startswith(grp + ".")}
    eps, eps_cov, coeff = float(z0["mean_bound"]), float(z0["cov_bound"]), float(z0["coeff"])
    project, value, tr_loss = euclid_ref.PROJECTION[name], euclid_ref.VALUE[name], euclid_ref.TR_LOSS[name]
    mean = z["mean"].clone().requires_grad_(True)
    S = z["S"].clone().requires_grad_(True)
    q = (z["mean_o"], z["S_o"])
    pm, pS = project((mean, S), q, eps, eps_cov)
    _close("proj_mean", pm, z["proj_mean"], 1e-12)
    _close("proj_S", pS, z["proj_S"], 1e-12)
    gm, gS = torch.autograd.grad((pm * z["R1"]).sum() + (pS * z["R2"]).sum(), [mean, S], retain_graph=True)
    assert bool(torch.isfinite(z["grad_mean"]).all()) and bool(torch.isfinite(z["grad_S"]).all())
    _close("grad_mean", gm, z["grad_mean"], 1e-10)
    _close("grad_S", gS, z["grad_S"], 1e-10)
    # trust-region regression loss: Frobenius -- the layer's own (projection NOT detached); W2 -- the base class's on the detached projection
    tr = tr_loss((mean, S), (pm, pS), coeff)
    _close("tr_loss", tr, z["tr_loss"], 1e-12)
    tgm, tgS = torch.autograd.grad(tr, [mean, S])
    _close("tr_grad_mean", tgm, z["tr_grad_mean"], 1e-10)
    _close("tr_grad_S", tgS, z["tr_grad_S"], 1e-10)
    # metrics of (p, proj_p) and trust_region_value(p, q)
    with torch.no_grad():
        p_, t_ = (z["mean"], z["S"]), (pm.detach(), pS.detach())
        km, kc = otr.gaussian_kl(p_, t_)
        m_, c_ = value(p_, t_)
        ent, ent_t = otr.entropy_std(z["S"]), otr.entropy_std(pS)
        want = {"kl": (km + kc).mean(), "constraint": (m_ + c_).mean(), "mean_constraint": m_.mean(), "cov_constraint": c_.mean(),
                "entropy": ent.mean(), "entropy_diff": (ent_t - ent).mean(), "kl_max": (km + kc).max(), "constraint_max": (m_ + c_).max(),
                "mean_constraint_max": m_.max(), "cov_constraint_max": c_.max(), "entropy_max": ent.max(),
                "entropy_diff_max": (ent_t - ent).max()}
        assert set(want) == {k[len("metric."):] for k in z if k.startswith("metric.")}
        for k, v in want.items():
            _close("metric." + k, v, z["metric." + k], 1e-12)
        vm, vc = value(p_, q)
        _close("value_mean", vm, z["value_mean"], 1e-12)
        _close("value_cov", vc, z["value_cov"], 1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_holds_every_activity_state_away_from_the_bounds(golden_dir, name):
    z = _load(golden_dir, name)
    eps, eps_cov = float(z["mean_bound"]), float(z["cov_bound"])
    for grp in GROUPS:
        assert z[f"{grp}.mean"].shape[0] == 11 and z[f"{grp}.mean"].dtype == torch.float64
        # float64 values of the parts, from the inputs (not from the recorded values)
        mp, cp = euclid_ref.VALUE[name]((z[f"{grp}.mean"], z[f"{grp}.S"]), (z[f"{grp}.mean_o"], z[f"{grp}.S_o"]))
        states = {(bool(a), bool(b)) for a, b in zip(mp > eps, cp > eps_cov)}
        assert states == {(False, False), (False, True), (True, False), (True, True)}, (grp, states)
        assert float((mp / eps - 1.0).abs().min()) > 1e-3 and float((cp / eps_cov - 1.0).abs().min()) > 1e-3, grp
        # the hand-placed rows are where they are meant to be
        assert (bool(mp[0] > eps), bool(cp[0] > eps_cov)) == (False, True)
        assert (bool(mp[1] > eps), bool(cp[1] > eps_cov)) == (True, False)
        assert (bool(mp[2] > eps), bool(cp[2] > eps_cov)) == (False, False)
        # and the projection moved exactly the active parts
        moved_m = (z[f"{grp}.proj_mean"] != z[f"{grp}.mean"]).any(-1)
        moved_c = (z[f"{grp}.proj_S"] != z[f"{grp}.S"]).any(-1)
        assert torch.equal(moved_m, mp > eps) and torch.equal(moved_c, cp > eps_cov), grp


@pytest.mark.parametrize("name", NAMES)
def test_restatement_gradient_matches_finite_differences(name):
    g = torch.Generator().manual_seed(7)
    B, A = 6, 5
    mean = torch.randn(B, A, generator=g, dtype=torch.float64)
    S = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    mean_o = mean + 0.3 * torch.randn(B, A, generator=g, dtype=torch.float64)
    S_o = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    mean_o[1] = mean[1] + 1e-3                                            # inside the mean bound only
    S_o[2] = S[2] * (1 + 1e-3 * torch.arange(A, dtype=torch.float64))    # inside the covariance bound only
    mean_o[3] = mean[3] - 1e-3                                            # inside both
    S_o[3] = S[3] * (1 - 1e-3 * torch.arange(A, dtype=torch.float64))
    R1, R2 = torch.randn(B, A, generator=g, dtype=torch.float64), torch.randn(B, A, generator=g, dtype=torch.float64)
    mp, cp = euclid_ref.VALUE[name]((mean, S), (mean_o, S_o))
    assert len({(bool(a), bool(b)) for a, b in zip(mp > 0.05, cp > 0.0025)}) == 4

    def f(m, s):
        pm, pS = euclid_ref.PROJECTION[name]((m, s), (mean_o, S_o), 0.05, 0.0025)
        return (pm * R1).sum() + (pS * R2).sum() + euclid_ref.TR_LOSS[name]((m, s), (pm, pS), 1.7)

    m_ = mean.clone().requires_grad_(True)
    s_ = S.clone().requires_grad_(True)
    gm, gS = torch.autograd.grad(f(m_, s_), [m_, s_])
    # the W2 regression loss sees a DETACHED projection: its finite difference must hold the target fixed
    with torch.no_grad():
        pm0, pS0 = euclid_ref.PROJECTION[name]((mean, S), (mean_o, S_o), 0.05, 0.0025)

    def f_fd(m, s):
        pm, pS = euclid_ref.PROJECTION[name]((m, s), (mean_o, S_o), 0.05, 0.0025)
        target = (pm, pS) if name == "frob" else (pm0, pS0)
        return (pm * R1).sum() + (pS * R2).sum() + euclid_ref.TR_LOSS[name]((m, s), target, 1.7)

    h = 1e-6
    for which, x, gx in (("mean", mean, gm), ("S", S, gS)):
        fd = torch.empty_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.clone(), x.clone()
            xp[idx] += h
            xm[idx] -= h
            with torch.no_grad():
                fp = f_fd(xp, S) if which == "mean" else f_fd(mean, xp)
                fm = f_fd(xm, S) if which == "mean" else f_fd(mean, xm)
            fd[idx] = (fp - fm) / (2 * h)
        err = float((fd - gx).abs().max())
        print(name, which, "max |fd - autograd|", err)
        assert err <= 1e-6 * max(1.0, float(gx.abs().max())), (which, err)


def test_factory_and_kernel_codes():
    from geometry_rl_amd import trpl
    kw = dict(action_dim=6, total_train_steps=1000, cpu=False, dtype=torch.float32, mean_bound=0.05, cov_bound=0.0005, trust_region_coeff=1.0,
              entropy_schedule=False, target_entropy=0.0, temperature=0.5, entropy_eq=False, entropy_first=False)
    for name, cls, code_true, code_false in (("kl", trpl.KLProjectionLayer, 0, 0), ("frob", trpl.FrobeniusProjectionLayer, 1, 6),
                                             ("w2", trpl.WassersteinProjectionLayer, 2, 7)):
        for flag, code in ((True, code_true), (False, code_false)):
            layer = trpl.get_projection_layer(name, scale_prec=flag, **kw)
            assert type(layer) is cls and layer.proj_code == code and layer.scale_prec is flag and layer.cov_bound == 0.0005
            assert trpl.KLProjectionLayer(proj_type=name, scale_prec=flag, **kw).proj_code == code
        assert trpl.get_projection_layer(name, **kw).proj_code == code_true   # the default here stays scale_prec=True
    assert trpl.get_projection_layer("w2_non_com", **kw).proj_code == 4
    with pytest.raises(NotImplementedError):
        trpl.get_projection_layer("w2_non_com", scale_prec=False, **kw)
    for name in ("kl", "frob", "w2", "w2_non_com"):
        for flag in (True, False):
            with pytest.raises(NotImplementedError):
                trpl.get_projection_layer(name, scale_prec=flag, mean_eq=True, **kw)
    for name in ("papi", "ppo"):
        with pytest.raises(NotImplementedError):
            trpl.get_projection_layer(name, scale_prec=False, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_trust_region_value_honours_the_flag(name):
    from geometry_rl_amd import trpl
    g = torch.Generator().manual_seed(2)
    m, s, mo, so = (torch.randn(4, 6, generator=g), torch.rand(4, 6, generator=g) + 0.5, torch.randn(4, 6, generator=g),
                    torch.rand(4, 6, generator=g) + 0.5)
    for flag, value in ((True, otr.PROJECTIONS[name][1]), (False, euclid_ref.VALUE[name])):
        layer = trpl.get_projection_layer(name, scale_prec=flag, mean_bound=0.05, cov_bound=0.0025)
        want = value((m.double(), s.double()), (mo.double(), so.double()))
        for p, q in (((m, s), (mo, so)), ((m, s.diag_embed()), (mo, so.diag_embed()))):   # diagonals or matrices
            got = layer.trust_region_value(None, p, q)
            assert got[0].shape == (4,) and got[1].shape == (4,)
            assert torch.allclose(got[0].double(), want[0], rtol=1e-5, atol=1e-6) and torch.allclose(got[1].double(), want[1], rtol=1e-5, atol=1e-6)
    s_g = s.clone().requires_grad_(True)   # differentiable
    layer.trust_region_value(None, (m, s_g), (mo, so))[1].sum().backward()
    assert bool(torch.isfinite(s_g.grad).all()) and float(s_g.grad.abs().max()) > 0.0


@pytest.mark.parametrize("proj_type,code", [("frob", 6), ("w2", 7), ("kl", 0)])
def test_agent_config_reaches_the_layer(proj_type, code):
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.trpl import TRPLLoss
    assert agent.AgentConfig().scale_prec is True
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, proj_type=proj_type, scale_prec=False)
    actor, critic, proj, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    assert isinstance(loss, TRPLLoss) and loss.projection is proj and proj.proj_code == code and proj.scale_prec is False
    with pytest.raises(NotImplementedError):
        agent.build_agent(graph.rigid_spec(), agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2,
                                                                proj_type="w2_non_com", scale_prec=False), device="cpu")
