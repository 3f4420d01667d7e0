"""Entropy control of the fused TRPL update, off the GPU:
  * the float64 restatement (tests/entropy_ref.py) against the reference's own layers called through BaseProjectionLayer.__call__ with a
    linear entropy schedule (tier2g fixture: Frobenius, Wasserstein, non-commuting Wasserstein x entropy_first x entropy_eq).  KL cannot
    be pinned this way (ITPAL is not available): for KL the reference IS oracle.trpl.kl_projection around the entropy functions that
    tests/golden/tier2e_std_entropy.npz pins, and its composition is checked against geometry_rl_amd.trpl's pinned host functions;
  * the restatement's autograd against central finite differences, every projection and mode;
  * the cases of tests/entropy_cases.py hit their regimes in every full workgroup (no case skipped or filtered);
  * the opt-in: TRPLLoss(entropy_control=True) and build_agent with a schedule construct."""
import os

import numpy as np
import pytest
import torch

import entropy_cases as ec
import entropy_ref
import trpl_cases as tc
from oracle import trpl as otr

LAYERS = ("frob", "w2", "w2_non_com")
MODE_IDS = [f"{'eq' if eq else 'ineq'}-{'first' if first else 'last'}" for eq, first in entropy_ref.MODES]
COMBOS = {(False, False), (False, True), (True, False), (True, True)}


def _load(golden_dir):
    z = np.load(os.path.join(golden_dir, "tier2g_entropy_projection.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _loss(name, mean, S, q, R1, R2, eps, eps_cov, coeff, beta, eq, first):
    """sum(w . proj) + the layer's trust-region loss (Frobenius: not detached from the projection), as the fixture's generator forms it."""
    pm, pS = entropy_ref.projection(name, (mean, S), q, eps, eps_cov, beta=beta, entropy_eq=eq, entropy_first=first)
    if name == "frob":
        trl = otr.frobenius_trust_region_loss((mean, S), (pm, pS), coeff)
    else:
        m_d, c_d = otr.wasserstein_value((mean, S), (pm.detach(), pS.detach()))
        trl = (m_d + c_d).mean() * coeff
    return pm, pS, trl, (pm * R1).sum() + (pS * R2).sum() + trl


@pytest.mark.parametrize("mode", entropy_ref.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", LAYERS)
def test_restatement_matches_the_reference_layers(golden_dir, name, mode):
    z = _load(golden_dir)
    eq, first = mode
    key = f"{name}.eq{int(eq)}.first{int(first)}."
    eps, eps_cov, coeff = float(z["mean_bound"]), float(z["cov_bound"]), float(z["coeff"])
    q = (z["mean_o"], z["S_o"])
    initial = otr.entropy_std(z["S_o"]).mean()
    assert torch.allclose(initial, z[key + "initial_entropy"], rtol=1e-5, atol=1e-7)
    step, total = int(z["step"]), int(z["total"])
    bound = step * (z["target_entropy"] - initial) / total + initial     # projection_utils.py:252-280, linear
    assert torch.allclose(bound, z[key + "bound"], rtol=1e-5, atol=1e-7)
    mean, S = z["mean"].clone().requires_grad_(True), z["S"].clone().requires_grad_(True)
    pm, pS, trl, total_loss = _loss(name, mean, S, q, z["R1"], z["R2"], eps, eps_cov, coeff, float(z[key + "bound"]), eq, first)
    assert torch.allclose(pm, z[key + "proj_mean"], rtol=1e-5, atol=1e-7)
    assert torch.allclose(pS, z[key + "proj_S"], rtol=1e-5, atol=1e-7)
    assert torch.allclose(trl, z[key + "tr_loss"], rtol=1e-5, atol=1e-7)
    g_mean, g_S = torch.autograd.grad(total_loss, [mean, S])
    assert torch.isfinite(z[key + "grad_mean"]).all() and torch.isfinite(z[key + "grad_S"]).all()
    assert torch.allclose(g_mean, z[key + "grad_mean"], rtol=1e-4, atol=1e-6)
    assert torch.allclose(g_S, z[key + "grad_S"], rtol=1e-4, atol=1e-6)


def test_fixture_frames_cover_the_four_combinations(golden_dir):
    z = _load(golden_dir)
    q = (z["mean_o"], z["S_o"])
    for name in LAYERS:
        for first in (False, True):
            e_act, t_act = entropy_ref.stage_activity(name, (z["mean"], z["S"]), q, float(z["mean_bound"]), float(z["cov_bound"]),
                                                      beta=float(z[f"{name}.eq0.first{int(first)}.bound"]), entropy_first=first)
            assert {(bool(a), bool(b)) for a, b in zip(e_act, t_act)} == COMBOS, (name, first)


@pytest.mark.parametrize("mode", entropy_ref.MODES, ids=MODE_IDS)
def test_kl_composition_is_the_pinned_host_functions_around_the_oracle(mode):
    """KL: oracle.trpl.kl_projection + geometry_rl_amd.trpl's entropy functions (pinned by the tier-2e fixture), composed by hand."""
    from geometry_rl_amd import trpl
    eq, first = mode
    e = ec.ECase(tc.Case(B=37, A=6, proj=0), eq, first)
    d = ec.make_case(e)
    p = (d["loc"].double(), d["sigma"].double() ** 2)
    q = (d["batch"]["loc"].double(), d["batch"]["var"].double())
    beta = torch.full((37,), d["beta"], dtype=torch.float64)
    host = trpl.entropy_equality_projection if eq else trpl.entropy_inequality_projection
    if first:
        want = otr.kl_projection(host(None, p, beta), q, tc.EPS, tc.EPS_COV)
    else:
        want = host(None, otr.kl_projection(p, q, tc.EPS, tc.EPS_COV), beta)
    got = entropy_ref.projection("kl", p, q, tc.EPS, tc.EPS_COV, beta=d["beta"], entropy_eq=eq, entropy_first=first)
    assert torch.equal(got[0], want[0]) and torch.allclose(got[1], want[1], rtol=1e-14, atol=0)


@pytest.mark.parametrize("mode", entropy_ref.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("proj", tc.PROJS, ids=[tc.PROJ_NAMES[p] for p in tc.PROJS])
def test_autograd_of_the_restatement_matches_finite_differences(proj, mode):
    """Central differences in fp64 (the bound of tests/test_w2nc_cpu.py: 1e-6 * max(1, |g|max)).  No frame sits on a regime boundary:
    entropy_cases keeps every frame >= NEAR from the entropy bound, trpl_cases 0.3x / 3x from the trust-region bounds.  The two min_std
    frames (S = 1e-10: no finite-difference step fits under it) are left out of the differentiated function, not of the case."""
    eq, first = mode
    e = ec.ECase(tc.Case(B=16, A=3, proj=proj), eq, first)
    d = ec.make_case(e)
    q = (d["batch"]["loc"].double(), d["batch"]["var"].double())
    g = torch.Generator().manual_seed(5)
    R1, R2 = torch.randn(16, 3, generator=g, dtype=torch.float64), torch.randn(16, 3, generator=g, dtype=torch.float64)
    keep = torch.tensor([r != "min_std" for r in tc.regimes_of(16)])

    def f(mean, S):
        pm, pS = entropy_ref.projection(tc.PROJ_NAMES[proj], (mean, S), q, tc.EPS, tc.EPS_COV, beta=d["beta"], entropy_eq=eq,
                                        entropy_first=first)
        return (pm * R1)[keep].sum() + (pS * R2)[keep].sum()

    mean0, S0 = d["loc"].double(), d["sigma"].double() ** 2
    mean, S = mean0.clone().requires_grad_(True), S0.clone().requires_grad_(True)
    g_mean, g_S = torch.autograd.grad(f(mean, S), [mean, S])
    worst = 0.0
    for which, x0, grad in (("mean", mean0, g_mean), ("S", S0, g_S)):
        for b in range(16):
            if not keep[b]:
                continue
            for i in range(3):
                h = 1e-6 * max(1.0, abs(float(x0[b, i])))
                xp, xm = x0.clone(), x0.clone()
                xp[b, i] += h
                xm[b, i] -= h
                with torch.no_grad():
                    fd = (f(xp, S0) - f(xm, S0)) / (2 * h) if which == "mean" else (f(mean0, xp) - f(mean0, xm)) / (2 * h)
                worst = max(worst, abs(float(fd) - float(grad[b, i])))
    gmax = max(float(g_mean.abs().max()), float(g_S.abs().max()))
    print(f"finite differences {tc.PROJ_NAMES[proj]} eq={eq} first={first}: worst {worst:.3e}, |g|max {gmax:.3e}")
    assert worst <= 1e-6 * max(1.0, gmax), (worst, gmax)


def test_cases_hit_their_regimes_in_every_full_workgroup():
    """Inequality modes: every FULL 16-frame workgroup of every case has a frame in each combination (entropy stage active / not) x
    (trust-region bound active / not), computed with entropy_ref alone.  Equality modes: the stage is active on every frame by
    definition.  Every case of the suite is walked; none is left out."""
    cases = ec.all_cases()
    n_wg = 0
    for e in cases:
        if e.entropy_eq:
            continue
        d = ec.make_case(e)
        e_act, t_act = ec.activity(e, d)
        for w in range(e.base.B // tc.TRPL_FPB):
            sl = slice(tc.TRPL_FPB * w, tc.TRPL_FPB * (w + 1))
            assert {(bool(a), bool(b)) for a, b in zip(e_act[sl], t_act[sl])} == COMBOS, (e.name, w)
            n_wg += 1
    assert n_wg > 900 and len(cases) == 4 * len(tc.lane_cases()) + len(tc.batch_cases())
    assert {(e.base.proj, e.mode, tc.lane_width(e.base.A)) for e in cases} >= {(p, m, L) for p in tc.PROJS for m in range(4) for L in (4, 8, 16)}


def test_opt_in_constructs_and_default_still_refuses():
    from geometry_rl_amd import agent, graph, trpl
    spec = graph.rigid_spec()
    kw = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    actor, critic, _, plain = agent.build_agent(spec, agent.AgentConfig(**kw), device="cpu")
    assert plain.entropy_control is False and not trpl.entropy_active(plain)
    layer = trpl.KLProjectionLayer(proj_type="kl", mean_bound=0.05, cov_bound=0.0025, trust_region_coeff=1.0, scale_prec=True,
                                   entropy_schedule="linear", action_dim=6, total_train_steps=100, target_entropy=-3.0, entropy_first=True)
    with pytest.raises(NotImplementedError, match="entropy schedule"):
        trpl.TRPLLoss(actor, critic, projection=layer)
    m = trpl.TRPLLoss(actor, critic, projection=layer, entropy_control=True)
    assert trpl.entropy_active(m) and layer.entropy_mode == 2 and layer.has_entropy_control
    # a layer without a schedule: the flag changes nothing
    assert not trpl.entropy_active(trpl.TRPLLoss(actor, critic, projection=plain.projection, entropy_control=True))
    _, _, proj, loss = agent.build_agent(spec, agent.AgentConfig(entropy_schedule="exp", target_entropy=-0.5, temperature=0.5, entropy_eq=True,
                                                                 total_train_steps=50, proj_type="w2", **kw), device="cpu")
    assert loss.projection is proj and proj.entropy_schedule_type == "exp" and proj.entropy_mode == 1 and trpl.entropy_active(loss)
    # the bound of a step is the layer's own float32 arithmetic, on a host copy of the latched initial entropy
    with pytest.raises(RuntimeError, match="latched"):
        proj.entropy_bounds([0])
    proj.initial_entropy = torch.tensor(1.25)
    for s in (0, 7, 49):
        assert proj.entropy_bounds([s])[0] == float(proj.get_entropy_bound(s))
