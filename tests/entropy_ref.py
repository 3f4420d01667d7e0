"""Float64 restatement of the projection layers' entropy half (base_projection_layer.py:14-68 entropy_inequality_projection /
entropy_equality_projection, :232-273 their place around the trust-region projection) composed with the oracle's trust-region
projections, as plain autograd code on the diagonal policy.  TEST INFRASTRUCTURE ONLY.  Pinned to the reference layers (Frobenius, W2,
non-commuting W2) by tests/golden/tier2g_entropy_projection.npz (tests/test_entropy_control_cpu.py); for KL the reference is
oracle.trpl.kl_projection around the same two entropy functions (ITPAL is not available, as for every KL check of this suite).

    ent(x) = k/2 log(2 pi e) + sum_i log x_i          (policy.entropy on the "std" diagonal x; oracle.trpl.entropy_std)
    alpha  = exp((beta - ent(x)) / k),  y = alpha x   on frames with ent(x) < beta (inequality) or on all frames (equality)

entropy_first=False: (mean, S) -> trust region -> (pm, pS) -> entropy stage on pS.
entropy_first=True : entropy stage on S -> trust region on (mean, y); the regression loss and the metrics of ``trpl_loss`` still compare
the ORIGINAL (mean, S) with the result (objectives/trpl.py:244, 306, 318) -- which is what ``oracle.trpl.trpl_loss`` does with whatever
its projection returns.  ``trpl_loss`` below returns exactly what ``oracle.trpl.trpl_loss`` returns."""
import contextlib

import torch

import w2nc_ref
from oracle import trpl as otr

MODES = ((False, False), (True, False), (False, True), (True, True))   # (entropy_eq, entropy_first)


def mode_word(entropy_eq, entropy_first):
    """The kernel's ent_mode (include/grl_hip.h)."""
    return (1 if entropy_eq else 0) | (2 if entropy_first else 0)


def entropy_stage(S, beta, entropy_eq):
    """(scaled S, mask of the scaled frames).  ``beta``: a float or a [B] tensor."""
    k = S.shape[-1]
    ent = otr.entropy_std(S)
    alpha = torch.exp((beta - ent) / k)
    if entropy_eq:
        return S * alpha[..., None], torch.ones_like(ent, dtype=torch.bool)
    mask = ent < beta
    return torch.where(mask[..., None], S * alpha[..., None], S), mask


def base_projections():
    """name -> the trust-region projection alone (the oracle's three and the non-commuting W2 restatement)."""
    out = {k: v[0] for k, v in otr.PROJECTIONS.items() if k != "w2_non_com"}
    out["w2_non_com"] = w2nc_ref.projection
    return out


def compose(project, beta, entropy_eq, entropy_first):
    """The layer's _projection (base_projection_layer.py:232-273) around the trust-region projection ``project``."""
    def composed(p, q, mean_bound, cov_bound):
        mean, S = p
        if entropy_first:
            S = entropy_stage(S, beta, entropy_eq)[0]
        pm, pS = project((mean, S), q, mean_bound, cov_bound)
        if not entropy_first:
            pS = entropy_stage(pS, beta, entropy_eq)[0]
        return pm, pS
    return composed


def projection(proj_type, p, q, mean_bound, cov_bound, *, beta, entropy_eq, entropy_first):
    return compose(base_projections()[proj_type], beta, entropy_eq, entropy_first)(p, q, mean_bound, cov_bound)


@contextlib.contextmanager
def registered(beta, entropy_eq, entropy_first):
    """Inside: every projection the oracle's ``trpl_loss`` can look up (and the one tests/trpl_cases.w2nc_registered registers) is the
    composed one, so ``trpl_cases.reference`` is the reference WITH entropy control."""
    base = base_projections()
    old_table, old_w2nc = dict(otr.PROJECTIONS), w2nc_ref.projection
    try:
        for name, fn in base.items():
            value = otr.PROJECTIONS[name][1] if name in otr.PROJECTIONS else otr.wasserstein_value
            otr.PROJECTIONS[name] = (compose(fn, beta, entropy_eq, entropy_first), value)
        w2nc_ref.projection = otr.PROJECTIONS["w2_non_com"][0]
        yield
    finally:
        w2nc_ref.projection = old_w2nc
        otr.PROJECTIONS.clear()
        otr.PROJECTIONS.update(old_table)


def trpl_loss(loc, var, batch, state_value, *, beta, entropy_eq, entropy_first, **kw):
    """oracle.trpl.trpl_loss with the scheduled entropy projection inside the projection step; same keys."""
    with registered(beta, entropy_eq, entropy_first):
        return otr.trpl_loss(loc, var, batch, state_value, **kw)


def stage_activity(proj_type, p, q, mean_bound, cov_bound, *, beta, entropy_first):
    """Per frame (entropy stage active in the inequality form, trust-region bound active), computed with this module alone."""
    mean, S = p
    with torch.no_grad():
        if entropy_first:
            S_in, e_act = entropy_stage(S, beta, False)
            pm, pS = base_projections()[proj_type]((mean, S_in), q, mean_bound, cov_bound)
        else:
            S_in = S
            pm, pS = base_projections()[proj_type]((mean, S), q, mean_bound, cov_bound)
            e_act = entropy_stage(pS, beta, False)[1]
        t_act = (pm != mean).any(-1) | ((pS - S_in).abs() > 1e-12 * S_in).any(-1)
    return e_act, t_act
