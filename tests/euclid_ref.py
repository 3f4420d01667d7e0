"""Float64 restatements of the Euclidean (``scale_prec=False``) forms of the Frobenius and the commutative Wasserstein projection
(frob_projection_layer.py, w2_projection_layer.py, projection_utils.py:9-31,70-149, base_projection_layer.py:71-100) on the diagonal
policy, as plain autograd code with the signatures of their ``oracle/trpl.py`` siblings.  Pinned to the reference layers by
tests/golden/tier2g_projection_{frob,w2}_euclid.npz (tests/test_euclid_proj_cpu.py); the GPU tests register them with the oracle as

    monkeypatch.setitem(oracle.trpl.PROJECTIONS, "frob", (frobenius_projection_euclid, frobenius_value_euclid))
    monkeypatch.setitem(oracle.trpl.PROJECTIONS, "w2", (wasserstein_projection_euclid, wasserstein_value_euclid))

(the key "frob" is kept: ``oracle.trpl.trpl_loss`` takes the Frobenius layer's own regression loss, maha(mean, proj_mean, S) +
|S - proj_S|^2 on the NOT detached projection, by that key -- the layer's loss does not read the flag).

S = the layer's "std" diagonal = the policy's covariance diagonal, as the oracle passes it.  Both forms:

    mp = sum (mu - mu_o)^2                      (no division by S_o, no factor 1/2)
    omega = sqrt(mp / eps) - 1 where mp > eps;  proj_mu = (mu + omega mu_o) / (1 + omega + 1e-16) there, mu elsewhere

Frobenius:  cp = sum (S_o^2 - S^2)^2 (unchanged by the flag);  proj_S = sqrt((S^2 + eta S_o^2) / (1 + eta + 1e-16))
Wasserstein:  cp = tr(S_o^2 + S^2 - 2 S_o S) = sum (S_o - S)^2;  proj_S = (S + eta S_o) / (1 + eta + 1e-16)
with eta = |sqrt(cp / eps_cov) - 1| where cp > eps_cov."""
import torch

from oracle import trpl as otr


def _mean_part(mean, mean_o):
    """projection_utils.py:26-29."""
    return (mean_o - mean).pow(2).sum(-1)


def frobenius_value_euclid(p, q):
    """gaussian_frobenius(scale_prec=False): (sum (mean - mean_o)^2, |S_o^2 - S^2|_F^2)."""
    (mean, S), (mean_o, S_o) = p, q
    return _mean_part(mean, mean_o), (S_o.pow(2) - S.pow(2)).pow(2).sum(-1)


def wasserstein_value_euclid(p, q):
    """gaussian_wasserstein_commutative(scale_prec=False): (sum (mean - mean_o)^2, tr(S_o^2 + S^2 - 2 S_o S))."""
    (mean, S), (mean_o, S_o) = p, q
    return _mean_part(mean, mean_o), (S_o.pow(2) + S.pow(2) - 2.0 * S_o * S).sum(-1)


def frobenius_projection_euclid(p, q, mean_bound, cov_bound):
    """frob_projection_layer.py:10-63 with the Euclidean mean part."""
    (mean, S), (mean_o, S_o) = p, q
    mean_part, cov_part = frobenius_value_euclid(p, q)
    proj_mean = otr.mean_projection(mean, mean_o, mean_part, mean_bound)
    mask, eta = otr._eta_from_part(cov_part, cov_bound)
    if mask.any():
        new_cov = (S.pow(2) + eta[..., None] * S_o.pow(2)) / (1.0 + eta + 1e-16)[..., None]
        proj_S = torch.where(mask[..., None], new_cov.sqrt(), S)
    else:
        proj_S = S
    return proj_mean, proj_S


def wasserstein_projection_euclid(p, q, mean_bound, cov_bound):
    """w2_projection_layer.py:15-68 with the Euclidean parts."""
    (mean, S), (mean_o, S_o) = p, q
    mean_part, cov_part = wasserstein_value_euclid(p, q)
    proj_mean = otr.mean_projection(mean, mean_o, mean_part, mean_bound)
    mask, eta = otr._eta_from_part(cov_part, cov_bound)
    if mask.any():
        new_S = (S + eta[..., None] * S_o) / (1.0 + eta + 1e-16)[..., None]
        proj_S = torch.where(mask[..., None], new_S, S)
    else:
        proj_S = S
    return proj_mean, proj_S


def frobenius_trust_region_loss(p, proj_p, coeff):
    """frob_projection_layer.py:73-88: the layer's own loss, whatever the flag (the oracle's)."""
    return otr.frobenius_trust_region_loss(p, proj_p, coeff)


def wasserstein_trust_region_loss_euclid(p, proj_p, coeff):
    """base_projection_layer.py:292-327 with the Euclidean W2 value: (p, stopgrad(proj_p))."""
    m_d, c_d = wasserstein_value_euclid(p, (proj_p[0].detach(), proj_p[1].detach()))
    return (m_d + c_d).mean() * coeff


VALUE = {"frob": frobenius_value_euclid, "w2": wasserstein_value_euclid}
PROJECTION = {"frob": frobenius_projection_euclid, "w2": wasserstein_projection_euclid}
TR_LOSS = {"frob": frobenius_trust_region_loss, "w2": wasserstein_trust_region_loss_euclid}
CODE = {"frob": 6, "w2": 7}
