"""Float64 restatement of the non-commuting Wasserstein projection (w2_projection_layer_non_com.py:13-86, torch_utils.py sqrtm_newton) on
the diagonal policy, as plain autograd code.  Pinned to the reference layer by tests/golden/tier2f_projection_w2_non_com.npz
(tests/test_w2nc_cpu.py); the GPU tests register it with the oracle as

    monkeypatch.setitem(oracle.trpl.PROJECTIONS, "w2_non_com", (w2nc_ref.projection, oracle.trpl.wasserstein_value))

Every matrix of the layer is diagonal here (S = the layer's "std" diagonal = the policy's covariance diagonal, as the oracle passes it):

    mp = sum ((mu - mu_o) / S_o)^2,  cp = sum (1 - S / S_o)^2
    mask = mp + cp > eps + eps_cov;  t = sqrt((eps + eps_cov) / (mp + cp + 1e-16)) where mask, else 1
    proj_mu = (1 - t) mu_o + t mu
    d = (1 - t) + t S S_o,  x = d^2 S_o^2,  n = sqrt(sum x^2)
    Y = x / n, Z = 1;  ten times: T = (3 - Z Y) / 2, Y = Y T, Z = T Z
    proj_S = Y sqrt(n) where mask, else S

The ten Newton-Schulz steps are the reference's semantics (not converged where x_i / n is small) and are differentiated through, n
included.  The reference differentiates an eigendecomposition instead; on a frame inside the bound whose ratios S / S_o are all equal its
autograd gives NaN (repeated eigenvalues), where this form gives the analytic pass-through."""
import torch

NS_STEPS = 10


def newton_schulz_diag(x, steps=NS_STEPS):
    """sqrtm_newton on diag(x), row-wise: the Frobenius norm of a diagonal matrix is the 2-norm of its diagonal."""
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    y, z = x / n, torch.ones_like(x)
    for _ in range(steps):
        T = 0.5 * (3.0 - z * y)
        y = y * T
        z = T * z
    return y * n.sqrt()


def projection(p, q, mean_bound, cov_bound, sqrt_fn=newton_schulz_diag):
    """(mean, S), (mean_o, S_o): [B, A] diagonals -> (proj_mean, proj_S).  ``sqrt_fn``: the square root of x (the layer's: ten
    Newton-Schulz steps)."""
    (mean, S), (mean_o, S_o) = p, q
    mp = ((mean - mean_o) / S_o).pow(2).sum(-1)
    cp = (1.0 - S / S_o).pow(2).sum(-1)
    mask = mp + cp > mean_bound + cov_bound
    t = torch.where(mask, torch.sqrt((mean_bound + cov_bound) / (mp + cp + 1e-16)), torch.ones_like(mp))[..., None]
    proj_mean = torch.where(mask[..., None], (1.0 - t) * mean_o + t * mean, mean)
    d = (1.0 - t) + t * S * S_o
    x = d * d * (S_o * S_o)
    proj_S = torch.where(mask[..., None], sqrt_fn(x), S)
    return proj_mean, proj_S


def value(p, q):
    """gaussian_wasserstein_non_commutative(scale_prec=True) on diagonal matrices = the commutative value: (maha, sum (1 - S/S_o)^2)."""
    (mean, S), (mean_o, S_o) = p, q
    return ((mean - mean_o) / S_o).pow(2).sum(-1), (1.0 - S / S_o).pow(2).sum(-1)


def x_over_n(p, q, mean_bound, cov_bound):
    """Per dimension x_i / n of the square root's argument (how far from converged the ten steps leave dimension i)."""
    (mean, S), (mean_o, S_o) = p, q
    mp = ((mean - mean_o) / S_o).pow(2).sum(-1)
    cp = (1.0 - S / S_o).pow(2).sum(-1)
    t = torch.sqrt((mean_bound + cov_bound) / (mp + cp + 1e-16))[..., None]
    x = ((1.0 - t) + t * S * S_o).pow(2) * S_o.pow(2)
    return x / x.pow(2).sum(-1, keepdim=True).sqrt()
