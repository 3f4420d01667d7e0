"""Float64 restatement of the two behaviour-cloning modes of the fused loss kernel (trpl_lanes_body, modes 8 and 9; csrc/head_ops.hip),
written from the formulas, without autograd (TEST INFRASTRUCTURE ONLY).  tests/test_bc_ref_cpu.py holds it to torch's own ``nn.MSELoss``
and ``Independent(Normal(mu, sigma), 1).log_prob``; tests/test_gpu_bc_ops.py compares the kernel with it.

With d = mu - a per dimension and se = sum_i d_i^2 per frame (A dimensions, B frames, G = the global batch):

    8, regression:    loss = sum_b se / (G A);   d loss / d mu = 2 d / (G A);   d loss / d sigma = 0
    9, Gaussian NLL:  nll = 1/2 sum_i (d_i / sigma_i)^2 + sum_i log sigma_i + A/2 log 2 pi   (= -MultivariateNormal(mu, diag sigma^2).log_prob(a))
                      loss = sum_b nll / G;   d loss / d mu = d / (sigma^2 G);   d loss / d sigma = (1 / sigma - d^2 / sigma^3) / G

Columns of the 12 sums (both modes): 0 the optimised loss (per-frame, before the 1 / G), 2 = 8 the policy's entropy, 3 se / A, 4 = 5 one per
frame, 6 se (its maximum: maxes[0]), 10 the count, 11 nll; the others and maxes[1] zero."""
import math
from typing import Dict

import torch

LOG_2PI = math.log(2.0 * math.pi)
MODES = {"mse": 8, "nll": 9}
SIGMAS = (1e-3, 1.0, 1e3)      # the std regimes of a case, per frame
DEVIATIONS = (0.0, 1e-4, 10.0)  # ... and |a - mu|: all nine pairs inside every 9 consecutive frames


def bc_reference(loc, sigma, action, mode, global_batch=None) -> Dict[str, torch.Tensor]:
    """float64 sums [12], maxes [2], dloc, dsigma [B, A] and the 14 reported values (grl_trpl_loss_values, entropy_coef = 0) of one launch
    on the inputs as given (fp32 tensors are widened, not re-rounded)."""
    mode = MODES.get(mode, mode)
    assert mode in (8, 9), mode
    mu, sg, a = loc.double(), sigma.double(), action.double().reshape(loc.shape)
    B, A = mu.shape
    G = float(global_batch or B)
    d = mu - a
    se = (d * d).sum(-1)
    nll = 0.5 * ((d / sg) ** 2).sum(-1) + sg.log().sum(-1) + 0.5 * A * LOG_2PI
    ent = 0.5 * A * (1.0 + LOG_2PI) + sg.log().sum(-1)
    if mode == 8:
        per_frame, dloc, dsigma = se / A, 2.0 * d / (G * A), torch.zeros_like(sg)
    else:
        per_frame, dloc, dsigma = nll, d / (sg * sg) / G, (1.0 / sg - d * d / sg ** 3) / G
    z = 0.0
    sums = torch.tensor([float(per_frame.sum()), z, float(ent.sum()), float((se / A).sum()), float(B), float(B), float(se.sum()), z,
                         float(ent.sum()), z, float(B), float(nll.sum())], dtype=torch.float64)
    maxes = torch.tensor([float(se.max()), 0.0], dtype=torch.float64)
    s = sums / B
    report = torch.tensor([float(s[0]), float(s[3]), z, z, 1.0, float(s[11]), float(s[6]), float(maxes[0]), z, z, float(s[8]), z, float(s[0]),
                           float(s[6])], dtype=torch.float64)
    return {"sums": sums, "maxes": maxes, "dloc": dloc, "dsigma": dsigma, "report": report, "se": se, "nll": nll, "entropy": ent,
            "loss": sums[0] / G}


def make_case(B, A, seed=0) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors loc, sigma, action [B, A].  Frame f has the std regime SIGMAS[f % 3] (times a per-dimension factor k / 128 in
    [0.5, 1.5)) and the deviation DEVIATIONS[(f // 3) % 3] with a random sign per dimension (0: action == loc bitwise) -- from a
    likelihood dominated by the quadratic term (sigma 1e-3, |d| 10: 1e8 per dimension) to one that is all log sigma."""
    g = torch.Generator().manual_seed(900 + 131 * A + B + seed)
    f = torch.arange(B)
    base = torch.tensor(SIGMAS, dtype=torch.float64)[f % 3][:, None]
    sigma = (base * torch.randint(64, 192, (B, A), generator=g).double() / 128.0).float()
    loc = torch.randn(B, A, generator=g).float()
    dev = torch.tensor(DEVIATIONS, dtype=torch.float64)[(f // 3) % 3][:, None]
    sign = torch.where(torch.rand(B, A, generator=g) < 0.5, -1.0, 1.0).double()
    action = (loc.double() + sign * dev).float()
    return {"loc": loc, "sigma": sigma, "action": action}
