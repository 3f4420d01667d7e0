#!/usr/bin/env python3
"""Generate tests/golden/tier2g_entropy_projection.npz: the reference's projection layers (Frobenius, Wasserstein, non-commuting
Wasserstein; pure torch) called through BaseProjectionLayer.__call__ with entropy_schedule="linear", for entropy_first x entropy_eq, on
the diagonal policy.  Run in float64 on float32-representable inputs (as tier 2f), B = 37, A = 6.

Run:  python tools/make_golden_entropy.py      (needs the reference checkout tools/make_golden.py names; name-only stubs as there)

Per layer and mode: proj_mean, proj_S, initial_entropy, the bound of the step, get_trust_region_loss, and the gradient of
sum(w . proj) + trust-region loss with respect to (mean, S).  Only arrays are written.  Frames 0, 4, 8, ... lie inside the trust region
(distinct ratios S / S_o: the non-commuting layer's eigendecomposition has no gradient at repeated ones), the others outside; the frames'
entropies are placed around the bound by a common scale of S and S_o (x 4, x 1/4, and -- frames 4, 12, ... -- to 0.02 below the bound, so
that with the entropy stage in front a scaled frame can still be inside the trust region)."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

import make_golden as mg

STEP, TOTAL, B, A = 40, 100, 37, 6
EPS, EPS_COV, COEFF = 0.05, 0.0025, 1.5


def inputs():
    g = torch.Generator().manual_seed(71)
    f32 = lambda t: t.float().double()
    mean = torch.randn(B, A, generator=g, dtype=torch.float64)
    S = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    mean_o = mean + 0.3 * torch.randn(B, A, generator=g, dtype=torch.float64)
    S_o = torch.rand(B, A, generator=g, dtype=torch.float64) + 0.5
    lin = torch.linspace(-1, 1, A, dtype=torch.float64)
    f = torch.arange(B)
    inside = (f % 4 == 0)[:, None]
    mean_o = torch.where(inside, mean + 1e-3 * lin, mean_o)
    S_o = torch.where(inside, S * (1 + 2e-4 * lin), S_o)   # (small enough for the Frobenius part of a frame scaled by 4: it is not scale-free)
    beta = 0.5 * A * math.log(2 * math.e * math.pi) - 0.3 * A
    ent = 0.5 * A * math.log(2 * math.e * math.pi) + S.log().sum(-1)
    cf = torch.where(f % 8 == 4, torch.exp((beta - 0.02 - ent) / A), torch.where((f % 2 == 1), 0.25, 4.0).double())[:, None]
    S2, S_o2 = f32(S * cf), f32(S_o * cf)
    mean, mean_o = f32(mean), f32(mean_o)
    mean = f32(mean_o + (mean - mean_o) * (S_o2 / S_o))
    return mean, S2, mean_o, S_o2, beta, torch.randn(B, A, generator=g, dtype=torch.float64), torch.randn(B, A, generator=g, dtype=torch.float64)


def main():
    mg.install_stubs()
    from geometry_rl.algorithms.trust_region_projections.projections.frob_projection_layer import FrobeniusProjectionLayer
    from geometry_rl.algorithms.trust_region_projections.projections.w2_projection_layer import WassersteinProjectionLayer
    from geometry_rl.algorithms.trust_region_projections.projections.w2_projection_layer_non_com import (
        WassersteinProjectionLayerNonCommuting)
    from geometry_rl.algorithms.trust_region_projections.models.policy.gnn_gaussian_policy_diag import GNNGaussianPolicyDiag
    torch.symeig = lambda c, eigenvectors=False, upper=True: torch.linalg.eigh(c, UPLO="U" if upper else "L")   # (as tier 2f)

    class FakeGNN(nn.Module):
        device = "cpu"

    class FakeData:
        pass

    policy = GNNGaussianPolicyDiag(gnn=FakeGNN(), hyper_data=FakeData(), action_dim=A, num_actuators=1, init="orthogonal",
                                   hidden_sizes=(64, 64), contextual_std=True, init_std=1.0, minimal_std=1e-5, share_action_dim=True,
                                   post_fc=False)
    mean, S, mean_o, S_o, beta, R1, R2 = inputs()
    initial = float(policy.entropy((mean_o, S_o.diag_embed())).mean())
    target = initial + (beta - initial) * TOTAL / STEP     # the linear schedule passes through ``beta`` at STEP
    rec = {"mean": mean, "S": S, "mean_o": mean_o, "S_o": S_o, "R1": R1, "R2": R2, "step": torch.tensor(STEP), "total": torch.tensor(TOTAL),
           "target_entropy": torch.tensor(target, dtype=torch.float64), "mean_bound": torch.tensor(EPS, dtype=torch.float64),
           "cov_bound": torch.tensor(EPS_COV, dtype=torch.float64), "coeff": torch.tensor(COEFF, dtype=torch.float64)}
    layers = {"frob": FrobeniusProjectionLayer, "w2": WassersteinProjectionLayer, "w2_non_com": WassersteinProjectionLayerNonCommuting}
    for name, cls in layers.items():
        for eq in (False, True):
            for first in (False, True):
                layer = cls(proj_type=name, mean_bound=EPS, cov_bound=EPS_COV, trust_region_coeff=COEFF, scale_prec=True,
                            entropy_schedule="linear", action_dim=A, total_train_steps=TOTAL, target_entropy=target, temperature=0.5,
                            entropy_eq=eq, entropy_first=first, cpu=True, dtype=torch.float64)
                mean_g, S_g = mean.clone().requires_grad_(True), S.clone().requires_grad_(True)
                p, q = (mean_g, S_g.diag_embed()), (mean_o, S_o.diag_embed())
                pm, pS = layer(policy, p, q, STEP)
                trl = layer.get_trust_region_loss(policy, p, (pm, pS))
                ((pm * R1).sum() + (pS.diagonal(dim1=-2, dim2=-1) * R2).sum() + trl).backward()
                key = f"{name}.eq{int(eq)}.first{int(first)}."
                rec.update({key + "proj_mean": pm, key + "proj_S": pS.diagonal(dim1=-2, dim2=-1), key + "initial_entropy": layer.initial_entropy,
                            key + "bound": layer.get_entropy_bound(STEP), key + "tr_loss": trl, key + "grad_mean": mean_g.grad,
                            key + "grad_S": S_g.grad})
    path = os.path.join(mg.OUT, "tier2g_entropy_projection.npz")
    np.savez(path, **mg.npd(rec))
    print("tier2g:", len(rec), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
