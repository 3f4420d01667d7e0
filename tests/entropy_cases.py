"""Cases for the per-op tests of the fused TRPL kernel's entropy stage, built on tests/trpl_cases.py (same eight trust-region regimes per
16-frame workgroup).  TEST INFRASTRUCTURE ONLY.

The bound ``beta`` is ONE scalar per launch, so the frames' entropies are placed around it: frame f gets a common scale c_f of S and
So -- 4 in the first half of its workgroup (f % 16 < 8), 1/4 in the second -- and the mean offset is scaled with So, so the KL and both
Wasserstein measures (functions of S / So and (mu - mo) / So) keep their values and every regime of trpl_cases stays what it was.  Powers
of four: sigma scales by an exact power of two, p == q stays bitwise on the ``equal`` frames.  The Frobenius covariance part,
sum (So^2 - S^2)^2, is not scale-free: there So is solved again for the SAME part along the frame's own direction log(S / So) (pointing
towards larger So on the scaled-down frames, where a smaller So cannot reach the part).  ``min_std`` frames keep their tiny sigma
unscaled (entropy far below any bound); the second ``equal`` frame of a workgroup is scaled to an entropy NEAR below the bound instead
(see make_case: with the stage in FRONT of the trust region, a frame scaled by much leaves the trust region).  With sigma = k / 128 in [0.5, 1.5): sum log S >= 0 on the scaled-up and <= -0.57 A on the
scaled-down frames, so beta = k/2 log(2 pi e) - 0.3 A separates them whatever the draw: each regime occurs once in either half, so every full
workgroup has entropy-active and entropy-inactive frames both inside (equal, inside) and outside the trust region
(tests/test_entropy_control_cpu.py checks exactly that, with entropy_ref alone)."""
import math
from dataclasses import dataclass, replace
from typing import Dict

import torch

import entropy_ref
import trpl_cases as tc
from oracle import trpl as otr


@dataclass(frozen=True)
class ECase:
    base: tc.Case
    entropy_eq: bool = False
    entropy_first: bool = False

    @property
    def name(self):
        return f"{self.base.name}-{'eq' if self.entropy_eq else 'ineq'}-{'first' if self.entropy_first else 'last'}"

    @property
    def mode(self):
        return entropy_ref.mode_word(self.entropy_eq, self.entropy_first)


NEAR = 0.02   # << sqrt(cov_bound A) = 0.05 sqrt(A): alpha^2 - 1 ~ 2 NEAR / A leaves every covariance part far below its bound


def beta_of(A):
    return 0.5 * A * math.log(2 * math.e * math.pi) - 0.3 * A


def lane_cases():
    return [ECase(c, eq, first) for c in tc.lane_cases() for eq, first in entropy_ref.MODES]


def batch_cases():
    return [ECase(c, *entropy_ref.MODES[i % 4]) for i, c in enumerate(tc.batch_cases())]


def all_cases():
    return lane_cases() + batch_cases()


def make_case(e: ECase) -> Dict[str, torch.Tensor]:
    c = e.base
    d = tc.make_case(c)
    B, A = c.B, c.A
    rid = tc.regimes_of(B, c.shift)
    f = torch.arange(B)
    up = (f % tc.TRPL_FPB) < 8
    keep = torch.tensor([r == "min_std" for r in rid])
    cf = torch.where(keep, torch.ones(B, dtype=torch.float64), torch.where(up, 4.0, 0.25).double())[:, None]
    sigma, mu = d["sigma"].double(), d["loc"].double()
    mo, So, act = d["batch"]["loc"].double(), d["batch"]["var"].double(), d["batch"]["action"].double()
    S = sigma ** 2
    # the second ``equal`` frame of a workgroup sits JUST below the bound (by NEAR): the stage scales it by exp(NEAR / A) only, so with the
    # stage in front the scaled frame is still inside the trust region -- the one combination the factors of four cannot produce there
    near = torch.tensor([r == "equal" for r in rid]) & ~up
    c_near = torch.exp((beta_of(A) - NEAR - otr.entropy_std(S)) / A)[:, None]
    cf = torch.where(near[:, None], c_near, cf)
    S2, So2 = S * cf, So * cf
    if c.proj == 1:   # Frobenius: the same covariance part along the frame's own direction
        solved = torch.tensor([r in ("inside", "mean_only", "cov_only", "both", "cov_split") for r in rid])
        _, part = tc.measures(1, mu, S, mo, So)
        u = (S / So).log()
        u = torch.where((~up)[:, None], -u.abs(), u)
        u = torch.where(u.abs().sum(-1, keepdim=True) > 0, u, torch.zeros_like(u))
        s = tc._solve_cov(1, S2, u, part)
        So2 = torch.where(solved[:, None] & (u != 0), S2 * torch.exp(-s * u), So2)
    So2 = So2.float().double()
    mu2 = (mo + (mu - mo) * (So2 / So)).float()
    act2 = (mo + (act - mo) * (So2 / So).sqrt()).float()
    noise = d["batch"]["sample_log_prob"].double() - otr.mvn_diag_log_prob(act, mo, So)
    logp2 = (otr.mvn_diag_log_prob(act2.double(), mo, So2) + noise).float()
    out = dict(d)
    out["loc"], out["sigma"] = mu2, (sigma * cf.sqrt()).float()
    out["batch"] = dict(d["batch"], var=So2.float(), action=act2, sample_log_prob=logp2)
    out["beta"] = beta_of(A)
    return out


def reference(e: ECase, d):
    """trpl_cases.reference with the composed projection (float64 oracle of the case on its fp32 inputs)."""
    with entropy_ref.registered(d["beta"], e.entropy_eq, e.entropy_first):
        return tc.reference(e.base, d)


def activity(e: ECase, d):
    """Per frame (entropy stage active in the inequality form, trust-region bound active)."""
    c = e.base
    p = (d["loc"].double(), d["sigma"].double() ** 2)
    q = (d["batch"]["loc"].double(), d["batch"]["var"].double())
    return entropy_ref.stage_activity(tc.PROJ_NAMES[c.proj], p, q, tc.EPS, tc.EPS_COV, beta=d["beta"], entropy_first=e.entropy_first)
