"""Cases and float64 references for the per-op tests of the fused TRPL / PPO loss kernel (trpl_lanes_kernel, head_ops.hip) and of the
rollout sampler (gaussian_sample_kernel).  TEST INFRASTRUCTURE ONLY: tests/test_gpu_trpl_kernel.py compares the kernel with these
references by the comparisons at the end of this file (the tests of the entropy stage and of the later projections use the same ones),
tests/test_trpl_kernel_cases_cpu.py checks on the CPU that the cases still hit every regime they are meant to.

Every 16-frame workgroup of a TRPL case holds the eight per-frame regimes of REGIMES twice (frame f has regime (f + shift) % 8):

    equal      p == q bitwise (sigma^2 exact in fp32): constraints 0, gradients pass straight through
    inside     both parts at 0.3 of their bounds
    mean_only  mean part 3x its bound, covariance part 0.3x
    cov_only   the other way round
    both       both parts 3x their bounds
    large      variance ratios 30 and 1/30 inside one frame, mean part 10x: eta large (KL phase-1 / phase-2 caps)
    cov_split  dimensions with S == So bitwise next to dimensions 3x over the covariance bound (om = 0 in the KL Newton derivative)
    min_std    dimension 0 at sigma = 1e-5 or 1e-3 (alternately) against an old variance of 1

"part" is the projection's own measure: KL (1/2 maha, 1/2 sum(rho - 1 - log rho) of rho = (S / So)^2, the "std" quirk), Frobenius
(maha, sum (So^2 - S^2)^2), Wasserstein (maha, sum (1 - S / So)^2); the non-commuting Wasserstein projection has one joint bound
mean_bound + cov_bound, against which both parts are then scaled.  Independently, frame f has the value-loss regime f % 5 of VREGIMES."""
import contextlib
import math
import os
from dataclasses import dataclass, replace
from typing import Dict

import numpy as np
import torch

import w2nc_ref
from oracle import trpl as otr
from ppo_ref import ppo_loss

EPS, EPS_COV = 0.05, 0.0025
PROJ_NAMES = {0: "kl", 1: "frob", 2: "w2", 4: "w2_non_com"}
REGIMES = ("equal", "inside", "mean_only", "cov_only", "both", "large", "cov_split", "min_std")
VREGIMES = ("inside_clip", "clip_wins_above", "clip_wins_below", "unclipped_wins", "on_edge")
CLIP_EDGE = 0.25     # |V - Vo| of the on_edge frames: exactly a clip_value of 0.25 (no difference of two floats equals the double 0.2)
U64 = 2.0 ** -53     # unit roundoff of fp64
U32 = 2.0 ** -24     # unit roundoff of fp32
TRPL_FPB = 16        # frames per workgroup of the kernel (grl_report.h)


@dataclass(frozen=True)
class Case:
    B: int
    A: int
    proj: int = 0                 # 0 KL, 1 Frobenius, 2 W2, 4 non-commuting W2
    seed: int = 0
    tr_coeff: float = 1.5
    ent_coef: float = 0.015625    # fp32-exact: the report multiplies by the float32 coefficient
    critic_coef: float = 0.5
    clip_value: float = 0.2
    value: bool = True
    adv_mode: str = "local"       # local (in-kernel sums) | kernel_stats (grl_adv_stats) | shard (global stats, global_batch != B) | none
    adv_kind: str = "randn"       # randn | const | tiny (spread below the 1e-6 floor) | offset3 | offset4 (mean 1e3 / 1e4 x the spread)
    shift: int = 0

    @property
    def name(self):
        return (f"B{self.B}-A{self.A}-{PROJ_NAMES[self.proj]}-tr{self.tr_coeff:g}-ent{self.ent_coef:g}-clip{self.clip_value:g}"
                f"-{'v' if self.value else 'nov'}-{self.adv_mode}-{self.adv_kind}")

    @property
    def global_batch(self):
        return 3 * self.B + 1 if self.adv_mode == "shard" else self.B


# ------------------------------------------------------------------------------------------------------------- the grids
PROJS = (0, 1, 2, 4)
A_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16)                            # L = 4, 8, 16 with 0 .. 15 padding lanes
B_SWEEP = (1, 2, 15, 16, 17, 16 * 63, 16 * 64, 16 * 64 + 1, 4097)         # fold: 1, 63, 64, 65, 257 slots (FOLD_NT = 256)
OPTIONS = (dict(tr_coeff=0.0), dict(ent_coef=0.0), dict(value=False), dict(clip_value=0.0), dict(clip_value=CLIP_EDGE),
           dict(adv_mode="kernel_stats"), dict(adv_mode="shard"), dict(adv_mode="none"), dict(adv_kind="const"), dict(adv_kind="tiny"),
           dict(adv_mode="kernel_stats", adv_kind="offset3"), dict(adv_kind="offset4"), dict(adv_mode="kernel_stats", adv_kind="offset4"),
           dict(B=1, adv_mode="shard", shift=4))
PPO_GRID = tuple((B, A) for A in (1, 3, 4, 5, 9, 16) for B in (1, 17, 4097))


def lane_cases():
    return [Case(B=37, A=A, proj=p) for A in A_SWEEP for p in PROJS]


def batch_cases():
    return [Case(B=B, A=A, proj=PROJS[(i + j) % len(PROJS)], shift=4 if B < 8 else 0)
            for j, A in enumerate((3, 6, 16)) for i, B in enumerate(B_SWEEP)]


def option_cases():
    return [replace(Case(B=37, A=5, proj=p), **o) for o in OPTIONS for p in PROJS]


def lane_width(A):
    return 4 if A <= 4 else (8 if A <= 8 else 16)


def regimes_of(B, shift=0):
    return [REGIMES[(f + shift) % len(REGIMES)] for f in range(B)]


def measures(proj, mu, S, mo, So):
    """(mean part, covariance part) as the kernel compares them with the bounds, float64 [B]."""
    maha = (((mu - mo) / So) ** 2).sum(-1)
    if proj == 0:
        rho = (S / So) ** 2
        return 0.5 * maha, 0.5 * (rho - 1.0 - rho.log()).sum(-1)
    if proj == 1:
        return maha, ((So ** 2 - S ** 2) ** 2).sum(-1)
    return maha, ((1.0 - S / So) ** 2).sum(-1)


def bounds(proj):
    return (EPS + EPS_COV, EPS + EPS_COV) if proj == 4 else (EPS, EPS_COV)


def _solve_cov(proj, S, u, target):
    """s >= 0 per frame with cov_part(S, So = S exp(-s u)) = target [B] (bisection: the part grows with s)."""
    lo = torch.zeros(S.shape[0], 1, dtype=torch.float64)
    hi = torch.full_like(lo, 8.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        _, c = measures(proj, S, S, S, S * torch.exp(-mid * u))
        over = (c > target)[:, None]
        hi = torch.where(over, mid, hi)
        lo = torch.where(over, lo, mid)
    return 0.5 * (lo + hi)


def make_case(c: Case) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors of one case: loc, sigma [B, A], value [B] (None without a critic), batch (action, loc, var, sample_log_prob,
    advantage, state_value, value_target) and adv_global (the advantages of the whole global batch, this batch's first)."""
    B, A = c.B, c.A
    g = torch.Generator().manual_seed(1000 * c.seed + 17 * A + B + 7 * c.proj)
    rid = torch.tensor([REGIMES.index(r) for r in regimes_of(B, c.shift)])
    is_ = lambda name: rid == REGIMES.index(name)
    mb, cb = bounds(c.proj)
    kfac = 0.5 if c.proj == 0 else 1.0
    fm = torch.tensor([0.0, 0.3, 3.0, 0.3, 3.0, 10.0, 0.3, 0.3], dtype=torch.float64)[rid]   # x the mean bound, by REGIMES
    fc = torch.tensor([0.0, 0.3, 0.3, 3.0, 3.0, 0.0, 3.0, 0.3], dtype=torch.float64)[rid]    # x the covariance bound
    sigma = (torch.randint(64, 192, (B, A), generator=g).double() / 128.0)   # k / 128: sigma^2 = k^2 / 2^14 exact in fp32
    S = sigma ** 2
    # covariance: So = S exp(-s u), u of mixed signs; cov_split: u = 0 (So == S) on the odd dimensions
    u = (0.5 + 0.5 * torch.rand(B, A, generator=g, dtype=torch.float64)) * torch.where(torch.rand(B, A, generator=g) < 0.5, -1.0, 1.0)
    split = is_("cov_split")[:, None] & (torch.arange(A)[None, :] % 2 == 1)
    u = torch.where(split, torch.zeros_like(u), u)
    s = _solve_cov(c.proj, S, u, fc * cb)
    So = torch.where(split, S, S * torch.exp(-s * u))
    ratio30 = torch.where(torch.arange(A) % 2 == 0, 1.0 / 30.0, 30.0).double()[None, :]   # So = S / 30 and S * 30
    So = torch.where(is_("large")[:, None], S * ratio30, So)
    So = torch.where(is_("equal")[:, None], S, So)
    # sigma near minimal_std on dimension 0 against an old variance of 1 (1e-5 and 1e-3 in turn)
    ms = is_("min_std")
    tiny = torch.where((torch.cumsum(ms.long(), 0) - 1) % 2 == 0, 1e-5, 1e-3).double()
    sigma[:, 0] = torch.where(ms, tiny, sigma[:, 0])
    So[:, 0] = torch.where(ms, torch.ones_like(So[:, 0]), So[:, 0])
    So = So.float().double()   # what the kernel reads
    # mean: mu = mo + m So v, v a unit vector, kfac m^2 = fm x the mean bound
    mo = torch.randn(B, A, generator=g).double()
    v = torch.randn(B, A, generator=g, dtype=torch.float64)
    v = v / v.norm(dim=-1, keepdim=True)
    mu = mo + (fm * mb / kfac).sqrt()[:, None] * So * v
    mu = torch.where(is_("equal")[:, None], mo, mu)
    old_mean, old_var = mo.float(), So.float()
    action = (old_mean.double() + old_var.double().sqrt() * torch.randn(B, A, generator=g, dtype=torch.float64)).float()
    logp = (otr.mvn_diag_log_prob(action.double(), old_mean.double(), old_var.double())
            + 0.1 * torch.randn(B, generator=g, dtype=torch.float64)).float()
    adv_global = _advantages(c.adv_kind, c.global_batch, g)
    batch = {"action": action, "loc": old_mean, "var": old_var, "sample_log_prob": logp, "advantage": adv_global[:B].clone()}
    vals = _values(B, g)
    value = vals.pop("_value")
    batch.update(vals)
    return {"loc": mu.float(), "sigma": sigma.float(), "value": value if c.value else None, "batch": batch, "adv_global": adv_global}


def _advantages(kind, n, g):
    if kind == "randn":
        return torch.randn(n, generator=g)
    if kind == "const":     # 0.1f: not dyadic, the sum of squares rounds; the normalised advantages must still be 0
        return torch.full((n,), 0.1)
    if kind == "tiny":      # 1 +- up to 3 fp32 ulp: std ~ 2e-7, below the 1e-6 floor that then sets the scale
        return 1.0 + torch.randint(-3, 4, (n,), generator=g).float() * 2.0 ** -23
    if kind in ("offset3", "offset4"):
        return (10.0 ** int(kind[-1]) + torch.randn(n, generator=g, dtype=torch.float64)).float()
    raise ValueError(kind)


def _values(B, g):
    """Old value Vo = k / 8 (so that Vo +- 0.25 is exact), value V and target R by the frame's value regime (VREGIMES), both signs."""
    Vo = torch.randint(-16, 16, (B,), generator=g).double() / 8.0
    V, R = Vo.clone(), Vo.clone()
    noise = torch.randn(B, generator=g, dtype=torch.float64)
    for f in range(B):
        r = VREGIMES[f % len(VREGIMES)]
        sgn = 1.0 if (f // len(VREGIMES)) % 2 == 0 else -1.0
        if r == "inside_clip":
            V[f], R[f] = Vo[f] + sgn * 0.05, Vo[f] + noise[f]
        elif r == "clip_wins_above":
            V[f], R[f] = Vo[f] + 0.5, Vo[f] + 1.0
        elif r == "clip_wins_below":
            V[f], R[f] = Vo[f] - 0.5, Vo[f] - 1.0
        elif r == "unclipped_wins":
            V[f], R[f] = Vo[f] + sgn * 0.5, Vo[f] - sgn * 0.3
        else:
            V[f], R[f] = Vo[f] + sgn * CLIP_EDGE, Vo[f] + sgn * 0.6
    return {"state_value": Vo.float(), "value_target": R.float(), "_value": V.float()}


@contextlib.contextmanager
def w2nc_registered():
    """The oracle's TRPL loss with the non-commuting W2 restatement registered (as tests/test_gpu_w2_non_com.py does)."""
    old = otr.PROJECTIONS.get("w2_non_com")
    otr.PROJECTIONS["w2_non_com"] = (w2nc_ref.projection, otr.wasserstein_value)
    try:
        yield
    finally:
        if old is None:
            del otr.PROJECTIONS["w2_non_com"]
        else:
            otr.PROJECTIONS["w2_non_com"] = old


def adv_reference_stats(c: Case, d):
    """(mean, unbiased std) the oracle normalises with (float64, two-pass), or None for no normalisation."""
    if c.adv_mode == "none" or c.global_batch <= 1:
        return None
    a = d["adv_global"].double()
    return a.mean(), a.std().clamp_min(1e-6)


def summation_depth(c: Case):
    """Longest chain of fp64 additions behind the advantage sums s0, s1: thread-strided partial sums, six wave butterfly levels, the
    waves in order -- of the in-kernel sums (16 L threads, L >= 4) and of grl_adv_stats (1024 threads); a bound for host sums too."""
    n = c.global_batch
    return max(-(-n // 64) + 6 + lane_width(c.A) // 4, -(-n // 1024) + 6 + 16)


def adv_error_bound(c: Case, d):
    """Bound on |a' - a'_exact| of the normalised advantages a' = (a - m) / sd as the kernel computes them: s0 = sum a, s1 = sum a^2
    (fp64 chains of depth <= d), m = s0 / n, var = (s1 - n m^2) / (n - 1), sd = max(sqrt(var), 1e-6).  With u = 2^-53:
        |dm| <= (d + 1) u (|m| + sigma)
        |d(s1 - n m^2)| <= (4 d + 8) u n (m^2 + sigma^2)        (one pass: m^2 + sigma^2, not sigma^2, sets the scale of the roundoff)
        |dsd| / sd <= (2 d + 5) u n / (n - 1) (1 + m^2 / sigma^2)     (sd above the floor)
        |da'| <= |a'| |dsd| / sd + |dm| / sd + 2 u |a'|
    The conditioning (m / sigma)^2 of the one-pass variance multiplies the roundoff: at m / sigma = 1e4 and d = 30 the bound is ~7e-7 |a'|,
    about twelve fp32 ulp; at 1e3 it is below one ulp.  Where sigma is under the floor, sd = 1e-6 if sqrt(var + |dvar|) stays below it."""
    if c.adv_mode == "none" or c.global_batch <= 1:
        return 0.0
    a = d["adv_global"].double()
    n = a.numel()
    m, sig = float(a.mean()), float(a.std())
    dep = summation_depth(c)
    dm = (dep + 1) * U64 * (abs(m) + sig)
    dvar = (4 * dep + 8) * U64 * n * (m * m + sig * sig) / (n - 1)
    sd = max(sig, 1e-6)
    anorm = float(((a - m) / sd).abs().max())
    if sig < 1e-6:
        assert math.sqrt(sig * sig + dvar) < 1e-6, "the floor decision itself lies within the roundoff"
        rel_sd = 0.0
    else:
        rel_sd = (2 * dep + 5) * U64 * n / (n - 1) * (1.0 + (m / sig) ** 2)
    return anorm * rel_sd + dm / sd + 2 * U64 * anorm


def reference(c: Case, d) -> Dict[str, torch.Tensor]:
    """float64 oracle of one case on the fp32 inputs: the 12 sums (head_ops.hip layout), 2 maxes, dloc, dsigma, dvalue, proj_mean,
    proj_S, the 14 reported values, and the sensitivities |d output / d a'| to the normalised advantages (for adv_error_bound)."""
    B = c.B
    loc_r = d["loc"].double().requires_grad_(True)
    sig_r = d["sigma"].double().requires_grad_(True)
    val_r = (d["value"] if c.value else torch.zeros(B)).double().requires_grad_(True)
    bd = {k: v.double() for k, v in d["batch"].items()}
    stats = adv_reference_stats(c, d)
    if stats is not None:   # normalised here: the oracle skips a batch of one even with global statistics, the kernel counts the global batch
        bd["advantage"] = (bd["advantage"] - stats[0]) / stats[1]
    kw = dict(mean_bound=EPS, cov_bound=EPS_COV, trust_region_coeff=c.tr_coeff, entropy_coef=c.ent_coef, critic_coef=c.critic_coef,
              clip_value=c.clip_value, normalize_advantage=False, proj_type=PROJ_NAMES[c.proj])
    scale = B / c.global_batch   # the kernel's gradients are those of sums / global_batch
    with w2nc_registered():
        ref = otr.trpl_loss(loc_r, sig_r ** 2, bd, val_r, **kw)
        d_loc, d_sig = torch.autograd.grad(ref["loss_objective"] + ref["loss_trust_region"] + ref["loss_entropy"], [loc_r, sig_r],
                                           retain_graph=True)
        (d_val,) = torch.autograd.grad(ref["loss_critic"], [val_r], retain_graph=True)
        pm, pS = ref["proj_mean"], ref["proj_S"]
        lw = otr.mvn_diag_log_prob(bd["action"], pm, pS) - bd["sample_log_prob"]
        s_loc, s_sig = torch.autograd.grad(-lw.exp().mean(), [loc_r, sig_r])   # the objective at a' = 1: linear in a'
    out = {"dloc": d_loc * scale, "dsigma": d_sig * scale, "dvalue": d_val * scale if c.value else None,
           "sens_dloc": s_loc.abs() * scale, "sens_dsigma": s_sig.abs() * scale}
    lw = lw.detach()
    out["lw"], out["proj_mean"], out["proj_S"] = lw, pm.detach(), pS.detach()
    f = lambda k: float(ref[k].detach()) * B
    out["sums"] = torch.tensor([f("loss_objective"), f("loss_trust_region"), f("entropy_dist"), f("loss_critic") if c.value else 0.0,
                                float(lw.exp().sum()), float((2 * lw).exp().sum()), f("mean_constraint"), f("cov_constraint"), f("entropy"),
                                f("entropy_diff"), float(B), f("kl")], dtype=torch.float64)
    out["sens_sums"] = torch.zeros(12, dtype=torch.float64)
    out["sens_sums"][0] = float(lw.exp().sum())
    out["maxes"] = torch.tensor([max(float(ref["mean_constraint_max"]), 0.0), max(float(ref["cov_constraint_max"]), 0.0)], dtype=torch.float64)
    s = out["sums"] / B
    tr, ent = float(s[1]), -c.ent_coef * float(s[2])
    out["report"] = torch.tensor([float(s[0]) + tr + ent, float(s[3]), tr, ent, float(ref["ESS"]), float(s[11]), float(s[6]),
                                  float(out["maxes"][0]), float(s[7]), float(out["maxes"][1]), float(s[8]), float(s[9]), float(s[0]),
                                  float(s[6] + s[7])], dtype=torch.float64)
    with torch.no_grad():   # per-frame parts of (p, q) and which part the oracle's projection changed
        S = d["sigma"].double() ** 2
        out["parts"] = measures(c.proj, d["loc"].double(), S, bd["loc"], bd["var"])
        out["mean_moved"] = (out["proj_mean"] != d["loc"].double()).any(-1)
        out["cov_moved"] = ((out["proj_S"] - S).abs() > 1e-12 * S).any(-1)   # (KL: eta = 0 still rounds through 1 / (1 / t))
    return out


# ------------------------------------------------------------------------------------------------------------- target terms
def target_reference(c: Case, d):
    """grl_trpl_target_terms with the detached target (old mean, old var): trust_region_coeff * mean(measure(p, target)), its gradient,
    and the metric sums of (p, target) by column."""
    B = c.B
    loc_r = d["loc"].double().requires_grad_(True)
    sig_r = d["sigma"].double().requires_grad_(True)
    S = sig_r ** 2
    tm, tS = d["batch"]["loc"].double(), d["batch"]["var"].double()
    p, t = (loc_r, S), (tm, tS)
    if c.proj == 1:
        tr = otr.frobenius_trust_region_loss(p, t, c.tr_coeff)
        mk, ck = otr.frobenius_value(p, t)
    else:
        mk, ck = otr.PROJECTIONS[PROJ_NAMES[c.proj]][1](p, t)
        tr = (mk + ck).mean() * c.tr_coeff
    d_loc, d_sig = torch.autograd.grad(tr, [loc_r, sig_r])
    with torch.no_grad():
        km, kc = otr.gaussian_kl(p, t)
        e_new, e_tgt = otr.entropy_std(S), otr.entropy_std(tS)
        sums = {1: float(tr) * B, 2: float(otr.mvn_diag_entropy(tS).sum()), 6: float(mk.sum()), 7: float(ck.sum()), 8: float(e_new.sum()),
                9: float((e_tgt - e_new).sum()), 10: float(B), 11: float((km + kc).sum())}
        maxes = torch.tensor([max(float(mk.max()), 0.0), max(float(ck.max()), 0.0)], dtype=torch.float64)
    return {"sums": sums, "maxes": maxes, "dloc": d_loc, "dsigma": d_sig}


# ------------------------------------------------------------------------------------------------------------- PPO
PPO_EPS = float(torch.tensor(0.2, dtype=torch.float32))   # the kernel reads clip_epsilon as a float32


def ppo_bounds():
    return math.log1p(-PPO_EPS), math.log1p(PPO_EPS)


def make_ppo_case(B, A, seed=0):
    """Log-ratios in seven regions (both sides of both clip bounds, inside; >= 0.045 from either bound), each region with both advantage
    signs (a 14-frame cycle), and the value regimes of the TRPL cases."""
    g = torch.Generator().manual_seed(500 + 31 * A + B + seed)
    lo, hi = ppo_bounds()
    reg = torch.tensor([lo - 0.6, lo - 0.05, 0.5 * lo, 0.0, 0.5 * hi, hi + 0.05, hi + 0.6], dtype=torch.float64)
    lw_t = reg[torch.arange(B) % 7] + 0.01 * (torch.rand(B, generator=g, dtype=torch.float64) - 0.5)
    loc = torch.randn(B, A, generator=g).float()
    sigma = (torch.rand(B, A, generator=g) + 0.4).float()
    action = (loc.double() + sigma.double() * torch.randn(B, A, generator=g, dtype=torch.float64)).float()
    logp = (otr.mvn_diag_log_prob(action.double(), loc.double(), sigma.double() ** 2) - lw_t).float()
    sgn = torch.where((torch.arange(B) // 7) % 2 == 0, 1.0, -1.0)
    adv = (sgn * (0.6 + 0.8 * torch.rand(B, generator=g))).float()
    batch = {"action": action, "sample_log_prob": logp, "advantage": adv}
    vals = _values(B, g)
    value = vals.pop("_value")
    batch.update(vals)
    return {"loc": loc, "sigma": sigma, "value": value, "batch": batch}


def ppo_reference(d, *, ent_coef, critic_coef, clip_value):
    B = d["loc"].shape[0]
    loc_r = d["loc"].double().requires_grad_(True)
    sig_r = d["sigma"].double().requires_grad_(True)
    val_r = d["value"].double().requires_grad_(True)
    bd = {k: v.double() for k, v in d["batch"].items()}
    ref = ppo_loss(loc_r, sig_r ** 2, bd, val_r, clip_epsilon=PPO_EPS, entropy_coef=ent_coef, critic_coef=critic_coef, clip_value=clip_value)
    d_loc, d_sig = torch.autograd.grad(ref["loss_objective"] + ref["loss_entropy"], [loc_r, sig_r])
    (d_val,) = torch.autograd.grad(ref["loss_critic"], [val_r])
    lw = ref["lw"]
    ent = float(ref["entropy"].detach()) * B
    sums = torch.tensor([float(ref["loss_objective"].detach()) * B, 0.0, ent, float(ref["loss_critic"].detach()) * B, float(lw.exp().sum()),
                         float((2 * lw).exp().sum()), 0.0, 0.0, ent, 0.0, float(B), 0.0], dtype=torch.float64)
    a = bd["advantage"]
    a_n = (a - a.mean()) / a.std().clamp_min(1e-6) if B > 1 else a
    return {"sums": sums, "dloc": d_loc, "dsigma": d_sig, "dvalue": d_val, "lw": lw, "adv_n": a_n}


# ------------------------------------------------------------------------------------------------------------- sampler
def sample_reference(loc, sigma, eps, action):
    """float64 action and var of gaussian_sample_kernel's inputs, and the log-prob at the kernel's own (rounded) action as
    MultivariateNormal.log_prob computes it, with a bound on the kernel's fp32 evaluation of it (A fused multiply-adds and logs)."""
    l, s, e = loc.double(), sigma.double(), eps.double()
    A = loc.shape[-1]
    dd = (action.double() - l) / s
    q = (dd * dd).sum(-1)
    logp = -0.5 * q - s.log().sum(-1) - 0.5 * A * otr.LOG_2PI
    bound = (A + 4) * U32 * (0.5 * q + s.log().abs().sum(-1) + 0.5 * A * otr.LOG_2PI) + 4 * U32 * q
    return l + s * e, s * s, logp, bound


# ------------------------------------------------------------------------------------------------------------- comparisons
RTOL32 = 4 * U32       # fp32 outputs: a few ulp
FLOOR = 1e-6           # ... plus this much of the frame's largest |ref|
RTOL64 = 1e-9          # fp64 sums
ATOL64 = 1e-11         # ... plus this much per frame
CANCEL = 1e-10         # fp32 tensors, plus this much of the tensor's largest |ref|: fp64 cancellation (the KL implicit gradient of a frame
                       # with a huge eta subtracts two terms ~1e15 x their difference; 1e-14 absolute at sigma = 1e-5)


def close(name, got, want, extra=None, per_frame=True):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    a = want.abs()
    scale = a.reshape(a.shape[0], -1).amax(-1).reshape(-1, *([1] * (a.dim() - 1))) if (per_frame and a.dim() > 1) else a.max()
    allowed = RTOL32 * a + FLOOR * scale + CANCEL * a.max()
    if extra is not None:
        allowed = allowed + extra
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all()), name
    bad = err > allowed
    i = int((err - allowed).flatten().argmax())
    print(f"  {name:12s} worst err {float(err.max()):.3e}  at [{i}]: err {float(err.flatten()[i]):.3e} allowed {float(allowed.flatten()[i]):.3e}")
    assert not bool(bad.any()), (name, int(bad.sum()), float(err.flatten()[i]), float(allowed.flatten()[i]), float(want.flatten()[i]))


def sums_close(name, got, want, B, extra=None):
    from geometry_rl_amd import ops
    got, want = got.cpu().double(), want.double()
    assert float(got[10]) == float(want[10]), (name, "count")
    allowed = RTOL64 * want.abs() + ATOL64 * B
    if extra is not None:
        allowed = allowed + extra
    err = (got - want).abs()
    k = int((err / allowed).argmax())
    print(f"  {name:12s} worst: {ops.TRPL_SUM_KEYS[k]} err {float(err[k]):.3e} allowed {float(allowed[k]):.3e}")
    assert bool((err <= allowed).all()), [(j, float(got[j]), float(want[j]), float(allowed[j])) for j in range(12) if err[j] > allowed[j]]


def maxes_close(name, got_bits, want):
    got = got_bits.cpu().view(torch.float32).double()
    w32 = want.float().double()
    allowed = 2 * U32 * w32.abs() + 1e-30
    print(f"  {name:12s} maxes {got.tolist()} want {w32.tolist()}")
    assert bool(((got - w32).abs() <= allowed).all()), (name, got.tolist(), w32.tolist())


def report_close(name, out, want, kap_obj):
    out, want = out.cpu().double(), want.double()
    scale = want.abs().clone()
    scale[0] = scale[12] = abs(float(want[12])) + abs(float(want[2])) + abs(float(want[3]))
    scale[13] = abs(float(want[6])) + abs(float(want[8]))
    allowed = RTOL32 * scale + 1e-30
    allowed[0] += kap_obj
    allowed[12] += kap_obj
    err = (out - want).abs()
    j = int((err / allowed).argmax())
    print(f"  {name:12s} worst out[{j}] err {float(err[j]):.3e} allowed {float(allowed[j]):.3e}")
    assert bool((err <= allowed).all()), [(i, float(out[i]), float(want[i])) for i in range(14) if err[i] > allowed[i]]


def launch_close(outs, ref, B, kap, value=True):
    """The seven outputs of one fused launch (ops.trpl_fwd_bwd, want_projection=True) against ``reference``'s entries, ``kap`` the case's
    adv_error_bound; without a critic there is no dvalue."""
    sums, maxes, dloc, dsigma, dvalue, pm, pv = outs
    sums_close("sums", sums, ref["sums"], B, kap * ref["sens_sums"])
    maxes_close("maxes", maxes, ref["maxes"])
    close("proj_mean", pm, ref["proj_mean"])
    close("proj_S", pv, ref["proj_S"])
    close("dloc", dloc, ref["dloc"], kap * ref["sens_dloc"])
    close("dsigma", dsigma, ref["dsigma"], kap * ref["sens_dsigma"])
    if value:
        close("dvalue", dvalue, ref["dvalue"])
    else:
        assert dvalue is None


def rel_close(name, got, want, tol, floor=1.0):
    """``got`` within ``tol`` of max(floor, the largest |want|)."""
    got, want = got.detach().cpu().double(), want.detach().double()
    err = float((got - want).abs().max())
    scale = max(floor, float(want.abs().max()))
    print(f"{name}: max err {err:.3e} of scale {scale:.3e}")
    assert np.isfinite(err) and err <= tol * scale, (name, err, tol * scale)


def projection_fixture(golden_dir, file_name, grp):
    """Group ``grp`` of a projection layer's golden file (tier2f / tier2g): its tensors by name, and the layer's three settings."""
    z = np.load(os.path.join(golden_dir, file_name))
    out = {k[len(grp) + 1:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(grp + ".")}
    out.update({k: float(z[k]) for k in ("mean_bound", "cov_bound", "coeff")})
    return out
