"""Float64 restatements of the training-loop kernels (csrc/train_ops.hip and the fused fold + Adam tail of csrc/node_ops.hip), with the
fp32 error allowance of each kernel's arithmetic, for tests/test_gpu_train_ops.py.  tests/test_train_ops_ref_cpu.py pins every restatement
against the thing it restates: torch.optim.Adam (+ clip_grad_norm_), oracle.trpl.gae_shifted, oracle.transforms.vecnorm_update.

Allowances are written in units of U = 2^-24, the unit roundoff of fp32: one rounding of an fp32 operation moves a value x by at most
U |x|; an error e in an operand is carried through to the result as |d result / d operand| * e.  A kernel's output is accepted when
|got - ref| <= allowance element by element (the tests report the worst ratio)."""
import numpy as np
import torch

U = 2.0 ** -24


def f32(x) -> float:
    """The fp32 value a float argument becomes when it is handed to a kernel (ctypes.c_float), as a Python double."""
    return float(np.float32(x))


def ulp32(t: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |t| (normal range; subnormal spacing below)."""
    a = t.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ---------------------------------------------------------------------------------------------------------------------------------- Adam
def bias_corrections(b1: float, b2: float, t: int):
    """bc1 = 1 - b1^t, bc2 = 1 - b2^t (exact for the given betas) and the error of the kernels' fp32 forms 1 - powf(b, t): powf is allowed
    2 ulp of b^t, the subtraction is exact (Sterbenz, b^t >= 1/2) or adds U; the cancellation 1 - b^t is what turns those few ulp into a
    large RELATIVE error of bc at small t (b2 = 0.999, t = 2: ~250 U)."""
    out = []
    for b in (b1, b2):
        bt = float(b) ** t
        ebt = 2.0 * float(ulp32(torch.tensor(bt))) if bt > 0 else 2.0 ** -149
        bc = 1.0 - bt
        out += [bc, ebt + U * bc]
    return out   # bc1, err_bc1, bc2, err_bc2


def adam(p, g, m, v, lr, b1, b2, eps, t, scale=1.0):
    """One torch.optim.Adam step (no amsgrad, no weight decay) in float64: the kernels' form
    m = b1 m + (1-b1) g s; v = b2 v + (1-b2) (g s)^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  -> (p, m, v)"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gs = g * scale
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - lr / bc1 * (m1 / (v1.sqrt() / bc2 ** 0.5 + eps)), m1, v1


def adam_allowance(p, g, m, v, lr, b1, b2, eps, t, scale=1.0, eg=None):
    """Per-element allowance of the fp32 kernels' (p, m, v) after one step from the fp32 state (p, g, m, v).

    m:  g*s rounds (U, +U for the scale product scale_host * scale_dev), (1-b1)*gs (U), b1*m (U), the sum (U):  5 U (|b1 m| + |(1-b1) gs|).
    v:  gs carries 2 U, squared 4 U + U, times (1-b2) U, b2*v U, the sum U:                                     8 U (|b2 v| + |(1-b2) gs^2|).
        (1 - b, b in [1/2, 1), is exact: Sterbenz.)  eg: an allowance of the gradient itself (a fold) is carried through as well.
    p:  upd = lr/bc1 * m / D, D = sqrt(v)/sqrt(bc2) + eps.  Six roundings (lr/bc1, sqrt, /sqrt(bc2), +eps, m/D, the product): 8 U |upd|;
        bc1 and bc2 from bias_corrections, carried as |upd| (ebc1/bc1 + 1/2 ebc2/bc2 * S/D), S = sqrt(v)/sqrt(bc2);
        m's allowance em as lr/bc1 * em / D; v's allowance ev as |upd| * 1/2 ev/v * S/D;  the final p - upd rounds: 1 ulp of max(|p|, |p'|).
    -> (ap, am, av)"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gs = g * scale
    am = 5 * U * ((b1 * m).abs() + ((1.0 - b1) * gs).abs())
    av = 8 * U * ((b2 * v).abs() + (1.0 - b2) * gs * gs)
    if eg is not None:
        eg = eg.double() * abs(scale)
        am = am + (1.0 - b1) * eg
        av = av + (1.0 - b2) * (2 * gs.abs() * eg + eg * eg)
    p1, m1, v1 = adam(p, g, m, v, lr, b1, b2, eps, t, scale)
    bc1, ebc1, bc2, ebc2 = bias_corrections(b1, b2, t)
    S = v1.sqrt() / bc2 ** 0.5
    D = S + eps
    upd = (lr / bc1 * m1 / D).abs()
    rel_v = torch.where(v1 > 0, 0.5 * av / v1.clamp_min(1e-300), torch.zeros_like(v1))
    # v -> v + ev moves S by at most S/2 * ev/v for ev <= v; past that (v ~ 0) by sqrt(ev)/sqrt(bc2)
    dS = torch.minimum(S * rel_v, av.sqrt() / bc2 ** 0.5)
    ap = (upd * (8 * U + ebc1 / bc1 + 0.5 * ebc2 / bc2 * S / D) + lr / bc1 * am / D + (lr / bc1 * (m1.abs() + am)) * dS / (D * D)
          + ulp32(torch.maximum(p.abs(), p1.abs())))
    return ap, am, av


def clip_coef(g: torch.Tensor, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (||g|| + 1e-6)) in float64."""
    return min(1.0, max_norm / (float(g.double().norm()) + 1e-6))


# ----------------------------------------------------------------------------------------------------------------------------------- GAE
def gae(reward, done, terminated, values, gamma, lmbda):
    """Shifted GAE in float64 (oracle.trpl.gae_shifted) plus the fp32 scan's allowance.

    The kernel: delta = r + gamma nt V' - V (gamma*nt exact: nt is 0 or 1; *V', +r, -V: 3 roundings, 3 U (|r| + gamma |V'| + |V|));
    run = delta + (gamma lmbda) nd run (gamma*lmbda, *nd exact, *run, +: 3 roundings, 3 U (|delta| + gamma lmbda |run|)).  The error of run
    is carried backwards with factor gamma lmbda nd, so E_t = gamma lmbda nd_t E_{t+1} + 6 U (|r| + gamma |V'| + |V| + gamma lmbda |run_{t+1}|)
    over-covers it; the value target a + V adds one rounding, U |a + V|.  -> (adv, target, adv_allowance, target_allowance)"""
    r, V = reward.double(), values.double()
    nt, nd = 1.0 - terminated.double(), 1.0 - done.double()
    N, T = r.shape
    delta = r + gamma * nt * V[:, 1:] - V[:, :-1]
    mag = r.abs() + gamma * V[:, 1:].abs() + V[:, :-1].abs()
    adv, err = torch.zeros_like(r), torch.zeros_like(r)
    run, e = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    gl = gamma * lmbda
    for t in range(T - 1, -1, -1):
        e = gl * nd[:, t] * e + 6 * U * (mag[:, t] + gl * run.abs())
        run = delta[:, t] + gl * nd[:, t] * run
        adv[:, t], err[:, t] = run, e
    tgt = adv + V[:, :-1]
    return adv, tgt, err, err + U * tgt.abs()


# -------------------------------------------------------------------------------------------------------------------------------- VecNorm
def vecnorm_state(x, state, decay: float, update: bool):
    """The decayed statistics [sum K | ssq K | count] in float64 from the fp32 state the kernel started from, and their allowance:
    colsums are accumulated in fp64 (error ~rows * 2^-53 |.|, negligible) and rounded to fp32 (U), state*decay (U), the sum (U):
    3 U (|decay * s| + |colsum|), the same for count with rows."""
    K = (state.numel() - 1) // 2
    st = state.double()
    if not update:
        return st.clone(), torch.zeros_like(st)
    xv = x.double().reshape(-1, K)
    add = torch.cat([xv.sum(0), (xv * xv).sum(0), torch.tensor([float(xv.shape[0])], dtype=torch.float64)])
    new = st * decay + add
    return new, 3 * U * ((st * decay).abs() + add.abs())


def vecnorm_apply(x, state, eps: float, lo: float, hi: float):
    """y = clip((x - mean) / max(std, eps)) in float64 from the kernel's own fp32 state (the statistics the launch used), and its allowance.

    mean = sum/count (U); var = ssq/count - mean^2 (ssq/count U, mean^2 3 U, the difference U): ev = 4 U (ssq/count + mean^2);
    std = sqrt(max(var, eps)) (max(., eps) is 1-Lipschitz): es = 1/2 ev / sqrt(max(var - ev, eps)) + U std; y = (x - mean) / std: (U |mean| + U |x - mean|) / std
    + |y| es / std + 2 U |y| (the division and slack).  Clipping is 1-Lipschitz: the allowance holds for the clipped value.
    -> (y, allowance)"""
    K = (state.numel() - 1) // 2
    st = state.double()
    s, q, c = st[:K], st[K:2 * K], st[2 * K]
    mean = s / c
    var = q / c - mean * mean
    std = var.clamp_min(eps).sqrt()
    den = std.clamp_min(eps)
    ev = 4 * U * (q.abs() / c + mean * mean) + 2 * U * var.abs()
    es = 0.5 * ev / (var - ev).clamp_min(eps).sqrt() + U * std
    xv = x.double().reshape(-1, K)
    y = (xv - mean) / den
    a = (U * mean.abs() + U * (xv - mean).abs()) / den + y.abs() * es / den + 2 * U * y.abs()
    return y.clamp(lo, hi).reshape(x.shape), a.reshape(x.shape)


# ------------------------------------------------------------------------------------------------------------------------------------ kNN
def knn(pos: torch.Tensor, n_valid, k: int) -> torch.Tensor:
    """pos [B, P, 3] -> [B, P, k]: for point i < n_valid[b], the k nearest OTHER points j < n_valid[b] in stable (squared distance, index)
    order; -1 where fewer exist and for every padding point.  n_valid None: all P points are valid; values past P are clamped.
    Exact for coordinates on a dyadic lattice (the squared distances are then exact in float64 and in the kernel's fp32)."""
    B, P, _ = pos.shape
    out = torch.full((B, P, k), -1, dtype=torch.int32)
    p = pos.double()
    for b in range(B):
        nv = P if n_valid is None else max(0, min(int(n_valid[b]), P))
        if nv == 0:
            continue
        d = ((p[b, :nv, None, :] - p[b, None, :nv, :]) ** 2).sum(-1)
        d.fill_diagonal_(float("inf"))
        ds, idx = torch.sort(d, dim=1, stable=True)
        kk = min(k, nv)
        sel = torch.where(torch.isinf(ds[:, :kk]), torch.full_like(idx[:, :kk], -1), idx[:, :kk])
        out[b, :nv, :kk] = sel.int()
    return out
