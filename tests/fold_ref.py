"""Float64 restatements of the gradient fold (csrc/node_ops.hip: reduce_partials_kernel, reduce_partials_seg_kernel,
reduce_partials_multi_kernel) and of the critic lane's value loss (csrc/head_ops.hip value_loss_kernel), their allowances, and the cases
tests/test_gpu_fold_ops.py runs them on.  Test infrastructure only, pure torch on CPU; tests/test_fold_ref_cpu.py pins it.

The fold: dst[j] (+)= sum over the slabs of a destination, over each slab's rows, of slab[row][start + j].  An fp32 sum of R terms in ANY
order is within (R - 1) U sum |terms| of the exact one (to first order in U = 2^-24); fold_allowance grants (R + 1) U sum |terms|, so it
does not restate the kernel's summation order and survives a re-tuned kernel.  Integer-valued slabs whose |terms| sum to less than 2^24
make every partial sum of every order exactly representable: the kernel must then return THE sum, bit for bit."""
import math

import torch

from oracle import trpl as otr
from train_ops_ref import U

# row counts around the main-loop strides of both paths (scalar: 32 rows, float4: 8 x depth) and column_sum4's depth switches (16, 32, 64)
ROWS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2048]
LENS = [1, 3, 4, 63, 64, 65, 127, 128, 132]
KINDS = ("int", "gauss")


def _terms(slabs, start, length):
    starts = [start] * len(slabs) if isinstance(start, int) else list(start)
    return [s[:, st:st + length].double() for s, st in zip(slabs, starts)]


def fold64(slabs, start, length, init=None):
    """Column sums of slab[:, start : start + length] over the listed slabs (``start``: one int or one per slab) in float64, plus the
    prior destination contents ``init`` when accumulating."""
    out = torch.zeros(length, dtype=torch.float64)
    for t in _terms(slabs, start, length):
        out = out + t.sum(0)
    return out if init is None else out + init.double()


def fold_allowance(slabs, start, length, init=None):
    """(R + 1) U sum |x| per column, R = the number of summed terms (every row of every slab, and the prior destination as one more)."""
    ts = _terms(slabs, start, length)
    R = sum(t.shape[0] for t in ts) + (0 if init is None else 1)
    mag = torch.zeros(length, dtype=torch.float64)
    for t in ts:
        mag = mag + t.abs().sum(0)
    if init is not None:
        mag = mag + init.double().abs()
    return (R + 1) * U * mag


def ratio(got, ref, allow):
    """max |got - ref| / allowance; an element with allowance 0 must be exact, and a NaN or infinite error counts as infinite."""
    err = (got.double().cpu() - ref.double()).abs()
    r = torch.where(allow > 0, err / allow.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    return float(r.nan_to_num(float("inf"), float("inf")).max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------------- fold cases
class Case:
    """One launch's worth of folds.  slabs: fp32 [rows, ld] tensors; segs: (slab index, start, len, destination key) in launch order;
    dst: key -> (len, offset in floats of the destination from a 16-byte boundary)."""

    def __init__(self, name, kind, slabs, segs, mis=None):
        self.name, self.kind, self.slabs, self.segs = name, kind, slabs, segs
        self.dst = {}
        for _, _, ln, k in segs:
            self.dst.setdefault(k, (ln, (mis or {}).get(k, 0)))

    def feeds(self, key):
        """(slabs, starts) of a destination, in launch order: the order the kernel sums them in."""
        idx = [(s, st) for s, st, _, k in self.segs if k == key]
        return [self.slabs[s] for s, _ in idx], [st for _, st in idx]

    def ref(self, key, init=None):
        sl, st = self.feeds(key)
        return fold64(sl, st, self.dst[key][0], init)

    def allow(self, key, init=None):
        sl, st = self.feeds(key)
        return fold_allowance(sl, st, self.dst[key][0], init)

    def float4_rule(self, key):
        """fold_fill's rule with 16-byte aligned slab and destination buffers: the length, the destination's offset, every slab's row
        stride and start are multiples of four floats."""
        ln, mis = self.dst[key]
        return ln % 4 == 0 and mis % 4 == 0 and all(self.slabs[s].shape[1] % 4 == 0 and st % 4 == 0 for s, st, _, k in self.segs if k == key)

    def init(self, key, g):
        """A non-zero prior destination of the case's kind."""
        ln = self.dst[key][0]
        if self.kind == "int":
            x = torch.randint(-8, 9, (ln,), generator=g).float()
            return torch.where(x == 0, torch.ones_like(x), x)
        return torch.randn(ln, generator=g)


def _slab(kind, rows, ld, g, scale=1.0):
    if kind == "int":
        return torch.randint(-8, 9, (rows, ld), generator=g).float()
    return torch.randn(rows, ld, generator=g) * scale


SWEEP_LD = (144, 147)                                          # a row stride divisible by four and one that is not
SWEEP_STARTS = ((0, 4), (0, 5), (0, 6), (1, 4), (1, 5))        # (slab, start): aligned / odd / even-but-unaligned, and both in the odd stride


def sweep(rows, kind):
    """Every length of LENS at every (slab, start) of SWEEP_STARTS from two slabs of ``rows`` rows, one destination each, plus "mis1": a
    destination 4 bytes past a 16-byte boundary with len % 4 == 0 and an aligned slab (the scalar path by the destination's address
    alone).  Gaussian slabs: one of the two is scaled by 1e3 or 1e-5 for two of every three row counts."""
    g = torch.Generator().manual_seed(1000 + rows + (0 if kind == "int" else 7))
    i = ROWS.index(rows) if rows in ROWS else rows
    sc = ((1.0, 1.0), (1e3, 1.0), (1.0, 1e-5))[i % 3]
    slabs = [_slab(kind, rows, ld, g, s) for ld, s in zip(SWEEP_LD, sc)]
    segs = [(s, st, ln, f"s{s}+{st}x{ln}") for s, st in SWEEP_STARTS for ln in LENS]
    segs.insert(len(segs) // 2, (0, 8, 64, "mis1"))
    return Case(f"sweep{rows}", kind, slabs, segs, {"mis1": 1})


def single(rows, kind):
    """grl_reduce_partials' shape: the whole slab, ld = len, for every length of LENS."""
    g = torch.Generator().manual_seed(2000 + rows + (0 if kind == "int" else 7))
    slabs = [_slab(kind, rows, n, g, (1.0, 1e3, 1e-5)[k % 3]) for k, n in enumerate(LENS)]
    return Case(f"single{rows}", kind, slabs, [(k, 0, n, f"n{n}") for k, n in enumerate(LENS)])


def shared(kind):
    """Several slabs per destination, given interleaved with other destinations' slabs; one slab scaled by 1e3, one by 1e-5; a zero-row
    slab among the feeds of "a" and of "b".  "a": float4 path; "b" (odd length) and "c" (odd start): scalar path."""
    g = torch.Generator().manual_seed(3000 + (0 if kind == "int" else 7))
    shapes = [(40, 260, 1.0), (7, 256, 1.0), (300, 512, 1e3), (33, 100, 1e-5), (2, 77, 1.0), (65, 200, 1.0), (0, 256, 1.0), (0, 81, 1.0)]
    slabs = [_slab(kind, r, ld, g, s) for r, ld, s in shapes]
    segs = [(0, 4, 256, "a"), (3, 5, 77, "b"), (1, 0, 256, "a"), (5, 3, 192, "c"), (6, 0, 256, "a"), (4, 0, 77, "b"), (2, 128, 256, "a"),
            (7, 2, 77, "b"), (2, 0, 192, "c")]
    return Case("shared", kind, slabs, segs)


def limit(n, kind):
    """n segments, each its own destination (64: the most one launch takes; 65: rejected)."""
    g = torch.Generator().manual_seed(4000 + n + (0 if kind == "int" else 7))
    slabs = [_slab(kind, 17, 144, g), _slab(kind, 64, 147, g)]
    lens = (1, 3, 4, 64, 65)
    return Case(f"limit{n}", kind, slabs, [(i % 2, (i * 3) % 8 if i % 2 else 4 * (i % 3), lens[i % 5], f"d{i}") for i in range(n)])


def all_cases():
    """Every (int, gauss) pair of cases the GPU test runs."""
    out = [tuple(sweep(r, k) for k in KINDS) for r in ROWS] + [tuple(single(r, k) for k in KINDS) for r in ROWS]
    return out + [tuple(shared(k) for k in KINDS), tuple(limit(64, k) for k in KINDS)]


# ----------------------------------------------------------------------------------------------------------------------------- value loss
def value_loss64(value, old, target, clip, coef, inv_batch):
    """torch float64 autograd through oracle.trpl.clipped_value_loss: -> (d (inv_batch * sum coef * loss) / d value, sum coef * loss,
    that sum * inv_batch).  ``clip`` 0: clipping off.  The sum is math.fsum's (correctly rounded), so the whole difference to an fp64 sum
    of the same terms in any order is that sum's own error."""
    v = value.double().clone().requires_grad_(True)
    terms = coef * otr.clipped_value_loss(v, old.double(), target.double(), clip)
    (terms.sum() * inv_batch).backward()
    total = math.fsum(terms.detach().tolist())
    return v.grad, total, total * inv_batch


def value_loss_allowances(value, old, target, clip, coef, inv_batch):
    """dvalue: the kernel rounds a double to fp32 once -- U |ref| plus the smallest fp32 subnormal.  The fp64 sum of B terms:
    B 2^-53 sum |terms|; the mean: that times inv_batch (its one more rounding is inside: the sum itself costs (B - 1) 2^-53)."""
    dv, _, _ = value_loss64(value, old, target, clip, coef, inv_batch)
    terms = coef * otr.clipped_value_loss(value.double(), old.double(), target.double(), clip)
    a_sum = value.numel() * 2.0 ** -53 * math.fsum(terms.abs().tolist())
    return U * dv.abs() + 2.0 ** -149, a_sum, a_sum * inv_batch


def value_rows(clip):
    """(name, old value, value, target) rows of every branch for a clip range ``clip`` > 0 (dyadic or an integer: every value below is
    an exact fp32 number, so 'on the bound' and 'tie' are exact)."""
    c = float(clip)
    return [("inside", 1.0, 1.0 + c / 2, 0.25),
            ("above, clipped loss larger", 1.0, 1.0 + 2 * c, 1.0 + 3 * c),     # |Vc - R| = 2c > |V - R| = c: gradient 0
            ("above, clipped loss smaller", 1.0, 1.0 + 2 * c, 1.0),            # |Vc - R| = c < |V - R| = 2c: the plain gradient
            ("below, clipped loss larger", 1.0, 1.0 - 2 * c, 1.0 - 3 * c),
            ("below, clipped loss smaller", 1.0, 1.0 - 2 * c, 1.0),
            ("on +clip", 0.5, 0.5 + c, 0.125),
            ("on -clip", 0.5, 0.5 - c, 0.125),
            ("V == R", 0.5, 0.75, 0.75),
            ("1e4", 1e4, 1e4 + 3.0, -1e4),
            ("-1e4", -1e4, -1e4 - c / 2, 1e4),
            ("tie outside", 0.0, 3 * c, 2 * c)]                                # (Vc - R)^2 == (V - R)^2: torch.max halves the gradient


def value_case(B, clip, seed):
    """B frames: the rows of value_rows first (for clip 0, clipping off, the rows of clip 0.25), then Gaussian frames around the range,
    a fifth of them at magnitudes of 1e4.  -> (value, old, target) fp32 and the names of the leading rows."""
    g = torch.Generator().manual_seed(seed)
    c = float(clip) if clip else 0.25
    rows = value_rows(c)[:B]
    n = B - len(rows)
    Vo = torch.randn(n, generator=g)
    V = Vo + torch.randn(n, generator=g) * min(c, 10.0) * 1.5
    R = torch.randn(n, generator=g) * 2
    big = torch.rand(n, generator=g) < 0.2
    Vo, V, R = (torch.where(big, x * 1e4, x) for x in (Vo, V, R))
    f = lambda i, x: torch.cat([torch.tensor([r[i] for r in rows], dtype=torch.float64).float(), x])
    return f(2, V), f(1, Vo), f(3, R), [r[0] for r in rows]
