"""Per-op checks of the gradient fold (csrc/node_ops.hip: grl_reduce_partials, _seg, _multi, _multi_ow, grl_fold_adam_report,
grl_fold_record_pairs) and of the critic lane's value loss (csrc/head_ops.hip grl_value_loss) against the float64 restatements of
tests/fold_ref.py (pinned on CPU by tests/test_fold_ref_cpu.py), plus grl_write_doubles and a satisfied grl_wait_flag_ge.

Every destination is a slice of one buffer with sentinel words around it, every slab a slice of a buffer with NaN rows in front of and
behind it; after every call the sentinels and the slab buffers must keep their bits (column and row overruns show without a fault).

Allowances, none of them measured (worst error / allowance on the MI355X in brackets):
* integer slabs in [-8, 8]: every entry point returns THE sum, bit for bit, on the scalar and on the float4 path  [exact];
* Gaussian slabs (one scaled by 1e3, one by 1e-5): (R + 1) U sum |terms|, R summed terms, no floor  [0.460, at 2 rows; 0.004 at 257];
* identities include/grl_hip.h promises: equal bits;
* grl_value_loss: dvalue U |ref| + 2^-149 (one rounding of a double)  [0.999]; the fp64 sums B 2^-53 sum |terms|  [0.028];
  mean_out the fp32 cast of the kernel's own out2[1]: equal bits.
Each test prints its worst error as a fraction of its allowance."""
import ctypes
import time

import pytest
import torch

import fold_ref as fr
from geometry_rl_amd import hip

pytestmark = pytest.mark.gpu

PAD = 1024               # NaN floats in front of and behind every slab (more than a row of the widest slab)
GUARD = 16               # sentinel words around every destination
SENT = 0x7F7F7F7F
FAMILY = ("multi", "multi_ow", "fold_adam", "record_pairs")   # entry points of reduce_partials_multi_kernel
BATCH, WORLD, RANK = 40, 3, 1                                 # the record workgroup of grl_fold_record_pairs


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32)


def vp(xs):
    return (ctypes.c_void_p * max(len(xs), 1))(*xs)


def ints(xs):
    return (ctypes.c_int * max(len(xs), 1))(*xs)


class Arena:
    """A case's slabs and destinations in device memory."""

    def __init__(self, case):
        d = dev()
        self.case = case
        self.sbuf, self.sptr = [], []
        for s in case.slabs:
            b = torch.full((2 * PAD + s.numel(),), float("nan"))
            b[PAD:PAD + s.numel()] = s.reshape(-1)
            b = b.to(d)
            self.sbuf.append(b)
            self.sptr.append(b.data_ptr() + 4 * PAD)
        self.skeep = [b.clone() for b in self.sbuf]
        self.off, pos = {}, GUARD
        for k, (ln, mis) in case.dst.items():
            pos = (pos + 3) // 4 * 4 + mis
            self.off[k] = pos
            pos += ln + GUARD
        self.n = (pos + 3) // 4 * 4
        self.covered = torch.zeros(self.n, dtype=torch.bool)
        for k, (ln, _) in case.dst.items():
            self.covered[self.off[k]:self.off[k] + ln] = True

    def dst(self, fill):
        """A destination buffer: sentinels everywhere, fill[key] (a tensor or a float) in each destination.  -> (device, host copy)"""
        host = bits(torch.empty(self.n)).fill_(SENT).view(torch.float32)
        for k, (ln, _) in self.case.dst.items():
            host[self.off[k]:self.off[k] + ln] = fill[k] if isinstance(fill, dict) else fill
        buf = host.to(dev())
        assert buf.data_ptr() % 16 == 0 and all(p % 16 == 0 for p in self.sptr)
        return buf, host

    def float4(self, buf, key):
        """fold_fill's rule on the real addresses."""
        ln, _ = self.case.dst[key]
        ok = ln % 4 == 0 and (buf.data_ptr() + 4 * self.off[key]) % 16 == 0
        for s, st, _, k in self.case.segs:
            if k == key:
                ok = ok and self.case.slabs[s].shape[1] % 4 == 0 and (self.sptr[s] + 4 * st) % 16 == 0
        return ok

    def args(self, buf, segs):
        sl = self.case.slabs
        return (len(segs), vp([self.sptr[s] for s, _, _, _ in segs]), ints([sl[s].shape[0] for s, _, _, _ in segs]),
                ints([sl[s].shape[1] for s, _, _, _ in segs]), ints([st for _, st, _, _ in segs]), ints([ln for _, _, ln, _ in segs]),
                vp([buf.data_ptr() + 4 * self.off[k] for _, _, _, k in segs]))

    def call(self, entry, buf, segs=None, ow=0, region=None, slots=None):
        """One launch of ``entry`` over ``segs`` (default: the case's).  entry "seg" / "single": one launch per slab and at most 8
        segments / per segment; there ``ow`` is the set of destination keys written instead of accumulated into."""
        segs = self.case.segs if segs is None else segs
        if entry == "multi":
            hip.call("grl_reduce_partials_multi", *self.args(buf, segs))
        elif entry == "multi_ow":
            hip.call("grl_reduce_partials_multi_ow", *self.args(buf, segs), ow)
        elif entry == "fold_adam":
            hip.call("grl_fold_adam_report", *self.args(buf, segs), ow, 0, None, None, None, None, None, 0.0, 0.0, 0.0, None, None, 0, None,
                     None, 0.0, None)
        elif entry == "record_pairs":
            hip.call("grl_fold_record_pairs", *self.args(buf, segs), ow, slots, BATCH, RANK, WORLD, region)
        elif entry == "seg":
            for s in range(len(self.case.slabs)):
                mine = [x for x in segs if x[0] == s]
                for i in range(0, len(mine), 8):
                    part = mine[i:i + 8]
                    sh = self.case.slabs[s].shape
                    hip.call("grl_reduce_partials_seg", ctypes.c_void_p(self.sptr[s]), sh[0], sh[1], len(part),
                             vp([buf.data_ptr() + 4 * self.off[k] for _, _, _, k in part]), ints([st for _, st, _, _ in part]),
                             ints([ln for _, _, ln, _ in part]), sum(1 << j for j, x in enumerate(part) if x[3] in ow))
        elif entry == "single":
            for s, st, ln, k in segs:
                assert st == 0 and ln == self.case.slabs[s].shape[1]
                hip.call("grl_reduce_partials", ctypes.c_void_p(self.sptr[s]), ctypes.c_void_p(buf.data_ptr() + 4 * self.off[k]),
                         self.case.slabs[s].shape[0], ln)
        else:
            raise ValueError(entry)

    def read(self, buf, host):
        """-> key -> destination contents (CPU), after checking that every sentinel and every slab buffer kept its bits."""
        out = buf.cpu()
        assert torch.equal(bits(out)[~self.covered], bits(host)[~self.covered]), (self.case.name, "a sentinel word was written")
        for b, k in zip(self.sbuf, self.skeep):
            assert torch.equal(bits(b), bits(k)), (self.case.name, "a slab buffer was written")
        return {k: out[self.off[k]:self.off[k] + ln] for k, (ln, _) in self.case.dst.items()}


def record_args():
    g = torch.Generator().manual_seed(9)
    slots = torch.randn(hip.query("grl_trpl_slot_doubles", BATCH), generator=g, dtype=torch.float64).abs().to(dev())
    return slots, torch.full((WORLD * 28,), 7.0, device=dev())


def run_entry(ar, entry, g, ow_keys):
    """``entry`` on the arena's case: destinations in ``ow_keys`` are NaN-filled and written, the others hold a non-zero prior value
    and are accumulated into.  -> (results, priors (None where written))"""
    case = ar.case
    init = {k: (None if k in ow_keys else case.init(k, g)) for k in case.dst}
    buf, host = ar.dst({k: (float("nan") if v is None else v) for k, v in init.items()})
    if entry in ("seg", "single"):
        ar.call(entry, buf, ow=ow_keys)
    else:
        slots, region = record_args() if entry == "record_pairs" else (None, None)
        ar.call(entry, buf, ow=1 if ow_keys else 0, region=region, slots=slots)
    return ar.read(buf, host), init


def plan(case):
    """(entry, keys written instead of accumulated into) for a case: accumulation through grl_reduce_partials_multi (and _multi_ow),
    overwrite through every entry point of the multi kernel, a mix of overwrite-mask bits through the segmented kernel."""
    keys = list(case.dst)
    multi_slab = len(case.segs) > len(case.dst)
    out = [("multi", set()), ("multi_ow", set()), ("multi_ow", set(keys)), ("fold_adam", set(keys)), ("record_pairs", set(keys))]
    if not multi_slab:   # (the segmented kernel folds ONE slab per launch: a destination with several feeds is not its business)
        out.append(("seg", {k for i, k in enumerate(keys) if (0b10110101 >> (i % 8)) & 1}))
    return out


def check_case(case):
    """Every entry of plan(case): exact for an integer case, within fold_allowance for a Gaussian one.  -> worst error / allowance"""
    ar = Arena(case)
    g = torch.Generator().manual_seed(77)
    worst = 0.0
    for entry, ow_keys in plan(case):
        got, init = run_entry(ar, entry, g, ow_keys)
        for k in case.dst:
            ref = case.ref(k, init[k])
            if case.kind == "int":
                assert torch.equal(got[k].double(), ref), (case.name, entry, k, int((got[k].double() != ref).sum()))
            else:
                r = fr.ratio(got[k], ref, case.allow(k, init[k]))
                assert r <= 1.0, (case.name, entry, k, r)
                worst = max(worst, r)
    return worst, ar


def check_single(rows, kind):
    """grl_reduce_partials (accumulating) and one-segment launches of grl_reduce_partials_seg (written and accumulated) on whole slabs."""
    case = fr.single(rows, kind)
    ar = Arena(case)
    g = torch.Generator().manual_seed(78)
    worst = 0.0
    keys = list(case.dst)
    for entry, ow_keys in (("single", set()), ("seg", set(keys[::2])), ("seg", set(keys[1::2]))):
        got, init = run_entry(ar, entry, g, ow_keys)
        for k in keys:
            ref = case.ref(k, init[k])
            if kind == "int":
                assert torch.equal(got[k].double(), ref), (case.name, entry, k)
            else:
                worst = max(worst, fr.ratio(got[k], ref, case.allow(k, init[k])))
                assert worst <= 1.0, (case.name, entry, k, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------------- exact sums
@pytest.mark.parametrize("rows", fr.ROWS)
def test_fold_exact_integer_sums(rows):
    """Integer slabs: any summation order gives the same fp32 result, so a row that is duplicated, dropped, or read clamped without
    being masked fails, whatever the kernel's tuning.  Both paths are known to run: the aligned destinations satisfy fold_fill's rule on
    their real addresses, the others (odd length, odd or unaligned start, odd row stride, a destination 4 bytes past a 16-byte boundary) do not."""
    case = fr.sweep(rows, "int")
    _, ar = check_case(case)
    buf, _ = ar.dst(0.0)
    vec = {k for k in case.dst if ar.float4(buf, k)}
    assert vec == {k for k in case.dst if case.float4_rule(k)} == {f"s0+4x{n}" for n in (4, 64, 128, 132)}
    assert not ar.float4(buf, "mis1") and case.dst["mis1"][0] % 4 == 0
    check_single(rows, "int")


@pytest.mark.parametrize("kind", fr.KINDS)
def test_fold_shared_destinations_and_64_segments(kind):
    """Several slabs per destination, interleaved with other destinations' slabs (a zero-row slab among them contributes nothing), and
    exactly 64 segments in one launch."""
    worst = max(check_case(fr.shared(kind))[0], check_case(fr.limit(64, kind))[0])
    print(f"fold shared / 64 segments {kind}: worst err/allowance {worst:.3f}")


# -------------------------------------------------------------------------------------------------------------------- Gaussian values
@pytest.mark.parametrize("rows", fr.ROWS)
def test_fold_gaussian(rows):
    worst = max(check_case(fr.sweep(rows, "gauss"))[0], check_single(rows, "gauss"))
    print(f"fold gaussian rows={rows}: worst err/allowance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ bitwise identities
@pytest.mark.parametrize("rows", [33, 257])
def test_fold_bitwise_identities(rows):
    """include/grl_hip.h: the fold is bitwise reproducible; a destination's sum does not depend on the other destinations of the launch
    nor on its place among them (the blk0 lookup); grl_reduce_partials_multi = _multi_ow(overwrite = 0); written into NaN = accumulated
    into zeros; grl_fold_adam_report(adam = 0) and grl_fold_record_pairs produce _multi_ow's gradients, and the latter's record is
    grl_trpl_fold_record_pairs'.  (Nothing says the scalar and the float4 path agree bitwise: not asserted.)"""
    case = fr.sweep(rows, "gauss")
    ar = Arena(case)
    g = torch.Generator().manual_seed(5)
    init = {k: case.init(k, g) for k in case.dst}

    def run(entry, fill, segs=None, ow=0, **kw):
        buf, host = ar.dst(fill)
        ar.call(entry, buf, segs=segs, ow=ow, **kw)
        return ar.read(buf, host)

    def same(a, b, keys=None):
        for k in (keys or case.dst):
            assert torch.equal(bits(a[k]), bits(b[k])), (k, int((bits(a[k]) != bits(b[k])).sum()))

    acc = run("multi", init)
    same(acc, run("multi", init))
    same(acc, run("multi_ow", init, ow=0))
    ow1 = run("multi_ow", float("nan"), ow=1)
    same(ow1, run("multi_ow", float("nan"), ow=1))
    same(ow1, run("multi_ow", 0.0, ow=0))
    same(ow1, run("multi_ow", float("nan"), segs=case.segs[::-1], ow=1))
    same(ow1, run("multi_ow", float("nan"), segs=case.segs[7:] + case.segs[:7], ow=1))
    for i in (0, 1, len(case.segs) // 2, len(case.segs) - 1):   # alone: its untouched neighbours keep their NaN
        k = case.segs[i][3]
        alone = run("multi_ow", float("nan"), segs=[case.segs[i]], ow=1)
        same(ow1, alone, [k])
        assert all(alone[o].isnan().all() for o in case.dst if o != k)
    same(ow1, run("fold_adam", float("nan"), ow=1))
    same(acc, run("fold_adam", init, ow=0))
    slots, region = record_args()
    same(ow1, run("record_pairs", float("nan"), ow=1, slots=slots, region=region))
    want = torch.full_like(region, 7.0)
    hip.call("grl_trpl_fold_record_pairs", slots, BATCH, RANK, WORLD, want)
    assert torch.equal(bits(region), bits(want)) and not torch.equal(region, torch.full_like(region, 7.0))
    hip.call("grl_fold_record_pairs", 0, vp([]), ints([]), ints([]), ints([]), ints([]), vp([]), 1, slots, BATCH, RANK, WORLD, region.fill_(7.0))
    assert torch.equal(bits(region), bits(want))                # (no segments: the record workgroup alone)


# ------------------------------------------------------------------------------------------------------------------------- rejections
def test_fold_rejections_write_nothing():
    """More than 64 (8 for the segmented kernel) segments: -2; two segments with one destination and different lengths: -3; nothing is
    launched (the destinations keep their bits)."""
    case = fr.limit(65, "int")
    ar = Arena(case)
    buf, host = ar.dst(float("nan"))
    for entry in FAMILY:
        slots, region = record_args() if entry == "record_pairs" else (None, None)
        with pytest.raises(RuntimeError, match="status -2"):
            ar.call(entry, buf, ow=1, slots=slots, region=region)
    one = [x for x in case.segs if x[0] == 0]
    sh = case.slabs[0].shape
    with pytest.raises(RuntimeError, match="status -2"):
        hip.call("grl_reduce_partials_seg", ctypes.c_void_p(ar.sptr[0]), sh[0], sh[1], 9, vp([buf.data_ptr() + 4 * ar.off[x[3]] for x in one[:9]]),
                 ints([x[1] for x in one[:9]]), ints([x[2] for x in one[:9]]), 0x1FF)
    k = case.segs[3][3]                                          # len 64
    clash = [case.segs[3], (1, 0, 4, k)]
    for entry in FAMILY:
        slots, region = record_args() if entry == "record_pairs" else (None, None)
        with pytest.raises(RuntimeError, match="status -3"):
            ar.call(entry, buf, segs=clash, ow=1, slots=slots, region=region)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf.cpu()), bits(host))


# ------------------------------------------------------------------------------------------------------------------------ non-finite rows
@pytest.mark.parametrize("rows", [9, 33, 129, 257])
def test_fold_nonfinite_rows(rows):
    """+inf in the LAST row of slabs whose row count leaves a remainder on both paths (the row the clamped remainder loads re-read): that
    column is +inf, not NaN (a 0/1 factor instead of a select would make it so); a NaN in one entry reaches its own column only; every
    other column stays within its allowance."""
    case = fr.sweep(rows, "gauss")
    for s in case.slabs:
        s[-1, 20] = float("inf")
        s[rows // 2, 40] = float("nan")
    ar = Arena(case)
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for entry, ow_keys in plan(case):
        got, init = run_entry(ar, entry, g, ow_keys)
        n_inf = n_nan = 0
        for k, (ln, _) in case.dst.items():
            ref = case.ref(k, init[k])
            fin = ref.isfinite()
            assert torch.equal(got[k].double()[~fin].nan_to_num(nan=-1.0), ref[~fin].nan_to_num(nan=-1.0)), (entry, k, got[k][~fin], ref[~fin])
            n_inf += int(ref.isinf().sum())
            n_nan += int(ref.isnan().sum())
            allow = case.allow(k, init[k])
            worst = max(worst, fr.ratio(got[k][fin], ref[fin], allow[fin]))
            assert worst <= 1.0, (entry, k, worst)
        assert n_inf >= 20 and n_nan >= 20                       # (the columns lie inside every destination of 63 or more entries)
    print(f"fold non-finite rows={rows}: worst err/allowance of the finite columns {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------ zero-row slabs
def test_fold_zero_row_destination():
    """include/grl_hip.h: the multi kernel's entry points treat a zero-row slab as a sum of nothing -- a destination fed by nothing else is
    written with zeros under overwrite and left alone otherwise; grl_reduce_partials and grl_reduce_partials_seg launch nothing for a
    zero-row slab, so their destinations keep their contents even under overwrite (no caller has such a slab: every *_blocks query
    returns at least 1)."""
    g = torch.Generator().manual_seed(1)
    slabs = [torch.randint(-8, 9, (5, 64), generator=g).float(), torch.zeros(0, 64), torch.zeros(0, 67)]
    case = fr.Case("zero", "int", slabs, [(0, 0, 64, "fed"), (1, 0, 64, "vec0"), (2, 3, 61, "scalar0")])
    ar = Arena(case)
    for entry in FAMILY:
        if entry == "multi":
            continue
        slots, region = record_args() if entry == "record_pairs" else (None, None)
        buf, host = ar.dst(float("nan"))
        ar.call(entry, buf, ow=1, slots=slots, region=region)
        got = ar.read(buf, host)
        assert torch.equal(got["fed"].double(), case.ref("fed")), entry
        assert torch.equal(bits(got["vec0"]), bits(torch.zeros(64))) and torch.equal(bits(got["scalar0"]), bits(torch.zeros(61))), entry
    buf, host = ar.dst(3.0)
    ar.call("multi", buf)
    got = ar.read(buf, host)
    assert torch.equal(got["fed"].double(), case.ref("fed") + 3.0) and (got["vec0"] == 3.0).all() and (got["scalar0"] == 3.0).all()
    buf, host = ar.dst(float("nan"))
    sh = slabs[1].shape
    hip.call("grl_reduce_partials_seg", ctypes.c_void_p(ar.sptr[1]), 0, sh[1], 1, vp([buf.data_ptr() + 4 * ar.off["vec0"]]), ints([0]), ints([64]), 1)
    hip.call("grl_reduce_partials", ctypes.c_void_p(ar.sptr[1]), ctypes.c_void_p(buf.data_ptr() + 4 * ar.off["vec0"]), 0, 64)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf.cpu()), bits(host))


# ---------------------------------------------------------------------------------------------------------------------------- value loss
def value_loss(V, Vo, R, clip, coef, inv, with_mean=True):
    d = dev()
    B = V.numel()
    dbuf = bits(torch.empty(B + 2 * GUARD)).fill_(SENT).view(torch.float32).to(d)
    out2 = torch.full((4,), -7.0, dtype=torch.float64, device=d)
    mean = bits(torch.empty(3)).fill_(SENT).view(torch.float32).to(d)
    hip.call("grl_value_loss", V.to(d), Vo.to(d), R.to(d), ctypes.c_double(clip), ctypes.c_double(coef), ctypes.c_double(inv),
             ctypes.c_void_p(dbuf.data_ptr() + 4 * GUARD), out2, ctypes.c_void_p(mean.data_ptr() + 4) if with_mean else None, B)
    dh, oh, mh = dbuf.cpu(), out2.cpu(), mean.cpu()
    assert (bits(dh)[:GUARD] == SENT).all() and (bits(dh)[GUARD + B:] == SENT).all() and (oh[2:] == -7.0).all()
    assert int(bits(mh)[0]) == SENT and int(bits(mh)[2]) == SENT and (with_mean or int(bits(mh)[1]) == SENT)
    return dh[GUARD:GUARD + B], oh[:2], mh[1]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_value_loss(B):
    """One workgroup of 1024 threads and 16 waves over B frames holding rows of every branch (fold_ref.value_rows), for clipping off,
    0.25 and 1e6, both coefficients, and 1/B and 1/(2B) (a two-rank shard), against float64 autograd through the oracle's loss."""
    worst = [0.0, 0.0, 0.0]
    for clip in (0.0, 0.25, 1e6):
        V, Vo, R, _ = fr.value_case(B, clip, B)
        for coef in (0.5, 1.0):
            for inv in (1.0 / B, 1.0 / (2 * B)):
                dv, out2, mean = value_loss(V, Vo, R, clip, coef, inv)
                rdv, rsum, rmean = fr.value_loss64(V, Vo, R, clip, coef, inv)
                a_dv, a_sum, a_mean = fr.value_loss_allowances(V, Vo, R, clip, coef, inv)
                r = (fr.ratio(dv, rdv, a_dv), abs(float(out2[0]) - rsum) / a_sum if a_sum > 0 else float(float(out2[0]) != rsum),
                     abs(float(out2[1]) - rmean) / a_mean if a_mean > 0 else float(float(out2[1]) != rmean))
                assert max(r) <= 1.0, (clip, coef, inv, r, (dv.double() - rdv).abs().argmax())
                assert torch.equal(bits(mean.reshape(1)), bits(out2[1].float().reshape(1))), (clip, coef, inv)
                worst = [max(a, b) for a, b in zip(worst, r)]
    _, out2, _ = value_loss(V, Vo, R, 0.25, 1.0, 1.0 / B, with_mean=False)   # mean_out is optional
    assert float(out2[1]) == float(out2[0]) * (1.0 / B)
    print(f"value loss B={B}: worst err/allowance dvalue {worst[0]:.3f}, sum {worst[1]:.3f}, mean {worst[2]:.3f}")


@pytest.mark.parametrize("clip", [0.25, 1e6])
def test_value_loss_branches_and_tie(clip):
    """The named rows one by one, in exact arithmetic: gradient 0 where the clipped loss is the larger one outside the range, the plain
    gradient where it is the smaller one, the clipped value's gradient on the bounds (they count as inside), 0 at V == R -- and on an exact
    tie outside the range HALF the plain gradient, as torch.max's autograd splits it."""
    rows = fr.value_rows(clip)
    t = lambda i: torch.tensor([r[i] for r in rows], dtype=torch.float64).float()
    V, Vo, R = t(2), t(1), t(3)
    B = len(rows)
    dv, _, _ = value_loss(V, Vo, R, clip, 1.0, 1.0)
    rdv, _, _ = fr.value_loss64(V, Vo, R, clip, 1.0, 1.0)
    got = dict(zip((r[0] for r in rows), dv.tolist()))
    print(f"value loss rows clip={clip}: " + ", ".join(f"{n}: {g:g} (float64 autograd {float(w):g})" for (n, g), w in zip(got.items(), rdv)))
    d = lambda n: next(float(v.double() - r.double()) for (m, _, _, _), v, r in zip(rows, V, R) if m == n)
    assert got["above, clipped loss larger"] == 0.0 and got["below, clipped loss larger"] == 0.0 and got["V == R"] == 0.0
    for n in ("inside", "above, clipped loss smaller", "below, clipped loss smaller", "on +clip", "on -clip", "1e4", "-1e4"):
        assert got[n] == float(torch.tensor(2 * d(n)).float()), n
    assert got["tie outside"] == d("tie outside"), (got["tie outside"], 2 * d("tie outside"))
    assert B == 11


def test_value_loss_rejects():
    d = dev()
    x = torch.zeros(4, device=d)
    out2 = torch.full((2,), -7.0, dtype=torch.float64, device=d)
    z = ctypes.c_double(0.0)
    for a in ((None, x, x, x, out2, 4), (x, None, x, x, out2, 4), (x, x, None, x, out2, 4), (x, x, x, None, out2, 4), (x, x, x, x, None, 4),
              (x, x, x, x, out2, 0), (x, x, x, x, out2, -1)):
        with pytest.raises(RuntimeError, match="status -2"):
            hip.call("grl_value_loss", a[0], a[1], a[2], z, z, z, a[3], a[4], None, a[5])
    torch.cuda.synchronize()
    assert (out2.cpu() == -7.0).all() and (x.cpu() == 0).all()


# ------------------------------------------------------------------------------------------------------------------------- small riders
@pytest.mark.parametrize("n", [1, 16])
def test_write_doubles(n):
    """The host doubles, bit for bit (values no float holds, an infinity, a negative zero, a subnormal), and nothing around them."""
    vals = [1.0 / 3.0, -0.0, float("inf"), 5e-324, -1e300, 2.0 ** 53 + 2.0] + [0.1 * k for k in range(10)]
    buf = torch.full((n + 8,), -7.0, dtype=torch.float64, device=dev())
    hip.call("grl_write_doubles", ctypes.c_void_p(buf.data_ptr() + 8 * 4), (ctypes.c_double * n)(*vals[:n]), n)
    h = buf.cpu()
    assert torch.equal(h[4:4 + n].view(torch.int64), torch.tensor(vals[:n], dtype=torch.float64).view(torch.int64))
    assert (h[:4] == -7.0).all() and (h[4 + n:] == -7.0).all()
    for bad in (0, 17):
        with pytest.raises(RuntimeError, match="status -2"):
            hip.call("grl_write_doubles", buf, (ctypes.c_double * 17)(), bad)


@pytest.mark.parametrize("flag,count,add", [(5, 4, 1), (9, 4, 1), (0, 0, 0), (-2 ** 31 + 1, 2 ** 31 - 2, 3), (-2 ** 31 + 5, 2 ** 31 - 2, 3),
                                            (2 ** 31 - 1, 2 ** 31 - 3, 2)])
def test_wait_flag_already_satisfied(flag, count, add):
    """flag >= count + add by SIGNED DIFFERENCE (the counters may wrap): the gate lets the stream pass at once -- the copy queued behind it
    completes long before the gate's own time limit (10 s here) could have released it."""
    d = dev()
    f = torch.tensor([flag], dtype=torch.int32, device=d)
    c = torch.tensor([count], dtype=torch.int32, device=d)
    src = torch.arange(1000, device=d, dtype=torch.float32)
    dst = torch.zeros_like(src)
    one = torch.ones(1, dtype=torch.int32, device=d)
    hip.call("grl_wait_flag_ge", one, one, 0, 10_000_000)      # (the kernel's code is loaded before the clock starts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip.call("grl_wait_flag_ge", f, c, add, 10_000_000)
    dst.copy_(src)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.equal(dst, src)
    assert dt < 2.0, dt
    with pytest.raises(RuntimeError, match="status -2"):
        hip.call("grl_wait_flag_ge", None, c, add, 1000)
