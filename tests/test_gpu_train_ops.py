"""Per-op checks of the training-loop kernels (csrc/train_ops.hip, the fused fold + Adam tail of csrc/node_ops.hip) against the float64
restatements of tests/train_ops_ref.py (pinned on CPU by tests/test_train_ops_ref_cpu.py).

* Adam, every device form (grl_adam_step_dev, grl_adam_report_record_pairs, grl_fold_adam_report): each step starts the reference from the
  kernel's own fp32 state, so errors do not compound, and every element of p, m, v must lie within the fp32 allowance that
  train_ops_ref.adam_allowance derives from the arithmetic; the three forms must agree bit for bit (include/grl_hip.h says so).
* GAE, VecNorm: within the allowances of train_ops_ref.gae / vecnorm_state / vecnorm_apply.
* kNN, gather_rows_many, copy_many: exactly equal to a brute force, index_select and a plain copy.
Each test prints its worst error as a fraction of its allowance."""
import ctypes

import pytest
import torch

import train_ops_ref as tr
from geometry_rl_amd import hip

pytestmark = pytest.mark.gpu

EPS = tr.f32(1e-5)
BETAS = [(tr.f32(0.9), tr.f32(0.999)), (tr.f32(0.8), tr.f32(0.99))]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def ratio(got, ref, allow):
    """max |got - ref| / allowance; an element with allowance 0 must be exact, and a NaN or infinite error counts as infinite."""
    err = (got.double().cpu() - ref.double()).abs()
    r = torch.where(allow > 0, err / allow.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    return float(r.nan_to_num(float("inf"), float("inf")).max())


def ptrs(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def ints(xs):
    return (ctypes.c_int * max(len(xs), 1))(*xs)


def grads(g, n, kinds=(0, 1, 2, 3)):
    """n gradient entries mixing exact zeros (denominator = eps), ~1e-5 (sqrt(v_hat) ~ eps), ordinary values and 1e3-1e4."""
    x = torch.randn(n, generator=g)
    kind = torch.tensor(kinds)[torch.randint(0, len(kinds), (n,), generator=g)]
    x = torch.where(kind == 0, torch.zeros_like(x), x)
    x = torch.where(kind == 1, x * 1e-5, x)
    return torch.where(kind == 3, x.sign() * (1e3 + 9e3 * torch.rand(n, generator=g)), x)


class AdamState:
    """p, m, v, gradient as slices at element offset ``off`` of buffers with a guard region behind them, plus the device lr / step."""

    def __init__(self, n, off, g):
        d = dev()
        self.n, self.off = n, off
        self.base = [torch.randn(off + n + 67, generator=g).to(d) for _ in range(4)]
        self.base[2].zero_()
        self.base[3].zero_()
        self.guard = [b.clone() for b in self.base]
        self.p, self.g, self.m, self.v = (b[off:off + n] for b in self.base)
        self.lr, self.step = torch.zeros(1, device=d), torch.zeros(1, device=d, dtype=torch.int32)
        self.slab = torch.zeros(1, n, device=d)
        rec = torch.zeros(2 * 14 * 2, device=d)   # two ranks' (hi, lo) records for the pairs form's report workgroup
        self.report = (rec, torch.zeros(12, device=d, dtype=torch.float64), torch.zeros(2, device=d, dtype=torch.int32),
                       torch.zeros(14, device=d))

    def run(self, form, b1, b2, coef=None, scale_host=1.0):
        n = self.n
        if form == "dev":
            hip.call("grl_adam_step_dev", self.p, self.g, self.m, self.v, n, self.lr, b1, b2, EPS, self.step, coef, scale_host)
        elif form == "pairs":
            rec, sums, maxes, out14 = self.report
            hip.call("grl_adam_report_record_pairs", self.p, self.g, self.m, self.v, n, self.lr, b1, b2, EPS, self.step, rec, 2, sums,
                     maxes, 0.0, out14)
        else:   # the fused tail: a one-row slab written over the gradient (overwrite = 1), so the folded gradient is g itself
            self.slab[0].copy_(self.g)
            hip.call("grl_fold_adam_report", 1, ptrs([self.slab]), ints([1]), ints([n]), ints([0]), ints([n]), ptrs([self.g]), 1, 1,
                     self.g, self.p, self.m, self.v, self.lr, b1, b2, EPS, self.step, None, 0, None, None, 0.0, None)

    def host(self):
        return [t.detach().cpu() for t in (self.p, self.g, self.m, self.v)]

    def check_guard(self):
        """Nothing outside [off, off + n) of any buffer was written."""
        for b, gd in zip(self.base, self.guard):
            assert torch.equal(b[:self.off], gd[:self.off]) and torch.equal(b[self.off + self.n:], gd[self.off + self.n:])


def adam_check(st, form, g_host, lr, t, b1, b2, coef=None, scale_host=1.0, scale_ref=None, eg=None):
    """One kernel step from the current state, checked element by element against the float64 step from the same fp32 state."""
    st.g.copy_(g_host.to(st.g.device))
    st.lr.fill_(lr)
    st.step.fill_(t)
    p0, g0, m0, v0 = st.host()
    st.run(form, b1, b2, coef, scale_host)
    p1, _, m1, v1 = st.host()
    if scale_ref is None:
        scale_ref = scale_host * (float(coef.cpu()) if coef is not None else 1.0)
    rp, rm, rv = tr.adam(p0, g0, m0, v0, lr, b1, b2, EPS, t, scale_ref)
    ap, am, av = tr.adam_allowance(p0, g0, m0, v0, lr, b1, b2, EPS, t, scale_ref, eg)
    return max(ratio(p1, rp, ap), ratio(m1, rm, am), ratio(v1, rv, av))


# ------------------------------------------------------------------------------------------------------------------- Adam: many steps
@pytest.mark.parametrize("form", ["dev", "pairs", "fold"])
@pytest.mark.parametrize("betas", BETAS)
def test_adam_steps(form, betas):
    """120 steps with a new gradient and a new learning rate each: t = 1..40, then runs continued at t = 10^4 and t = 10^6; the slices
    start at an odd element offset (the fused form takes its scalar path there)."""
    g = torch.Generator().manual_seed(11)
    st = AdamState(4097, 3, g)
    worst = 0.0
    for t0 in (1, 10 ** 4, 10 ** 6):
        for s in range(40):
            lr = tr.f32(1e-3 * (1.0 - s / 50.0))
            worst = max(worst, adam_check(st, form, grads(g, st.n), lr, t0 + s, *betas))
            assert worst <= 1.0, (form, t0 + s, worst)
    st.check_guard()
    print(f"adam steps {form} {betas}: worst err/allowance {worst:.3f}")


def _flat_numel():
    from geometry_rl_amd import agent, graph
    kw = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    _, _, _, loss = agent.build_agent(graph.rigid_spec(), agent.AgentConfig(**kw), device=dev())
    return agent.PolicyUpdater(loss).flat.numel()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262143, 262144, 262145, 1000003, "flat"])
def test_adam_sizes(n):
    """Every form at the grid-stride edges (1024 workgroups of 256: 262 144 elements), past them and at the real flat buffer's size.  No
    gradient entry is zero, so an element that is skipped or updated twice cannot sit inside its allowance."""
    if n == "flat":
        n = _flat_numel()
    g = torch.Generator().manual_seed(n)
    worst = 0.0
    for form, off in (("dev", 1), ("pairs", 0), ("pairs", 5), ("fold", 0), ("fold", 2)):
        st = AdamState(n, off, g)
        for t in (1, 2, 3):
            worst = max(worst, adam_check(st, form, grads(g, n, (1, 2, 3)), tr.f32(3e-4 / t), t, *BETAS[0]))
            assert worst <= 1.0, (form, off, t, worst)
        st.check_guard()
    print(f"adam n={n}: worst err/allowance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------- Adam: clipping
@pytest.mark.parametrize("max_norm", [0.5, 1e7])
def test_adam_clipped(max_norm):
    """grl_clip_coef then grl_adam_step_dev(scale_dev = coef), as PolicyUpdater._adam does with clip_grad_norm, against
    clip_grad_norm_ + torch.optim.Adam in float64 (train_ops_ref.adam with the float64 clip coefficient, pinned to torch on CPU).  The
    coefficient: the squared norm is summed in fp64, sqrt, + 1e-6f, the division and the conversions: within 4 U of the float64 one -- an
    allowance of 4 U |g| on the gradient.  Also scale_host != 1 (a 1/world factor in front of the coefficient)."""
    d = dev()
    g = torch.Generator().manual_seed(21)
    st = AdamState(50001, 7, g)
    sq, coef = torch.zeros(1, device=d, dtype=torch.float64), torch.zeros(1, device=d)
    worst, coef_worst = 0.0, 0.0
    for s in range(30):
        gr = grads(g, st.n)
        st.g.copy_(gr.to(d))
        hip.call("grl_clip_coef", st.g, st.n, tr.f32(max_norm), sq, coef)
        c_ref = tr.clip_coef(gr, tr.f32(max_norm))
        r = abs(float(coef.cpu()) - c_ref) / (4 * tr.U * c_ref)
        assert r <= 1.0, (s, r)
        coef_worst = max(coef_worst, r)
        ssq = float(gr.double().pow(2).sum())   # exact fp64 products, any summation order: within n 2^-53 of each other
        assert abs(float(sq.cpu()) - ssq) <= st.n * 2.0 ** -53 * ssq
        scale_host = 1.0 if s % 2 == 0 else 0.5
        worst = max(worst, adam_check(st, "dev", gr, tr.f32(1e-3), s + 1, *BETAS[s % 2], coef, scale_host, scale_host * c_ref,
                                      eg=gr.abs() * 4 * tr.U))
        assert coef_worst <= 1.0 and worst <= 1.0, (s, coef_worst, worst)
    if max_norm < 1:
        assert c_ref < 1e-2   # the clip was active
    st.check_guard()
    print(f"adam clipped max_norm={max_norm}: worst err/allowance {worst:.3f}, coef {coef_worst:.3f}")


# ---------------------------------------------------------------------------------------------------------- Adam: the three forms agree
@pytest.mark.parametrize("n", [4096, 4099])
def test_adam_forms_bitwise(n):
    """include/grl_hip.h: the fused tail uses grl_adam_step_dev's arithmetic bit for bit, and grl_adam_report_record_pairs is
    grl_adam_step_dev with scale 1.  The same fp32 (p, g, m, v, lr, step) through each form: identical bits (n = 4096: the fused form's
    float4 path, 4099: its scalar path)."""
    g = torch.Generator().manual_seed(n)
    p0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    v0 = torch.rand(n, generator=g) * 1e-3
    for t, b in ((1, BETAS[0]), (2, BETAS[1]), (7, BETAS[0]), (10 ** 4, BETAS[0]), (10 ** 6, BETAS[1])):
        gr = grads(g, n)
        outs = []
        for form in ("dev", "pairs", "fold"):
            st = AdamState(n, 0, torch.Generator().manual_seed(0))
            st.p.copy_(p0)
            st.m.copy_(m0)
            st.v.copy_(v0)
            st.g.copy_(gr)
            st.lr.fill_(tr.f32(7e-4))
            st.step.fill_(t)
            st.run(form, *b)
            outs.append([x.view(torch.int32) for x in (st.p.cpu(), st.m.cpu(), st.v.cpu())])
        for form, o in zip(("pairs", "fold"), outs[1:]):
            for name, a, r in zip("pmv", o, outs[0]):
                assert torch.equal(a, r), (form, name, t, int((a != r).sum()))


# ------------------------------------------------------------------------------------------------------------ Adam: the fused fold tail
@pytest.mark.parametrize("overwrite", [1, 0])
@pytest.mark.parametrize("report", [False, True])
def test_fold_adam(overwrite, report):
    """grl_fold_adam_report over a flat gradient buffer with parallel params / exp_avg / exp_avg_sq: destination A (float4 path, three
    slabs), B (odd start and length: scalar path, two slabs), C (aligned, but a slab starts at an odd column: scalar path).  The folded
    gradient against the float64 fold (an fp32 sum of R terms: (R + 1) U sum |terms|), Adam against the float64 step from the kernel's
    own stored gradient and the prior state, and every entry that no slab covers keeps p, m, v and gradient bit for bit.  overwrite = 0
    accumulates into a non-zero gradient: Adam must see the accumulated value.  With the report workgroup the sums must be the slots'
    column sums and p, m, v the bits of the run without it."""
    d = dev()
    g = torch.Generator().manual_seed(31 + overwrite)
    N = 1200
    dsts = [(16, 256), (301, 77), (640, 192)]
    slabs = [  # (dst index, rows, ld, start)
        (0, 40, 260, 4), (0, 7, 256, 0), (0, 300, 512, 128),
        (1, 33, 100, 5), (1, 2, 77, 0),
        (2, 65, 200, 3)]
    flat = [torch.randn(N, generator=g) for _ in range(4)]
    flat[2] *= 1e-2
    flat[3] = flat[3].abs() * 1e-3
    b1, b2 = BETAS[0]
    steps = []
    for t in (1, 2, 3):
        parts = [torch.randn(r, ld, generator=g) * (1e3 if t == 2 and i == 0 else 1.0) for i, (_, r, ld, _) in enumerate(slabs)]
        steps.append((t, tr.f32(1e-3 / t), parts))

    def run(with_report):
        gb, pb, mb, vb = (x.clone().to(d) for x in flat)
        if overwrite:
            gb.fill_(float("nan"))
            gb[[i for i in range(N) if not any(o <= i < o + L for o, L in dsts)]] = 0.0
        lr, step = torch.zeros(1, device=d), torch.zeros(1, device=d, dtype=torch.int32)
        batch = 40
        slots = torch.randn(hip.query("grl_trpl_slot_doubles", batch), generator=g, dtype=torch.float64).to(d)
        sums, maxes, out14 = (torch.zeros(12, device=d, dtype=torch.float64), torch.zeros(2, device=d, dtype=torch.int32),
                              torch.zeros(14, device=d))
        worst, hist = 0.0, []
        for t, lrv, parts in steps:
            dp = [x.to(d) for x in parts]
            lr.fill_(lrv)
            step.fill_(t)
            g0, p0, m0, v0 = (x.cpu() for x in (gb, pb, mb, vb))
            hip.call("grl_fold_adam_report", len(slabs), ptrs(dp), ints([s[1] for s in slabs]), ints([s[2] for s in slabs]),
                     ints([s[3] for s in slabs]), ints([dsts[s[0]][1] for s in slabs]), ptrs([gb[dsts[s[0]][0]:] for s in slabs]),
                     overwrite, 1, gb, pb, mb, vb, lr, b1, b2, EPS, step, slots if with_report else None, batch, sums, maxes, 0.01,
                     out14)
            g1, p1, m1, v1 = (x.cpu() for x in (gb, pb, mb, vb))
            covered = torch.zeros(N, dtype=torch.bool)
            for di, (o, L) in enumerate(dsts):
                covered[o:o + L] = True
                terms = [x[:, st_:st_ + L].double() for (dj, _, _, st_), x in zip(slabs, parts) if dj == di]
                ref = sum(x.sum(0) for x in terms) + (0.0 if overwrite else g0[o:o + L].double())
                R = sum(x.shape[0] for x in terms) + (0 if overwrite else 1)
                allow = (R + 1) * tr.U * (sum(x.abs().sum(0) for x in terms) + (0.0 if overwrite else g0[o:o + L].double().abs()))
                worst = max(worst, ratio(g1[o:o + L], ref, allow))
                gk = g1[o:o + L]
                rp, rm, rv = tr.adam(p0[o:o + L], gk, m0[o:o + L], v0[o:o + L], lrv, b1, b2, EPS, t)
                ap, am, av = tr.adam_allowance(p0[o:o + L], gk, m0[o:o + L], v0[o:o + L], lrv, b1, b2, EPS, t)
                worst = max(worst, ratio(p1[o:o + L], rp, ap), ratio(m1[o:o + L], rm, am), ratio(v1[o:o + L], rv, av))
            for a, b in ((g1, g0), (p1, p0), (m1, m0), (v1, v0)):
                assert torch.equal(a[~covered].view(torch.int32), b[~covered].view(torch.int32))
            assert worst <= 1.0, (t, worst)
            if with_report:
                col = slots.cpu().view(-1, 14)
                assert torch.allclose(sums.cpu(), col[:, :12].sum(0), rtol=1e-12, atol=1e-12)
            hist.append((p1, m1, v1, g1))
        return worst, hist

    worst, hist = run(report)
    if report:
        _, plain = run(False)
        for a, b in zip(hist, plain):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    print(f"fold+adam overwrite={overwrite} report={report}: worst err/allowance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------ Adam: trajectory vs torch fp32
def test_adam_trajectory_vs_torch_fp32():
    """200 steps of grl_adam_step_dev against torch.optim.Adam(eps=1e-5) in fp32 on CPU (the optimizer the reference trains with), each
    side on its own trajectory.  Per step both sides stay within a few U of the float64 update (32 U for the roundings of either side) plus
    the bias corrections' error (torch's are float64, the kernel's fp32), the betas (torch's are the float64 0.9 / 0.999, the kernel's their
    fp32 values: a relative difference |b - b_f32| / (1 - b) in each new term's weight, more through the decayed ones), and the relative error
    of m and v grows by at most ~4 U a step;
    measured on the magnitude M_s = lr/bc1 EMA(|g|) / D (no cancellation in it), plus 2 ulp of p per step.  The allowance is the sum
    over the steps so far."""
    d = dev()
    g = torch.Generator().manual_seed(41)
    n = 10007
    b1, b2 = 0.9, 0.999
    p0 = torch.randn(n, generator=g)
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([w], lr=1e-3, betas=(b1, b2), eps=1e-5)
    st = AdamState(n, 0, g)
    st.p.copy_(p0)
    mabs, vref = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    tol = torch.zeros(n, dtype=torch.float64)
    worst = 0.0
    for t in range(1, 201):
        lr = 1e-3 * (1.0 - t / 400)
        gr = grads(g, n, (1, 2, 3))
        opt.param_groups[0]["lr"] = lr
        w.grad = gr.clone()
        opt.step()
        st.g.copy_(gr.to(d))
        st.lr.fill_(lr)
        st.step.fill_(t)
        st.run("dev", tr.f32(b1), tr.f32(b2))
        mabs = b1 * mabs + (1 - b1) * gr.double().abs()
        vref = b2 * vref + (1 - b2) * gr.double() ** 2
        bc1, ebc1, bc2, ebc2 = tr.bias_corrections(tr.f32(b1), tr.f32(b2), t)
        M = lr / bc1 * mabs / (vref.sqrt() / bc2 ** 0.5 + 1e-5)
        tol += ((32 + 4 * t) * tr.U + 2 * (ebc1 / bc1 + ebc2 / bc2) + 16 * abs(tr.f32(b1) - b1) / (1 - b1) + 4 * abs(tr.f32(b2) - b2) / (1 - b2)) * M \
            + 2 * tr.ulp32(w.detach())
        worst = max(worst, ratio(st.p.cpu(), w.detach().double(), tol))
        assert worst <= 1.0, (t, worst)
    print(f"adam trajectory vs torch fp32 (200 steps): worst err/allowance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------------ GAE
def _gae_case(N, T, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(N, T, generator=g)
    V = torch.randn(N, T + 1, generator=g) * 3
    r[: N // 5] *= 1e3
    done = torch.rand(N, T, generator=g) < 0.04
    term = torch.rand(N, T, generator=g) < 0.04       # independent of done: done without terminated and terminated without done
    for i, t in enumerate((0, 63, 64, 127, T - 1)):   # episode ends on and around the 64-step tiles
        if t < T and i < N:
            rows = torch.arange(i, N, 5)
            done[rows, t] = True
            term[rows[::2], t] = True
    return r, done, term, V


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_gae(N):
    """agent.gae (grl_gae_scan) against the float64 scan within train_ops_ref.gae's allowance (error of each step's delta and run carried
    backwards with gamma lambda: it grows with T and the magnitudes, not a fixed bar) for T across the 64-step tiles and two (gamma, lmbda)."""
    from geometry_rl_amd import agent
    d = dev()
    worst = 0.0
    for T in (1, 2, 63, 64, 65, 128, 129, 300):
        for gamma, lmbda in ((0.99, 0.95), (0.9, 0.5)):
            r, done, term, V = _gae_case(N, T, N * 1000 + T)
            adv, tgt = agent.gae(r.to(d), done.to(d), term.to(d), V.to(d), gamma, lmbda)
            ra, rt, ea, et = tr.gae(r, done, term, V, tr.f32(gamma), tr.f32(lmbda))
            worst = max(worst, ratio(adv, ra, ea), ratio(tgt, rt, et))
            assert worst <= 1.0, (T, gamma, worst)
    print(f"gae N={N}: worst err/allowance {worst:.3f}")


# -------------------------------------------------------------------------------------------------------------------------------- VecNorm
@pytest.mark.parametrize("K", [1, 3, 5, 7, 63, 64])
def test_vecnorm(K):
    """grl_vecnorm at rows 1, 256 * floor(256/K) +- 1 (the partial kernel's one sweep of its 256 workgroups) and > 10x that (its grid-stride
    loop), three updating calls then a frozen one, two decays, clip bounds that are hit, and each of y_norm / y_clip left out.  The state
    against the float64 update from the kernel's previous state (train_ops_ref.vecnorm_state), y_norm against the float64 normalisation
    from the kernel's new state, y_clip exactly; a frozen call leaves the state's bits alone."""
    d = dev()
    per = 256 // K
    scratch = torch.empty(hip.query("grl_vecnorm_scratch_bytes", K), device=d, dtype=torch.uint8)
    lo, hi, eps = -2.5, 2.5, tr.f32(1e-2)
    worst = {"state": (0.0,), "y_norm": (0.0,)}
    for rows in (1, 256 * per - 1, 256 * per + 1, 10 * 256 * per + 7):
        for decay in (tr.f32(0.99999), tr.f32(0.9)):
            g = torch.Generator().manual_seed(rows * K)
            state = torch.zeros(2 * K + 1, device=d)
            for call, (update, want) in enumerate(((1, "both"), (1, "norm"), (1, "clip"), (0, "both"))):
                x = (torch.randn(rows, K, generator=g) * 3 + torch.arange(K) % 5 - 2).to(d)
                yn = torch.full_like(x, float("nan")) if want in ("both", "norm") else None
                yc = torch.full_like(x, float("nan")) if want in ("both", "clip") else None
                s0 = state.cpu()
                hip.call("grl_vecnorm", x, ctypes.c_longlong(rows), K, decay, eps, update, lo, hi, state, scratch, yn, yc)
                s1 = state.cpu()
                rs, rsa = tr.vecnorm_state(x.cpu(), s0, decay, bool(update))
                if update:
                    worst["state"] = max(worst["state"], (ratio(s1, rs, rsa), rows, decay, call))
                else:
                    assert torch.equal(s1.view(torch.int32), s0.view(torch.int32))
                if yn is not None:
                    ry, ra = tr.vecnorm_apply(x.cpu(), s1, eps, lo, hi)
                    worst["y_norm"] = max(worst["y_norm"], (ratio(yn, ry, ra), rows, decay, call))
                if yc is not None:
                    assert torch.equal(yc.cpu(), x.cpu().clamp(lo, hi))
                assert max(w[0] for w in worst.values()) <= 1.0, (rows, decay, call, worst)
    print(f"vecnorm K={K}: worst err/allowance (ratio, rows, decay, call) {worst}")


def test_vecnorm_rejects_bad_widths():
    d = dev()
    x = torch.zeros(65 * 4, device=d)
    state = torch.zeros(2 * 65 + 1, device=d)
    scratch = torch.empty(hip.query("grl_vecnorm_scratch_bytes", 64), device=d, dtype=torch.uint8)
    for K in (0, 65):
        with pytest.raises(RuntimeError, match="status -2"):
            hip.call("grl_vecnorm", x, ctypes.c_longlong(4), K, 0.99, 0.01, 1, -5.0, 5.0, state, scratch, x, None)


# ------------------------------------------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("P", [1, 2, 3, 4, 31, 127, 128])
def test_knn(P):
    """grl_knn_topology on a coarse integer lattice (duplicates and exact ties everywhere; the fp32 squared distances are exact) against
    the float64 brute force in stable (distance, index) order with -1 padding, for n_valid in {0, 1, k, k+1, P, > P} and a null n_valid."""
    d = dev()
    for k in (1, 3, 8):
        g = torch.Generator().manual_seed(P * 10 + k)
        nv = torch.tensor([0, 1, k, k + 1, P, P + 3, max(P - 1, 0)], dtype=torch.int32)
        B = nv.numel()
        pos = torch.randint(-2, 3, (B, P, 3), generator=g).float() * 0.5
        for n_valid in (nv, None):
            out = torch.full((B, P, k), -7, device=d, dtype=torch.int32)
            hip.call("grl_knn_topology", pos.to(d), n_valid.to(d) if n_valid is not None else None, out, B, P, k)
            ref = tr.knn(pos, n_valid, k)
            assert torch.equal(out.cpu(), ref), (k, n_valid, int((out.cpu() != ref).sum()))


def test_knn_rejects_bad_sizes():
    d = dev()
    pos = torch.zeros(1, 129, 3, device=d)
    out = torch.zeros(129 * 9, device=d, dtype=torch.int32)
    for P, k in ((129, 3), (8, 0), (8, 9)):
        with pytest.raises(RuntimeError, match="status -2"):
            hip.call("grl_knn_topology", pos, None, out, 1, P, k)


# -------------------------------------------------------------------------------------------------------------- gather_rows / copy_many
@pytest.mark.parametrize("n_t", [1, 5, 24])
def test_gather_rows_many(n_t):
    """dst[k] = src[k][idx] for n_t tensors with rows of 1, 3, 7, 64 and 195 words; n_rows not a multiple of the grid stride; repeated
    indices and the last row: bitwise index_select, and nothing behind each destination written."""
    d = dev()
    g = torch.Generator().manual_seed(n_t)
    R, n_rows = 1000, 777
    widths = [(1, 3, 7, 64, 195)[i % 5] for i in range(n_t)]
    src = [torch.randint(-2 ** 31, 2 ** 31 - 1, (R, w), generator=g, dtype=torch.int32).to(d) for w in widths]
    dst = [torch.full((n_rows + 1, w), 0x7F7F7F7F, device=d, dtype=torch.int32) for w in widths]
    idx = torch.randint(0, R, (n_rows,), generator=g)
    idx[:3] = R - 1
    idx[10:20] = 5
    idx = idx.to(d)
    hip.call("grl_gather_rows_many", ptrs(dst), ptrs(src), (ctypes.c_longlong * n_t)(*[4 * w for w in widths]), n_t, idx, n_rows)
    for s, o in zip(src, dst):
        assert torch.equal(o[:n_rows], s.index_select(0, idx))
        assert (o[n_rows] == 0x7F7F7F7F).all()


def test_gather_rows_many_rejects():
    d = dev()
    a = torch.zeros(4, 4, device=d)
    idx = torch.zeros(2, dtype=torch.long, device=d)
    with pytest.raises(RuntimeError, match="status -3"):
        hip.call("grl_gather_rows_many", ptrs([a]), ptrs([a]), (ctypes.c_longlong * 1)(6), 1, idx, 2)
    with pytest.raises(RuntimeError, match="status -2"):
        hip.call("grl_gather_rows_many", ptrs([a] * 25), ptrs([a] * 25), (ctypes.c_longlong * 25)(*[16] * 25), 25, idx, 2)


def test_copy_many():
    """24 jobs: byte counts 0, 1, 15, 16, 17 and a few MB, source and destination both 16-byte aligned (the uint4 path and its byte tail)
    or offset by 1-15 bytes (the byte path): the destination equals the source bitwise, and the bytes around it are untouched."""
    d = dev()
    g = torch.Generator().manual_seed(51)
    sizes = [0, 1, 15, 16, 17, 3 * 2 ** 20 + 5]
    jobs = []
    for i in range(24):
        nb = sizes[i % len(sizes)]
        so, do = (0, 0) if i < 12 else (1 + i % 15, 1 + (i * 7) % 15)
        src = torch.randint(0, 256, (nb + 64,), generator=g, dtype=torch.uint8).to(d)
        dst = torch.randint(0, 256, (nb + 64,), generator=g, dtype=torch.uint8).to(d)
        jobs.append((src, dst, so, do, nb, dst.clone()))
    hip.call("grl_copy_many", (ctypes.c_void_p * 24)(*[j[1].data_ptr() + j[3] for j in jobs]),
             (ctypes.c_void_p * 24)(*[j[0].data_ptr() + j[2] for j in jobs]), (ctypes.c_longlong * 24)(*[j[4] for j in jobs]), 24)
    for src, dst, so, do, nb, before in jobs:
        assert torch.equal(dst[do:do + nb], src[so:so + nb]), (nb, so, do)
        assert torch.equal(dst[:do], before[:do]) and torch.equal(dst[do + nb:], before[do + nb:]), (nb, so, do)
