"""The loss, optimiser and rollout kernels on poisoned, guarded buffers (tests/footprint.py): head_ops.hip (the fused TRPL / PPO /
KL-penalty launch and every consumer of its per-workgroup slots, grl_value_loss, grl_adv_stats, grl_gaussian_sample, the small writers),
train_ops.hip / node_ops.hip (the three Adam forms, grl_clip_coef, the fold family, grl_gae_scan, grl_vecnorm, grl_knn_topology),
stats_ops.hip, the time-batched critic pass, and whole eager paths through ``PolicyUpdater`` and the collector.

Like tests/test_gpu_footprint.py every case runs three times from identical inputs (``fp.three_runs``): plain, under ``Guarded(NAN)`` and
under ``Guarded(HUGE)``.  Every input and index array is wrapped, every output, workspace and scratch comes from the ledger (through the
interposed module where a wrapper allocates it, through ``w.out`` where the test calls ``hip.call`` itself), every buffer a kernel
changes in place is an in/out buffer (``w.inout``; ``w.fresh`` where the kernel has to write all of it: it then starts from the poison).
Asserted: ``ledger.check`` of both guarded runs and that every result is BITWISE the plain run's -- no tolerance anywhere; the float64
comparisons stay in test_gpu_trpl_kernel.py, test_gpu_entropy_control.py, test_gpu_klpen.py, test_gpu_train_ops.py, test_gpu_fold_ops.py,
test_gpu_stats_ops.py and test_gpu_rollout.py, whose case tables these tests run.  Every case prints its interposed and wrapped counts;
the last test prints every entry point the file launched."""
import types

import pytest
import torch

import entropy_cases as ec
import fold_ref as fr
import footprint as fp
import train_ops_ref as tr
import trpl_cases as tc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, I32 = torch.float32, torch.float64, torch.int32
LAUNCHED = set()   # every entry point this file's tests launched
RAN = set()        # ... and the tests that ran
NAMED = ("grl_trpl_fwd_bwd", "grl_trpl_fwd_bwd_ent", "grl_ppo_fwd_bwd", "grl_klpen_fwd_bwd", "grl_trpl_target_terms", "grl_trpl_fold",
         "grl_trpl_report", "grl_trpl_fold_record", "grl_trpl_report_records", "grl_trpl_fold_record_pairs", "grl_trpl_report_record_pairs",
         "grl_trpl_loss_values", "grl_adv_stats", "grl_value_loss", "grl_klpen_adapt", "grl_write_doubles", "grl_write_floats",
         "grl_gaussian_sample", "grl_adam_step_dev", "grl_adam_report_record_pairs", "grl_fold_adam_report", "grl_clip_coef",
         "grl_reduce_partials", "grl_reduce_partials_seg", "grl_reduce_partials_multi", "grl_reduce_partials_multi_ow", "grl_gae_scan",
         "grl_vecnorm", "grl_knn_topology", "grl_explained_variance", "grl_episode_scan", "grl_stats_accumulate", "grl_deepsets_fwd1_groups")


@pytest.fixture(autouse=True)
def record_launches(request, monkeypatch):
    from geometry_rl_amd import hip
    assert torch.cuda.is_available(), "these tests need the MI355X"
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (LAUNCHED.add(entry), real_call(entry, *a, **k))[1])
    RAN.add(request.node.originalname)
    yield


def whole_path_modules():
    from geometry_rl_amd import agent, graph, klpen, ops, policy, ppo, rollout, transforms, trpl, updater
    return (ops, graph, updater, trpl, ppo, klpen, agent, policy, transforms, rollout)


def out(w, n, dtype=F32):
    return w.out(n if isinstance(n, tuple) else (n,), dtype, DEV)


# ================================================================================================ the loss family
RECORDS = (1, 2, 8)
PAIRS = ((0, 1), (0, 2), (1, 2), (7, 8))


def slot_consumers(w, fold, B, ent_coef):
    """Every consumer of a deferred launch's slots, each into buffers of its own taken from the ledger."""
    from geometry_rl_amd import hip
    ent = float(ent_coef)
    res = {}
    s, m, o14 = out(w, 12, F64), out(w, 2, I32), out(w, 14)
    hip.call("grl_trpl_report", fold.slots, B, s, m, ent, o14)
    res["report"] = [s, m, o14]
    for n in RECORDS:
        rec = out(w, (n, 14), F64)
        for i in range(n):
            hip.call("grl_trpl_fold_record", fold.slots, B, rec[i])
        s, m, o14 = out(w, 12, F64), out(w, 2, I32), out(w, 14)
        hip.call("grl_trpl_report_records", rec, n, s, m, ent, o14)
        res[f"records{n}"] = [rec, s, m, o14]
    for rank, world in PAIRS:
        region = out(w, (world, 14, 2))   # the rank's own row written, every other row zeroed: a row left alone shows as poison
        hip.call("grl_trpl_fold_record_pairs", fold.slots, B, rank, world, region)
        s, m, o14 = out(w, 12, F64), out(w, 2, I32), out(w, 14)
        hip.call("grl_trpl_report_record_pairs", region, world, s, m, ent, o14)
        res[f"pairs{rank}of{world}"] = [region, s, m, o14]
    sums, maxes = fold()
    o14 = out(w, 14)
    hip.call("grl_trpl_loss_values", sums, maxes, ent, o14)
    res["fold"] = [sums, maxes, o14]
    return res


def finish(w, outs, B, ent_coef, defer):
    """The tuple a loss launch returned -> results; a deferred launch's slots through every consumer, a direct one's sums through
    grl_trpl_loss_values."""
    from geometry_rl_amd import hip
    sums, rest = outs[0], list(outs[1:])
    if defer:
        return {"launch": rest, "consumers": slot_consumers(w, sums, B, ent_coef)}
    o14 = out(w, 14)
    hip.call("grl_trpl_loss_values", sums, rest[0], float(ent_coef), o14)
    return {"launch": [sums] + rest, "values": o14}


VARIANTS = [(p, v, d) for p in (False, True) for v in (False, True) for d in (False, True)]   # want_projection, value, defer_fold


def variant_name(p, v, d):
    return f"proj={int(p)} value={int(v)} defer={int(d)}"


def trpl_inputs(c, d):
    I = {"loc": d["loc"].to(DEV), "sigma": d["sigma"].to(DEV), "value": d["value"].to(DEV) if d["value"] is not None else None,
         "batch": {k: v.to(DEV) for k, v in d["batch"].items()}}
    if c.adv_mode == "shard":   # the global batch's statistics, as the all-reduced grl_adv_stats of the data-parallel ranks
        a = d["adv_global"].double()
        I["adv_stats"] = torch.tensor([float(a.sum()), float((a * a).sum())], dtype=F64, device=DEV)
    return I


def run_trpl(op, c, d, proj_type=None, ent=None, label=None):
    """One TRPL case through every variant; ``ent`` = (mode word, bound): the scheduled entropy stage inside the launch, its bound wrapped."""
    from geometry_rl_amd import hip, ops
    I = trpl_inputs(c, d)
    has_value = I["value"] is not None
    proj = c.proj if proj_type is None else proj_type

    def run(w, want_proj, value, defer):
        batch = {k: w(v) for k, v in I["batch"].items()}
        adv_stats = None
        if c.adv_mode == "kernel_stats":
            adv_stats = out(w, 2, F64)
            hip.call("grl_adv_stats", batch["advantage"], adv_stats, c.B)
        elif c.adv_mode == "shard":
            adv_stats = w(I["adv_stats"])
        kw = dict(ent_mode=ent[0], ent_beta=w(torch.tensor([ent[1]], dtype=F64, device=DEV))) if ent is not None else {}
        outs = ops.trpl_fwd_bwd(w(I["loc"]), w(I["sigma"]), batch, w(I["value"]) if value else None, mean_bound=tc.EPS, cov_bound=tc.EPS_COV,
                                trust_region_coeff=c.tr_coeff, entropy_coef=c.ent_coef, critic_coef=c.critic_coef, clip_value=c.clip_value,
                                global_batch=c.global_batch, adv_stats=adv_stats, want_projection=want_proj, proj_type=proj,
                                defer_fold=defer, adv_local=c.adv_mode == "local", **kw)
        assert (outs[4] is not None) == value and (outs[5] is not None) == want_proj
        return finish(w, outs, c.B, c.ent_coef, defer)

    for p, v, df in VARIANTS:
        if v and not has_value:
            continue
        fp.three_runs(op, f"{label or c.name} code={proj} {variant_name(p, v, df)}", lambda w: run(w, p, v, df))


def run_target_terms(c, d, proj):
    from geometry_rl_amd import ops
    loc, sigma, tm, tS = (t.to(DEV) for t in (d["loc"], d["sigma"], d["batch"]["loc"], d["batch"]["var"]))

    def run(w):
        outs = ops.trpl_target_terms(w(loc), w(sigma), w(tm), w(tS), mean_bound=tc.EPS, cov_bound=tc.EPS_COV,
                                     trust_region_coeff=c.tr_coeff, global_batch=c.B, proj_type=proj)
        return dict(zip(("sums", "maxes", "dloc", "dsigma"), outs))

    fp.three_runs("trpl_target_terms", f"B={c.B} A={c.A} code={proj}", run)


EUCLID = {6: 1, 7: 2}   # the Euclidean codes run on the inputs of the precision-scaled projection they are the other form of
LANE_CODES = [(A, p) for A in range(1, 17) for p in (0, 1, 2, 4, 6, 7)]


@pytest.mark.parametrize("A,code", LANE_CODES, ids=[f"A{A}-code{p}" for A, p in LANE_CODES])
def test_trpl_lane_widths(A, code):
    """A = 1 .. 16 at B = 37 (three workgroups, the last with five frames), every projection code; and grl_trpl_target_terms on the same."""
    c = tc.Case(B=37, A=A, proj=EUCLID.get(code, code))
    d = tc.make_case(c)
    run_trpl("trpl_fwd_bwd", c, d, proj_type=code)
    run_target_terms(c, d, code)


@pytest.mark.parametrize("c", tc.batch_cases(), ids=lambda c: c.name)
def test_trpl_batch_and_fold_edges(c):
    """B = 1, 2, 15, 16, 17, 1008, 1024, 1025, 4097: 1, 63, 64, 65 and 257 slots under the 256-thread fold."""
    run_trpl("trpl_fwd_bwd", c, tc.make_case(c))


@pytest.mark.parametrize("c", tc.option_cases(), ids=lambda c: c.name)
def test_trpl_options(c):
    run_trpl("trpl_fwd_bwd", c, tc.make_case(c))


@pytest.mark.parametrize("e", ec.all_cases(), ids=lambda e: e.name)
def test_trpl_entropy_stage(e):
    """grl_trpl_fwd_bwd_ent at entropy_cases' lane and batch cases, the bound a wrapped device double."""
    d = ec.make_case(e)
    run_trpl("trpl_fwd_bwd_ent", e.base, d, ent=(e.mode, d["beta"]), label=e.name)


def ppo_like(op, B, A, launch, scalar):
    """The PPO grid for the two modes that take a one-element device scalar (clip epsilon / beta, wrapped) in front of the batch."""
    d = tc.make_ppo_case(B, A)
    g = torch.Generator().manual_seed(900 + 31 * A + B)
    batch = dict(d["batch"])   # an old distribution for the KL-penalty mode: 0.3 away per dimension, variances up to 4x either way
    batch["loc"] = d["loc"] + 0.3 * torch.randn(B, A, generator=g)
    batch["var"] = (d["sigma"] ** 2 * torch.exp2(4 * torch.rand(B, A, generator=g) - 2)).float()
    I = {"loc": d["loc"].to(DEV), "sigma": d["sigma"].to(DEV), "value": d["value"].to(DEV), "batch": {k: v.to(DEV) for k, v in batch.items()}}
    s0 = torch.tensor(scalar, dtype=F32, device=DEV)

    def run(w, value, defer):
        outs = launch(w(I["loc"]), w(I["sigma"]), {k: w(v) for k, v in I["batch"].items()}, w(I["value"]) if value else None, w(s0),
                      entropy_coef=0.015625, critic_coef=0.5, clip_value=0.2, global_batch=B, adv_stats=None, defer_fold=defer, adv_local=True)
        assert len(outs) == 5 and (outs[4] is not None) == value
        return finish(w, outs, B, 0.015625, defer)

    for v in (False, True):
        for df in (False, True):
            fp.three_runs(op, f"B={B} A={A} {variant_name(False, v, df)}", lambda w: run(w, v, df))


@pytest.mark.parametrize("B,A", tc.PPO_GRID)
def test_ppo_mode(B, A):
    from geometry_rl_amd import ops
    ppo_like("ppo_fwd_bwd", B, A, lambda loc, sigma, batch, value, ce, **kw: ops.ppo_fwd_bwd(loc, sigma, batch, value, clip_epsilon=ce, **kw),
             tc.PPO_EPS)


@pytest.mark.parametrize("B,A", tc.PPO_GRID)
def test_klpen_mode(B, A):
    from geometry_rl_amd import ops
    ppo_like("klpen_fwd_bwd", B, A, lambda loc, sigma, batch, value, beta, **kw: ops.klpen_fwd_bwd(loc, sigma, batch, value, beta=beta, **kw),
             1.5)


@pytest.mark.parametrize("poison", fp.POISONS)
def test_a_slot_no_workgroup_wrote_is_noticed(poison):
    """That the guarded runs see what plain runs cannot, on the real kernels and inside the allocations: a fold told 16 frames more than
    the launch had reads one slot no workgroup wrote.  On a fresh ``torch.empty`` that slot is very often zero; poisoned, it reaches the
    sums and check (c) reports it.  The extra slot lies inside the slots buffer's own back guard (asserted before anything is launched)."""
    from geometry_rl_amd import hip, ops
    c = tc.Case(B=37, A=5)
    d = tc.make_case(c)
    extra = hip.query("grl_trpl_slot_doubles", c.B + 16) - hip.query("grl_trpl_slot_doubles", c.B)
    assert 0 < extra < fp.guard_width((hip.query("grl_trpl_slot_doubles", c.B),), F64), extra
    I = trpl_inputs(c, d)
    with fp.Guarded(poison) as ledger:
        w = ledger.guard
        fold, maxes, dloc, dsigma, dvalue, pm, pv = ops.trpl_fwd_bwd(
            w(I["loc"]), w(I["sigma"]), {k: w(v) for k, v in I["batch"].items()}, w(I["value"]), mean_bound=tc.EPS, cov_bound=tc.EPS_COV,
            trust_region_coeff=c.tr_coeff, entropy_coef=c.ent_coef, critic_coef=c.critic_coef, clip_value=c.clip_value, global_batch=c.B,
            adv_stats=None, want_projection=True, proj_type=0, defer_fold=True, adv_local=True)
        hip.call("grl_trpl_fold", fold.slots, c.B + 16, fold.sums, fold.maxes)
        torch.cuda.synchronize()
    ledger.check({"dloc": dloc, "dsigma": dsigma, "dvalue": dvalue, "proj": [pm, pv]})   # what the launch writes itself is sound
    with pytest.raises(AssertionError, match=r"\(c\) result sums "):
        ledger.check({"sums": fold.sums})


# ------------------------------------------------------------------------------------------------ the loss family's small kernels
@pytest.mark.parametrize("B", tc.B_SWEEP)
def test_adv_stats(B):
    from geometry_rl_amd import hip
    adv = torch.randn(B, generator=torch.Generator().manual_seed(B)).to(DEV)

    def run(w):
        stats = out(w, 2, F64)
        hip.call("grl_adv_stats", w(adv), stats, B)
        return {"stats": stats}

    fp.three_runs("grl_adv_stats", f"B={B}", run)


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_value_loss(B, with_mean):
    from geometry_rl_amd import hip
    V, Vo, R, _ = (t.to(DEV) if torch.is_tensor(t) else t for t in fr.value_case(B, 0.25, B))

    def run(w, clip):
        dvalue, out2, mean = out(w, B), out(w, 2, F64), out(w, 1) if with_mean else None
        hip.call("grl_value_loss", w(V), w(Vo), w(R), clip, 0.5, 1.0 / B, dvalue, out2, mean, B)
        return {"dvalue": dvalue, "out2": out2, "mean": mean}

    for clip in (0.0, 0.25):
        fp.three_runs("grl_value_loss", f"B={B} clip={clip} mean_out={with_mean}", lambda w: run(w, clip))


@pytest.mark.parametrize("factor,want", [(2.0, 2.0), (1.0, 1.0), (0.4, 0.5)])
def test_klpen_adapt(factor, want):
    """All three branches, beta in/out; the 14-float report it reads is written into a ledger buffer by grl_write_floats."""
    from geometry_rl_amd import ops
    dtarg = 0.01
    rep = torch.randn(14, generator=torch.Generator().manual_seed(5)).tolist()
    rep[5] = factor * dtarg

    def run(w):
        out14, beta = out(w, 14), w.inout(torch.tensor([3.0], device=DEV))
        ops.write_floats(out14, rep)
        ops.klpen_adapt(out14, beta, dtarg, 2.0, 0.5)
        return {"out14": out14, "beta": beta}

    plain = fp.three_runs("grl_klpen_adapt", f"kl={factor} dtarg", run)
    assert float(plain["beta"]) == 3.0 * want


@pytest.mark.parametrize("n", [1, 16])
def test_write_doubles(n):
    from geometry_rl_amd import ops
    vals = ([1.0 / 3.0, -0.0, 5e-324, -1e300, 2.0 ** 53 + 2.0] + [0.1 * k for k in range(11)])[:n]

    def run(w):
        dst = out(w, n, F64)
        ops.write_doubles(dst, vals)
        return {"dst": dst}

    plain = fp.three_runs("grl_write_doubles", f"n={n}", run)
    assert plain["dst"].cpu().tolist() == vals


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("n", [1, 64])
def test_write_floats(n, mirror):
    from geometry_rl_amd import ops
    vals = [0.1 * (k + 1) for k in range(n)]

    def run(w):
        dst, mir = out(w, n), out(w, 1) if mirror else None
        ops.write_floats(dst, vals, mir, n - 1)
        return {"dst": dst, "mirror": mir}

    plain = fp.three_runs("grl_write_floats", f"n={n} mirror={mirror}", run)
    assert torch.equal(plain["dst"].cpu(), torch.tensor(vals, dtype=F32))
    assert not mirror or float(plain["mirror"]) == float(plain["dst"][n - 1])


@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("A", [1, 3, 16])
def test_gaussian_sample(A, B):
    from geometry_rl_amd import hip
    g = torch.Generator().manual_seed(70 + A + B)
    loc, sigma, eps = torch.randn(B, A, generator=g).to(DEV), (torch.rand(B, A, generator=g) * 1.7 + 0.3).to(DEV), torch.randn(B, A, generator=g).to(DEV)

    def run(w):
        action, var, logp = out(w, (B, A)), out(w, (B, A)), out(w, B)
        hip.call("grl_gaussian_sample", w(loc), w(sigma), w(eps), action, logp, var, B, A)
        return {"action": action, "var": var, "logp": logp}

    fp.three_runs("grl_gaussian_sample", f"A={A} B={B}", run)


# ================================================================================================ optimiser and fold
ADAM_EPS = tr.f32(1e-5)
B1, B2 = tr.f32(0.9), tr.f32(0.999)
ADAM_SIZES = [1, 255, 256, 257, 4099, 262143, 262144, 262145]


def adam_state(n):
    g = torch.Generator().manual_seed(n)
    p, grad, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    v = torch.rand(n, generator=g) * 1e-3
    return [t.to(DEV) for t in (p, grad, m, v)], g


@pytest.mark.parametrize("clip", [None, 0.5, 1e7], ids=["noclip", "clip0.5", "clip1e7"])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_step_dev(n, clip):
    """grl_adam_step_dev, params and both moments in/out, gradient / lr / step wrapped; with clipping grl_clip_coef in front of it, its
    squared norm and coefficient from the ledger (0.5: the clip is active; 1e7: it is not)."""
    from geometry_rl_amd import hip
    (p0, g0, m0, v0), _ = adam_state(n)
    lr, step = torch.tensor([tr.f32(7e-4)], device=DEV), torch.tensor([3], dtype=I32, device=DEV)

    def run(w):
        p, m, v, grad = w.inout(p0), w.inout(m0), w.inout(v0), w(g0)
        sq = coef = None
        if clip is not None:
            sq, coef = out(w, 1, F64), out(w, 1)
            hip.call("grl_clip_coef", grad, n, tr.f32(clip), sq, coef)
        hip.call("grl_adam_step_dev", p, grad, m, v, n, w(lr), B1, B2, ADAM_EPS, w(step), coef, 1.0)
        return {"p": p, "m": m, "v": v, "sq": sq, "coef": coef}

    plain = fp.three_runs("grl_adam_step_dev", f"n={n} clip={clip}", run, direct=True)
    assert not torch.equal(plain["p"], p0)
    if clip is not None and n >= 255:
        assert (float(plain["coef"]) < 1.0) == (clip < 1.0), float(plain["coef"])


def test_an_adam_tail_one_element_past_the_buffers_is_noticed():
    """The hole the in/out buffers close, on the real kernel and inside the allocations: grl_adam_step_dev told n + 1 updates one element
    behind params and both moments -- invisible on exact-size tensors from a caching allocator, where it lands in a neighbouring block.
    Here the element is the first back guard word of each in/out buffer, and what the kernel reads there is the poison: with the huge
    finite one the second moment b2 v + (1 - b2) g^2 overflows to +inf, so that guard word changes for certain and (a) reports it, while
    the n elements themselves are the plain run's bit for bit.  (Under the NaN poison every operand of that element is the same NaN and
    the result may carry its payload back: nothing is asserted there -- the reason each case runs under both poisons.)"""
    from geometry_rl_amd import hip
    n, extra = 257, 1
    assert extra < fp.guard_width((n,), F32), "the extra element stays inside the test's own buffers"
    (p0, g0, m0, v0), _ = adam_state(n)
    lr, step = torch.tensor([tr.f32(7e-4)], device=DEV), torch.tensor([3], dtype=I32, device=DEV)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    hip.call("grl_adam_step_dev", p, g0, m, v, n, lr, B1, B2, ADAM_EPS, step, None, 1.0)
    with fp.Guarded(fp.HUGE) as ledger:
        gp, gm, gv = ledger.inout(p0), ledger.inout(m0), ledger.inout(v0)
        hip.call("grl_adam_step_dev", gp, ledger.guard(g0), gm, gv, n + extra, ledger.guard(lr), B1, B2, ADAM_EPS, ledger.guard(step), None, 1.0)
        torch.cuda.synchronize()
    assert not fp.same_bits({"p": p, "m": m, "v": v}, {"p": gp, "m": gm, "v": gv})
    with pytest.raises(AssertionError, match=r"\(a\) guard words changed: inout buffer of shape \(257,\), torch.float32, back guard.*"
                                             r"0 element\(s\) behind the last"):
        ledger.check({"p": gp, "m": gm, "v": gv}, direct=True)


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_report_record_pairs(n):
    """The data-parallel tail: Adam plus the report workgroup over two ranks' (hi, lo) records."""
    from geometry_rl_amd import hip
    (p0, g0, m0, v0), g = adam_state(n)
    lr, step = torch.tensor([tr.f32(7e-4)], device=DEV), torch.tensor([3], dtype=I32, device=DEV)
    rec = torch.randn(2 * 14 * 2, generator=g).abs().to(DEV)

    def run(w):
        p, m, v = w.inout(p0), w.inout(m0), w.inout(v0)
        sums, maxes, out14 = out(w, 12, F64), out(w, 2, I32), out(w, 14)
        hip.call("grl_adam_report_record_pairs", p, w(g0), m, v, n, w(lr), B1, B2, ADAM_EPS, w(step), w(rec), 2, sums, maxes, 0.01, out14)
        return {"p": p, "m": m, "v": v, "sums": sums, "maxes": maxes, "out14": out14}

    fp.three_runs("grl_adam_report_record_pairs", f"n={n}", run)


@pytest.mark.parametrize("report", [False, True])
@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_fold_adam_report(n, overwrite, report):
    """The fused tail over a whole flat buffer: three slab rows folded into the gradient (written from the poison under overwrite,
    accumulated in place otherwise), Adam on params and both moments in place, with and without the report workgroup."""
    from geometry_rl_amd import hip
    (p0, g0, m0, v0), g = adam_state(n)
    lr, step = torch.tensor([tr.f32(7e-4)], device=DEV), torch.tensor([3], dtype=I32, device=DEV)
    slab = torch.randn(3, n, generator=g).to(DEV)
    batch = 40
    slots = torch.randn(hip.query("grl_trpl_slot_doubles", batch), generator=g, dtype=F64).abs().to(DEV)

    def run(w):
        p, m, v = w.inout(p0), w.inout(m0), w.inout(v0)
        grad = w.fresh((n,), F32, DEV) if overwrite else w.inout(g0)
        sums, maxes, out14 = (out(w, 12, F64), out(w, 2, I32), out(w, 14)) if report else (None, None, None)
        hip.call("grl_fold_adam_report", 1, [w(slab)], [3], [n], [0], [n], [grad], overwrite, 1, grad, p, m, v, w(lr), B1, B2, ADAM_EPS,
                 w(step), w(slots) if report else None, batch, sums, maxes, 0.01, out14)
        return {"p": p, "m": m, "v": v, "grad": grad, "sums": sums, "maxes": maxes, "out14": out14}

    fp.three_runs("grl_fold_adam_report", f"n={n} overwrite={overwrite} report={report}", run, direct=True)


WORLD, RANK, BATCH = 3, 1, 40


def fold_entries(case):
    """(entry, overwritten destination keys): accumulation through every accumulating form, overwrite through every writing one, a mix of
    overwrite-mask bits through the segmented kernel (which folds one slab per launch: no destination with several feeds)."""
    keys = list(case.dst)
    entries = [("multi", set()), ("multi_ow", set()), ("multi_ow", set(keys)), ("record_pairs", set(keys))]
    if len(case.segs) == len(case.dst):
        entries.append(("seg", {k for i, k in enumerate(keys) if (0b10110101 >> (i % 8)) & 1}))
    if all(st == 0 and ln == case.slabs[s].shape[1] for s, st, ln, _ in case.segs) and len(case.segs) == len(case.dst):
        entries.append(("single", set()))
    return entries


def run_fold_case(case):
    """Slabs wrapped, every destination a buffer of its own at the case's offset from a 16-byte boundary: in/out from a non-zero prior
    where the form accumulates, started from the poison where it overwrites."""
    from geometry_rl_amd import hip
    g = torch.Generator().manual_seed(77)
    slabs = [s.to(DEV) for s in case.slabs]
    init = {k: case.init(k, g).to(DEV) for k in case.dst}
    slots = torch.randn(hip.query("grl_trpl_slot_doubles", BATCH), generator=g, dtype=F64).abs().to(DEV)

    def run(w, entry, ow):
        sl = [w(s) for s in slabs]
        dst = {k: (w.fresh((ln,), F32, DEV, mis) if k in ow else w.inout(init[k], mis)) for k, (ln, mis) in case.dst.items()}
        segs = case.segs
        head = (len(segs), [sl[s] for s, _, _, _ in segs], [sl[s].shape[0] for s, _, _, _ in segs], [sl[s].shape[1] for s, _, _, _ in segs],
                [st for _, st, _, _ in segs], [ln for _, _, ln, _ in segs], [dst[k] for _, _, _, k in segs])
        res = {"dst": dst}
        if entry == "multi":
            hip.call("grl_reduce_partials_multi", *head)
        elif entry == "multi_ow":
            hip.call("grl_reduce_partials_multi_ow", *head, 1 if ow else 0)
        elif entry == "record_pairs":
            res["region"] = out(w, (WORLD, 14, 2))
            hip.call("grl_fold_record_pairs", *head, 1, w(slots), BATCH, RANK, WORLD, res["region"])
        elif entry == "seg":
            for s in range(len(sl)):
                mine = [x for x in segs if x[0] == s]
                for i in range(0, len(mine), 8):
                    part = mine[i:i + 8]
                    hip.call("grl_reduce_partials_seg", sl[s], sl[s].shape[0], sl[s].shape[1], len(part), [dst[x[3]] for x in part],
                             [x[1] for x in part], [x[2] for x in part], sum(1 << j for j, x in enumerate(part) if x[3] in ow))
        else:
            for s, _, ln, k in segs:
                hip.call("grl_reduce_partials", sl[s], dst[k], sl[s].shape[0], ln)
        return res

    for entry, ow in fold_entries(case):
        fp.three_runs("fold " + entry, f"{case.name} {case.kind} overwrite={len(ow)}/{len(case.dst)}", lambda w: run(w, entry, ow), direct=True)


@pytest.mark.parametrize("rows", fr.ROWS)
def test_fold_sweep_and_single(rows):
    """fold_ref.sweep (every length at aligned, odd and even-but-unaligned starts of two slabs, one destination 4 bytes past a 16-byte
    boundary) and fold_ref.single (grl_reduce_partials' shape) at every row count of fold_ref.ROWS."""
    run_fold_case(fr.sweep(rows, "gauss"))
    run_fold_case(fr.single(rows, "gauss"))


def test_fold_shared_destinations():
    """Several slabs per destination, zero-row slabs among them."""
    run_fold_case(fr.shared("gauss"))


# ================================================================================================ the rollout side
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_gae(N):
    """agent.gae on test_gpu_train_ops' cases (episode ends on and around the 64-step tiles); done / terminated as bytes already, so that
    the wrapper's conversion hands the wrapped arrays on."""
    from test_gpu_train_ops import _gae_case
    from geometry_rl_amd import agent, graph, ops
    for T in (1, 2, 63, 64, 65, 129):
        r, done, term, V = (t.to(DEV) for t in _gae_case(N, T, N * 1000 + T))
        done, term = done.to(torch.uint8), term.to(torch.uint8)

        def run(w):
            wd, wt = w(done), w(term)
            adv, tgt = agent.gae(w(r), wd, wt, w(V), 0.99, 0.95)
            return {"advantage": adv, "value_target": tgt}

        fp.three_runs("agent.gae", f"N={N} T={T}", run, modules=(ops, graph, agent))


@pytest.mark.parametrize("K", [1, 3, 5, 7, 63, 64])
def test_vecnorm(K):
    """ObservationNormalizer._run: three updating calls (both outputs, y_norm alone, y_clip alone) and a frozen one; the running state is
    an in/out buffer, the byte scratch (sized by grl_vecnorm_scratch_bytes) and the outputs come from the ledger through the interposed
    module.  The frozen call leaves the state's bits alone."""
    from geometry_rl_amd import graph, ops, transforms
    per = 256 // K
    for rows in (1, 256 * per - 1, 256 * per + 1, 10 * 256 * per + 7):
        g = torch.Generator().manual_seed(rows * K)
        xs = [(torch.randn(rows, K, generator=g) * 3 + torch.arange(K) % 5 - 2).to(DEV) for _ in range(4)]
        state0 = torch.zeros(2 * K + 1, device=DEV)

        def run(w):
            norm = transforms.ObservationNormalizer(eps=1e-2, low=-2.5, high=2.5, device=DEV)
            norm.state["x"] = w.inout(state0)
            res = []
            for x, (update, want) in zip(xs, ((True, "both"), (True, "norm"), (True, "clip"), (False, "both"))):
                before = norm.state["x"].clone()
                res.append(norm._run("x", w(x), K, update, want in ("both", "norm"), want in ("both", "clip")))
                if not update:
                    assert torch.equal(fp.bits_view(norm.state["x"]), fp.bits_view(before)), "a frozen call changed the state"
            return {"y": res, "state": norm.state["x"]}

        fp.three_runs("grl_vecnorm", f"K={K} rows={rows}", run, modules=(ops, graph, transforms))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 31, 127, 128])
def test_knn(P):
    from geometry_rl_amd import hip
    for k in (1, 3, 8):
        g = torch.Generator().manual_seed(P * 10 + k)
        nv = torch.tensor([0, 1, k, k + 1, P, P + 3, max(P - 1, 0)], dtype=I32)
        B = nv.numel()
        pos = (torch.randint(-2, 3, (B, P, 3), generator=g).float() * 0.5).to(DEV)
        for n_valid in (nv.to(DEV), None):

            def run(w):
                nbr = out(w, (B, P, k), I32)
                hip.call("grl_knn_topology", w(pos), w(n_valid) if n_valid is not None else None, nbr, B, P, k)
                return {"nbr": nbr}

            plain = fp.three_runs("grl_knn_topology", f"P={P} k={k} n_valid={'table' if n_valid is not None else 'null'}", run)
            assert torch.equal(plain["nbr"].cpu(), tr.knn(pos.cpu(), n_valid.cpu() if n_valid is not None else None, k))


@pytest.mark.parametrize("N,T", [(2, 1), (5, 3), (64, 64), (65, 130), (300, 7), (1, 4)])
def test_explained_variance(N, T):
    """rollout.explained_variance on test_gpu_stats_ops' cases (a constant target column, value == target, one environment): the scratch,
    sized by grl_explained_variance_scratch_bytes, and the result come from the ledger through the interposed module."""
    from test_gpu_stats_ops import _ev_case
    from geometry_rl_amd import graph, ops, rollout
    value, target = (t.to(DEV) for t in _ev_case(N, T))

    def run(w):
        return {"ev": rollout.explained_variance(w(value), w(target))}

    fp.three_runs("rollout.explained_variance", f"N={N} T={T}", run, modules=(ops, graph, rollout))


@pytest.mark.parametrize("pattern", ["none", "all", "random", "last"])
@pytest.mark.parametrize("N,T", [(1, 1), (3, 5), (64, 64), (70, 130), (130, 65)])
def test_episode_scan(N, T, pattern):
    """EpisodeStats.scan, twice (the state carried): the running return and length are in/out buffers, the outputs and the sums come
    from the ledger through the interposed module."""
    from test_gpu_stats_ops import _episode_case
    from geometry_rl_amd import graph, ops, rollout
    reward, done = _episode_case(N, T, pattern)
    reward, done = reward.to(DEV), done.to(torch.uint8).to(DEV)   # (bytes already: scan's conversion hands the wrapped array on)
    g = torch.Generator().manual_seed(7)
    ret0 = (torch.randint(-512, 513, (N,), generator=g).float() / 256).to(DEV)
    len0 = torch.randint(0, 50, (N,), generator=g).int().to(DEV)

    def run(w):
        es = rollout.EpisodeStats(N, DEV)
        es.ret_state, es.len_state = w.inout(ret0), w.inout(len0)
        first = es.scan(w(reward), w(done))
        sums1 = es.sums.clone()
        second = es.scan(w(reward), w(done))
        return {"first": list(first), "sums1": sums1, "second": list(second), "sums": es.sums, "ret": es.ret_state, "len": es.len_state}

    fp.three_runs("EpisodeStats.scan", f"N={N} T={T} {pattern}", run, modules=(ops, graph, rollout))


@pytest.mark.parametrize("n", [1, 14])
def test_stats_accumulate(n):
    from geometry_rl_amd import hip
    g = torch.Generator().manual_seed(n)
    src = (torch.randint(-8 * 1024, 8 * 1024 + 1, (3, n), generator=g).float() / 1024).to(DEV)
    acc0 = torch.arange(n + 1, dtype=F64, device=DEV)

    def run(w):
        acc = w.inout(acc0)
        for i in range(3):
            hip.call("grl_stats_accumulate", w(src[i]), n, acc)
        return {"acc": acc}

    plain = fp.three_runs("grl_stats_accumulate", f"n={n}", run, direct=True)
    assert float(plain["acc"][n]) == n + 3


ROLLOUTS = {}


def rollout_of(N, T):
    from updater_cases import make_rollout
    if (N, T) not in ROLLOUTS:
        ROLLOUTS[N, T] = make_rollout(N, T, seed=33)
    return ROLLOUTS[N, T]


@pytest.mark.parametrize("N,T,budget", [(8, 4, None), (96, 7, None), (96, 7, 3 * 96 * 33 * 256)])
def test_time_batched_critic_pass(N, T, budget):
    """GNNVFNet._values_time_batched: the features of all frames, the grouped DeepSets stages and their statistic slots, also with the
    byte budget that cuts the time axis into chunks of three steps.  Each run starts from an empty topology cache."""
    from geometry_rl_amd import graph, ops, policy
    r = rollout_of(N, T)
    vf = r.loss.critic_network._network1
    obs = [r.data[k] for k in r.spec.in_features]

    def run(w):
        vf.hyper_data.reset_cache()
        vf.__dict__.pop("_rollout_topo_key", None)
        with torch.no_grad():
            return {"values": vf._values_time_batched([w(a) if a.is_floating_point() else a for a in obs])}

    keep = vf.GROUPED_BYTES
    try:
        if budget is not None:
            vf.GROUPED_BYTES = budget
        plain = fp.three_runs("GNNVFNet._values_time_batched", f"N={N} T={T} budget={budget}", run, modules=(ops, graph, policy))
    finally:
        vf.GROUPED_BYTES = keep
        vf.hyper_data.reset_cache()
        vf.__dict__.pop("_rollout_topo_key", None)
    assert plain["values"].shape == (N, T)


# ================================================================================================ whole paths
UPDATES = {"ppo": (dict(algorithm="ppo"), {}, ("grl_ppo_fwd_bwd",)),
           "kl_ppo": (dict(algorithm="kl_ppo", dtarg=0.01), {}, ("grl_klpen_fwd_bwd", "grl_klpen_adapt")),
           "trpl_entropy": (dict(entropy_schedule="linear", total_train_steps=100, target_entropy=-1.0), {}, ("grl_trpl_fwd_bwd_ent",)),
           "track_stats": ({}, dict(track_stats=True), ("grl_stats_accumulate",)),
           "anneal_lr": ({}, dict(anneal_lr=True, total_network_updates=100), ("grl_write_floats",))}


@pytest.mark.parametrize("name", list(UPDATES))
def test_one_eager_update(name, monkeypatch):
    """One eager ``PolicyUpdater.step`` at B = 12 on rigid_tiny from a fresh seeded agent, with the proxy in every module of the update
    path: the flat parameter / gradient / moment buffers, the step counters and the learning-rate and schedule tables are born guarded
    (``torch.zeros`` / ``torch.full`` in updater.py).  Results: flat gradient, parameters, both Adam moments, the report, the loss
    module's device scalars (beta / clip epsilon)."""
    from geometry_rl_amd import agent, hip, synthetic as syn
    from oracle_cases import make_case
    B = 12
    cfg_kw, upd_kw, wanted = UPDATES[name]
    _, spec, kw, obs = make_case("rigid_tiny", B)
    cfg = agent.AgentConfig(**dict(kw, **cfg_kw))
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=B))
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    launched = []
    recording = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), recording(entry, *a, **k))[1])

    def run(w):
        torch.manual_seed(3)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
        upd = agent.PolicyUpdater(loss, **upd_kw)
        res = upd.step({k: (w(v) if v.is_floating_point() else v) for k, v in dbatch.items()})
        upd.join_lanes()
        torch.cuda.synchronize()
        assert not upd.mode.startswith("graph")
        stats = [upd.stats_actor, upd.stats_critic] if upd.track_stats else None
        return {"gradient": upd.gflat, "parameters": upd.flat, "exp_avg": upd.exp_avg, "exp_avg_sq": upd.exp_avg_sq,
                "report": {k: v for k, v in res.items() if torch.is_tensor(v)}, "scalars": dict(loss.device_scalars), "stats": stats,
                "lr": upd.lr_dev, "steps": [upd.step_dev, upd.step_dev_c]}

    plain = fp.three_runs("eager update", name, run, modules=whole_path_modules())
    assert bool(plain["gradient"].abs().max() > 0) and bool(plain["exp_avg_sq"].abs().max() > 0)
    names = sorted(set(launched))
    print(f"eager update {name}: entry points launched: {names}")
    for want in wanted:
        assert want in names, (want, names)


def test_one_eager_collector_to_advantages_pass():
    """Normaliser, ``PolicyActor`` without graph, the critic pass, GAE, the episode scan and the explained variance on the smallest rollout
    updater_cases.make_rollout builds (N = 8, T = 4), the proxy in every module on the way."""
    from geometry_rl_amd import rollout as ro, transforms
    N, T = 8, 4
    r = rollout_of(N, T)
    raw_keys = [k for k in r.spec.in_features if not k.startswith("norm_")]
    frames = [{k: r.data[k][:, t].contiguous() for k in raw_keys} for t in range(T)] + [{k: r.next_last[k][:, 0].contiguous() for k in raw_keys}]
    g = torch.Generator().manual_seed(4)
    rewards = [torch.randn(N, generator=g).to(DEV) for _ in range(T)]
    dones = [(torch.rand(N, generator=g) < 0.3).to(DEV) for _ in range(T)]
    vf = r.loss.critic_network._network1
    hds = (vf.hyper_data, r.actor.hyper_data)

    def run(w):
        for hd in hds:
            hd.reset_cache()
        vf.__dict__.pop("_rollout_topo_key", None)
        state = {"t": 0}

        def env_step(action):
            state["t"] += 1
            t = state["t"]
            return ({k: w(v) for k, v in frames[t].items()}, w(rewards[t - 1]), dones[t - 1], torch.zeros(N, dtype=torch.bool, device=DEV))

        norm = transforms.ObservationNormalizer(device=DEV)
        es = ro.EpisodeStats(N, DEV)
        actor = ro.PolicyActor(r.actor, r.spec, use_graph=False, seed=1)
        buf, next_last = ro.collect(env_step, {k: w(v) for k, v in frames[0].items()}, actor, T, normalizer=norm, episode_stats=es)
        ro.RolloutDriver(types.SimpleNamespace(loss_module=r.loss), r.spec).compute_advantages(buf, next_last)   # (takes the critic alone)
        ev = ro.explained_variance(buf.data["state_value"], buf.data["value_target"])
        keys = ("loc", "var", "action", "sample_log_prob", "state_value", "advantage", "value_target", "episode_reward", "step_count")
        return {"buffer": {k: buf.data[k] for k in keys}, "observations": {k: buf.data[k] for k in r.spec.in_features},
                "normaliser": dict(norm.state), "episodes": [es.ret_state, es.len_state, es.sums], "explained_variance": ev}

    try:
        fp.three_runs("collector to advantages", f"N={N} T={T}", run, modules=whole_path_modules())
    finally:
        for hd in hds:
            hd.reset_cache()
        vf.__dict__.pop("_rollout_topo_key", None)
    for want in ("grl_vecnorm", "grl_gaussian_sample", "grl_gae_scan", "grl_episode_scan", "grl_explained_variance"):
        assert want in LAUNCHED, want


def test_every_named_entry_point_was_launched():
    """Printed: the set of entry points this file's tests launched and the interposed / wrapped totals per group.  Asserted (when the
    whole file ran in this process): every entry point the file is for is among them."""
    print(f"entry points launched by this file ({len(LAUNCHED)}): {sorted(LAUNCHED)}")
    for op, (runs, interposed, wrapped) in sorted(fp.COUNTS.items()):
        print(f"footprint totals {op}: {runs} guarded runs, {interposed} interposed, {wrapped} wrapped")
    mine = {k for k, v in globals().items() if k.startswith("test_") and callable(v)} - {"test_every_named_entry_point_was_launched"}
    if mine <= RAN:
        missing = [n for n in NAMED if n not in LAUNCHED]
        assert not missing, missing
    else:
        print(f"(a partial run: {sorted(mine - RAN)} did not run in this process)")
