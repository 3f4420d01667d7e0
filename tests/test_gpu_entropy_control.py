"""The scheduled entropy projection inside the fused TRPL launch (grl_trpl_fwd_bwd_ent: trpl_lanes_body's ENT instances) and the update
path around it, on the GPU:
  * the kernel per op against tests/entropy_ref.py (float64, same fp32 inputs): sums, maxes, dmean, dsigma, proj_mean, proj_var over
    A_SWEEP x four projections x four modes and the batch / fold edges of B_SWEEP, with the allowances of tests/test_gpu_trpl_kernel.py
    (tests/trpl_cases.py's comparisons, as they are);
  * an inactive stage is free of effect: beta = -inf (inequality) is BITWISE grl_trpl_fwd_bwd;
  * properties that need no reference (projected entropy == / >= beta; the KL bound's residual with the stage in front);
  * TRPLLoss.forward (opt-in) against the oracle actor + entropy_ref; compute_metrics' entropy_constraint;
  * PolicyUpdater: every program bitwise the eager step-by-step loop while the bound moves, nothing recorded again;
  * data parallel: the latched initial entropy is the global mean, the update the one-rank update."""
import contextlib
import math

import numpy as np
import pytest
import torch

import entropy_cases as ec
import entropy_ref
import trpl_cases as tc
from geometry_rl_amd import ops
from oracle import trpl as otr
from updater_cases import DEV, assert_ranks_match, dp_ref, make_rollout, run_single, spawn_dp

pytestmark = pytest.mark.gpu


def _beta_dev(beta):
    return torch.tensor([beta], dtype=torch.float64, device=DEV)


def _launch(e, d, beta=None, ent=True):
    c = e.base
    db = {k: v.to(DEV) for k, v in d["batch"].items()}
    kw = dict(ent_mode=e.mode, ent_beta=_beta_dev(d["beta"] if beta is None else beta)) if ent else {}
    return ops.trpl_fwd_bwd(d["loc"].to(DEV), d["sigma"].to(DEV), db, d["value"].to(DEV) if c.value else None, mean_bound=tc.EPS,
                            cov_bound=tc.EPS_COV, trust_region_coeff=c.tr_coeff, entropy_coef=c.ent_coef, critic_coef=c.critic_coef,
                            clip_value=c.clip_value, global_batch=c.global_batch, adv_stats=None, want_projection=True, proj_type=c.proj,
                            adv_local=True, **kw)


def _check_case(e):
    d = ec.make_case(e)
    ref = ec.reference(e, d)
    kap = tc.adv_error_bound(e.base, d)
    print(f"{e.name}: beta {d['beta']:.6f}, adv bound {kap:.2e}")
    tc.launch_close(_launch(e, d), ref, e.base.B, kap)


@pytest.mark.parametrize("e", ec.lane_cases(), ids=lambda e: e.name)
def test_lane_widths_projections_and_modes(e):
    _check_case(e)


@pytest.mark.parametrize("e", ec.batch_cases(), ids=lambda e: e.name)
def test_batch_and_fold_edges(e):
    _check_case(e)


@pytest.mark.parametrize("first", (False, True))
@pytest.mark.parametrize("proj", tc.PROJS)
@pytest.mark.parametrize("A", (3, 7, 12))
def test_inactive_stage_is_bitwise_the_plain_launch(A, proj, first):
    e = ec.ECase(tc.Case(B=4097 if A == 7 else 37, A=A, proj=proj), False, first)
    d = ec.make_case(e)
    got = _launch(e, d, beta=-math.inf)
    want = _launch(e, d, ent=False)
    for name, a, b in zip(("sums", "maxes", "dloc", "dsigma", "dvalue", "proj_mean", "proj_var"), got, want):
        assert torch.equal(a, b), name + " differs at " + str((a != b).reshape(-1).nonzero().reshape(-1)[:12].tolist())


@pytest.mark.parametrize("proj", tc.PROJS)
@pytest.mark.parametrize("A", (2, 6, 16))
def test_projected_entropy_meets_the_bound(A, proj):
    """Entropy stage behind the trust region: equality form -> every frame's entropy IS beta, inequality form -> >= beta, up to the rounding
    of the fp32 proj_var: k logs whose arguments are each off by one fp32 rounding (relative 2^-24) -> k 2^-24, doubled for the fp64
    evaluation on either side."""
    allowed = 2 * A * tc.U32
    for eq in (True, False):
        e = ec.ECase(tc.Case(B=53, A=A, proj=proj), eq, False)
        d = ec.make_case(e)
        pv = _launch(e, d)[6].cpu().double()
        ent = otr.entropy_std(pv)
        gap = ent - d["beta"]
        print(f"proj {proj} A {A} eq {eq}: entropy - beta in [{float(gap.min()):.3e}, {float(gap.max()):.3e}], allowed {allowed:.3e}")
        if eq:
            assert float(gap.abs().max()) <= allowed
        else:
            assert float(gap.min()) >= -allowed and float(gap.max()) > 0.1


@pytest.mark.parametrize("eq", (False, True))
def test_kl_bound_holds_behind_an_entropy_stage_in_front(eq):
    """Entropy first + KL: the trust-region projection runs on the scaled S; frames on the covariance bound end ON it (the residual of
    tests/test_gpu_trpl_selfcheck.py)."""
    e = ec.ECase(tc.Case(B=64, A=6, proj=0), eq, True)
    d = ec.make_case(e)
    pv = _launch(e, d)[6].cpu().double()
    S, So = d["sigma"].double() ** 2, d["batch"]["var"].double()
    S_in = entropy_ref.entropy_stage(S, d["beta"], eq)[0]
    kl = lambda s_, o_: 0.5 * ((s_ / o_) ** 2 - 1.0 - 2.0 * (s_ / o_).log()).sum(-1)
    active = kl(S_in, So) > tc.EPS_COV
    res = float((kl(pv, So)[active] - tc.EPS_COV).abs().max())
    print(f"KL bound residual with the entropy stage in front (eq={eq}): {res:.2e} on {int(active.sum())} frames")
    assert int(active.sum()) > 10 and res <= 1e-6


# ---------------------------------------------------------------------------------------------------- the loss module and the updater
def _initial_of(batch):
    """mean of policy.entropy(q) in the layer's float32 arithmetic (base_projection_layer.py:202-203)."""
    var = batch["var"].float()
    return (0.5 * (var.shape[-1] * np.log(2 * np.e * np.pi) + 2 * var.log().sum(-1))).mean()


@pytest.mark.parametrize("proj_type,eq,first", [("kl", False, False), ("kl", True, True), ("w2", False, True), ("frob", True, False),
                                                ("w2_non_com", False, False)])
def test_loss_forward_matches_the_oracle_with_entropy_ref(proj_type, eq, first):
    """The small rigid HEPi case of tests/test_gpu_step.py: all 13 loss-dict entries and the actor's parameter gradients, at that file's
    tolerances, for update number 3 of a linear schedule."""
    import oracle_cases as oc
    from geometry_rl_amd import agent, synthetic as syn
    B, step, total = 24, 3, 10
    o_spec, spec, kw, obs = oc.make_case("rigid_g1", B)
    kw = dict(kw, proj_type=proj_type, trust_region_coeff=2.0)
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, 6, seed=B))
    initial = float(_initial_of(batch))
    ekw = dict(entropy_schedule="linear", target_entropy=initial + 4.0, entropy_eq=eq, entropy_first=first, total_train_steps=total)
    pair = oc.build_pair((o_spec, spec, kw), seed=11, d_kw=ekw, dev=DEV)
    oracle, actor, proj, loss = pair.oracle, pair.actor, pair.proj, pair.loss
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    oc.adopt_calibration(pair, batch, device_first=True)
    upd = agent.PolicyUpdater(loss, lr=3e-4)
    upd.gflat.zero_()
    loss._global_steps = step
    out = loss(dbatch)
    assert abs(float(proj.initial_entropy) - initial) <= 1e-6 * abs(initial)     # (latched on the device: another summation order)
    beta = float(proj.get_entropy_bound(step))
    assert float(loss.entropy_beta(DEV)[0]) == beta
    (out["loss_objective"] + out["loss_entropy"] + out["loss_trust_region"]).backward()
    with tc.w2nc_registered(), entropy_ref.registered(beta, eq, first):
        ref, ref_grads = oracle.update(batch)
    for k in oc.LOSS_KEYS:
        oc.check(k, out[k], ref[k])
    bad, _ = oc.gradients_off_scale(actor, pair.critic, ref_grads, nets=("actor",))
    assert not bad, bad
    # compute_metrics of the scheduled layer: entropy_constraint = mean(entropy - bound(step)) (base_projection_layer.py:380-382)
    p = (out["loc"].detach(), (out["sigma"].detach() ** 2).diag_embed())
    q = (dbatch["loc"], dbatch["var"].diag_embed())
    mt = proj.compute_metrics(actor, p, q, step=step)
    want = float((actor.entropy(p) - proj.get_entropy_bound(step)).mean())
    assert abs(float(mt["entropy_constraint"]) - want) <= 1e-5 * max(1.0, abs(want))
    with pytest.raises(AssertionError):
        proj.compute_metrics(actor, p, q)
    assert "entropy_constraint" not in out.keys()


def _run_form(form, schedule, n_updates, total):
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import RolloutBuffer, RolloutDriver
    # updater inputs in the manner of tests/test_gpu_rollout.py, with a schedule steep enough to move the active set
    r = make_rollout(8, 12, seed=33, entropy_schedule=schedule, total_train_steps=total, entropy_first=True, temperature=0.5)
    spec, proj, loss = r.spec, r.proj, r.loss
    kw = dict(eager=dict(use_graph=False), lanes=dict(use_graph=True), one_stream=dict(use_graph=True, overlap_critic=False),
              step_from=dict(use_graph=True), unrolled=dict(use_graph=True), per_step=dict(use_graph=True))[form]
    upd = agent.PolicyUpdater(loss, lr=r.cfg.lr, **kw)
    upd.autotune_form = False
    if form == "unrolled":
        upd.epoch_unroll = 4
    if form == "per_step":
        upd.epoch_unroll, upd.form_by_size = 4, {8: "per_step"}
    buf = RolloutBuffer(dict(r.data))
    drv = RolloutDriver(upd, spec, ppo_epochs=1, seed=9)
    drv.compute_advantages(buf, r.next_last)
    idxs = drv.epoch_minibatches(buf.N, buf.T, DEV)[:n_updates]
    assert len(idxs) == n_updates
    keys = list(spec.in_features) + ["action", "loc", "var", "sample_log_prob", "state_value", "advantage", "value_target"]
    # the target relative to the first minibatch: the linear bound starts at the old distribution's mean entropy (the latch) and passes the
    # policy's own entropy level half-way through the schedule, so frames enter the scaled set along the updates
    b0 = buf.rows(idxs[0], keys)
    with torch.no_grad():
        _, sg = loss.actor_network.forward_diag(*[b0[k] for k in spec.in_features], train=True)
    level, init = float(otr.entropy_std(sg.double().cpu() ** 2).mean()), float(_initial_of(b0))
    proj.target_entropy = init + 2.0 * (level - init)
    REPORTED = ("kl", "entropy", "loss_trust_region", "loss_objective", "loss_critic")
    outs, sigmas, programs = [], [], []
    if form in ("unrolled", "per_step"):
        upd.run_minibatches(buf, torch.stack(idxs[:1]))     # the eager first step of the size
        for lo in range(1, n_updates, 4):
            hi = min(lo + 4, n_updates)
            upd.run_minibatches(buf, torch.stack(idxs[lo:hi]))
            programs.append((upd._program, upd._epoch))
            if form == "unrolled" and hi - lo == 4:
                outs = [(lo + i, {k: o[k].detach().clone() for k in REPORTED}) for i, o in enumerate(upd.last_outs)]
        torch.cuda.synchronize()
        return upd, proj, (outs, None), programs
    for j, idx in enumerate(idxs):
        out = upd.step_from(buf, idx) if form == "step_from" else upd.step(buf.rows(idx, keys))
        outs.append((j, {k: out[k].detach().clone() for k in REPORTED}))
        sigmas.append(out["sigma"].detach().clone())
        programs.append((upd._program, None))
    torch.cuda.synchronize()
    return upd, proj, (outs, sigmas), programs


@pytest.mark.parametrize("schedule,n_updates", [("linear", 12), ("exp", 3)])
def test_updater_programs_are_bitwise_the_eager_loop_while_the_bound_moves(schedule, n_updates):
    total = 12
    ref_upd, proj, (ref_outs, sigmas), _ = _run_form("eager", schedule, n_updates, total)
    assert ref_upd.steps == n_updates
    # the bound the kernel read at update s is float(layer.get_entropy_bound(s)); the active set (entropy first: frames whose own entropy
    # is below the bound) changes along the way
    counts = []
    for s in range(n_updates):
        bound = float(proj.get_entropy_bound(s))
        assert proj.entropy_bounds([s])[0] == bound
        ent = otr.entropy_std(sigmas[s].double().cpu() ** 2)
        counts.append(int((ent < bound).sum()))
    print(f"{schedule}: frames scaled per update {counts}; last bound written {float(ref_upd.beta_table[0]):.6f}")
    assert float(ref_upd.beta_table[0]) == float(proj.get_entropy_bound(n_updates - 1))
    if schedule == "linear":
        assert min(counts) < max(counts), counts     # the active set changes along the way
    for form in ("lanes", "one_stream", "step_from", "unrolled", "per_step"):
        upd, proj_f, (outs, _sg), programs = _run_form(form, schedule, n_updates, total)
        assert upd.steps == n_updates and float(proj_f.initial_entropy) == float(proj.initial_entropy)
        for name, a, b in (("flat", upd.flat, ref_upd.flat), ("exp_avg", upd.exp_avg, ref_upd.exp_avg), ("exp_avg_sq", upd.exp_avg_sq, ref_upd.exp_avg_sq)):
            assert torch.equal(a, b), (form, name, float((a - b).abs().max()))
        assert outs or form == "per_step" or n_updates < 5
        for s, got in outs:
            for k, v in ref_outs[s][1].items():
                assert torch.equal(got[k], v), (form, s, k)
        # the number of recorded programs does not grow after the first recording of each kind: the bound is data, not a constant of it
        if form in ("lanes", "one_stream", "step_from"):
            assert programs[1][0] is not None and all(p[0] is programs[1][0] for p in programs[1:]), form
        elif form == "unrolled" and n_updates >= 9:
            assert programs[0][1] is not None and programs[1][1] is programs[0][1], form


# ---------------------------------------------------------------------------------------------------- data parallel
def _spread_entropies(batch):
    batch["var"] = batch["var"] * torch.linspace(0.5, 2.0, batch["var"].shape[0])[:, None]     # the shards' mean entropies differ
    return dict(target_entropy=float(_initial_of(batch)) + 3.0)


@contextlib.contextmanager
def _outline_is_stable(case, upd, shard, rank, ret):
    outline = upd.program_outline()
    yield
    assert upd.program_outline() == outline
    ret[f"initial_entropy{rank}"] = float(case.proj.initial_entropy)


def test_two_ranks_latch_the_global_mean_and_match_one_rank():
    world = 2
    case_ref = dp_ref(16, cfg_kw=dict(entropy_schedule="linear", total_train_steps=10, entropy_first=False),
                      batch_hook=(__name__, "_spread_entropies"))
    kw = dict(use_graph=False, n_steps=2, keys=("loss_objective", "loss_trust_region", "loss_entropy", "kl", "entropy_diff"), updater_kw={})
    ref, ref_flat, case = run_single(case_ref, **kw)
    want_init = float(_initial_of(case.batch))
    assert abs(float(case.proj.initial_entropy) - want_init) <= 1e-6 * abs(want_init)
    ret = spawn_dp(case_ref, world, extra=(__name__, "_outline_is_stable"), **kw)
    for r in range(world):
        init = ret[f"initial_entropy{r}"]
        print(f"rank {r}: initial entropy {init:.6f}")
        assert abs(init - want_init) <= 1e-6 * abs(want_init), (r, init, want_init)    # the GLOBAL mean, not the shard's
    assert_ranks_match(ref, ref_flat, ret, world, 1e-5, 2e-6)
