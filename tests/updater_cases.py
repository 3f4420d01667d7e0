"""Shared scaffolding of the GPU tests that drive ``PolicyUpdater``: the rollout-shaped inputs, the bodies that run one case through several
program forms, and the data-parallel pair (one rank on the whole batch, ``world`` ranks on its shards).  TEST INFRASTRUCTURE ONLY, a plain
module like tests/trpl_cases.py.  The runners return what each form left behind and compare NOTHING: every comparison, with its operator
and tolerance, stays in the test that owns it, or in an ``assert_...`` body that several files share whole.

Pieces that a spawned rank needs from a test file are named ``(module, function, ...)`` and looked up in the child: closures do not
survive ``mp.spawn``, the test directory is importable there."""
import contextlib
import importlib
import math
import os
from collections import namedtuple
from functools import partial

import torch

from spawn_util import spawn_ranks

DEV = torch.device("cuda:0")
RIGID2 = dict(G=2, angular_velocity=False, object_velocity=False)    # the data-parallel tests' spec: two grippers, positions only

Rollout = namedtuple("Rollout", "spec cfg actor critic proj loss data next_last")
DPCase = namedtuple("DPCase", "spec cfg actor critic proj loss batch")


def _named(ref):
    return getattr(importlib.import_module(ref[0]), ref[1])


def calibrate(actor, spec, batch):
    """The first training forward: the data-dependent re-initialisation of the convolutions."""
    with torch.no_grad():
        actor.forward_diag(*[batch[k] for k in spec.in_features], train=True)


# ------------------------------------------------------------------------------------------------------------- rollout-shaped inputs
def make_rollout(N, T, seed, *, spec=None, after_build=None, **cfg_kw):
    """The small rigid HEPi agent (or ``spec``, a rigid one) with T + 1 synthetic frame sets of N environments: [N, T] data with GAE inputs,
    the frame behind the last as ``next_last``, calibrated on time step 0.  ``after_build(actor, critic, proj, loss)`` runs before the
    calibrating forward."""
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec() if spec is None else spec
    cfg = agent.AgentConfig(**dict(dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2), **cfg_kw))
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    if after_build is not None:
        after_build(actor, critic, proj, loss)
    frames = []
    for t in range(T + 1):  # one synthetic frame set per time step (same env -> same point count: env_offset 0)
        b = dict(syn.make_rigid_obs(N, seed=seed + t))
        b.update(syn.make_ppo_fields(N, 6, seed=seed + t))
        frames.append(b)
    data = {k: torch.stack([f[k] for f in frames[:T]], dim=1).to(DEV) for k in frames[0]}
    g = syn.make_gae_inputs(N, T, seed=seed)
    data.update(reward=g["reward"].reshape(N, T, 1).to(DEV), done=g["done"].reshape(N, T, 1).to(DEV),
                terminated=g["terminated"].reshape(N, T, 1).to(DEV))
    next_last = {k: frames[T][k].unsqueeze(1).to(DEV) for k in spec.in_features}
    calibrate(actor, spec, {k: data[k][:, 0].contiguous() for k in spec.in_features})
    return Rollout(spec, cfg, actor, critic, proj, loss, data, next_last)


# ------------------------------------------------------------------------------------------------------------- program forms
def snapshot(upd, outs):
    return upd.flat.detach().clone(), upd.exp_avg.detach().clone(), upd.exp_avg_sq.detach().clone(), outs


def _around(per_mode, mode, r, upd):
    """``per_mode(mode, rollout, updater)``: a context manager around a mode's updates and the synchronisation behind them."""
    return contextlib.nullcontext() if per_mode is None else per_mode(mode, r, upd)


def run_loop_and_launches(make, form, *, N, T, ppo_epochs, driver_seed, unroll, keys, per_mode=None):
    """``ppo_epochs`` epochs of T minibatches, "loop": step_from one by one, "launches": run_minibatches with ``unroll`` steps per launch
    (``form`` "per_step": the size pinned to the per-step program).  -> {mode: snapshot}, outs = every step's loss dict ("loop") or the
    last one ("launches"), restricted to ``keys``."""
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import RolloutBuffer, RolloutDriver
    res = {}
    for mode in ("loop", "launches"):
        r = make()
        upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=True)
        upd.epoch_unroll = unroll if mode == "launches" else 1
        if form == "per_step":
            upd.form_by_size[N] = "per_step"   # the gated per-step program (the critic's lane waits for the first edge convolution)
        buf = RolloutBuffer(dict(r.data))
        drv = RolloutDriver(upd, r.spec, ppo_epochs=ppo_epochs, seed=driver_seed)
        drv.compute_advantages(buf, r.next_last)
        outs = []
        with _around(per_mode, mode, r, upd):
            if mode == "loop":
                for idx in drv.minibatches(buf):
                    o = upd.step_from(buf, idx)
                    outs.append({k: o[k].clone() for k in keys})
            else:
                for _ in range(ppo_epochs):
                    o = upd.run_minibatches(buf, torch.stack(drv.epoch_minibatches(buf.N, buf.T, DEV)))
                assert (upd._epoch is not None) == (form != "per_step")
                outs.append({k: o[k].clone() for k in keys})
            torch.cuda.synchronize()
        assert upd.steps == ppo_epochs * T
        res[mode] = snapshot(upd, outs)
    return res


def run_step_modes(make, modes, k, keys, updater_kw_of_mode, before_step=None, per_mode=None):
    """Per mode a fresh ``make()`` and ``k`` updates of its time step 0 by ``PolicyUpdater(**updater_kw_of_mode(mode))``;
    ``before_step(mode, rollout)`` runs in front of every update.  -> {mode: snapshot}, outs = every step's loss dict restricted to ``keys``."""
    from geometry_rl_amd import agent
    res = {}
    for mode in modes:
        r = make()
        batch = {kk: v[:, 0].contiguous() for kk, v in r.data.items()}
        upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, **updater_kw_of_mode(mode))
        outs = []
        with _around(per_mode, mode, r, upd):
            for _ in range(k):
                if before_step is not None:
                    before_step(mode, r)
                outs.append({kk: v.clone() for kk, v in upd.step(batch).items() if kk in keys})
            torch.cuda.synchronize()
        res[mode] = snapshot(upd, outs)
    return res


@contextlib.contextmanager
def graph_modes_are_recorded(mode, r, upd, proj_codes=None):
    """A ``per_mode`` of run_step_modes: the recording modes did record (and the rollout's projection is one of ``proj_codes``)."""
    assert proj_codes is None or r.proj.proj_code in proj_codes
    yield
    if mode in ("graph", "one_stream"):
        assert upd.mode.startswith("graph") and upd._program is not None


def assert_two_runs_bitwise_identical(keys, **rollout_kw):
    """Two fresh ``make_rollout(16, 3, seed=45, **rollout_kw)`` through three recorded updates each: parameters and every step's ``keys``."""
    from geometry_rl_amd import agent
    res = []
    for _ in range(2):
        r = make_rollout(16, 3, seed=45, **rollout_kw)
        upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=True)
        outs = [{kk: v.clone() for kk, v in upd.step({k: v[:, t].contiguous() for k, v in r.data.items()}).items() if kk in keys}
                for t in range(3)]
        torch.cuda.synchronize()
        res.append((upd.flat.detach().clone(), outs))
    assert torch.equal(res[0][0], res[1][0])
    for oa, ob in zip(res[0][1], res[1][1]):
        for kk in keys:
            assert torch.equal(oa[kk], ob[kk]), kk


# ------------------------------------------------------------------------------------------------------------- tracked statistics
STATS_N, STATS_T = 16, 12     # 16 frames per minibatch, 12 minibatches: one epoch of the rigid synthetic rollout
STATS_FORMS = {   # form -> (PolicyUpdater keywords, the calls of the tracked run as row ranges, the calls of the step-by-step run)
    "one_stream": (dict(use_graph=True, overlap_critic=False), None, None),
    "lanes": (dict(use_graph=True), None, None),
    # unroll = 4: one eager step, two launches of four steps, three single steps
    "launches": (dict(use_graph=True), [(0, 12)], [(0, 1), (1, 5), (5, 9), (9, 10), (10, 11), (11, 12)]),
    "eager": (dict(use_graph=False), None, None),
}


def run_stats_epoch(form, track, cfg_kw, keys):
    """The 12 minibatches of one epoch through ``form`` -> (updater, rollout, buffer, every step's reported values [12] as dicts of 0-d
    tensors -- collected only with tracking off, where the sequence is cut into calls whose steps can all be read)."""
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import RolloutBuffer, RolloutDriver
    N, T = STATS_N, STATS_T
    kw, tracked_calls, stepwise_calls = STATS_FORMS[form]
    r = make_rollout(N, T, 21, **cfg_kw)
    upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, **kw, **(dict(track_stats=True) if track else {}))
    upd.autotune_form = False
    buf = RolloutBuffer(dict(r.data))
    drv = RolloutDriver(upd, r.spec, ppo_epochs=1, seed=3)
    drv.compute_advantages(buf, r.next_last)
    rows = torch.stack(drv.epoch_minibatches(N, T, DEV))
    assert rows.shape == (T, N)
    vals = []
    if tracked_calls is None:
        for j in range(T):
            out = upd.step_from(buf, rows[j])
            if not track:
                vals.append({k: out[k].clone() for k in keys})
    else:
        for lo, hi in (tracked_calls if track else stepwise_calls):
            out = upd.run_minibatches(buf, rows[lo:hi], unroll=4)
            if not track:
                outs = upd.last_outs if hi - lo == 4 else [out]
                assert len(outs) == hi - lo
                vals += [{k: o[k].clone() for k in keys} for o in outs]
        assert upd._epoch is not None, "the multi-step launch was not taken"
    torch.cuda.synchronize()
    assert upd.steps == T
    return upd, r, buf, vals


def assert_stats_means(means, vals, keys):
    """``stats_read()`` of a tracked epoch against the fp64 mean of the values its steps reported: to T * 2^-53 * max |v| of math.fsum / T."""
    T = STATS_T
    assert means["updates"] == T
    assert set(means) == set(keys) | {"updates"}, sorted(means)
    for k in keys:
        v = [float(s[k]) for s in vals]
        want = math.fsum(v) / T
        bound = T * 2.0 ** -53 * max(abs(x) for x in v)
        print(f"{k}: mean {means[k]!r}, fsum / {T} = {want!r}, |diff| {abs(means[k] - want):.3e} (bound {bound:.3e})")
        assert isinstance(means[k], float) and abs(means[k] - want) <= bound, (k, means[k], want)


# ------------------------------------------------------------------------------------------------------------- K updates against the oracle
def merge_grad_scales(g_scale, ref_grads):
    """The running largest gradient scale of every tensor over the updates so far (``g_scale`` None before the first)."""
    from parity_util import grad_scales
    sc = {net: grad_scales(ref_grads[net]) for net in ("actor", "critic")}
    return sc if g_scale is None else {net: {k: max(v, g_scale[net].get(k, 0.0)) for k, v in sc[net].items()} for net in sc}


def moments_and_params_after(upd, actor, critic, oracle, cfg, g_scale, K, m_tol, v_tol):
    """After K updates on both sides (tests/test_gpu_multistep_oracle.py's rules): exp_avg of every parameter tensor against ``m_tol``,
    exp_avg_sq against ``v_tol`` (of the tensor's own largest reference entry, floored as for gradients), the parameters against K times the
    first-step bound.  Prints every margin -> (the tensors that miss a rule, the worst fractions); the assertion stays with the caller."""
    import numpy as np
    from parity_util import adam_first_step_bound, grad_scales
    if upd.flat.is_cuda:
        torch.cuda.synchronize()
    off = lambda p: (p.data_ptr() - upd.flat.data_ptr()) // 4
    bad, worst = [], {"exp_avg": 0.0, "exp_avg_sq": 0.0, "param": 0.0}
    for net, mod, ref_p, optim, strip in (("actor", actor, oracle.actor, oracle.actor_optim, 0),
                                          ("critic", critic, oracle.critic, oracle.critic_optim, len("_network1."))):
        states = {kk: optim.state.get(ref_p[kk], {}) for kk in ref_p}
        m_ref = {kk: s_["exp_avg"] for kk, s_ in states.items() if "exp_avg" in s_}
        v_ref = {kk: s_["exp_avg_sq"] for kk, s_ in states.items() if "exp_avg_sq" in s_}
        m_sc, v_sc = grad_scales(m_ref), grad_scales(v_ref)
        for k, p in mod.named_parameters():
            kk = k[strip:]
            if kk not in m_ref:
                continue
            o, n = off(p), p.numel()
            em = float((upd.exp_avg[o:o + n].view_as(p).cpu().double() - m_ref[kk].double()).abs().max())
            ev = float((upd.exp_avg_sq[o:o + n].view_as(p).cpu().double() - v_ref[kk].double()).abs().max())
            ep = float((p.detach().cpu().double() - ref_p[kk].detach().double()).abs().max())
            allowed_p = K * adam_first_step_bound(cfg.lr, 1e-5, g_scale[net].get(kk, 0.0), cfg.clip_grad_norm, p_ref=ref_p[kk])
            print(f"{net} {kk}: exp_avg {em / m_sc[kk]:.2e} of scale, exp_avg_sq {ev / v_sc[kk]:.2e} of scale, param err {ep:.2e} (allowed {allowed_p:.2e})")
            worst["exp_avg"] = max(worst["exp_avg"], em / m_sc[kk])
            worst["exp_avg_sq"] = max(worst["exp_avg_sq"], ev / v_sc[kk])
            worst["param"] = max(worst["param"], ep / allowed_p)
            if not (em <= m_tol * m_sc[kk] and ev <= v_tol * v_sc[kk] and ep <= allowed_p and np.isfinite(em + ev + ep)):
                bad.append((net, kk, em / m_sc[kk], ev / v_sc[kk], ep, allowed_p))
    print("worst (fraction of scale / of allowed):", worst)
    return bad, worst


# ------------------------------------------------------------------------------------------------------------- data parallel
def dp_case(B, group, *, cfg_kw, batch_hook=None, calibrate_first=True):
    """The data-parallel tests' agent and minibatch: two-gripper rigid spec, ``seed=4`` fields, replicas from one seed, calibrated on the
    WHOLE batch so that every rank starts from identical weights.  ``batch_hook`` names a function that may edit the (host) batch and
    returns further AgentConfig keywords derived from it."""
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec(**RIGID2)
    batch = dict(syn.make_rigid_obs(B, seed=4, **RIGID2))
    batch.update(syn.make_ppo_fields(B, 6, seed=4))
    if batch_hook is not None:
        cfg_kw = dict(cfg_kw, **_named(batch_hook)(batch))
    cfg = agent.AgentConfig(**cfg_kw)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV, group=group)
    batch = {k: v.to(DEV) for k, v in batch.items()}
    if calibrate_first:
        calibrate(actor, spec, batch)
    return DPCase(spec, cfg, actor, critic, proj, loss, batch)


def dp_ref(B, **case_kw):
    """What ``dp_worker`` and ``run_single`` take as ``case_ref``: (module, function, keywords) of a builder called with ``group=``."""
    return (__name__, "dp_case", dict(B=B, **case_kw))


@contextlib.contextmanager
def rendezvous(rank, world, port, backend="gloo", **init_kw):
    """The one place a rank joins its process group (and leaves it, when nothing raised)."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group(backend, rank=rank, world_size=world, **init_kw)
    yield dist.group.WORLD
    dist.destroy_process_group()


def shard_of(batch, rank, world):
    B = next(iter(batch.values())).shape[0]
    lo, hi = rank * B // world, (rank + 1) * B // world
    return {k: v[lo:hi].contiguous() for k, v in batch.items()}


def dp_worker(rank, world, port, case_ref, ret, *, use_graph, n_steps, keys, updater_kw, extra=None):
    """One rank: rendezvous, the case built on the group, its shard, ``n_steps`` updates -> ret[rank] = (last loss dict restricted to
    ``keys``, parameters).  ``extra`` = (module, function, *args) names a context manager ``f(case, upd, shard, rank, ret, *args)`` around the
    updates; what it yields, if anything, is called with the step number in front of every update."""
    from geometry_rl_amd import agent
    with rendezvous(rank, world, port) as group:
        case = _named(case_ref)(group=group, **case_ref[2])
        shard = shard_of(case.batch, rank, world)
        upd = agent.PolicyUpdater(case.loss, lr=case.cfg.lr, group=group, use_graph=use_graph, **updater_kw)
        hook = contextlib.nullcontext() if extra is None else _named(extra)(case, upd, shard, rank, ret, *extra[2:])
        with hook as before_step:
            for i in range(n_steps):
                if before_step is not None:
                    before_step(i)
                out = upd.step(shard)
        ret[rank] = ({k: float(out[k].detach()) for k in keys}, upd.flat.detach().cpu())


def spawn_dp(case_ref, world, **worker_kw):
    """``world`` ranks of ``dp_worker`` -> what they left in ``ret``, as a plain dict."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    spawn_ranks(partial(dp_worker, **worker_kw), world, (world,), (case_ref, ret))
    assert all(r in ret for r in range(world))
    return dict(ret)


def run_single(case_ref, *, use_graph, n_steps, keys, updater_kw):
    """The one-rank side: the same case on the whole batch -> (last loss dict restricted to ``keys``, parameters, the case)."""
    from geometry_rl_amd import agent
    case = _named(case_ref)(group=None, **case_ref[2])
    upd = agent.PolicyUpdater(case.loss, lr=case.cfg.lr, use_graph=use_graph, **updater_kw)
    for _ in range(n_steps):
        out = upd.step(case.batch)
    return {k: float(out[k].detach()) for k in keys}, upd.flat.detach().cpu(), case


def run_two_ranks(case_ref, world=2, *, use_graph, dp_use_graph, n_steps, keys, updater_kw, extra=None):
    """-> (one rank's losses, one rank's parameters, the ranks' ``ret``); ``use_graph`` is the one-rank updater's, ``dp_use_graph`` the ranks'."""
    ref_losses, ref_flat, _ = run_single(case_ref, use_graph=use_graph, n_steps=n_steps, keys=keys, updater_kw=updater_kw)
    ret = spawn_dp(case_ref, world, use_graph=dp_use_graph, n_steps=n_steps, keys=keys, updater_kw=updater_kw, extra=extra)
    return ref_losses, ref_flat, ret


def assert_ranks_match(ref_losses, ref_flat, ret, world, loss_rtol, flat_atol):
    """Every rank's (losses, parameters) against the one-rank side: losses to ``loss_rtol * max(1, |v|)``, parameters to ``flat_atol``."""
    for r in range(world):
        losses, flat = ret[r]
        for k, v in ref_losses.items():
            assert abs(losses[k] - v) <= loss_rtol * max(1.0, abs(v)), (r, k, losses[k], v)
        err = (flat - ref_flat).abs().max().item()
        print(f"rank {r}: max |param - single-rank param| = {err:.3e}")
        assert err <= flat_atol, (r, err)
