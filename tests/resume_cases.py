"""Scaffolding of the save-and-resume tests (tests/test_gpu_resume*.py, tests/test_checkpoint_cpu.py).  TEST INFRASTRUCTURE ONLY, a plain
module like tests/updater_cases.py, whose rollout builder and spawn harness it uses.

A run here is two iterations of the small rigid agent: N = 8 environments, T = 4, ppo_epochs = 2, one frame per environment per minibatch,
``epoch_unroll = 2`` -- so an iteration is ``compute_advantages`` and then 2 epochs x 2 launches x 2 steps, and the whole run LAUNCHES = 8
launches, 16 updates.  ``run_launches`` issues launches ``start .. stop - 1`` and keeps every step's loss dict and, behind every
iteration, a snapshot of everything two runs are compared in.  Rollout buffers are not part of a training state: a run that stops inside
an iteration hands its buffer and the epoch's minibatch rows on as ``carry``, as the caller of a real run would.

``differences(a, b)`` is the ONE comparison: every tensor with ``torch.equal``, every other value with ``==``, no tolerance anywhere; it
returns what differs as text, and tests/test_checkpoint_cpu.py checks that it reports each kind of omission."""
import torch

N, T, EPOCHS, UNROLL = 8, 4, 2, 2
PER_ITER = EPOCHS * (T // UNROLL)      # launches per iteration
LAUNCHES = 2 * PER_ITER
DATA_SEEDS = (21, 33)                  # one synthetic rollout per iteration
DRIVER_SEED = 7

CASES = {
    # TRPL (kl) with training noise and the scheduled entropy bound: noise words, latched initial entropy, bounds formed from ``steps``
    "trpl": dict(training_noise=True, entropy_schedule="linear", total_train_steps=64),
    # clipped PPO with both per-update schedules: lr and clip epsilon of update n come from ``steps``
    "ppo": dict(algorithm="ppo", anneal_lr=True, anneal_clip_epsilon=True, total_train_steps=64),
    # KL-penalty PPO: beta is device data in both directions; the synthetic old distribution is far from the policy's, so beta moves at once
    "kl_ppo": dict(algorithm="kl_ppo", dtarg=1e-3),
    "empn": dict(model="empn"),
}


def rollout_data(seed, dev, spec, lo=0, hi=N):
    """updater_cases.make_rollout's inputs without an agent: ([N, T, ...] data with GAE inputs, the frame behind the last); rows lo:hi."""
    from geometry_rl_amd import synthetic as syn
    frames = []
    for t in range(T + 1):
        b = dict(syn.make_rigid_obs(N, seed=seed + t))
        b.update(syn.make_ppo_fields(N, 6, seed=seed + t))
        frames.append(b)
    data = {k: torch.stack([f[k] for f in frames[:T]], dim=1)[lo:hi].contiguous().to(dev) for k in frames[0]}
    g = syn.make_gae_inputs(N, T, seed=seed)
    data.update({k: g[k].reshape(N, T, 1)[lo:hi].contiguous().to(dev) for k in ("reward", "done", "terminated")})
    next_last = {k: frames[T][k][lo:hi].unsqueeze(1).contiguous().to(dev) for k in spec.in_features}
    return data, next_last


def build_objects(case, dev, *, torch_seed, driver_seed, use_graph=True, form=None, track=False, group=None, calibrate_on=None):
    """A fresh agent (``build_agent`` under ``torch_seed``), updater and driver.  ``calibrate_on``: the minibatch of the calibrating forward
    (the uninterrupted run's, as make_rollout does); None: none -- a resumed run must not need one."""
    from geometry_rl_amd import agent, graph
    from geometry_rl_amd.rollout import RolloutDriver
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(**dict(dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2), **CASES[case]))
    torch.manual_seed(torch_seed)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev, group=group)
    if calibrate_on is not None:
        with torch.no_grad():
            actor.forward_diag(*[calibrate_on[k] for k in spec.in_features], train=True)
    upd = agent.PolicyUpdater(loss, use_graph=use_graph, group=group, track_stats=track, **agent.updater_kwargs(cfg))
    upd.epoch_unroll = UNROLL
    if form is not None:
        upd.form_by_size[N] = form
    drv = RolloutDriver(upd, spec, ppo_epochs=EPOCHS, seed=driver_seed)
    return dict(spec=spec, cfg=cfg, actor=actor, critic=critic, proj=proj, loss=loss, upd=upd, drv=drv)


def latches(actor):
    return {n: bool(b) for n, b in actor.named_buffers() if n.endswith("callibrated")}


def snapshot(upd, drv, extra=None):
    """Everything two runs are compared in behind an iteration, on the CPU."""
    upd.join_lanes()
    if upd.flat.is_cuda:
        torch.cuda.synchronize()
    m = upd.loss_module
    ent = getattr(getattr(m, "projection", None), "initial_entropy", None)
    snap = {
        "flat": upd.flat.detach().cpu().clone(), "exp_avg": upd.exp_avg.detach().cpu().clone(), "exp_avg_sq": upd.exp_avg_sq.detach().cpu().clone(),
        "noise": {k: tuple(hd.noise_state()) for k, hd in upd._data_objects().items()},
        "lr": upd.lr, "scalars": {k: t.detach().cpu().clone() for k, t in m.device_scalars.items()},
        "steps": {"host": upd.steps, "step_dev": int(upd.step_dev), "step_dev_c": int(upd.step_dev_c)},
        "initial_entropy": None if ent is None else torch.as_tensor(ent).detach().cpu().clone(),
        "generator": None if drv is None or drv.gen is None else drv.gen.get_state().clone(),
        "latches": latches(m.actor_network),
    }
    if upd.track_stats:
        snap["stats"] = upd.stats_read()
    snap.update(extra or {})
    return snap


def _launch(upd, buf, rows):
    """The ``UNROLL`` minibatches ``rows`` as run_minibatches issues them -> every step's loss dict (cloned: recorded steps hand out views).
    Where run_minibatches takes the multi-step launch, ``last_outs`` has the steps; where it loops over ``step_from`` (the first, eager
    step of a size; the per-step form; an eager or data-parallel updater) the same loop runs here, one row per call."""
    keep = lambda o: {k: v.detach().clone() for k, v in o.items() if torch.is_tensor(v)}
    if upd._epoch_ok() and int(rows.shape[1]) in upd._eager_sizes and upd.form_by_size.get(int(rows.shape[1])) != "per_step":
        upd.run_minibatches(buf, rows)
        assert upd._epoch is not None and len(upd.last_outs) == rows.shape[0], "the multi-step launch was not taken"
        return [keep(o) for o in upd.last_outs]
    return [keep(upd.run_minibatches(buf, rows[j:j + 1])) for j in range(rows.shape[0])]


def run_launches(objs, datas, start=0, stop=LAUNCHES, carry=None, at=None):
    """Launches ``start .. stop - 1`` of the run -> ({"outs": [per step], "iterations": [snapshot behind each finished iteration]}, carry).
    ``carry``: (buffer, the epoch's rows) of a run that stopped inside an iteration.  ``at``: {launch index: callable()} run IN FRONT of
    that launch (a save between two launches)."""
    from geometry_rl_amd.rollout import RolloutBuffer
    upd, drv = objs["upd"], objs["drv"]
    dev = upd.flat.device
    rec = {"outs": [], "iterations": []}
    buf, rows = carry if carry is not None else (None, None)
    for L in range(start, stop):
        it, half = L // PER_ITER, L % (T // UNROLL)
        if at and L in at:
            at[L]()
        if L % PER_ITER == 0:
            data, next_last = datas[it]
            buf = RolloutBuffer(dict(data))
            drv.compute_advantages(buf, next_last)
            if upd.track_stats:
                upd.stats_reset()
        if half == 0:
            idxs = drv.epoch_minibatches(buf.N, buf.T, dev)
            drv.publish_advantage_stats(buf, idxs)
            rows = torch.stack(idxs)
        rec["outs"] += _launch(upd, buf, rows[half * UNROLL:(half + 1) * UNROLL])
        if L % PER_ITER == PER_ITER - 1:
            rec["iterations"].append(snapshot(upd, drv))
    return rec, (buf, rows)


def uninterrupted(case, dev, datas, **kw):
    """The run that is never interrupted: built under seed 0 and calibrated on time step 0 of the first rollout, all 8 launches."""
    spec_feats = list(datas[0][1])
    objs = build_objects(case, dev, torch_seed=0, driver_seed=DRIVER_SEED, calibrate_on={k: datas[0][0][k][:, 0].contiguous() for k in spec_feats}, **kw)
    rec, _ = run_launches(objs, datas)
    return objs, rec


def interrupted_then_resumed(case, dev, datas, path, save_at, **kw):
    """Launches 0 .. save_at - 1, ``checkpoint.save``, then EVERYTHING built again from nothing -- ``build_agent`` under another torch seed
    (other parameters, other noise key), no calibrating forward, a new updater, a new driver with another seed -- ``checkpoint.restore`` and
    launches save_at .. 7.  -> (resumed objects, {"outs", "iterations"} of the resumed part, what ``checks(objs, state)`` returned right
    behind the restore)."""
    from geometry_rl_amd import checkpoint
    feats = list(datas[0][1])
    first = build_objects(case, dev, torch_seed=0, driver_seed=DRIVER_SEED, calibrate_on={k: datas[0][0][k][:, 0].contiguous() for k in feats}, **kw)
    _, carry = run_launches(first, datas, 0, save_at)
    at_save = snapshot(first["upd"], first["drv"])
    checkpoint.save(path, updater=first["upd"], driver=first["drv"])
    del first
    objs = build_objects(case, dev, torch_seed=1, driver_seed=DRIVER_SEED + 92, **kw)
    fresh = snapshot(objs["upd"], objs["drv"])
    state = checkpoint.load(path)
    checkpoint.restore(state, updater=objs["upd"], driver=objs["drv"])
    restored = snapshot(objs["upd"], objs["drv"])
    rec, _ = run_launches(objs, datas, save_at, LAUNCHES, carry=carry if save_at % PER_ITER else None)
    return objs, rec, dict(at_save=at_save, fresh=fresh, restored=restored, state=state)


def tail_of(rec, save_at):
    """The part of an uninterrupted recording a run resumed at launch ``save_at`` repeats."""
    return {"outs": rec["outs"][save_at * UNROLL:], "iterations": rec["iterations"][save_at // PER_ITER:]}


# ------------------------------------------------------------------------------------------------------------- the comparison
def differences(a, b, path="run"):
    """What differs between two recordings / snapshots, as a list of "<path>: <what>" lines ([] = equal): tensors by ``torch.equal`` (and
    dtype and shape), containers entry by entry (a missing key or a different length is a difference), everything else by ``==``."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            return [f"{path}: {type(a).__name__} against {type(b).__name__}"]
        if a.dtype != b.dtype or a.shape != b.shape:
            return [f"{path}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"]
        if not torch.equal(a.cpu(), b.cpu()):
            n = int((a.cpu() != b.cpu()).sum())
            return [f"{path}: {n} of {a.numel()} entries differ"]
        return []
    if isinstance(a, dict) and isinstance(b, dict):
        out = [f"{path}.{k}: only in the {'first' if k in a else 'second'}" for k in sorted(set(a) ^ set(b), key=str)]
        for k in a:
            if k in b:
                out += differences(a[k], b[k], f"{path}.{k}")
        return out
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [f"{path}: {len(a)} entries against {len(b)}"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{path}[{i}]")]
    if type(a) is not type(b) or a != b:
        return [f"{path}: {a!r} against {b!r}"]
    return []


def assert_same(a, b, what):
    diff = differences(a, b, what)
    assert not diff, "\n".join(diff[:20])


# ------------------------------------------------------------------------------------------------------------- two ranks
def dp_worker(rank, world, port, tmp, ret):
    """One rank of the two-rank case: the uninterrupted run and the interrupted-then-resumed run on this rank's half of the environments,
    the state in a file of the rank's own -> ret[rank] = (uninterrupted parameters, resumed parameters, the noise keys of both)."""
    import os
    from updater_cases import rendezvous
    dev = torch.device("cuda:0")
    with rendezvous(rank, world, port) as group:
        from geometry_rl_amd import graph
        spec = graph.rigid_spec()
        lo, hi = rank * N // world, (rank + 1) * N // world
        datas = [rollout_data(s, dev, spec, lo, hi) for s in DATA_SEEDS]
        base = build_objects("trpl", dev, torch_seed=0, driver_seed=DRIVER_SEED, group=group)   # (the natural order: the first update calibrates)
        rec_a, _ = run_launches(base, datas)
        objs, rec_b, info = interrupted_then_resumed_dp(dev, datas, os.path.join(tmp, f"state_rank{rank}.pt"), group)
        diff = differences(tail_of(rec_a, PER_ITER), rec_b, f"rank{rank}")
        ret[rank] = (rec_a["iterations"][-1]["flat"], rec_b["iterations"][-1]["flat"], rec_a["iterations"][-1]["noise"]["actor"],
                     rec_b["iterations"][-1]["noise"]["actor"], info["fresh"]["noise"]["actor"], diff)


def interrupted_then_resumed_dp(dev, datas, path, group):
    """``interrupted_then_resumed`` on a process group: saved behind the first iteration, both ranks rebuilt under torch seed 1."""
    from geometry_rl_amd import checkpoint
    first = build_objects("trpl", dev, torch_seed=0, driver_seed=DRIVER_SEED, group=group)
    run_launches(first, datas, 0, PER_ITER)
    checkpoint.save(path, updater=first["upd"], driver=first["drv"])
    del first
    objs = build_objects("trpl", dev, torch_seed=1, driver_seed=DRIVER_SEED + 92, group=group)
    fresh = snapshot(objs["upd"], objs["drv"])
    checkpoint.restore(checkpoint.load(path), updater=objs["upd"], driver=objs["drv"])
    rec, _ = run_launches(objs, datas, PER_ITER, LAUNCHES)
    return objs, rec, dict(fresh=fresh)
