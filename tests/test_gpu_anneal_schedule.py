"""The per-update schedule inside the recorded programs (PolicyUpdater(anneal_lr=True, total_network_updates=...), ClipPPOLoss2(
anneal_clip_epsilon=True): train.py:263-276) against the host's own way of following it -- ``upd.anneal_lr(base, n, total)`` and
``loss.clip_epsilon.copy_(eps * alpha)`` in front of every ``step_from`` (the path tests/test_gpu_boundary.py holds against the
reference-style torch loop) -- BITWISE: parameters, both Adam moments, every entry of every step's loss dict, ``upd.lr``.

One epoch of the small rigid HEPi rollout, 16 environments x 12 time steps, 16-frame minibatches, ``epoch_unroll = 4``: one eager update,
two launches of four updates (the second a replay), three replays of the per-step program.  total_network_updates = 40, so that the
values of neighbouring updates differ in many float32 bits (lr by 2.5 % of the base per update)."""
import functools
import math

import numpy as np
import pytest
import torch

from spawn_util import spawn_ranks
from updater_cases import DEV, dp_case, make_rollout, rendezvous, shard_of

pytestmark = pytest.mark.gpu

N, T, TOTAL = 16, 12, 40
CUT = [(0, 1), (1, 5), (5, 9), (9, 10), (10, 11), (11, 12)]   # calls after which every step's loss dict can be read
WHOLE = [(0, 12)]                                              # the epoch's index matrix in one call
STEPWISE = [(n, n + 1) for n in range(12)]                     # (the forms without a multi-step launch: a loop of step_from either way)
FORMS = {"lanes": dict(use_graph=True), "one_stream": dict(use_graph=True, overlap_critic=False), "eager": dict(use_graph=False)}


def _alpha(n):
    return 1.0 - n / float(TOTAL)


def _clone(out):
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _ratios_near_the_clip_bounds(r, buf):
    """PPO: the synthetic old log-probabilities put the probability ratios far outside every clip range, where the epsilon reaches the
    reported objective but no gradient.  Replace them so that every frame's ratio under the CURRENT policy lies in [0.78, 0.88] or
    [1.12, 1.22] -- around the bounds 1 -+ epsilon that the schedule moves (0.2 -> 0.145 over the epoch): which frames are clipped, and with
    it the parameters, then depends on each update's epsilon.  A pure function of the seeded agent, the same on every side."""
    flat = lambda k: buf.data[k].reshape(N * T, -1)
    with torch.no_grad():
        loc, sigma = r.actor.forward_diag(*[flat(k) for k in r.loss.in_features], train=True)
        act = flat("action")
        logp = -0.5 * (((act - loc) / sigma) ** 2).sum(-1) - sigma.log().sum(-1) - 0.5 * act.shape[1] * math.log(2 * math.pi)
    g = torch.Generator().manual_seed(5)
    ratio = 0.78 + 0.10 * torch.rand(N * T, generator=g) + 0.34 * (torch.rand(N * T, generator=g) < 0.5)
    buf.data["sample_log_prob"] = (logp - ratio.to(DEV).log()).reshape(buf.data["sample_log_prob"].shape).contiguous()


def _epoch(algo, form_kw, *, lr_on=False, eps_on=False, host_lr=False, host_eps=None, calls=CUT, epochs=1, setup=None, driver=False):
    """``epochs`` epochs on a fresh, identically seeded agent.  ``lr_on`` / ``eps_on``: the updater's own schedule, driven by
    run_minibatches over ``calls`` (row ranges of the epochs' stacked index matrices) or, ``driver``, by ``RolloutDriver.run`` (the
    result then carries its ``iteration_log``).  ``host_lr`` / ``host_eps="step"``: the host writes the value of update n in front of every
    step_from; ``host_eps="call"``: in front of every CALL only -- the epsilon of a launch's first update, held for the whole launch.
    ``setup(upd)`` runs on the fresh updater."""
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import RolloutBuffer, RolloutDriver
    r = make_rollout(N, T, 21, algorithm=algo, **(dict(anneal_clip_epsilon=True) if eps_on else {}))
    base, eps0 = r.cfg.lr, r.cfg.clip_epsilon
    upd = agent.PolicyUpdater(r.loss, lr=base, **form_kw, **(dict(anneal_lr=True) if lr_on else {}),
                              **(dict(total_network_updates=TOTAL) if (lr_on or eps_on) else {}))
    upd.epoch_unroll = 4
    if setup is not None:
        setup(upd)
    buf = RolloutBuffer(dict(r.data))
    drv = RolloutDriver(upd, r.spec, ppo_epochs=epochs, seed=3)
    drv.compute_advantages(buf, r.next_last)
    if algo == "ppo":
        _ratios_near_the_clip_bounds(r, buf)
    n_upd, log = T * epochs, None
    outs = {}
    if driver:
        outs[n_upd - 1] = _clone(drv.run(buf))
        log = drv.iteration_log(buf)
        calls = []
    else:
        rows = torch.cat([torch.stack(drv.epoch_minibatches(N, T, DEV)) for _ in range(epochs)])
        assert rows.shape == (n_upd, N)
    if host_lr or host_eps == "step":
        for n in range(n_upd):
            if host_lr:
                upd.anneal_lr(base, n, TOTAL)
            if host_eps:
                r.loss.clip_epsilon.copy_(eps0 * _alpha(n))          # train.py:274
            outs[n] = _clone(upd.step_from(buf, rows[n]))
    else:
        for lo, hi in calls:
            if host_eps == "call":
                r.loss.clip_epsilon.copy_(eps0 * _alpha(lo))
            out = upd.run_minibatches(buf, rows[lo:hi])
            if epochs == 1 and hi - lo >= 4 and upd._epoch is not None:   # ``last_outs``: the four steps of the call's last multi-step launch
                first = lo + (1 if lo == 0 else 0)         # (update 0 runs eagerly)
                start = first + 4 * ((hi - first) // 4 - 1)
                assert len(upd.last_outs) == 4
                outs.update({start + i: _clone(o) for i, o in enumerate(upd.last_outs)})
            outs[hi - 1] = _clone(out)
        if form_kw.get("use_graph") and form_kw.get("overlap_critic", True):
            assert upd._epoch is not None and upd._program is not None, "both recorded forms must have run"
    torch.cuda.synchronize()
    assert upd.steps == n_upd
    eps = float(r.loss.clip_epsilon) if algo == "ppo" else None
    return dict(flat=upd.flat.detach().clone(), exp_avg=upd.exp_avg.detach().clone(), exp_avg_sq=upd.exp_avg_sq.detach().clone(),
                outs=outs, lr=upd.lr, eps=eps, log=log, form_times=dict(upd.form_times))


@functools.lru_cache(maxsize=None)
def _host_side(algo, form, eps=False, epochs=1):
    """The host-driven epoch(s) of a case, computed once and shared (read-only) by the tests that compare with it."""
    return _epoch(algo, FORMS[form], host_lr=True, host_eps="step" if eps else None, epochs=epochs)


def _assert_bitwise(a, b):
    for k in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    assert a["outs"] and set(a["outs"]) <= set(b["outs"])
    for n, oa in a["outs"].items():
        assert set(oa) == set(b["outs"][n])
        for k, v in oa.items():
            assert torch.equal(v, b["outs"][n][k]), (n, k)
    assert a["lr"] == b["lr"]


@pytest.mark.parametrize("form", ["lanes", "one_stream", "eager"])
@pytest.mark.parametrize("algo", ["trpl", "ppo"])
def test_lr_schedule_equals_the_host_loop_bitwise(algo, form):
    a = _epoch(algo, FORMS[form], lr_on=True, calls=CUT if form == "lanes" else STEPWISE)
    assert set(a["outs"]) == set(range(T))                           # every step's loss dict
    _assert_bitwise(a, _host_side(algo, form))
    assert a["lr"] == 3e-4 * _alpha(T - 1)                             # the rate of the last issued update
    if algo == "ppo":
        assert a["eps"] == float(np.float32(0.2))                      # (lr alone: the epsilon is not touched)


@pytest.mark.parametrize("algo", ["trpl", "ppo"])
def test_lr_schedule_over_the_whole_index_matrix_in_one_call(algo):
    a = _epoch(algo, FORMS["lanes"], lr_on=True, calls=WHOLE)
    assert set(a["outs"]) == {5, 6, 7, 8, 11}                          # (the last launch's four steps and the last step)
    _assert_bitwise(a, _host_side(algo, "lanes"))


@pytest.mark.parametrize("calls", [CUT, WHOLE], ids=["cut", "whole"])
def test_clip_epsilon_schedule_equals_the_host_loop_bitwise(calls):
    a = _epoch("ppo", FORMS["lanes"], lr_on=True, eps_on=True, calls=calls)
    b = _host_side("ppo", "lanes", eps=True)
    _assert_bitwise(a, b)
    want = float(np.float32(0.2 * (1 - 11 / 40)))
    assert a["eps"] == want == b["eps"]                                # the loss module's buffer: the last issued update's epsilon
    if calls is CUT:
        # the comparison can notice a miss: the same run with the epsilon of a launch's FIRST update held for the whole launch ends elsewhere
        held = _epoch("ppo", FORMS["lanes"], lr_on=True, host_eps="call", calls=CUT)
        assert not torch.equal(a["flat"], held["flat"])
        assert torch.equal(a["outs"][1]["loss_objective"], held["outs"][1]["loss_objective"])      # (first step of a launch: the same epsilon)
        assert not torch.equal(a["outs"][4]["loss_objective"], held["outs"][4]["loss_objective"])  # (its last step: another one)


def test_clip_epsilon_schedule_alone_on_one_stream_and_eager():
    """Epsilon annealed, the learning rate the host's (constant): the table's lr entries are not read."""
    for form in ("one_stream", "eager"):
        a = _epoch("ppo", FORMS[form], eps_on=True, calls=STEPWISE)
        b = _epoch("ppo", FORMS[form], host_eps="step")
        _assert_bitwise(a, b)
        assert a["lr"] == 3e-4 and a["eps"] == float(np.float32(0.2 * (1 - 11 / 40)))


def test_schedule_through_the_measured_choice_of_the_form():
    """``_tune_form``: one call with enough minibatches (two epochs' 24) records both forms and times alternating blocks of them -- every
    block ordinary updates of the next minibatches, each at its own update's values."""
    def tune_at_every_size(upd):
        upd.epoch_unroll_max_gated_frames = 0      # (16 frames count as "above the table's small sizes": the choice is measured)
    a = _epoch("ppo", FORMS["lanes"], lr_on=True, eps_on=True, calls=[(0, 2 * T)], epochs=2, setup=tune_at_every_size)
    assert N in a["form_times"], "the two forms were not measured"
    _assert_bitwise(a, _host_side("ppo", "lanes", eps=True, epochs=2))
    assert a["eps"] == float(np.float32(0.2 * _alpha(2 * T - 1)))


def test_rollout_driver_runs_the_updaters_schedule_and_logs_the_last_updates_values():
    """``RolloutDriver.run`` takes no new argument: two epochs through the updater's schedule equal the host loop, and ``iteration_log``
    reports the learning rate and the clip epsilon of the iteration's last update (train.py:326-331)."""
    a = _epoch("ppo", dict(FORMS["lanes"], track_stats=True), lr_on=True, eps_on=True, epochs=2, driver=True)
    b = _host_side("ppo", "lanes", eps=True, epochs=2)
    _assert_bitwise(a, b)
    assert a["log"]["train/lr"] == 3e-4 * _alpha(2 * T - 1) == b["lr"]
    assert a["log"]["train/clip_epsilon"] == float(np.float32(0.2 * _alpha(2 * T - 1))) == b["eps"]


def test_setting_lr_moves_the_schedules_base_without_recording_again():
    upd, batch = _single(16, "trpl", FORMS["lanes"], True)
    ref, _ = _single(16, "trpl", FORMS["lanes"], False)
    for n in range(6):
        if n == 3:
            upd.lr = 1e-3
            assert upd._program is not None and upd.lr == 3e-4 * _alpha(2)     # (still the last issued update's rate)
        program = upd._program
        ref.anneal_lr(3e-4 if n < 3 else 1e-3, n, TOTAL)
        upd.step(batch)
        ref.step(batch)
        assert n < 2 or upd._program is program, "the recording was dropped"
        assert upd.lr == ref.lr
    torch.cuda.synchronize()
    assert torch.equal(upd.flat, ref.flat) and torch.equal(upd.exp_avg_sq, ref.exp_avg_sq)


@pytest.mark.parametrize("gate", [False, "edge0"])
def test_critic_lane_late_or_early_reads_its_own_steps_rate(gate):
    """The critic's lane never gated (it runs ahead of the actor's inside a launch) and always gated (it trails the actor's first edge
    convolution of every step): its Adam of step j reads entry j either way -- bitwise the host loop's result."""
    a = _epoch("trpl", dict(use_graph=True, critic_after_first_conv=gate), lr_on=True)
    _assert_bitwise(a, _host_side("trpl", "lanes"))


@pytest.mark.parametrize("n", [1, 2, 8, 63, 64])
def test_write_floats(n):
    """grl_write_floats: exactly dst[0..n) is written, each value the float32 of its Python float, the mirror gets values[index]; shapes it
    does not take are refused on the host."""
    from geometry_rl_amd import hip, ops
    vals = [3e-4 * (1.0 - i / 77.0) for i in range(64)]
    buf = torch.full((72,), 7.0, device=DEV)
    mirror = torch.full((3,), 7.0, device=DEV)
    ops.write_floats(buf[4:], vals[:n], mirror[1:2], n - 1)
    want = torch.full((72,), 7.0)
    want[4:4 + n] = torch.tensor(np.array(vals[:n]).astype(np.float32))
    assert torch.equal(buf.cpu(), want)
    assert torch.equal(mirror.cpu(), torch.tensor([7.0, float(np.float32(vals[n - 1])), 7.0]))
    ops.write_floats(buf, [1.5] * n)                       # (no mirror)
    assert torch.equal(buf[:n].cpu(), torch.full((n,), 1.5))
    if n == 1:
        import ctypes
        for bad_n, idx in ((0, 0), (65, 0), (4, 4), (4, -1)):
            with pytest.raises(RuntimeError, match="status -2"):
                hip.call("grl_write_floats", buf, (ctypes.c_float * 65)(), bad_n, mirror[:1], idx)
        with pytest.raises(ValueError):
            ops.write_floats(buf, [0.0] * 65)
        with pytest.raises(ValueError):
            ops.write_floats(buf[:2], [0.0] * 3)
    torch.cuda.synchronize()


# ---- data parallel: two ranks on one GPU (gloo; the pieces of updater_cases' two-rank harness), one eager update and three recorded ones
DP_STEPS = 4
DP_KEYS = ("loss_objective", "loss_critic", "kl")


def _dp_worker(rank, world, port, ret):
    """One rank: the data-parallel case twice on one process group -- its updater following the schedule by itself, then a default updater
    with the host's ``anneal_lr`` in front of every update."""
    from geometry_rl_amd import agent
    with rendezvous(rank, world, port) as group:
        for side in ("schedule", "host"):
            case = dp_case(16, group, cfg_kw={})
            shard = shard_of(case.batch, rank, world)
            kw = dict(anneal_lr=True, total_network_updates=TOTAL) if side == "schedule" else {}
            upd = agent.PolicyUpdater(case.loss, lr=case.cfg.lr, group=group, use_graph=True, **kw)
            for i in range(DP_STEPS):
                if side == "host":
                    upd.anneal_lr(case.cfg.lr, i, TOTAL)
                out = upd.step(shard)
            torch.cuda.synchronize()
            ret[(side, rank)] = (upd.flat.detach().cpu(), {k: float(out[k].detach()) for k in DP_KEYS}, upd.lr, upd.mode,
                                 upd._program is not None)


def test_two_ranks_follow_the_schedule_bitwise():
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    spawn_ranks(_dp_worker, 2, (2,), (ret,))
    ret = dict(ret)
    a, b = [ret[("schedule", r)] for r in (0, 1)], [ret[("host", r)] for r in (0, 1)]
    for r in (0, 1):
        assert a[r][3:] == ("graph", True) == b[r][3:]
    assert torch.equal(a[0][0], a[1][0]), "the ranks' parameters diverged"
    assert a[0][2] == a[1][2] == 3e-4 * _alpha(DP_STEPS - 1)               # every rank's upd.lr
    for r in (0, 1):
        assert torch.equal(a[r][0], b[r][0]), r                            # ... and the same ranks driven by the host's anneal_lr
        assert a[r][1] == b[r][1] and a[r][2] == b[r][2]


# ---- nothing else moved: the C-ABI calls of a step, schedule off against on
def _single(B, algo, form_kw, on):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, algorithm=algo, anneal_clip_epsilon=on)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    batch = dict(syn.make_rigid_obs(B, seed=1))
    batch.update(syn.make_ppo_fields(B, 6, seed=1))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)
    return agent.PolicyUpdater(loss, lr=cfg.lr, **form_kw, **(dict(anneal_lr=True, total_network_updates=TOTAL) if on else {})), batch


@pytest.mark.parametrize("form", ["lanes", "one_stream"])
@pytest.mark.parametrize("B", [16, 512])
def test_a_step_issues_the_same_launches_plus_one_fill_in_front(monkeypatch, B, form):
    """The entry points the host calls for the eager, the recording and a replayed step (PPO: both values scheduled): with the schedule on
    they are the schedule-off step's, behind ONE grl_write_floats -- no launch inside a step is added, and off nothing is."""
    from geometry_rl_amd import hip
    names, real = [], hip.call

    def logging_call(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(hip, "call", logging_call)
    seen = {}
    for on in (False, True):
        upd, batch = _single(B, "ppo", FORMS[form], on)
        assert (upd.sched_table is not None) == on
        seen[on] = []
        for _ in range(3):
            del names[:]
            upd.step(batch)
            seen[on].append(list(names))
        torch.cuda.synchronize()
        assert upd._program is not None
    for off_step, on_step in zip(seen[False], seen[True]):
        assert "grl_write_floats" not in off_step
        assert on_step[0] == "grl_write_floats" and on_step[1:] == off_step
