"""The per-update schedule of train.py:263-276 (PolicyUpdater(anneal_lr=True, total_network_updates=...), ClipPPOLoss2(anneal_clip_epsilon=
True)) without a GPU: the schedule function to float32 bits, the total of train.py:54-59, the defaults, the refusals, what build_agent and
updater_kwargs hand through -- and that the programs' entries are what they were, schedule off and on."""
import ctypes

import numpy as np
import pytest
import torch

from geometry_rl_amd import agent, graph, updater

SMALL = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)


def _f32_bits(x: float) -> int:
    """The float32 a C cast makes of a Python float (what the kernel-argument array of ops.write_floats holds), as its 32 bits."""
    return ctypes.c_uint32.from_buffer_copy(ctypes.c_float(x)).value


def _build(**cfg_kw):
    cfg = agent.AgentConfig(**dict(SMALL, **cfg_kw))
    torch.manual_seed(0)
    return cfg, agent.build_agent(graph.rigid_spec(), cfg, device="cpu")


@pytest.mark.parametrize("total", [1, 7, 640])
@pytest.mark.parametrize("base", [3e-4, 0.2])   # the configs' learning rate and clip epsilon
def test_schedule_function_to_float32_bits(total, base):
    for n in range(total):
        want = np.float32(base * (1.0 - n / float(total)))
        got = updater.annealed(base, n, total)
        assert isinstance(got, float) and got == base * (1.0 - n / float(total))          # float64, the reference's expression
        assert _f32_bits(got) == int(want.view(np.uint32)), (n, total, got, want)         # rounded once, as numpy rounds it
        assert torch.full((1,), got, dtype=torch.float32).view(torch.int32).item() == int(want.view(np.int32))   # ... and as fill_ stores it
    assert updater.annealed(base, 0, total) == base


def test_total_is_derived_as_the_reference_derives_it():
    # train.py:54-59: (total_frames // frames_per_batch) * ppo_epochs * (frames_per_batch // mini_batch_size)
    assert updater.total_network_updates(total_frames=4096 * 128 * 10, frames_per_batch=4096 * 128, ppo_epochs=5, mini_batch_size=4096) == 10 * 5 * 128
    assert updater.total_network_updates(1000, 300, 5, 128) == 3 * 5 * 2        # both divisions round down
    assert updater.total_network_updates(16 * 12, 16 * 12, 1, 16) == 12


def test_defaults_leave_everything_off_and_allocate_nothing():
    cfg = agent.AgentConfig()
    assert cfg.anneal_lr is False and cfg.anneal_clip_epsilon is False
    for algo_kw in (dict(), dict(algorithm="ppo"), dict(algorithm="kl_ppo", dtarg=0.01)):
        cfg, (_, _, _, loss) = _build(**algo_kw)
        assert not getattr(loss, "anneal_clip_epsilon", False)
        upd = agent.PolicyUpdater(loss, **agent.updater_kwargs(cfg))
        assert upd.sched_table is None and not upd.anneals_lr and not upd.anneals_eps
        assert upd._sched_slots(0) == {}
        # the host-side entry points behave as before
        assert upd.anneal_lr(3e-4, 3, 12) == 3e-4 * (1.0 - 3 / 12.0) == upd.lr
        assert float(upd.lr_dev) == np.float32(upd.lr)
        upd.lr = 1e-3
        assert upd.lr == 1e-3 and float(upd.lr_dev) == np.float32(1e-3)


def test_switching_on_without_a_total_raises():
    cfg, (_, _, _, loss) = _build()
    with pytest.raises(ValueError, match="total_network_updates"):
        agent.PolicyUpdater(loss, anneal_lr=True)
    with pytest.raises(ValueError, match="total_network_updates"):
        agent.PolicyUpdater(loss, anneal_lr=True, total_network_updates=0)
    cfg, (_, _, _, ppo) = _build(algorithm="ppo", anneal_clip_epsilon=True)
    with pytest.raises(ValueError, match="total_network_updates"):
        agent.PolicyUpdater(ppo)                       # the loss module's flag alone needs the total as well
    assert agent.PolicyUpdater(ppo, total_network_updates=5).anneals_eps


def test_an_update_behind_the_total_is_refused_before_the_count_moves():
    cfg, (_, _, _, loss) = _build()
    upd = agent.PolicyUpdater(loss, anneal_lr=True, total_network_updates=3)
    issued = []
    upd.steps = 3                                     # (three updates have run)
    with pytest.raises(ValueError, match="total_network_updates = 3"):
        upd._advance(None, 1, lambda: issued.append(1))
    assert upd.steps == 3 and not issued and loss._global_steps == 0
    upd.steps = 1                                     # a launch of several steps whose LAST update lies behind the total
    with pytest.raises(ValueError, match="update 3 "):
        upd._advance(None, 3, lambda: issued.append(1))
    assert upd.steps == 1 and not issued
    upd.steps = 3
    with pytest.raises(ValueError, match="total_network_updates = 3"):
        upd.step_from(None, None)                     # (refused in front of the gather: the buffer is not touched)
    off = agent.PolicyUpdater(loss)                   # no schedule: no limit
    off.steps = 10 ** 6
    off._schedule_check(8)


def test_anneal_lr_call_is_refused_by_an_annealing_updater_and_lr_sets_the_base():
    cfg, (_, _, _, loss) = _build()
    upd = agent.PolicyUpdater(loss, lr=3e-4, anneal_lr=True, total_network_updates=40)
    assert upd.lr == 3e-4
    with pytest.raises(RuntimeError, match="per update"):
        upd.anneal_lr(3e-4, 1, 40)
    upd._program = object()                           # (a recording)
    upd.lr = 1e-3
    assert upd._base_lr == 1e-3 and upd._program is not None, "setting the base rate must not drop recordings"
    assert upd.lr == 3e-4                             # still the rate of the last issued update (none yet: the start value)


def test_build_agent_and_updater_kwargs_hand_the_flags_through():
    for algo_kw in (dict(), dict(algorithm="ppo", clip_epsilon=0.3), dict(algorithm="kl_ppo", dtarg=0.01)):
        cfg, (_, _, _, loss) = _build(anneal_lr=True, anneal_clip_epsilon=True, total_train_steps=640, lr=1e-3, **algo_kw)
        kw = agent.updater_kwargs(cfg)
        assert kw["anneal_lr"] is True and kw["total_network_updates"] == 640 and kw["lr"] == 1e-3
        upd = agent.PolicyUpdater(loss, **kw)
        assert upd.anneals_lr and upd.total_network_updates == 640 and upd.sched_table.numel() == 2 * upd.SCHED_SLOTS
        is_ppo = cfg.algorithm == "ppo"                # train.py:272: the epsilon schedule is PPO's alone
        assert upd.anneals_eps == is_ppo
        if is_ppo:
            assert loss.anneal_clip_epsilon and loss.base_clip_epsilon == 0.3 and float(loss.clip_epsilon) == np.float32(0.3)
        assert set(upd._sched_slots(2)) == ({"lr", "eps"} if is_ppo else {"lr"})
        sl = upd._sched_slots(2)
        assert sl["lr"].data_ptr() == upd.sched_table.data_ptr() + 4 * 4 and sl["lr"].numel() == 1
        if is_ppo:
            assert sl["eps"].data_ptr() == upd.sched_table.data_ptr() + 4 * 5
    cfg, (_, _, _, ppo) = _build(algorithm="ppo", anneal_clip_epsilon=True, total_train_steps=9)
    upd = agent.PolicyUpdater(ppo, **agent.updater_kwargs(cfg))     # epsilon alone: lr stays the host's
    assert upd.anneals_eps and not upd.anneals_lr and set(upd._sched_slots(0)) == {"eps"}
    assert upd.anneal_lr(3e-4, 1, 2) == 1.5e-4


# ---- the programs' entries: (kind, lane, label, eager) of every entry, as the commit before the schedule lays them out
_ONE_STREAM = [("run", "m", None, False)] * 4 + [("run_host", "m", None, False)]
_LANES = [("fork", "m", None, False), ("run", "m", None, False), ("run", "s", "critic_gate_wait", False), ("run", "s", None, False),
          ("join", "m", None, False), ("run_host", "m", None, False)]
_DP = [("fork", "m", None, False), ("run", "m", None, False), ("sum", "m", "advantage_stats", False), ("run", "s", None, False),
       ("sum", "s", "critic_ln1_fwd_stats", False), ("run", "s", None, False), ("sum", "s", "critic_ln2_fwd_stats", False),
       ("run", "m", None, False), ("sum", "m", "flat_gradient_actor+loss_records", False), ("run", "s", None, False),
       ("sum", "s", "critic_ln2_bwd_stats", False), ("run", "s", None, False), ("sum", "s", "critic_ln1_bwd_stats", False),
       ("run", "m", None, True), ("run", "s", None, False), ("sum", "s", "flat_gradient_critic", False),
       ("sum", "s", "loss_critic_sum", False), ("run", "s", None, False), ("join", "m", "join_critic_lane", False),
       ("run_host", "m", None, False)]
_DP_OUTLINE = [("fork", "m", None, None), ("run", "s", None, None), ("sum", "s", "critic_ln1_fwd_stats", "group"), ("run", "s", None, None),
               ("sum", "s", "critic_ln2_fwd_stats", "group"), ("run", "m", None, None),
               ("sum", "m", "flat_gradient_actor+loss_records", "group"), ("run", "s", None, None),
               ("sum", "s", "critic_ln2_bwd_stats", "group"), ("run", "s", None, None), ("sum", "s", "critic_ln1_bwd_stats", "group"),
               ("run", "m", None, None), ("run", "s", None, None), ("sum", "s", "flat_gradient_critic", "group"),
               ("sum", "s", "loss_critic_sum", "group"), ("run", "s", None, None), ("join", "m", "join_critic_lane", None),
               ("run_host", "m", None, None)]


@pytest.mark.parametrize("schedule", [False, True])
@pytest.mark.parametrize("algo_kw", [dict(), dict(algorithm="ppo"), dict(algorithm="kl_ppo", dtarg=0.01)], ids=["trpl", "ppo", "kl_ppo"])
def test_program_entries_are_unchanged(schedule, algo_kw):
    """Nothing is added to a program: the fill launch is issued in front of it (``_advance``), never as one of its entries."""
    on = dict(anneal_lr=True, anneal_clip_epsilon=True, total_train_steps=640) if schedule else {}
    cfg, (_, _, _, loss) = _build(**algo_kw, **on)
    upd = agent.PolicyUpdater(loss, **agent.updater_kwargs(cfg))
    assert (upd.sched_table is not None) == schedule
    assert upd.program_outline() == _DP_OUTLINE
    assert upd.program_outline(published=False) == [e[:3] + (None if e[0] != "sum" else "group",) for e in _DP]
    for frames in (16, 512):
        batch = {"x": torch.zeros(frames)}
        for plan, want in (("_plan_one_stream", _ONE_STREAM), ("_plan_lanes", _LANES), ("_plan_dp", _DP)):
            got = [(e.kind, e.lane, e.label, e.eager) for e in getattr(upd, plan)(batch, {})]
            assert got == want, (plan, frames)
