"""A run that is saved (``checkpoint.save``), built again from nothing and restored (``checkpoint.restore``) continues BIT FOR BIT as the run
that was never interrupted: every step's loss dict, and behind every iteration the parameters, both moments, the noise words, the rate, the
loss module's device scalars, the step counts, the latched initial entropy and the sampler's generator -- all through ``torch.equal`` /
``==`` (resume_cases.differences), no tolerance.  The shapes and the run are resume_cases.py's: N = 8, T = 4, 2 epochs, 2 steps per launch.

The rebuilt side is built under another torch seed (other parameters, another noise key), runs NO calibrating forward and gets a driver with
another seed: whatever the restore leaves out shows."""
import functools

import pytest
import torch

import resume_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _datas():
    from geometry_rl_amd import graph
    return tuple(rc.rollout_data(s, DEV, graph.rigid_spec()) for s in rc.DATA_SEEDS)


@functools.lru_cache(maxsize=None)
def _reference(case, use_graph=True, form=None, track=False):
    """The uninterrupted run of a case: computed once, shared by the tests that compare against it, never changed."""
    objs, rec = rc.uninterrupted(case, DEV, _datas(), use_graph=use_graph, form=form, track=track)
    return rec


def _resume(case, tmp_path, save_at, **kw):
    ref = _reference(case, **kw)
    objs, rec, info = rc.interrupted_then_resumed(case, DEV, _datas(), str(tmp_path / "state.pt"), save_at, **kw)
    # the restore itself: the state at the save, in the rebuilt objects, before anything runs
    rc.assert_same(info["at_save"], info["restored"], "restored")
    assert info["fresh"]["latches"] != info["restored"]["latches"] and any(info["restored"]["latches"].values()), \
        "the rebuilt actor's calibration latches are not the saved ones before its first forward"
    assert rc.differences(info["fresh"]["flat"], info["restored"]["flat"]), "the rebuilt agent started from the saved parameters: the case shows nothing"
    # ... and the continuation
    rc.assert_same(rc.tail_of(ref, save_at), rec, f"{case} resumed at launch {save_at}")
    assert objs["upd"].steps == rc.LAUNCHES * rc.UNROLL
    return objs, rec, info


@pytest.mark.parametrize("case", ["trpl", "ppo", "kl_ppo", "empn"])
def test_resumed_run_continues_bit_for_bit(case, tmp_path):
    """Saved between the two iterations, recorded programs through run_minibatches."""
    objs, rec, info = _resume(case, tmp_path, rc.PER_ITER)
    at_save, m = info["at_save"], objs["loss"]
    assert at_save["steps"]["host"] == rc.PER_ITER * rc.UNROLL
    if case == "trpl":
        assert at_save["initial_entropy"] is not None and at_save["noise"]["actor"][1] > 0
        assert info["fresh"]["noise"]["actor"][0] != at_save["noise"]["actor"][0], "the rebuilt actor drew its noise key from the same seed"
    if case == "kl_ppo":   # the case cannot pass on an untouched beta
        assert float(at_save["scalars"]["kl_beta"]) != objs["cfg"].kl_beta, "beta has not moved by the save point"
    if case == "ppo":
        assert float(at_save["scalars"]["clip_epsilon"]) != objs["cfg"].clip_epsilon and at_save["lr"] != objs["cfg"].lr
    assert info["fresh"]["generator"] is None and not rc.differences(info["restored"]["generator"], at_save["generator"])


def test_kernels_are_not_recalibrated_after_a_restore(tmp_path):
    """The rebuilt actor's latches are the saved ones BEFORE its first forward, and a training forward leaves the convolutions' kernels
    bitwise the saved ones (PPO case: no training noise, so the extra forward consumes no state)."""
    from geometry_rl_amd import checkpoint
    data = _datas()
    feats = list(data[0][1])
    first = rc.build_objects("ppo", DEV, torch_seed=0, driver_seed=rc.DRIVER_SEED, calibrate_on={k: data[0][0][k][:, 0].contiguous() for k in feats})
    rc.run_launches(first, data, 0, 1)
    path = str(tmp_path / "state.pt")
    checkpoint.save(path, updater=first["upd"], driver=first["drv"])
    objs = rc.build_objects("ppo", DEV, torch_seed=1, driver_seed=3)
    assert not any(rc.latches(objs["actor"]).values())
    state = checkpoint.load(path)
    checkpoint.restore(state, updater=objs["upd"], driver=objs["drv"])
    saved = state["parts"]["updater"]["actor"]
    assert rc.latches(objs["actor"]) == rc.latches(first["actor"]) and any(rc.latches(objs["actor"]).values())
    with torch.no_grad():
        objs["actor"].forward_diag(*[data[1][0][k][:, 2].contiguous() for k in feats], train=True)
    torch.cuda.synchronize()
    kernels = [k for k in saved if "kernel" in k and k.endswith("weight")]
    assert kernels
    for k, v in objs["actor"].state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k
    # a training-state file is also a model checkpoint
    from geometry_rl_amd import agent
    other = rc.build_objects("ppo", DEV, torch_seed=2, driver_seed=3)
    agent.load_reference_checkpoint(state["model"], other["actor"], other["critic"], strict=True)
    for k, v in other["actor"].state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k


def test_resumed_eager_run_continues_bit_for_bit(tmp_path):
    _resume("trpl", tmp_path, rc.PER_ITER, use_graph=False)


def test_resumed_between_the_two_launches_of_an_epoch(tmp_path):
    """Saved inside the second iteration, behind the first launch of its first epoch: the sampler's generator is mid-sequence (it has drawn
    three of four epochs), 10 updates have run; the buffer and the epoch's rows are the caller's and are handed on."""
    save_at = rc.PER_ITER + 1
    objs, rec, info = _resume("trpl", tmp_path, save_at)
    assert info["at_save"]["steps"]["host"] == save_at * rc.UNROLL == 10


def test_restore_into_live_objects_keeps_the_recordings(tmp_path):
    """Iteration 1, save, iteration 2, restore into the SAME objects, iteration 2 again: equal results, nothing recorded was dropped."""
    from geometry_rl_amd import checkpoint
    data = _datas()
    feats = list(data[0][1])
    objs = rc.build_objects("trpl", DEV, torch_seed=0, driver_seed=rc.DRIVER_SEED, calibrate_on={k: data[0][0][k][:, 0].contiguous() for k in feats})
    upd = objs["upd"]
    rc.run_launches(objs, data, 0, rc.PER_ITER)
    path = str(tmp_path / "state.pt")
    checkpoint.save(path, updater=upd, driver=objs["drv"])
    once, _ = rc.run_launches(objs, data, rc.PER_ITER, rc.LAUNCHES)
    rc.assert_same(rc.tail_of(_reference("trpl"), rc.PER_ITER), once, "saving changed the run")
    recorded = (upd._program, upd._static, upd._epoch)
    assert all(r is not None for r in recorded)
    checkpoint.restore(checkpoint.load(path), updater=upd, driver=objs["drv"])
    assert upd._program is recorded[0] and upd._static is recorded[1] and upd._epoch is recorded[2]
    assert upd.steps == rc.PER_ITER * rc.UNROLL
    again, _ = rc.run_launches(objs, data, rc.PER_ITER, rc.LAUNCHES)
    rc.assert_same(once, again, "restored into live objects")


def test_one_step_count_everywhere_and_the_gated_program(tmp_path):
    """After a restore at ``steps = k > 0`` the three device-side counts read k, and the gated per-step program -- whose critic lane waits
    for ``lane_flag >= step_dev_c + 1`` -- goes on as in the uninterrupted run."""
    from geometry_rl_amd import checkpoint
    data = _datas()
    feats = list(data[0][1])
    ref = _reference("trpl", form="per_step")
    first = rc.build_objects("trpl", DEV, torch_seed=0, driver_seed=rc.DRIVER_SEED, form="per_step",
                             calibrate_on={k: data[0][0][k][:, 0].contiguous() for k in feats})
    rc.run_launches(first, data, 0, rc.PER_ITER)
    path = str(tmp_path / "state.pt")
    checkpoint.save(path, updater=first["upd"], driver=first["drv"])
    objs = rc.build_objects("trpl", DEV, torch_seed=1, driver_seed=5, form="per_step")
    upd = objs["upd"]
    checkpoint.restore(checkpoint.load(path), updater=upd, driver=objs["drv"])
    k = rc.PER_ITER * rc.UNROLL
    torch.cuda.synchronize()
    assert (upd.steps, int(upd.step_dev), int(upd.step_dev_c), int(upd.lane_flag)) == (k, k, k, k)
    assert upd._gate_for(rc.N), "the case is meant to run the gated program"
    rec, _ = rc.run_launches(objs, data, rc.PER_ITER, rc.LAUNCHES)
    assert upd._epoch is None and upd._program is not None, "the per-step program was not taken"
    rc.assert_same(rc.tail_of(ref, rc.PER_ITER), rec, "gated per-step program resumed")


def test_tracked_statistics_resume_mid_iteration(tmp_path):
    """track_stats=True, saved in the middle of the second iteration: ``stats_read()`` at its end is the uninterrupted run's, to the bit."""
    save_at = rc.PER_ITER + 2
    objs, rec, info = _resume("ppo", tmp_path, save_at, track=True)
    want = _reference("ppo", track=True)["iterations"][-1]["stats"]
    got = rec["iterations"][-1]["stats"]
    assert got["updates"] == rc.PER_ITER * rc.UNROLL and got == want, (got, want)
    assert info["at_save"]["stats"]["updates"] == 2 * rc.UNROLL
