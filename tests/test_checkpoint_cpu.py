"""The training state without a GPU (device="cpu" objects; nothing is launched): the round trip of every object's ``state_dict`` through one
file that ``torch.load(weights_only=True)`` reads, the file as a model checkpoint, one test per refusal (with the target bitwise unchanged
behind it), the comparison helper of the GPU tests on synthetic snapshots with seeded omissions, and the ``python -m`` listing."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import resume_cases as rc
from geometry_rl_amd import agent, checkpoint, graph

SMALL = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = {
    "trpl": dict(entropy_schedule="linear", total_train_steps=64, training_noise=True, anneal_lr=True),
    "ppo": dict(algorithm="ppo", anneal_clip_epsilon=True, total_train_steps=64),
    "kl_ppo": dict(algorithm="kl_ppo", dtarg=0.01),
}
BIG = 0xDEADBEEFCAFEF00D   # a noise key above 2^63: the words are unsigned


def _build(torch_seed=0, upd_kw=None, **cfg_kw):
    cfg = agent.AgentConfig(**dict(SMALL, **cfg_kw))
    torch.manual_seed(torch_seed)
    actor, critic, proj, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    upd = agent.PolicyUpdater(loss, **dict(agent.updater_kwargs(cfg), **(upd_kw or {})))
    return dict(cfg=cfg, actor=actor, critic=critic, proj=proj, loss=loss, upd=upd)


def _fake_topology(hd, B=2):
    """A hand-made cached topology of ``B`` frames (two valid points each, a ring of internal edges): what the kNN build leaves on a GPU."""
    from geometry_rl_amd import ops
    spec = hd.spec
    main = spec.edge_types[0][0]
    n_per = {t: (4 if t == main else 1) for t in hd.node_type_list}
    n_main = 2 * B
    ei = torch.tensor([[0, 1, 2, 3][:n_main], [1, 0, 3, 2][:n_main]])
    n_types = len(spec.node_types)
    one_hot = {}
    for t in hd.node_type_list:
        oh = torch.zeros(n_main if t == main else B * n_per[t], n_types)
        oh[:, spec.node_types.index(t)] = 1
        one_hot[t] = oh
    perm = torch.tensor([1, 0, 3, 2][:n_main])
    hd._cache[B] = dict(n_per=n_per, main=main, gather_main=torch.tensor([0, 1, 4, 5][:n_main]), n_main=n_main,
                        edges={spec.edge_types[0]: ops.build_edge_set(ei, n_main, n_main)}, one_hot=one_hot, G=1,
                        n_valid=torch.full((B,), 2), permuted=True, natural_id={main: perm})


def _fill(o, seed=3):
    """Every piece of state at a value of its own."""
    upd, loss = o["upd"], o["loss"]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        upd.flat.copy_(torch.randn(upd.flat.numel(), generator=g))
        upd.exp_avg.copy_(torch.randn(upd.flat.numel(), generator=g))
        upd.exp_avg_sq.copy_(torch.rand(upd.flat.numel(), generator=g))
        upd.steps = 9
        upd.step_dev.fill_(9)
        upd._lr, upd._base_lr = 1.25e-4, 2.5e-4
        upd.lr_dev.fill_(upd._lr)
        for i, t in enumerate(loss.device_scalars.values()):
            t.fill_(0.375 + i)
        if o["proj"] is not None:
            o["proj"].initial_entropy = torch.tensor(2.625)
        if upd.track_stats:
            upd.stats_actor.copy_(torch.arange(15, dtype=torch.float64) + 0.5)
            upd.stats_critic.copy_(torch.tensor([7.25, 3.0], dtype=torch.float64))
        for i, (n, b) in enumerate(o["actor"].named_buffers()):
            if n.endswith("callibrated"):
                b.fill_(i % 2 == 0)
        for p in list(o["actor"].parameters()) + list(o["critic"].parameters()):
            if not p.requires_grad:
                p.copy_(torch.randn(p.shape, generator=g))
    o["actor"].hyper_data.set_noise_state(BIG, 17)
    o["critic"]._network1.hyper_data.set_noise_state(123, 4)
    _fake_topology(o["actor"].hyper_data)
    upd.form_by_size[8] = "per_step"


def _state(o):
    """The updater's whole state as the round trip must reproduce it (its own state_dict, plus what lives beside the saved items)."""
    upd = o["upd"]
    sd = upd.state_dict()
    sd["device_counts"] = [int(upd.step_dev), int(upd.step_dev_c), int(upd.lane_flag)]
    sd["lr_dev"] = upd.lr_dev.clone()
    sd["global_steps"] = o["loss"]._global_steps
    return sd


@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_round_trip_through_one_file(algo, tmp_path):
    a = _build(0, upd_kw=dict(track_stats=True), **ALGOS[algo])
    _fill(a)
    from geometry_rl_amd.rollout import RolloutDriver
    drv_a = RolloutDriver(a["upd"], graph.rigid_spec(), ppo_epochs=2, seed=11)
    drv_a.epoch_minibatches(8, 4, torch.device("cpu"))                      # (the generator exists and has drawn)
    path = tmp_path / "state.pt"
    checkpoint.save(path, updater=a["upd"], driver=drv_a)
    assert not [f for f in os.listdir(tmp_path) if f != "state.pt"], "the temporary file was left behind"
    state = torch.load(path, weights_only=True, map_location="cpu")        # nothing in the file needs unpickling code
    assert state["format"] == checkpoint.FORMAT and state["version"] == 1 and set(state["parts"]) == {"updater", "driver"}
    b = _build(1, upd_kw=dict(track_stats=True), **ALGOS[algo])
    drv_b = RolloutDriver(b["upd"], graph.rigid_spec(), ppo_epochs=2, seed=12)
    assert rc.differences(a["upd"].flat, b["upd"].flat)
    checkpoint.restore(checkpoint.load(path), updater=b["upd"], driver=drv_b)
    want, got = _state(a), _state(b)
    want["device_counts"] = [9, 9, 9]                                       # ONE count, everywhere
    want["global_steps"] = 9
    rc.assert_same(want, got, "round trip")
    sd = state["parts"]["updater"]
    assert sd["steps"] == 9 and sd["data"]["actor"]["noise"] == [BIG, 17] and sd["data"]["critic"]["noise"] == [123, 4]
    assert sd["form_by_size"] == {8: "per_step"} and b["upd"].form_by_size == {8: "per_step"}
    assert torch.equal(b["upd"].lr_dev, torch.full((1,), 1.25e-4)) and b["upd"].lr == 1.25e-4 and b["upd"]._base_lr == 2.5e-4
    for p in b["upd"].params:                                               # the modules' parameters are still views of ``flat``
        assert b["upd"].flat.data_ptr() <= p.data_ptr() < b["upd"].flat.data_ptr() + 4 * b["upd"].flat.numel()
    if a["proj"] is not None:
        assert float(b["proj"].initial_entropy) == 2.625 and getattr(b["proj"], "_init_host_src", None) is None
    assert b["actor"]._calib_checked is False and b["upd"]._calib_synced is True
    assert rc.latches(b["actor"]) == rc.latches(a["actor"]) and len(set(rc.latches(b["actor"]).values())) == 2
    # the sampler goes on where the saved one stood
    assert torch.equal(torch.stack(drv_a.epoch_minibatches(8, 4, torch.device("cpu"))), torch.stack(drv_b.epoch_minibatches(8, 4, torch.device("cpu"))))
    # the topology is installed as the arrays it was saved from
    ta, tb = a["actor"].hyper_data._cache[2], b["actor"].hyper_data._cache[2]
    ea, eb = ta["edges"][graph.rigid_spec().edge_types[0]], tb["edges"][graph.rigid_spec().edge_types[0]]
    rc.assert_same({k: v for k, v in vars(ea).items()}, {k: v for k, v in vars(eb).items()}, "edge set")
    rc.assert_same({k: ta[k] for k in ("n_per", "main", "gather_main", "n_main", "one_hot", "G", "n_valid", "permuted", "natural_id")},
                   {k: tb[k] for k in ("n_per", "main", "gather_main", "n_main", "one_hot", "G", "n_valid", "permuted", "natural_id")}, "topology")


def test_advisory_form_table_is_kept_where_the_loader_has_measured():
    a, b = _build(0), _build(1)
    _fill(a)
    b["upd"].form_by_size[8] = "unrolled"
    b["upd"].load_state_dict(a["upd"].state_dict())
    assert b["upd"].form_by_size == {8: "unrolled"}


def test_state_behind_a_failed_update_is_refused():
    a = _build(0)
    a["upd"].steps = 3                     # (the device-side count says 0)
    with pytest.raises(RuntimeError, match="cannot be resumed"):
        a["upd"].state_dict()


def test_file_is_a_reference_checkpoint(tmp_path):
    a = _build(0, **ALGOS["ppo"])
    _fill(a)
    checkpoint.save(tmp_path / "s.pt", updater=a["upd"])
    model = checkpoint.load(tmp_path / "s.pt")["model"]
    assert set(model) == {"env", "actor", "critic", "reward"} and all(k.startswith(agent.ACTOR_PREFIX) for k in model["actor"])
    b = _build(1, **ALGOS["ppo"])
    agent.load_reference_checkpoint(model, b["actor"], b["critic"], strict=True)
    for mod_a, mod_b in ((a["actor"], b["actor"]), (a["critic"], b["critic"])):
        sa, sb = mod_a.state_dict(), mod_b.state_dict()
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------------------- refusals
def _refused(target, sd, match):
    before = _state(target)
    with pytest.raises(ValueError, match=match):
        target["upd"].load_state_dict(sd)
    rc.assert_same(before, _state(target), "the target of a refused load")


def _saved(**kw):
    a = _build(0, **kw)
    _fill(a)
    return a["upd"].state_dict()


def test_refuses_another_layout():
    _refused(_build(1, output_dim=1), _saved(), "layout")


def test_refuses_another_algorithm():
    _refused(_build(1, algorithm="ppo"), _saved(), "algorithm")
    _refused(_build(1, proj_type="w2"), _saved(), "algorithm")
    _refused(_build(1, entropy_schedule="linear", total_train_steps=64), _saved(), "algorithm")


@pytest.mark.parametrize("name, kw", [("eps", dict(eps=1e-8)), ("betas", dict(betas=(0.8, 0.999))), ("clip", dict(clip_grad_norm=True)),
                                      ("max_norm", dict(max_grad_norm=0.5)), ("anneals_lr", dict(anneal_lr=True, total_network_updates=64)),
                                      ("total_network_updates", dict(total_network_updates=32)), ("track_stats", dict(track_stats=True))])
def test_refuses_another_hyper_parameter(name, kw):
    saved = _build(0, upd_kw=dict(total_network_updates=64))
    _fill(saved)
    _refused(_build(1, upd_kw=dict(dict(total_network_updates=64), **kw)), saved["upd"].state_dict(), name)


def test_refuses_another_epsilon_schedule():
    _refused(_build(1, algorithm="ppo", anneal_clip_epsilon=True, total_train_steps=64), _saved(algorithm="ppo", total_train_steps=64), "anneals_eps")


@pytest.mark.parametrize("key, value", [("rank", 1), ("world", 2)])
def test_refuses_another_rank_or_world(key, value):
    sd = _saved()
    sd[key] = value
    _refused(_build(1), sd, "rank")


def test_refuses_another_version(tmp_path):
    sd = _saved()
    sd["version"] = 2
    _refused(_build(1), sd, "version")
    a = _build(0)
    state = checkpoint.save(tmp_path / "s.pt", updater=a["upd"])
    with pytest.raises(ValueError, match="version"):
        checkpoint.restore(dict(state, version=2), updater=a["upd"])
    torch.save(dict(state, version=2), tmp_path / "v2.pt")
    with pytest.raises(ValueError, match="version"):
        checkpoint.load(tmp_path / "v2.pt")
    torch.save({"actor": {}}, tmp_path / "other.pt")
    with pytest.raises(ValueError, match="not a training-state file"):
        checkpoint.load(tmp_path / "other.pt")


def test_refuses_a_topology_built_from_another_first_batch():
    sd = _saved()
    b = _build(1)
    _fake_topology(b["actor"].hyper_data)
    b["actor"].hyper_data._cache[2]["gather_main"] = torch.tensor([0, 2, 4, 6])
    _refused(b, sd, "reset_cache")


def test_refuses_a_missing_and_an_unrequested_part(tmp_path):
    from geometry_rl_amd.rollout import RolloutDriver
    a, b = _build(0), _build(1)
    _fill(a)
    drv = RolloutDriver(b["upd"], graph.rigid_spec(), seed=1)
    state = checkpoint.save(tmp_path / "s.pt", updater=a["upd"])
    before = _state(b)
    with pytest.raises(ValueError, match="holds no part"):
        checkpoint.restore(state, updater=b["upd"], driver=drv)
    state = checkpoint.save(tmp_path / "s.pt", updater=a["upd"], driver=RolloutDriver(a["upd"], graph.rigid_spec(), seed=1))
    with pytest.raises(ValueError, match="not asked for"):
        checkpoint.restore(state, updater=b["upd"])
    rc.assert_same(before, _state(b), "the target of a refused restore")


# ------------------------------------------------------------------------------------------------------------- the other objects
def test_driver_saves_the_seed_until_it_has_drawn():
    from geometry_rl_amd.rollout import RolloutDriver
    a, b = _build(0), _build(1)
    d1, d2 = RolloutDriver(a["upd"], graph.rigid_spec(), seed=4), RolloutDriver(b["upd"], graph.rigid_spec(), seed=5)
    sd = d1.state_dict()
    assert sd["generator"]["state"] is None and sd["generator"]["seed"] == 4
    d2.load_state_dict(sd)
    assert d2.gen is None and d2.seed == 4
    cpu = torch.device("cpu")
    assert torch.equal(torch.stack(d1.epoch_minibatches(8, 4, cpu)), torch.stack(d2.epoch_minibatches(8, 4, cpu)))
    with pytest.raises(ValueError, match="ppo_epochs"):
        RolloutDriver(b["upd"], graph.rigid_spec(), ppo_epochs=3).load_state_dict(sd)


def test_collector_normaliser_and_episode_statistics_round_trip():
    from geometry_rl_amd.rollout import EpisodeStats, PolicyActor
    from geometry_rl_amd.transforms import ObservationNormalizer
    a, b = _build(0), _build(1)
    p1, p2 = PolicyActor(a["actor"], graph.rigid_spec(), seed=3), PolicyActor(b["actor"], graph.rigid_spec(), seed=8)
    p1.gen, p1._calls = torch.Generator().manual_seed(3), 6
    torch.rand(5, generator=p1.gen)
    p2._graph = object()
    p2.load_state_dict(p1.state_dict())
    assert p2._calls == 6 and p2._graph is None and p2._resumed and p2.gen is not p1.gen and torch.equal(p2.gen.get_state(), p1.gen.get_state())
    with pytest.raises(ValueError, match="deterministic"):
        PolicyActor(b["actor"], graph.rigid_spec(), deterministic=True).load_state_dict(p1.state_dict())
    n1, n2 = ObservationNormalizer(device="cpu"), ObservationNormalizer(device="cpu")
    n1.state = {"position_vectors": torch.arange(7.0), "scalars": torch.arange(3.0) + 0.5}
    n2.state = {"position_vectors": torch.zeros(7), "stale": torch.zeros(3)}
    kept = n2.state["position_vectors"]
    n2.load_state_dict(n1.state_dict())
    rc.assert_same(n1.state, n2.state, "normaliser")
    assert n2.state["position_vectors"] is kept                            # in place where the storage exists
    with pytest.raises(ValueError, match="decay"):
        ObservationNormalizer(decay=0.5, device="cpu").load_state_dict(n1.state_dict())
    e1, e2 = EpisodeStats(4, "cpu"), EpisodeStats(4, "cpu")
    e1.ret_state.copy_(torch.tensor([1.5, -2.0, 0.0, 3.25]))
    e1.len_state.copy_(torch.tensor([3, 1, 0, 7], dtype=torch.int32))
    e1.sums.copy_(torch.tensor([4.5, 9.0, 2.0], dtype=torch.float64))
    e2.load_state_dict(e1.state_dict())
    rc.assert_same([e1.ret_state, e1.len_state, e1.sums], [e2.ret_state, e2.len_state, e2.sums], "episode statistics")
    with pytest.raises(ValueError, match="environments"):
        EpisodeStats(5, "cpu").load_state_dict(e1.state_dict())


def test_behaviour_cloning_round_trip(tmp_path):
    from geometry_rl_amd import bc
    from geometry_rl_amd.rollout import RolloutBuffer
    spec = graph.rigid_spec()

    def make(torch_seed, seed):
        torch.manual_seed(torch_seed)
        actor, *_ = agent.build_agent(spec, agent.AgentConfig(**SMALL), device="cpu")
        upd = bc.BCUpdater(bc.BCLoss(actor, objective="nll"), use_graph=False)
        data = {k: torch.zeros(10, 4, sum(spec.obs_dims[k.replace("norm_", "")])) for k in spec.in_features}
        data["action"] = torch.zeros(10, 4, 6)
        return actor, upd, bc.BehaviorCloner(upd, spec, RolloutBuffer(data), mini_batch_size=8, seed=seed)

    a_actor, a_upd, a_cl = make(0, 5)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for t in (a_upd.flat, a_upd.exp_avg, a_upd.exp_avg_sq):
            t.copy_(torch.rand(t.numel(), generator=g))
        a_upd.steps = 6
        a_upd.step_dev.fill_(6)
        a_upd.stats.copy_(torch.arange(15, dtype=torch.float64))
    a_upd.lr = 1e-3
    a_cl.epoch_minibatches()
    a_cl.epochs_done = 3
    checkpoint.save(tmp_path / "bc.pt", updater=a_upd, cloner=a_cl)
    state = checkpoint.load(tmp_path / "bc.pt")
    assert set(state["model"]) == {"env", "actor", "reward"}               # (no critic: still loads as a model checkpoint)
    b_actor, b_upd, b_cl = make(1, 6)
    checkpoint.restore(state, updater=b_upd, cloner=b_cl)
    agent.load_reference_checkpoint(state["model"], make(2, 0)[0], strict=True)
    rc.assert_same(a_upd.state_dict(), b_upd.state_dict(), "BCUpdater")
    assert (b_upd.steps, int(b_upd.step_dev), b_upd.lr, float(b_upd.lr_dev)) == (6, 6, 1e-3, float(torch.tensor(1e-3, dtype=torch.float32)))
    assert b_cl.epochs_done == 3 and torch.equal(torch.stack(a_cl.epoch_minibatches()), torch.stack(b_cl.epoch_minibatches()))
    other = bc.BCUpdater(bc.BCLoss(make(3, 0)[0], objective="mse"), use_graph=False)
    before = other.state_dict()
    with pytest.raises(ValueError, match="objective"):
        other.load_state_dict(a_upd.state_dict())
    rc.assert_same(before, other.state_dict(), "the target of a refused load")


# ------------------------------------------------------------------------------------------------------------- the comparison helper
def _recording():
    """A synthetic recording of the shape resume_cases.run_launches returns: two steps, one iteration."""
    gen = torch.Generator().manual_seed(7)
    seed_state = gen.get_state().clone()
    torch.rand(3, generator=gen)
    snap = {"flat": torch.arange(6.0), "exp_avg": torch.arange(6.0) * 0.5, "exp_avg_sq": torch.arange(6.0) ** 2,
            "noise": {"actor": (BIG, 5), "critic": (9, 0)}, "lr": 3e-4, "scalars": {"kl_beta": torch.tensor(2.0)},
            "steps": {"host": 8, "step_dev": 8, "step_dev_c": 8}, "initial_entropy": torch.tensor(1.5), "generator": gen.get_state().clone(),
            "latches": {"conv.callibrated": True}}
    return {"outs": [{"kl": torch.tensor(0.25)}, {"kl": torch.tensor(0.5)}], "iterations": [snap]}, seed_state


def _omit(what, rec, seed_state):
    snap = rec["iterations"][0]
    if what == "a zeroed draw counter":
        snap["noise"]["actor"] = (BIG, 0)
        return "iterations[0].noise.actor"
    if what == "a step count left at 0":
        snap["steps"]["step_dev_c"] = 0
        return "iterations[0].steps.step_dev_c"
    if what == "a missing exp_avg_sq":
        del snap["exp_avg_sq"]
        return "iterations[0].exp_avg_sq"
    if what == "an unlatched initial entropy":
        snap["initial_entropy"] = None
        return "iterations[0].initial_entropy"
    if what == "a generator left at its seed":
        snap["generator"] = seed_state
        return "iterations[0].generator"
    if what == "one step's loss in the last bit":
        rec["outs"][1]["kl"] = torch.nextafter(rec["outs"][1]["kl"], torch.tensor(1.0))
        return "outs[1].kl"
    if what == "a moment of another dtype":
        snap["exp_avg"] = snap["exp_avg"].double()
        return "iterations[0].exp_avg"
    raise KeyError(what)


def test_comparison_helper_passes_equal_recordings():
    a, _ = _recording()
    b, _ = _recording()
    assert rc.differences(a, b) == []
    rc.assert_same(a, b, "equal")


@pytest.mark.parametrize("what", ["a zeroed draw counter", "a step count left at 0", "a missing exp_avg_sq", "an unlatched initial entropy",
                                  "a generator left at its seed", "one step's loss in the last bit", "a moment of another dtype"])
def test_comparison_helper_reports_each_omission(what):
    a, _ = _recording()
    b, seed_state = _recording()
    where = _omit(what, b, seed_state)
    for x, y in ((a, b), (b, a)):
        diff = rc.differences(x, y)
        assert len(diff) == 1 and diff[0].startswith("run." + where), diff
        with pytest.raises(AssertionError, match="run"):
            rc.assert_same(x, y, "run")
    assert rc.differences(a, copy.deepcopy(a)) == []


# ------------------------------------------------------------------------------------------------------------- the listing
def test_listing_names_every_part(tmp_path):
    from geometry_rl_amd.rollout import EpisodeStats, RolloutDriver
    a = _build(0, **ALGOS["trpl"])
    _fill(a)
    path = tmp_path / "state.pt"
    checkpoint.save(path, updater=a["upd"], driver=RolloutDriver(a["upd"], graph.rigid_spec(), seed=1), episodes=EpisodeStats(4, "cpu"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-m", "geometry_rl_amd.checkpoint", str(path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    text = out.stdout
    for part in ("updater", "driver", "episodes", "model"):
        assert f"part {part}:" in text, text[:2000]
    assert "step count 9" in text and "loss=TRPLLoss" in text and "projection=kl" in text and "rank 0 of 1" in text
    n = a["upd"].flat.numel()
    assert f"updater.flat: float32 [{n}]" in text and f"updater.exp_avg_sq: float32 [{n}]" in text and "episodes.sums: float64 [3]" in text
    total = int(text.strip().splitlines()[-1].split()[1])
    assert total >= 3 * 4 * n and total <= os.path.getsize(path)
