"""The behaviour-cloning driver without a GPU (geometry_rl_amd.bc on device="cpu" objects; nothing is launched): the split by environment,
both samplers (every training row exactly once per epoch, the short last minibatch kept or dropped), the ragged-task guard, and what the
three classes refuse."""
import pytest
import torch


def _agent(spec, **kw):
    from geometry_rl_amd import agent
    torch.manual_seed(0)
    return agent.build_agent(spec, agent.AgentConfig(**kw), device="cpu")


def _rigid():
    from geometry_rl_amd import graph
    spec = graph.rigid_spec()
    return spec, _agent(spec, only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)[0]


def _cloth():
    from geometry_rl_amd import graph
    spec = graph.cloth_spec(n_particles=25, E_cloth=40)
    return spec, _agent(spec)[0]


def _buffer(spec, N, T, A):
    """[N, T] zeros of the right widths: the samplers never read the data."""
    from geometry_rl_amd.rollout import RolloutBuffer
    data = {k: torch.zeros(N, T, sum(spec.obs_dims[k.replace("norm_", "")])) for k in spec.in_features}
    data["action"] = torch.zeros(N, T, A)
    return RolloutBuffer(data)


def _cloner(N=5, T=8, mbs=12, **kw):
    from geometry_rl_amd import bc
    spec, actor = _cloth()
    upd = bc.BCUpdater(bc.BCLoss(actor), use_graph=False)
    return bc.BehaviorCloner(upd, spec, _buffer(spec, N, T, 12), mini_batch_size=mbs, **kw)


def test_defaults_follow_the_reference():
    from geometry_rl_amd import bc
    spec, actor = _cloth()
    loss = bc.BCLoss(actor)
    upd = bc.BCUpdater(loss)
    assert loss.objective == "mse" and loss.out_keys == ["loss_bc", "mse", "nll", "entropy", "max_sq_err"] and loss.in_features == spec.in_features
    assert (upd.lr, upd.eps, upd.betas, upd.clip) == (5e-4, 1e-8, (0.9, 0.999), False)   # torch.optim.Adam(lr=5e-4): eps is NOT the RL loop's 1e-5
    import geometry_rl_amd
    assert geometry_rl_amd.BCLoss is bc.BCLoss


@pytest.mark.parametrize("which", ["bc", "policy"])
def test_flat_layout_holds_the_actor_alone(which):
    """FlatUpdater's layout rules under both updaters -- BCUpdater on the actor's trainable parameters only, PolicyUpdater on the actor's
    followed by the critic's: 16-byte aligned starts, p.data / p.grad views of the flat buffers at one offset, the values kept."""
    from geometry_rl_amd import agent, bc, graph
    if which == "bc":
        spec, actor = _rigid()
        nets = {"actor": actor}
    else:
        torch.manual_seed(0)
        actor, critic, _, loss = agent.build_agent(graph.rigid_spec(), agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2),
                                                   device="cpu")
        nets = {"actor": actor, "critic": critic}
    named = [(f"{n}.{k}", p) for n, net in nets.items() for k, p in net.named_parameters() if p.requires_grad]
    want = {k: p.detach().clone() for k, p in named}
    upd = bc.BCUpdater(bc.BCLoss(actor)) if which == "bc" else agent.PolicyUpdater(loss)
    pad4 = lambda k: (k + 3) & ~3
    assert [id(p) for p in upd.params] == [id(p) for _, p in named]
    assert upd.flat.numel() == sum(pad4(p.numel()) for _, p in named) == upd.gflat.numel() == upd.exp_avg.numel() == upd.exp_avg_sq.numel()
    if which == "policy":
        assert upd.n_actor == sum(pad4(p.numel()) for p in actor.parameters() if p.requires_grad)
        assert upd.gbuf.numel() - upd.gflat.numel() == 28                  # one rank's loss record in front of the gradient
        assert upd.gflat.data_ptr() - upd.gbuf.data_ptr() == 4 * 28
    lo, hi = upd.flat.data_ptr(), upd.flat.data_ptr() + 4 * upd.flat.numel()
    for k, p in named:
        assert lo <= p.data_ptr() < hi and (p.data_ptr() - lo) % 16 == 0, k
        assert p.grad.data_ptr() - upd.gflat.data_ptr() == p.data_ptr() - lo and p.grad.shape == p.shape, k
        assert torch.equal(p.detach(), want[k]), k
    upd.release()
    for k, p in named:
        assert not (lo <= p.data_ptr() < hi) and p.grad is None and torch.equal(p.detach(), want[k]), k
    if which == "bc":
        with pytest.raises(RuntimeError):
            upd.step({})


def test_both_updaters_take_the_overwrite_rule_from_flat():
    """``flat.fold_overwrite`` is the ONE rule: HEPi overwrites, the attention gate as torch modules accumulates, on HIP kernels it
    overwrites, the transformer actor accumulates -- and both constructors give what the function gives."""
    from geometry_rl_amd import agent, bc, flat, graph
    small = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    cases = [(dict(small), True), (dict(small, aggr="AttentionalAggregation"), False),
             (dict(small, aggr="AttentionalAggregation", attention_gate="hip"), True), (dict(small, model="transformer"), False)]
    for kw, want in cases:
        made = []
        for _ in range(2):   # (an actor is laid out by one updater at a time)
            torch.manual_seed(0)
            made.append(agent.build_agent(graph.rigid_spec(), agent.AgentConfig(**kw), device="cpu"))
        (actor_p, _, _, loss_p), (actor_b, *_) = made
        assert flat.fold_overwrite(actor_p) is want, kw
        p_upd, b_upd = agent.PolicyUpdater(loss_p), bc.BCUpdater(bc.BCLoss(actor_b))
        assert p_upd._fold_overwrite is b_upd._fold_overwrite is want, kw
        assert p_upd._overwrite_checked is b_upd._overwrite_checked is (not want), kw
    assert not hasattr(bc, "fold_overwrite")


def test_cloner_and_driver_share_one_sampler():
    """N = 4, T = 6, minibatches of 8 (k = 2 permutation columns), seed 3: over two consecutive epochs ``BehaviorCloner`` with every
    environment training and ``RolloutDriver`` hand out the same index tensors, element for element -- one sampler, one draw order."""
    from types import SimpleNamespace
    from geometry_rl_amd.rollout import RolloutDriver
    c = _cloner(N=4, T=6, mbs=8, train_fraction=1.0, seed=3)
    drv = RolloutDriver(SimpleNamespace(flat=torch.zeros(1)), c.spec, mini_batch_size=8, seed=3)
    for _ in range(2):
        mine, theirs = c.epoch_minibatches(), drv.epoch_minibatches(4, 6, "cpu")
        assert [i.tolist() for i in mine] == [i.tolist() for i in theirs] and len(mine) == 3 and all(i.numel() == 8 for i in mine)


def test_split_by_environment():
    """The reference's first 80 % of the row-major [N, T] rollout: the first int(0.8 N) environments train, the others are held out."""
    c = _cloner(N=5, T=8)
    assert c.n_train == 4
    assert c.train_rows().tolist() == list(range(32))
    held = c.heldout_rows()
    assert sorted(held.tolist()) == list(range(32, 40)) and set((held // 8).tolist()) == {4}
    c7 = _cloner(N=7, T=3, mbs=5, sampling="uniform")
    assert c7.n_train == 5 and sorted(c7.heldout_rows().tolist()) == list(range(15, 21))
    assert (c7.heldout_rows() // 3).tolist() == [5, 6] * 3   # time step after time step: row i belongs to held-out environment i mod 2
    assert _cloner(N=5, T=8, train_fraction=1.0, mbs=5).evaluate() == {}


@pytest.mark.parametrize("sampling,mbs,sizes", [("uniform", 12, [12, 12, 8]), ("env_aligned", 12, [12, 12, 8]), ("env_aligned", 8, [8] * 4),
                                                ("uniform", 32, [32]), ("uniform", 5, [5] * 6 + [2])])
def test_every_training_row_once_per_epoch(sampling, mbs, sizes):
    c = _cloner(N=5, T=8, mbs=mbs, sampling=sampling, seed=3)
    epochs = [c.epoch_minibatches() for _ in range(3)]
    for mb in epochs:
        assert [int(i.numel()) for i in mb] == sizes
        assert all(i.dtype == torch.int64 for i in mb)
        assert sorted(torch.cat(mb).tolist()) == list(range(32))           # the 4 training environments' rows, each exactly once
        if sampling == "env_aligned":                                      # row i of every minibatch belongs to environment i mod n_train
            for i in mb:
                assert ((i // 8) == torch.arange(i.numel()) % 4).all()
    assert not torch.equal(torch.cat(epochs[0]), torch.cat(epochs[1]))     # a fresh permutation per epoch
    again = _cloner(N=5, T=8, mbs=mbs, sampling=sampling, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(again.epoch_minibatches(), epochs[0]))   # ... reproducible from the seed


@pytest.mark.parametrize("sampling", ["uniform", "env_aligned"])
def test_drop_last(sampling):
    c = _cloner(N=5, T=8, mbs=12, sampling=sampling, drop_last=True)
    mb = c.epoch_minibatches()
    assert [int(i.numel()) for i in mb] == [12, 12]
    assert len(set(torch.cat(mb).tolist())) == 24
    full = _cloner(N=5, T=8, mbs=8, sampling=sampling, drop_last=True)
    assert [int(i.numel()) for i in full.epoch_minibatches()] == [8] * 4     # nothing short: nothing dropped


def test_ragged_guard():
    """Uniform sampling is refused where the topology depends on the row (rigid: object_num_points), exactly as RolloutDriver refuses it."""
    from geometry_rl_amd import bc, graph
    spec, actor = _rigid()
    upd = bc.BCUpdater(bc.BCLoss(actor), use_graph=False)
    buf = _buffer(spec, 5, 4, 6)
    with pytest.raises(ValueError, match="allow_stale_topology"):
        bc.BehaviorCloner(upd, spec, buf, mini_batch_size=4, sampling="uniform")
    bc.BehaviorCloner(upd, spec, buf, mini_batch_size=4, sampling="uniform", allow_stale_topology=True)
    bc.BehaviorCloner(upd, spec, buf, mini_batch_size=4, sampling="env_aligned")
    assert "object_num_points" in graph.rigid_spec().obs_names["infos"]
    _cloner(sampling="uniform")   # cloth: one topology for every row


def test_refusals():
    from geometry_rl_amd import bc
    spec, actor = _cloth()
    with pytest.raises(ValueError, match="mse"):
        bc.BCLoss(actor, objective="huber")
    with pytest.raises(NotImplementedError, match="one rank"):
        bc.BCLoss(actor, group=object())
    with pytest.raises(NotImplementedError, match="one rank"):
        bc.BCUpdater(bc.BCLoss(actor), group=object())
    with pytest.raises(ValueError, match="multiple"):
        _cloner(N=5, T=8, mbs=10, sampling="env_aligned")    # 4 training environments
    _cloner(N=5, T=8, mbs=10, sampling="uniform")
    with pytest.raises(ValueError):
        _cloner(sampling="sequential")
    with pytest.raises(ValueError):
        _cloner(N=1, T=8, mbs=1)                             # int(0.8 * 1) = 0 environments to train on
    upd = bc.BCUpdater(bc.BCLoss(actor), use_graph=False)
    with pytest.raises(KeyError, match="action"):
        upd.step({k: torch.zeros(2, 1) for k in spec.in_features})
