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


def test_flat_layout_holds_the_actor_alone():
    """PolicyUpdater's layout rules on the actor's trainable parameters only: 16-byte aligned starts, p.data / p.grad views of the flat buffers."""
    from geometry_rl_amd import bc
    spec, actor = _rigid()
    want = {k: p.detach().clone() for k, p in actor.named_parameters()}
    upd = bc.BCUpdater(bc.BCLoss(actor))
    params = [p for p in actor.parameters() if p.requires_grad]
    assert [id(p) for p in upd.params] == [id(p) for p in params]
    assert upd.flat.numel() == sum((p.numel() + 3) & ~3 for p in params) == upd.gflat.numel() == upd.exp_avg.numel() == upd.exp_avg_sq.numel()
    lo, hi = upd.flat.data_ptr(), upd.flat.data_ptr() + 4 * upd.flat.numel()
    for k, p in actor.named_parameters():
        assert lo <= p.data_ptr() < hi and (p.data_ptr() - lo) % 16 == 0, k
        assert p.grad.data_ptr() - upd.gflat.data_ptr() == p.data_ptr() - lo and p.grad.shape == p.shape, k
        assert torch.equal(p.detach(), want[k]), k
    upd.release()
    for k, p in actor.named_parameters():
        assert not (lo <= p.data_ptr() < hi) and p.grad is None and torch.equal(p.detach(), want[k]), k
    with pytest.raises(RuntimeError):
        upd.step({})


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
