"""``BCUpdater`` / ``BehaviorCloner`` in their forms, and the hand-over to ``PolicyUpdater`` -- every comparison BITWISE:
  * three steps eager == three steps recorded, at two minibatch sizes inside one updater, per actor family (fp32 HEPi, bf16 rope HEPi, EMPN
    with key / query attention, HEPi's attention gate on HIP kernels, the transformer actor on HIP kernels; the stock-torch transformer
    runs eagerly only); with training noise: both draw the same noise;
  * ``run_minibatches`` over an epoch == the loop of ``step_from``; a second updater from the same seed repeats the first;
  * ``fit``: the epoch means are the float64 means of the same steps issued by hand, the held-out report is ``evaluate``'s;
  * two BC steps, ``release()``, a ``PolicyUpdater`` on the same actor, one TRPL step == a freshly built agent loaded with the state_dict
    saved after the two BC steps, one TRPL step."""
import pytest
import torch

from geometry_rl_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("loss_bc", "mse", "nll", "entropy", "max_sq_err", "loc", "sigma")
RIGID2 = dict(G=2, angular_velocity=False, object_velocity=False)
HEMI = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)


def _specs():
    from geometry_rl_amd import graph
    return {
        "rigid_g1": (graph.rigid_spec, HEMI, lambda B, s: syn.make_rigid_obs(B, seed=s)),
        "rope_bf16": (lambda: graph.rope_spec(n_links=20), dict(dim=2, precision="bf16"), lambda B, s: syn.make_rope_obs(B, n_links=20, seed=s)),
        "empn_attention": (lambda: graph.rigid_spec(**RIGID2), dict(model="empn", attention=True), lambda B, s: syn.make_rigid_obs(B, seed=s, **RIGID2)),
        "gate_hip": (lambda: graph.rigid_spec(**RIGID2), dict(aggr="AttentionalAggregation", attention_gate="hip"),
                     lambda B, s: syn.make_rigid_obs(B, seed=s, **RIGID2)),
        "transformer_hip": (graph.rigid_spec, dict(model="transformer", output_dim=2, output_dim_vec=2, transformer_kernels="hip"),
                            lambda B, s: syn.make_rigid_obs(B, seed=s)),
        "transformer_torch": (graph.rigid_spec, dict(model="transformer", output_dim=2, output_dim_vec=2), lambda B, s: syn.make_rigid_obs(B, seed=s)),
        "cloth": (lambda: graph.cloth_spec(n_particles=25, E_cloth=40), {}, lambda B, s: syn.make_cloth_obs(B, n_particles=25, E_cloth=40, seed=s)),
    }


def build(case, **cfg_kw):
    """-> (spec, cfg, (actor, critic, proj, loss), obs(B, seed), action width) of a fresh agent from seed 0"""
    from geometry_rl_amd import agent
    make_spec, kw, obs = _specs()[case]
    spec = make_spec()
    cfg = agent.AgentConfig(**dict(kw, **cfg_kw))
    torch.manual_seed(0)
    built = agent.build_agent(spec, cfg, device=DEV)
    return spec, cfg, built, obs, spec.num_actuators * cfg.output_dim_vec * 3


def batch_of(obs, B, A, seed, keys):
    b = dict(obs(B, seed))
    b["action"] = syn.make_ppo_fields(B, A, seed=seed)["action"]
    return {k: b[k].to(DEV) for k in list(keys) + ["action"]}


def buffer_of(obs, N, T, A, seed, keys):
    from geometry_rl_amd.rollout import RolloutBuffer
    frames = [batch_of(obs, N, A, seed + t, keys) for t in range(T)]   # (one frame set per time step: same environments, same point counts)
    return RolloutBuffer({k: torch.stack([f[k] for f in frames], dim=1) for k in frames[0]})


def keep(out):
    return {k: out[k].detach().clone() for k in KEYS}


def state(upd, outs):
    torch.cuda.synchronize()
    return {"flat": upd.flat.clone(), "exp_avg": upd.exp_avg.clone(), "exp_avg_sq": upd.exp_avg_sq.clone(), "steps": upd.step_dev.clone(),
            "stats": upd.stats.clone(), "outs": outs}


def assert_same(a, b):
    for k in ("flat", "exp_avg", "exp_avg_sq", "steps", "stats"):
        assert torch.equal(a[k], b[k]), k
    assert len(a["outs"]) == len(b["outs"])
    for i, (oa, ob) in enumerate(zip(a["outs"], b["outs"])):
        for k in KEYS:
            assert torch.equal(oa[k], ob[k]), (i, k)


def run_steps(case, use_graph, objective="mse", sizes=(8, 5), steps=3, clip=False, **cfg_kw):
    """``steps`` updates at each size, the sizes taking turns, through ONE updater -> (its final state, the updater)."""
    from geometry_rl_amd import bc
    spec, cfg, (actor, *_), obs, A = build(case, **cfg_kw)
    loss = bc.BCLoss(actor, objective=objective)
    upd = bc.BCUpdater(loss, clip_grad_norm=clip, use_graph=use_graph)
    outs = []
    for t in range(steps):
        for B in sizes:
            outs.append(keep(upd.step(batch_of(obs, B, A, 50 + t, loss.in_features))))
    assert upd.steps == steps * len(sizes)
    return state(upd, outs), upd


@pytest.mark.parametrize("case,objective", [("rigid_g1", "mse"), ("rope_bf16", "nll"), ("empn_attention", "mse"), ("gate_hip", "nll"),
                                            ("transformer_hip", "nll")])
def test_eager_equals_recorded_at_two_sizes(case, objective):
    eager, upd_e = run_steps(case, False, objective)
    graph, upd_g = run_steps(case, True, objective)
    assert upd_e.mode == "eager" and not upd_e._programs
    assert upd_g.mode == "graph" and sorted(upd_g._programs) == [5, 8]   # one program per minibatch size, both alive
    assert all(e.kind == "graph" for B in (5, 8) for e in upd_g._programs[B][0]) and all(len(upd_g._programs[B][0]) == 1 for B in (5, 8))
    assert_same(eager, graph)
    assert not torch.equal(eager["outs"][0]["loss_bc"], eager["outs"][-1]["loss_bc"])


def test_stock_torch_transformer_runs_eagerly():
    a, upd = run_steps("transformer_torch", True, "mse", sizes=(8,), steps=2)
    assert upd.mode.startswith("eager") and not upd._programs and not upd.use_graph
    b, _ = run_steps("transformer_torch", False, "mse", sizes=(8,), steps=2)
    assert_same(a, b)


def test_clipped_update_eager_equals_recorded():
    assert_same(run_steps("rope_bf16", False, "nll", sizes=(8,), clip=True)[0], run_steps("rope_bf16", True, "nll", sizes=(8,), clip=True)[0])


def test_training_noise_eager_and_recorded_draw_the_same_noise():
    noisy_e = run_steps("rigid_g1", False, sizes=(8,), training_noise=True)[0]
    noisy_g = run_steps("rigid_g1", True, sizes=(8,), training_noise=True)[0]
    clean = run_steps("rigid_g1", False, sizes=(8,))[0]
    assert_same(noisy_e, noisy_g)
    assert not torch.equal(noisy_e["outs"][-1]["loc"], clean["outs"][-1]["loc"])   # (the noise is on: another trajectory)


def _epoch(form, objective="mse"):
    """One epoch of env-aligned minibatches (N = 8, T = 6, 8 frames each: all 8 environments train) through ``form``."""
    from geometry_rl_amd import bc
    spec, cfg, (actor, *_), obs, A = build("rigid_g1")
    loss = bc.BCLoss(actor, objective=objective)
    upd = bc.BCUpdater(loss, use_graph=True)
    buf = buffer_of(obs, 8, 6, A, 70, loss.in_features)
    cl = bc.BehaviorCloner(upd, spec, buf, mini_batch_size=8, train_fraction=1.0, seed=5)
    rows = cl.epoch_minibatches()
    assert len(rows) == 6
    if form == "loop":
        outs = [keep(upd.step_from(buf, r)) for r in rows]
    else:
        outs = [keep(upd.run_minibatches(buf, torch.stack(rows)))]
    assert 8 in upd._programs
    return state(upd, outs)


def test_run_minibatches_is_the_loop_of_step_from_and_repeats():
    loop, launches, again = _epoch("loop"), _epoch("launches"), _epoch("loop")
    assert_same(loop, again)   # a second updater from the same seed repeats the first bit for bit
    last = dict(loop, outs=loop["outs"][-1:])
    assert_same(last, launches)


def test_fit_means_and_heldout_report():
    """cloth, N = 5, T = 8, mini_batch_size = 12, uniform: 32 training rows give 12, 12, 8 and 8 rows are held out."""
    from geometry_rl_amd import bc

    def make():
        spec, cfg, (actor, *_), obs, A = build("cloth")
        loss = bc.BCLoss(actor, objective="nll")
        upd = bc.BCUpdater(loss, use_graph=True)
        buf = buffer_of(obs, 5, 8, A, 90, loss.in_features)
        return upd, bc.BehaviorCloner(upd, spec, buf, mini_batch_size=12, sampling="uniform", seed=2)

    upd, cl = make()
    hist = cl.fit(epochs=2, eval_every=1)
    after = cl.evaluate()
    assert upd.steps == 6 and sorted(upd._eager_sizes) == [8, 12]
    assert list(hist["eval"]) == [1] and hist["eval"][1] == after and set(after) == set(upd.loss_module.out_keys)
    assert len(hist["loss"]) == 2 and [m["updates"] for m in hist["train"]] == [3, 3]

    upd2, cl2 = make()   # the same steps issued by hand
    for epoch in range(2):
        rows = cl2.epoch_minibatches()
        assert [int(r.numel()) for r in rows] == [12, 12, 8]
        outs = [keep(upd2.step_from(cl2.data, r)) for r in rows]
        for k in upd.loss_module.out_keys:
            want = sum(float(o[k]) for o in outs) / len(outs)   # float64, in issue order: what the running sums hold
            assert hist["train"][epoch][k] == want, (epoch, k, hist["train"][epoch][k], want)
        assert hist["loss"][epoch] == hist["train"][epoch]["loss_bc"]
    held = upd2.evaluate(cl2.data, cl2.heldout_rows())
    assert {k: float(held[k]) for k in upd.loss_module.out_keys} == after
    assert sorted((cl2.heldout_rows() // 8).unique().tolist()) == [4]
    torch.cuda.synchronize()
    assert torch.equal(upd.flat, upd2.flat)   # evaluate updates nothing


def test_evaluate_changes_nothing_and_takes_no_noise():
    from geometry_rl_amd import bc
    spec, cfg, (actor, *_), obs, A = build("rigid_g1", training_noise=True)
    loss = bc.BCLoss(actor)
    upd = bc.BCUpdater(loss, use_graph=False)
    buf = buffer_of(obs, 8, 2, A, 70, loss.in_features)
    upd.step_from(buf, torch.arange(8, device=DEV) * 2)   # every environment's first frame (row = environment * T + time step)
    before = state(upd, [])
    idx = torch.arange(8, device=DEV) * 2 + 1               # ... and its second
    a, b = upd.evaluate(buf, idx), upd.evaluate(buf, idx)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k   # train=False: no training noise, the same report twice
    assert_same(before, state(upd, []))
    assert actor.training


def test_handover_to_policy_updater():
    """A: two BC steps, release(), PolicyUpdater on the same actor, one TRPL step.  B: a freshly built agent loaded with the state_dict
    saved after the two BC steps, one TRPL step.  Outputs and every parameter agree bit for bit."""
    from geometry_rl_amd import agent, bc
    B = 8

    def trpl_step(spec, cfg, actor, critic, loss, obs, A):
        batch = dict(obs(B, 50))   # (the observations of the BC steps: the topology cached for this size is theirs in both sequences)
        batch.update(syn.make_ppo_fields(B, A, seed=3))
        upd = agent.PolicyUpdater(loss, lr=cfg.lr, use_graph=False)
        out = upd.step({k: v.to(DEV) for k, v in batch.items()})
        upd.join_lanes()
        torch.cuda.synchronize()
        outs = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        params = {"actor." + k: p.detach().clone() for k, p in actor.named_parameters()}
        params.update({"critic." + k: p.detach().clone() for k, p in critic.named_parameters()})
        return outs, params

    spec, cfg, (actor, critic, proj, loss), obs, A = build("rigid_g1")
    bc_loss = bc.BCLoss(actor, objective="nll")
    upd = bc.BCUpdater(bc_loss, use_graph=False)
    start = {k: p.detach().clone() for k, p in actor.named_parameters()}
    for t in range(2):
        upd.step(batch_of(obs, B, A, 50, bc_loss.in_features))
    upd.release()
    saved = {k: v.detach().clone() for k, v in actor.state_dict().items()}
    assert any(not torch.equal(saved[k], v) for k, v in start.items())   # the cloning moved the actor (the std head too: nll)
    assert not torch.equal(saved["_pre_std.weight"], start["_pre_std.weight"])
    outs_a, params_a = trpl_step(spec, cfg, actor, critic, loss, obs, A)

    spec, cfg, (actor, critic, proj, loss), obs, A = build("rigid_g1")
    actor.load_state_dict(saved)
    outs_b, params_b = trpl_step(spec, cfg, actor, critic, loss, obs, A)
    assert set(outs_a) == set(outs_b) and set(params_a) == set(params_b)
    for k in outs_a:
        assert torch.equal(outs_a[k], outs_b[k]), k
    for k in params_a:
        assert torch.equal(params_a[k], params_b[k]), k
    assert any(not torch.equal(params_a["actor." + k], saved[k]) for k in start)   # ... and the TRPL step moved it on from there
