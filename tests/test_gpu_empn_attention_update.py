"""The attention-enabled EMPN actor -- AgentConfig(model="empn", attention=True), PonitaGCN(attention=True): the first GPU pin of that
option, which tests/data_fixtures.py still lists as unpinned -- through ``PolicyUpdater`` (builds on tests/updater_cases.py): the tiny
two-agent rigid spec, 8-frame minibatches, three updates through four paths -- the eager loop, the one-stream program
(``_plan_one_stream``), the two-lane program (``_plan_lanes``) and one ``run_minibatches`` launch.  All four must leave bitwise-equal
parameters, Adam moments and reports.  After the first eager step the flat gradient must equal the per-parameter gradients of a plain
autograd pass from the same parameters (the key / query leaves arrive through the fold queue like every other EMPN leaf).

"Equal" is equality to fp32 rounding, not of bits: the step issues the same arithmetic through other launches than ``loss(batch)``
followed by two ``backward()`` calls (the merged head launch, the fused loss kernel, the queued folds), so sums are grouped differently
-- for EVERY parameter, the attention-free ones included (measured on the MI355X: up to 1.8 ulp of a module's gradient scale, the
actor's tensors not bitwise equal).  The bar comes from the number format: 16 ulp (16 * 2^-23 = 1.9e-6) of the module's largest gradient entry, one ulp for
each of the roughly ten roundings that can differ between the two routes and a little headroom; a misrouted or doubled slab is off by
the whole scale."""
import pytest
import torch

from updater_cases import DEV, RIGID2, Rollout, calibrate, snapshot

pytestmark = pytest.mark.gpu

KEYS = ("loss_objective", "loss_trust_region", "loss_critic", "kl", "constraint", "entropy", "ESS")
N, T = 8, 3   # 8-frame minibatches, three of them
ULPS = 16     # (module docstring)


def _make(seed=51):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec(**RIGID2)
    cfg = agent.AgentConfig(model="empn", attention=True)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    assert actor.gnn.attention and not actor.gnn.prune_last_layer
    frames = []
    for t in range(T + 1):
        b = dict(syn.make_rigid_obs(N, seed=seed + t, **RIGID2))
        b.update(syn.make_ppo_fields(N, 6, seed=seed + t))
        frames.append(b)
    data = {k: torch.stack([f[k] for f in frames[:T]], dim=1).to(DEV) for k in frames[0]}
    g = syn.make_gae_inputs(N, T, seed=seed)
    data.update(reward=g["reward"].reshape(N, T, 1).to(DEV), done=g["done"].reshape(N, T, 1).to(DEV),
                terminated=g["terminated"].reshape(N, T, 1).to(DEV))
    next_last = {k: frames[T][k].unsqueeze(1).to(DEV) for k in spec.in_features}
    calibrate(actor, spec, {k: data[k][:, 0].contiguous() for k in spec.in_features})
    return Rollout(spec, cfg, actor, critic, proj, loss, data, next_last)


PATHS = {"eager": dict(use_graph=False), "one_stream": dict(use_graph=True, overlap_critic=False), "lanes": dict(use_graph=True),
         "launch": dict(use_graph=True)}


def _run(path):
    from geometry_rl_amd import agent
    from geometry_rl_amd.rollout import RolloutBuffer, RolloutDriver
    r = _make()
    upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, **PATHS[path])
    assert not upd._fold_overwrite   # (updater.py: a module with a true ``attention`` attribute folds in accumulate mode)
    buf = RolloutBuffer(dict(r.data))
    drv = RolloutDriver(upd, r.spec, ppo_epochs=1, seed=9)
    drv.compute_advantages(buf, r.next_last)
    rows = drv.epoch_minibatches(buf.N, buf.T, DEV)
    assert len(rows) == T and all(i.numel() == N for i in rows)
    outs = []
    if path == "launch":
        upd.epoch_unroll = T
        o = upd.run_minibatches(buf, torch.stack(rows))
        outs.append({k: o[k].clone() for k in KEYS})
    else:
        for idx in rows:
            o = upd.step_from(buf, idx)
            outs.append({k: o[k].clone() for k in KEYS})
    torch.cuda.synchronize()
    assert upd.steps == T
    if path != "eager":
        assert upd.mode.startswith("graph") and (upd._program is not None or upd._epoch is not None)
    return snapshot(upd, outs)


def test_four_paths_bitwise_equal():
    res = {p: _run(p) for p in PATHS}
    ref = res["eager"]
    assert bool(torch.isfinite(ref[0]).all())
    for p, got in res.items():
        for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), ref[:3], got[:3]):
            print(f"{p}: {name} max |difference from the eager loop| {float((a - b).abs().max()):.3e}")
    for p, got in res.items():
        for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), ref[:3], got[:3]):
            assert torch.equal(a, b), (p, name, float((a - b).abs().max()))
        for k in KEYS:   # the last update's report (the launch returns only that one); the step-by-step paths: every update's
            assert torch.equal(ref[3][-1][k], got[3][-1][k]), (p, k)
        if p != "launch":
            for oa, ob in zip(ref[3], got[3]):
                for k in KEYS:
                    assert torch.equal(oa[k], ob[k]), (p, k)


def test_flat_gradient_of_the_first_eager_step_equals_plain_autograd():
    from geometry_rl_amd import agent
    r = _make()
    batch = {k: v[:, 0].contiguous() for k, v in r.data.items()}
    upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=False)
    upd.gflat.zero_()
    out = r.loss(batch)
    (out["loss_objective"] + out["loss_entropy"] + out["loss_trust_region"]).backward()
    out["loss_critic"].backward()
    named = dict(list(r.actor.named_parameters()) + [("critic." + k, p) for k, p in r.critic.named_parameters()])
    plain = {k: p.grad.detach().clone() for k, p in named.items()}
    kq = [k for k in plain if "key_transform" in k or "query_transform" in k]
    assert len(kq) == 8 and all(bool(plain[k].abs().sum() > 0) for k in kq)   # two layers x (Wk, bk, Wq, bq), all reached
    upd.step(batch)
    torch.cuda.synchronize()
    # Per module (a Linear's bias gradient is a column sum of the rows whose products make its weight gradient, so its rounding error
    # lives on the weight gradient's scale: the key bias gradient is a sum that cancels to ~1e-10): 16 ulp of the module's largest
    # gradient entry.
    scale = {}
    for k in named:
        mod = k.rsplit(".", 1)[0]
        scale[mod] = max(scale.get(mod, 0.0), float(plain[k].abs().max()))
    worst = 0.0
    for k, p in named.items():
        d, s = float((p.grad - plain[k]).abs().max()), scale[k.rsplit(".", 1)[0]]
        worst = max(worst, d / s if s > 0 else (0.0 if d == 0 else float("inf")))
        print(f"  {k}: max |step - plain| {d:.3e}, module gradient scale {s:.3e}")
    print(f"worst difference: {worst / 2.0 ** -23:.2f} ulp of the module's gradient scale (allowed {ULPS})")
    for k, p in named.items():
        s = scale[k.rsplit(".", 1)[0]]
        assert float((p.grad - plain[k]).abs().max()) <= ULPS * 2.0 ** -23 * s, k
