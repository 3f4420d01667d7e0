"""Footprint of the EMPN key / query attention kernels (csrc/attention_ops.hip) under tests/footprint.py, as tests/test_gpu_footprint.py
does it for the other actor kernels: ``ops.KeyQueryProject``, ``ops.EdgeAttention`` and one eager update of the attention-enabled EMPN
actor (AgentConfig(model="empn", attention=True) -- the option tests/data_fixtures.py still lists as unpinned) run plain, under the NaN
poison and under the huge-finite poison from identical inputs.  Checked: untouched guards and inputs, no poisoned or non-finite element
in any result, every result bitwise the plain run's.  The huge-finite poison is the one that shows a read past the end feeding the global
maximum M (a max drops a NaN)."""
import pytest
import torch

import empn_attention_ref as ar
import footprint as fp
from test_gpu_footprint import dev, grads_of, leaf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [24, 26, 96])
def test_key_query_project(n):
    from geometry_rl_amd import ops
    d = dev()
    c = ar.ProjectCase(n)
    x, ws, Rk, Rq = c.x.to(d), [t.to(d) for t in c.w], c.Rk.to(d), c.Rq.to(d)

    def run(w):
        L = {"x": leaf(w, x)}
        L.update({k: leaf(w, t) for k, t in zip(("wk", "bk", "wq", "bq"), ws)})
        k, q = ops.KeyQueryProject.apply(L["x"], L["wk"], L["bk"], L["wq"], L["bq"])
        torch.autograd.backward([k, q], [w(Rk), w(Rq)])
        return {"k": k.detach(), "q": q.detach(), "grads": grads_of(L)}

    fp.three_runs("KeyQueryProject", f"{n} nodes", run)


@pytest.mark.parametrize("graph,span", [("degrees", 1.0), ("degrees", 20.0), ("hub", 10.0), ("half_block", 3.0), ("self_loops", 20.0),
                                        ("empty", 1.0)])
def test_edge_attention(graph, span):
    from geometry_rl_amd import ops
    d = dev()
    c = ar.AttentionCase(graph, span)
    probe = ops.build_edge_set(c.ei.to(d), c.n, c.n)
    c.with_edges(torch.stack([probe.src_d.long(), probe.dst_d.long()]).cpu())
    k0, q0, msg0, R, ei_d = c.k.to(d), c.q.to(d), c.msg.to(d), c.R.to(d), c.ei.to(d)

    def run(w):
        es = fp.guard_edge_set(ops.build_edge_set(ei_d, c.n, c.n), w)
        L = {"k": leaf(w, k0), "q": leaf(w, q0), "msg": leaf(w, msg0)}
        x1 = ops.EdgeAttention.apply(L["k"], L["q"], L["msg"], es)
        x1.backward(w(R))
        return {"x1": x1.detach(), "grads": grads_of(L)}

    plain = fp.three_runs("EdgeAttention", f"{graph} span {span:g}", run)
    if graph == "empty":
        assert not bool(plain["x1"].abs().sum() > 0) and not bool(plain["grads"]["k"].abs().sum() > 0)


def test_one_eager_update(monkeypatch):
    """loss(batch) and both backward passes of the attention-enabled EMPN agent as PolicyUpdater issues them eagerly, at B = 12 from a
    fresh seeded agent: the flat gradient and the parameters after the step, bit for bit, and every attention entry point launched."""
    from geometry_rl_amd import agent, hip, synthetic as syn
    from oracle_cases import make_case
    d, B = dev(), 12
    _, spec, kw, obs = make_case("empn_g2", B)
    cfg = agent.AgentConfig(**dict(kw, attention=True))
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=B))
    dbatch = {k: v.to(d) for k, v in batch.items()}

    def run(w):
        torch.manual_seed(3)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=d)
        assert actor.gnn.attention
        upd = agent.PolicyUpdater(loss)
        out = upd.step({k: (w(v) if v.is_floating_point() else v) for k, v in dbatch.items()})
        torch.cuda.synchronize()
        assert not upd.mode.startswith("graph")
        return {"gradient": upd.gflat.clone(), "parameters": upd.flat.clone(), "loc": out["loc"], "state_value": out["state_value"]}

    launched = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), real_call(entry, *a, **k))[1])
    plain = fp.three_runs("eager update", "empn attention", run)
    assert bool(plain["gradient"].abs().max() > 0)
    names = set(launched)
    print(f"eager update empn attention: entry points launched: {sorted(names)}")
    for want in ("grl_kq_project_fwd", "grl_kq_project_bwd", "grl_edge_logits_fwd", "grl_edge_logits_bwd", "grl_edge_attend_fwd",
                 "grl_edge_attend_bwd", "grl_edge_messages_fwd", "grl_edge_messages_bwd"):
        assert want in names, (want, sorted(names))
    assert "grl_edge_conv_fwd_balanced" not in names
