"""The HIP PonitaGCN(attention=True) against the REFERENCE's own numbers: tests/golden/tier2h_<case>_attention.npz / _attention_grad.npz,
what the reference's PonitaGCN(attention=True) computed on the two EMPN cases of tier2h (tools/make_golden.py empn_attention).  This
pins the option tests/data_fixtures.py still lists as unpinned.  The route is that of tests/test_gpu_reference_golden.py: the agent
from ``agent.build_agent``, the data class from the recorded names / dims / keywords, the reference state dict loaded strictly by name,
the calibrated state reached through ``actor.forward_diag`` on the padded calibration graph; bars as there (1e-4 absolute / relative
for outputs and calibrated weights, 1e-4 * max(1, max|ref|) for gradients).

Also here: the three refusals (bf16, more than one rank, a model other than EMPN), and ``attention=False`` giving the bits of a model
built without the key."""
import pytest
import torch

import data_fixtures as dfx
import empn_attention_ref as ar
from test_gpu_reference_golden import check

pytestmark = pytest.mark.gpu


def _agent(fx, dev, **cfg_kw):
    from geometry_rl_amd import agent, graph
    m = fx.model
    cls = {"rigid": graph.RigidTasksData, "rope": graph.RopeTasksData}[fx.family]
    hd = cls(observation_dim=fx.observation_dim, observation_names=fx.observation_names, training_noise=False, **fx.kwargs, **dfx.ACTOR)
    cfg = agent.AgentConfig(model="empn", dim=m["dim"], only_upper_hemisphere=bool(m["upper"]), output_dim=m["output_dim"],
                            output_dim_vec=m["output_dim_vec"], **cfg_kw)
    actor, _, _, _ = agent.build_agent(hd.spec, cfg, device=dev)
    actor.hyper_data = hd
    return actor, hd


@pytest.mark.parametrize("case", list(ar.ATTENTION_CASES))
def test_attention_actor_matches_reference_fixture(golden_dir, case):
    dev = torch.device("cuda:0")
    fx = ar.AttentionFixture(golden_dir, case)
    z = fx.z
    actor, hd = _agent(fx, dev, attention=True)
    gnn = actor.gnn

    # --- reference checkpoint, strictly by name (key_transform / query_transform included)
    sd = gnn.state_dict()
    assert set(fx.init) == set(sd), set(fx.init) ^ set(sd)
    assert sum("key_transform" in k or "query_transform" in k for k in sd) == 8
    for k in sd:
        assert sd[k].shape == fx.init[k].shape, k
    gnn.load_state_dict({k: v.to(dev) for k, v in fx.init.items()}, strict=True)
    assert not gnn.calibrated

    obs = [a.to(dev) for a in fx.args()]
    g, u = hd.build_data(*obs, train=True)
    assert g.node_types == fx.node_types() and g.compact

    print(case)
    with torch.no_grad():
        out0, hid0 = gnn.one_step(g, u)
    check("out_first_call", out0, z["out_first_call"], 1e-4)
    check("hidden_first_call", hid0, z["hidden_first_call"], 1e-4)

    with torch.no_grad():
        loc, _ = actor.forward_diag(*obs, train=True)
    for k, v in gnn.state_dict().items():
        ref = fx.cal[k]
        if ref.dtype.is_floating_point:
            check("cal." + k, v, ref, 1e-4, ref_distance=fx.ref_distance("cal." + k) if k in fx.changed else None)
            assert torch.equal(v.cpu(), fx.init[k]) == (k not in fx.changed), k   # key / query layers are never rescaled
        else:
            assert bool(v.cpu()) == bool(ref), k
    check("forward_diag mean", loc.reshape(-1, 3), z["out"], 1e-4, ref_distance=fx.ref_distance("out"))

    gnn.load_state_dict({k: v.to(dev) for k, v in fx.cal.items()}, strict=True)
    gnn.zero_grad()
    out, hid = gnn.one_step(g, u)
    check("out", out, z["out"], 1e-4, ref_distance=fx.ref_distance("out"))
    check("hidden", hid, z["hidden"], 1e-4, ref_distance=fx.ref_distance("hidden"))
    ((out * z["R_out"].to(dev)).sum() + (hid * z["R_hidden"].to(dev)).sum()).backward()
    n = 0
    for k, p in gnn.named_parameters():
        if k in fx.grad:
            ref = fx.grad[k]
            check("grad." + k, p.grad, ref, 1e-4 * max(1.0, ref.abs().max().item()))
            n += 1
        else:
            assert p.grad is None or not bool(p.grad.abs().sum() > 0), k
    assert n == len(fx.grad) >= 28


def test_refusals(golden_dir, monkeypatch):
    from geometry_rl_amd import agent, graph, ponita_gcn
    dev = torch.device("cuda:0")
    spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        agent.build_agent(spec, agent.AgentConfig(model="empn", attention=True, precision="bf16"), device=dev)
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        ponita_gcn.PonitaGCN(7, 1, 1, attention=True, precision="bf16", device=dev)
    for model in ("hepi", "transformer"):
        with pytest.raises(ValueError, match="model='empn'"):
            agent.build_agent(spec, agent.AgentConfig(model=model, attention=True), device=dev)
    # more than one rank: the group is only asked for its size
    import torch.distributed as dist
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    with pytest.raises(NotImplementedError, match="all-reduce max of M"):
        agent.build_agent(spec, agent.AgentConfig(model="empn", attention=True), device=dev, group=group)
    gnn = ponita_gcn.PonitaGCN(7, 1, 1, attention=True, device=dev)
    with pytest.raises(NotImplementedError, match="one rank only"):
        gnn.calibrate(None, None, group=group)
    ponita_gcn.check_attention_group(True, None)        # no group, or one rank: fine
    ponita_gcn.check_attention_group(False, group)      # without attention the group is nobody's business here


def test_attention_false_is_the_model_without_the_key(golden_dir):
    """``attention=False`` changes nothing: same parameters, same launches, same bits as a model built without the key."""
    dev = torch.device("cuda:0")
    fx = dfx.ModelFixture(golden_dir, "empn_rigid_g2_pad")
    res = []
    for kw in ({}, {"attention": False}):
        actor, hd = _agent(fx, dev, **kw)
        gnn = actor.gnn
        gnn.load_state_dict({k: v.to(dev) for k, v in fx.cal.items()}, strict=True)
        assert gnn.prune_last_layer and not gnn.attention
        g, u = hd.build_data(*[a.to(dev) for a in fx.args()], train=True)
        gnn.zero_grad()
        out, hid = gnn.one_step(g, u)
        ((out * fx.z["R_out"].to(dev)).sum() + (hid * fx.z["R_hidden"].to(dev)).sum()).backward()
        res.append([out.detach(), hid.detach()] + [p.grad.clone() for p in gnn.parameters() if p.grad is not None])
    assert len(res[0]) == len(res[1]) and all(torch.equal(a, b) for a, b in zip(*res))
