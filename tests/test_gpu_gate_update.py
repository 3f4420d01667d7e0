"""The attention model with its gate network on HIP kernels (AgentConfig(attention_gate="hip"), csrc/grl_gate.h) through the policy update:
the ``rigid_attn`` case against the CPU oracle with the checkers and bars the torch-gate model is held to (tests/test_gpu_step.py), and
three updates recorded and eager, bit for bit, in the overwrite mode of the gradient fold (every leaf gradient of the model now comes
through the fold queue)."""
import pytest
import torch

import oracle_cases as oc
from geometry_rl_amd import synthetic as syn
from oracle_cases import LOSS_KEYS, check

pytestmark = pytest.mark.gpu


def test_policy_update_step_gate_hip():
    """tests/test_gpu_step.py::test_policy_update_step[rigid_attn-12] with attention_gate="hip"."""
    from geometry_rl_amd import agent
    dev = torch.device("cuda:0")
    B = 12
    o_spec, spec, kw, obs = oc.make_case("rigid_attn", B)
    pair = oc.build_pair((o_spec, spec, kw), seed=11, d_kw=dict(attention_gate="hip"))
    cfg, oracle, actor, critic, loss = pair.cfg, pair.oracle, pair.actor, pair.critic, pair.loss
    convs = [c for r in actor.gnn.processor for _, c in r.items()]
    assert convs and all(c.attention and c.gate_kernels == "hip" for c in convs)
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, A, seed=B))
    dbatch = {k: v.to(dev) for k, v in batch.items()}

    own = oc.adopt_calibration(pair, batch, device_first=True)
    for k, v in oracle.actor.items():
        if "kernel.weight" in k:
            check("calibrated " + k, own[k], v, 1e-4)

    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm)
    assert upd._fold_overwrite, "with the gate on HIP kernels every leaf gradient comes through the fold queue"
    ref, ref_grads = oracle.update(batch)
    upd.gflat.zero_()
    out = loss(dbatch)
    (out["loss_objective"] + out["loss_entropy"] + out["loss_trust_region"]).backward()
    out["loss_critic"].backward()
    check("loc", out["loc"], ref["loc"])
    check("var", out["sigma"] ** 2, ref["var"])
    check("state_value", out["state_value"], ref["state_value"])
    for k in LOSS_KEYS:
        check(k, out[k], ref[k])
    assert any("gate_nn.0.weight" in k for k, p in actor.named_parameters() if p.grad is not None)
    bad, scales = oc.gradients_off_scale(actor, critic, ref_grads)
    assert not bad, bad
    upd.step(dbatch)   # (the first eager step: the overwrite-coverage check runs here)
    assert upd._overwrite_checked and upd._fold_overwrite
    bad = oc.first_step_params_off(actor, critic, oracle, cfg, ref_grads, scales)
    assert not bad, bad


def test_gate_hip_update_recorded_equals_eager():
    """Three updates recorded (hipGraph) and eager from the same start: identical parameters, bit for bit; the fold writes the gradients."""
    from geometry_rl_amd import agent, graph
    d = torch.device("cuda:0")
    B = 12
    spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
    cfg = agent.AgentConfig(aggr="AttentionalAggregation", attention_gate="hip")
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batches = []
    for i in range(3):
        b = dict(syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=30 + i))
        b.update(syn.make_ppo_fields(B, A, seed=40 + i))
        batches.append({k: v.to(d) for k, v in b.items()})

    def run(use_graph):
        torch.manual_seed(3)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=d)
        upd = agent.PolicyUpdater(loss, use_graph=use_graph)
        assert upd._fold_overwrite
        for b in batches:
            upd.step(b)
        torch.cuda.synchronize()
        assert upd._fold_overwrite and upd._overwrite_checked
        return upd.flat.clone(), upd.mode

    (p0, m0), (p1, m1) = run(False), run(True)
    print(f"attention gate hip: eager mode {m0!r}, recorded mode {m1!r}")
    assert m1.startswith("graph") and not m0.startswith("graph"), (m0, m1)
    assert torch.equal(p0, p1), f"parameters differ: max |diff| {(p0 - p1).abs().max().item():.3e}"
