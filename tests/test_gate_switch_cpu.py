"""The attention gate's switch (FiberBundleConv.gate_kernels / HEPi(gate_kernels=...) / AgentConfig(attention_gate=...)) and the grown
argument lists of the four softmax-aggregation entry points, without a GPU.

The fused gate network (csrc/grl_gate.h) arrives behind grl_softmax_aggregate_fwd / _bwd and their _bf16 twins: (Wg, bg, stat[, partial],
n_blocks) in front of ``stream``, under the unchanged ABI number and with no entry point added."""
import os

import pytest
import torch

from geometry_rl_amd import agent, graph, hip
from test_abi_and_host import ROOT

FWD_TAIL = [("const float*", "Wg"), ("const float*", "bg"), ("float*", "stat"), ("int", "n_blocks"), ("hipStream_t", "stream")]
BWD_TAIL = [("const float*", "Wg"), ("const float*", "bg"), ("const float*", "stat"), ("float*", "partial"), ("int", "n_blocks"),
            ("hipStream_t", "stream")]


def test_four_argument_lists_grew_and_nothing_else():
    text = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    decls = hip.parse_header(text)
    for sfx in ("", "_bf16"):
        fwd, bwd = decls["grl_softmax_aggregate_fwd" + sfx], decls["grl_softmax_aggregate_bwd" + sfx]
        assert [(t, n) for t, n, _ in fwd[-5:]] == FWD_TAIL and [n for _, n, _ in fwd[:5]] == ["gate", "msg", "rowptr", "n_dst", "x1"]
        assert [(t, n) for t, n, _ in bwd[-6:]] == BWD_TAIL
        assert [n for _, n, _ in bwd[:8]] == ["gate", "msg", "x1", "dx1", "rowptr", "n_dst", "dgate", "dmsg"]
        assert len(fwd) == 10 and len(bwd) == 14
    counts = [len(hip.parse_header(open(l.paths()[1]).read())) for l in hip.LIBRARIES]
    assert counts == [138, 9, 10] and hip.ABI_VERSION == 216
    assert "grl_gate.h" in os.listdir(hip.CSRC) and "FOUR ARGUMENT LISTS GREW" in text


def _cfg(**kw):
    return agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, **kw)


def test_switch_defaults_and_reaches_the_attention_convolutions():
    spec = graph.rigid_spec()
    assert agent.AgentConfig().attention_gate == "torch"
    for gate in ("torch", "hip"):
        actor, _, _, _ = agent.build_agent(spec, _cfg(aggr="AttentionalAggregation", attention_gate=gate), device="cpu")
        convs = [c for r in actor.gnn.processor for _, c in r.items()]
        assert actor.gnn.gate_kernels == gate and convs and all(c.attention and c.gate_kernels == gate for c in convs)
    actor.gnn.set_gate_kernels("torch")
    assert all(c.gate_kernels == "torch" for c in convs)
    plain, _, _, _ = agent.build_agent(spec, _cfg(), device="cpu")
    assert plain.gnn.gate_kernels == "torch" and all(c.gate_kernels == "torch" for r in plain.gnn.processor for _, c in r.items())


def test_switch_refusals():
    spec = graph.rigid_spec()
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        agent.build_agent(spec, _cfg(aggr="AttentionalAggregation", attention_gate="rocblas"), device="cpu")
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        agent.build_agent(spec, _cfg(aggr="AttentionalAggregation", attention_gate="hip", precision="bf16"), device="cpu")
    with pytest.raises(NotImplementedError, match="attention convolutions"):
        agent.build_agent(spec, _cfg(attention_gate="hip"), device="cpu")
    for model in ("empn", "transformer"):
        with pytest.raises(NotImplementedError, match="attention convolutions"):
            agent.build_agent(spec, agent.AgentConfig(model=model, attention_gate="hip"), device="cpu")
    # the model's own constructor and setter refuse the same
    actor, _, _, _ = agent.build_agent(spec, _cfg(), device="cpu")
    with pytest.raises(NotImplementedError, match="attention convolutions"):
        actor.gnn.set_gate_kernels("hip")
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        actor.gnn.set_gate_kernels("HIP")
    b16, _, _, _ = agent.build_agent(spec, _cfg(aggr="AttentionalAggregation", precision="bf16"), device="cpu")
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        b16.gnn.set_gate_kernels("hip")
    assert b16.gnn.gate_kernels == "torch"


def test_state_dict_is_the_same_under_both_settings():
    spec = graph.rigid_spec()
    sds = []
    for gate in ("torch", "hip"):
        torch.manual_seed(5)
        actor, _, _, _ = agent.build_agent(spec, _cfg(aggr="AttentionalAggregation", attention_gate=gate), device="cpu")
        sds.append(actor.state_dict())
    assert list(sds[0]) == list(sds[1]) and any(k.endswith("aggr_module.gate_nn.0.weight") for k in sds[0])
    assert all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])


def test_gated_op_refuses_the_bf16_build():
    from geometry_rl_amd import ops
    z = torch.zeros(0, 16, 64)
    with pytest.raises(NotImplementedError, match="fp32 build only"):
        ops.GatedSoftmaxAggregate.apply(z, torch.zeros(64, 64), torch.zeros(64), None, "_bf16")
    assert [ops.GatedSoftmaxAggregate.blocks(n) for n in (0, 1, 4, 5, 1024, 1025, 10 ** 6)] == [1, 1, 1, 2, 256, 256, 256]


def test_switch_through_the_reference_configs():
    """refconfig.build_from_config(..., attention_gate=) hands the switch to HEPi and refuses what HEPi refuses, before building."""
    import refconfig_cases as rc
    att = ["algorithm/policy/pyg_agent/model=../../../pyg_agent/model/hepi_attention"]
    name = "rigid_insertion_multi_hepi"
    for gate in ("torch", "hip"):
        _, (actor, _, _, _) = rc.build(name, att, attention_gate=gate)
        convs = [c for r in actor.gnn.processor for _, c in r.items()]
        assert actor.gnn.gate_kernels == gate and convs and all(c.gate_kernels == gate for c in convs)
    _, (plain, _, _, _) = rc.build(name)
    assert plain.gnn.gate_kernels == "torch"
    with pytest.raises(NotImplementedError, match="attention convolutions"):
        rc.build(name, attention_gate="hip")
    with pytest.raises(NotImplementedError, match="attention convolutions"):
        rc.build("rigid_insertion_multi_empn", attention_gate="hip")
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        rc.build(name, att, attention_gate="hip", precision="bf16")
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        rc.build(name, att, attention_gate="mfma")
