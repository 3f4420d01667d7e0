"""tests/transformer_ref.py against torch and the reference fixture, its checker against seeded mistakes, and the CPU-visible side of
``TransformerVanilla(kernels="hip")``: parameter holders and refusals (no GPU; the kernels' library: tests/test_kernel_libraries_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import transformer_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "tier2d_transformer_post_fc.npz")


@pytest.mark.parametrize("B,n,d_in,m0,G", [(2, 33, 15, 32, 1), (3, 7, 13, 2, 4), (1, 1, 1, 0, 1)])
def test_restatement_equals_torch_in_float64(B, n, d_in, m0, G):
    m = tr.stock_module(d_in, seed=n, dtype=torch.float64)
    g = torch.Generator().manual_seed(n)
    u = torch.randn(B, n, d_in, generator=g, dtype=torch.float64)
    R = torch.randn(B * G, 64, generator=g, dtype=torch.float64)
    ps = tr.module_params(m)
    want = m.one_step(tr.Graph(B, m0, G), u)
    got = tr.encode(u, ps, m0, G)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for k, a, b in zip(tr.PARAM_NAMES, torch.autograd.grad(got, ps, R), torch.autograd.grad(want, ps, R)):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), k


def fixture_inputs():
    """(z, u [B,n,d], state_dict, m0, G) of tests/golden/tier2d_transformer_post_fc.npz (tools/make_golden.py tier2d)."""
    z = np.load(GOLD)
    B, P, G = int(z["B"]), int(z["P"]), int(z["G"])
    u_obj, u_grip = torch.from_numpy(z["u_object_geometry"]), torch.from_numpy(z["u_grippers"])
    d = u_obj.shape[1]
    u = torch.cat([u_obj.reshape(B, P, d), u_grip.reshape(B, G, d)], dim=1)
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    return z, u, sd, P, G


def test_restatement_reproduces_the_reference_fixture():
    z, u, sd, m0, G = fixture_inputs()
    B = u.shape[0]
    hidden = tr.encode(u.double(), [sd["gnn." + k].double() for k in tr.PARAM_NAMES], m0, G)
    shift = torch.log(torch.expm1(torch.tensor(1.0 - 1e-5, dtype=torch.float64)))   # init_std 1, minimal_std 1e-5 (the policy's defaults)
    mean, sigma = tr.head(hidden, sd["_mean.weight"].double(), sd["_mean.bias"].double(), sd["_pre_std.weight"].double(),
                          sd["_pre_std.bias"].double(), shift, 1e-5)
    loc, cov = torch.from_numpy(z["loc"]).double(), torch.from_numpy(z["cov"]).double()
    assert float((mean.reshape(B, -1) - loc).abs().max()) <= 1e-5
    assert float(((sigma.reshape(B, -1) ** 2).diag_embed() - cov).abs().max()) <= 1e-5 * float(cov.max())


@pytest.mark.parametrize("mistake", ["no_scale", "pre_norm", "interleaved_heads"])
def test_checker_notices_seeded_mistakes(mistake):
    c = tr.EncoderCase(2, 9, 13, 3, 2)
    right = tr.encode(c.u.double(), [p.double() for p in c.params], c.m0, c.G)
    tr.check("hidden", right.float(), c.ref["hidden"], c.stock["hidden"])
    p64 = [p.double().requires_grad_(True) for p in c.params]
    wrong = tr.encode(c.u.double(), p64, c.m0, c.G, mistake=mistake)
    with pytest.raises(AssertionError):
        tr.check("hidden", wrong.detach().float(), c.ref["hidden"], c.stock["hidden"])
    grads = torch.autograd.grad(wrong, p64, c.R.double(), allow_unused=True)
    k = "d transformer_encoder.layers.0.self_attn.in_proj_weight"
    with pytest.raises(AssertionError):
        tr.check(k, grads[2].float(), c.ref[k], c.stock[k])


def test_value_cases_do_what_they_say():
    c = tr.EncoderCase(3, 33, 15, 32, 1, value="logits60")
    s = tr.first_layer_logits(c.u, c.params)
    assert 59.9 <= float(s.abs().max()) <= 60.1 and float(s.max()) > 30 and float(s.min()) < -30
    assert float(torch.exp(-(s.max(-1).values - s.min(-1).values).max()).float()) < 1e-30   # un-shifted, a row's ends are 2^100 apart
    c = tr.EncoderCase(1, 5, 13, 0, 1, value="zero_variance")
    x = c.u @ c.params[0].T + c.params[1]
    assert float((x - x[..., :1]).abs().max()) == 0.0
    c = tr.EncoderCase(1, 5, 13, 0, 1, value="relu_zero")
    assert float(c.ref["d transformer_encoder.layers.0.linear1.weight"][5].abs().max()) == 0.0


def test_hip_module_keeps_the_stock_parameter_holders():
    from geometry_rl_amd.transformer import TransformerVanilla
    torch.manual_seed(0)
    a = TransformerVanilla(15, 64, dropout=0.0, kernels="torch")
    b = TransformerVanilla(15, 64, dropout=0.0, kernels="hip")
    assert list(a.state_dict()) == list(b.state_dict())
    assert {k.split(".")[0] for k in b.state_dict()} == {"cls_token", "embedding", "transformer_encoder_layer", "transformer_encoder", "fc_out"}
    b.load_state_dict(a.state_dict(), strict=True)
    assert a.kernels == "torch" and b.kernels == "hip" and TransformerVanilla(15, 64, dropout=0.0).kernels == "torch"
    a.set_kernels("hip")      # one module, flipped for an A/B run
    a.set_kernels("torch")
    assert len(b.encoder_parameters()) == 28 and [tuple(p.shape) for p in b.encoder_parameters()[:4]] == [(64, 15), (64,), (192, 64), (192,)]


@pytest.mark.parametrize("kw", [dict(concat_global=True), dict(dropout=0.1), dict(num_heads=4), dict(num_heads=1), dict(hidden_dim=128),
                                dict(output_dim=32), dict(n_tokens=257)])
def test_hip_module_refusals(kw):
    from geometry_rl_amd.transformer import TransformerVanilla
    args = dict(dict(input_dim_node=15, output_dim=64, dropout=0.0, kernels="hip"), **kw)
    with pytest.raises(NotImplementedError, match="configs/algorithm/pyg_agent/model/transformer.yaml"):
        TransformerVanilla(**args)
    TransformerVanilla(**dict(args, kernels="torch"))   # the stock path takes all of them
    with pytest.raises(ValueError):
        TransformerVanilla(15, 64, kernels="triton")


def test_agent_config_refusals():
    from geometry_rl_amd import agent, graph
    assert agent.AgentConfig().transformer_kernels == "torch"
    spec = graph.rigid_spec()
    ref = "configs/algorithm/pyg_agent/model/transformer.yaml"
    with pytest.raises(NotImplementedError, match=ref):
        agent.build_agent(spec, agent.AgentConfig(model="transformer", precision="bf16", transformer_kernels="hip"), device="cpu")
    for model in ("hepi", "empn"):
        with pytest.raises(NotImplementedError, match=ref):
            agent.build_agent(spec, agent.AgentConfig(model=model, transformer_kernels="hip"), device="cpu")
    with pytest.raises(NotImplementedError, match=ref):   # 1 + 300 tokens per sample
        agent.build_agent(graph.rigid_spec(P=300), agent.AgentConfig(model="transformer", transformer_kernels="hip"), device="cpu")
