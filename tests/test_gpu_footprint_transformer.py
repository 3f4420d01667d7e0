"""Footprint of the transformer actor's kernels (csrc/transformer_ops.hip) under tests/footprint.py, as
tests/test_gpu_footprint_attention.py does it for the EMPN attention kernels: ``ops.TransformerEncode``, ``ops.PostFcHead`` and one
eager update of AgentConfig(model="transformer", transformer_kernels="hip") run plain, under the NaN poison and under the huge-finite
poison from identical inputs.  Checked: untouched guards and inputs, no poisoned or non-finite element in any result, every result
bitwise the plain run's."""
import pytest
import torch

import footprint as fp
import transformer_ref as tr
from test_gpu_footprint import dev, grads_of, leaf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,m0,G", [(1, 0, 1), (65, 30, 4)])
def test_transformer_encode(n, m0, G):
    from geometry_rl_amd import ops
    d, B = dev(), 3
    g = torch.Generator().manual_seed(n)
    u = torch.randn(B, n, 13, generator=g).to(d)
    R = torch.randn(B * G, 64, generator=g).to(d)
    params = [p.detach().to(d) for p in tr.module_params(tr.stock_module(13, seed=n))]

    def run(w):
        L = {k: leaf(w, p) for k, p in zip(tr.PARAM_NAMES, params)}
        hidden = ops.TransformerEncode.apply(w(u), m0, G, *L.values())
        hidden.backward(w(R))
        return {"hidden": hidden.detach(), "grads": grads_of(L)}

    plain = fp.three_runs("TransformerEncode", f"B={B} n={n}", run)
    assert all(v is not None and bool(v.abs().max() > 0) for v in plain["grads"].values())


@pytest.mark.parametrize("n", [1, 65])
def test_postfc_head(n):
    from geometry_rl_amd import ops
    d, A = dev(), 6
    g = torch.Generator().manual_seed(n)
    I = {"hidden": torch.randn(3 * n, 64, generator=g), "wm": torch.randn(A, 64, generator=g) * 0.3, "bm": torch.randn(A, generator=g),
         "ws": torch.randn(A, 64, generator=g) * 0.3, "bs": torch.randn(A, generator=g)}
    I = {k: v.to(d) for k, v in I.items()}
    Rm, Rs = torch.randn(3 * n, A, generator=g).to(d), torch.randn(3 * n, A, generator=g).to(d)

    def run(w):
        L = {k: leaf(w, v) for k, v in I.items()}
        mean, sigma = ops.PostFcHead.apply(L["hidden"], L["wm"], L["bm"], L["ws"], L["bs"], 0.5413, 1e-5)
        torch.autograd.backward([mean, sigma], [w(Rm), w(Rs)])
        return {"mean": mean.detach(), "sigma": sigma.detach(), "grads": grads_of(L)}

    fp.three_runs("PostFcHead", f"rows={3 * n}", run)


def test_one_eager_update(monkeypatch):
    """loss(batch) and both backward passes of the transformer agent on HIP kernels as PolicyUpdater issues them eagerly, at B = 3 from a
    fresh seeded agent: the flat gradient and the parameters after the step, bit for bit, and every new entry point launched."""
    from geometry_rl_amd import agent, graph, hip, synthetic as syn
    d, B = dev(), 3
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(model="transformer", output_dim=2, output_dim_vec=2, transformer_kernels="hip")
    batch = dict(syn.make_rigid_obs(B, seed=B))
    batch.update(syn.make_ppo_fields(B, 6, seed=B))
    dbatch = {k: v.to(d) for k, v in batch.items()}

    def run(w):
        torch.manual_seed(3)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=d)
        upd = agent.PolicyUpdater(loss, use_graph=False)
        out = upd.step({k: (w(v) if v.is_floating_point() else v) for k, v in dbatch.items()})
        torch.cuda.synchronize()
        return {"gradient": upd.gflat.clone(), "parameters": upd.flat.clone(), "loc": out["loc"], "state_value": out["state_value"]}

    launched = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), real_call(entry, *a, **k))[1])
    plain = fp.three_runs("eager update", "transformer hip", run)
    assert bool(plain["gradient"].abs().max() > 0)
    names = set(launched)
    print(f"eager update transformer hip: entry points launched: {sorted(names)}")
    for want in ("grl_transformer_fwd", "grl_transformer_bwd", "grl_postfc_head_fwd", "grl_postfc_head_bwd"):
        assert want in names, (want, sorted(names))
