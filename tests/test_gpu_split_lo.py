"""The split-bf16 operand forming of the fused edge backward (csrc/edge_conv16.hip: hi halves where a layer's output is produced, lo halves
beside the MFMAs of the layer that consumes them, the weight-gradient MFMAs interleaved with the splits) and of the kernels around it: edge
convolution forward + backward and the ConvNeXt block forward + backward on one small graph whose rows hold the values at which a split can
go wrong -- exact zeros, -0.0, denormals, values whose low mantissa half is zero (lo = 0 exactly) or all ones.  24 nodes, 60 edges; node 0
has no out-edge (its d x row is the empty-run path), node 1 has nine (multi-edge accumulation), the other sources change from edge to
edge (node-change path).  Reference and bars: the float64 reference and the MFMA bars of tests/test_gpu_actor_ops.py (values 1e-4,
gradients 2e-4 of each tensor's own scale); two identical launches must be bitwise equal.
Measured on the MI355X: worst margin 3.8e-5 on the values, 5.6e-5 on the gradients."""
import pytest
import torch

import actor_cases as ac
import ops_ref
from ops_ref import margin

pytestmark = pytest.mark.gpu

N, E = 24, 60


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def special_rows(x, g):
    """Rows of the values a split must get right, written into the randn tensor x [N,16,64]."""
    x = x.clone()
    x[2] = 0.0                                               # exact zeros: hi = lo = 0
    x[3] = -0.0                                              # -0.0: hi = 0x8000, lo = +0
    x[4] = torch.randn(16, 64, generator=g) * 1e-40          # denormals (low half only: hi is a signed zero)
    x[5] = torch.randn(16, 64, generator=g) * 1e-38          # around the smallest normal
    t = torch.randn(16, 64, generator=g)
    x[6] = (t.view(torch.int32) & -65536).view(torch.float32)            # low mantissa half zero: lo = 0 exactly
    x[7, :, ::2] = 0.0                                       # zeros and plain values side by side in one packed pair
    x[8, :, 1::2] = -0.0
    x[9] = ((t.view(torch.int32) & -65536) | 0xFFFF).view(torch.float32)  # low half all ones
    return x


def graph(g):
    src = [1] * 9 + [5, 5, 5, 5] + [2, 3, 4, 6, 7, 8, 9]     # node 1: nine out-edges; the special rows are sources as well
    src += torch.randint(1, N, (E - len(src),), generator=g).tolist()   # node 0 never a source: out-degree 0
    dst = torch.randint(0, N, (E,), generator=g)
    ei = torch.stack([torch.tensor(src), dst])
    deg_out = torch.bincount(ei[0], minlength=N)
    assert ei.shape == (2, E) and deg_out[0] == 0 and deg_out.max() >= 4
    return ei


@pytest.fixture(scope="module")
def case():
    g = ac.gen(41, N, E)
    ei = graph(g)
    pos = torch.rand(N, 3, generator=g) * 2 - 1
    we = ac.weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])
    wm = [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1] + ac.weights(g, [(256, 64), (256,), (64, 256), (64,)])
    inputs = {"x": special_rows(torch.randn(N, 16, 64, generator=g), g), "pos": pos, "grid": ac.grid_of("upper"), "src": ei[0], "dst": ei[1]}
    inputs.update({f"e{i}": w for i, w in enumerate(we)})
    inputs.update({f"m{i}": w for i, w in enumerate(wm)})

    def ref(t):
        x1 = ops_ref.edge_conv(t["x"], t["src"], t["dst"], N, t["grid"], t["pos"], t["pos"], *[t[f"e{i}"] for i in range(5)])
        return {"x1": x1, "out": ops_ref.node_mlp(x1, t["x"], *[t[f"m{i}"] for i in range(6)])}
    c = ac.Case(f"conv + node block on special rows n={N} E={E}", inputs, ["x"] + [f"e{i}" for i in range(5)] + [f"m{i}" for i in range(6)],
                ref, {"x1": None, "out": torch.randn(N, 16, 64, generator=g)})   # (x1 is compared, the loss is on out alone)
    c.ei = ei
    c.ref64 = c.evaluate(torch.float64, "cpu")   # computed once, shared, never written to
    return c


def launch(c):
    """x -> edge convolution -> ConvNeXt block (x is also the block's residual, as in hepi._conv), both backward."""
    from geometry_rl_amd import ops
    d = dev()
    L = {k: c.inputs[k].clone().to(d).requires_grad_(True) for k in c.diff}
    es = ops.build_edge_set(c.ei.to(d), N, N)
    pos = c.inputs["pos"].to(d)
    res = {}
    x1 = ops.EdgeConv.apply(L["x"], pos, pos, ac.grid3_of("upper").to(d), *[L[f"e{i}"] for i in range(5)], es, 3, res)
    out = ops.NodeMLP.apply(x1, L["x"], *[L[f"m{i}"] for i in range(6)], None, res)
    out.backward(c.ups["out"].to(d))
    assert res == {}, "the edge backward consumes the block's residual gradient"
    return {"x1": x1.detach(), "out": out.detach()}, {k: v.grad for k, v in L.items()}


@pytest.fixture(scope="module")
def first(case):
    return launch(case)


def test_special_rows_against_float64(case, first):
    outs, grads = first
    o64, g64 = case.ref64
    worst_v = max(margin(k, v, o64[k], ops_ref.MFMA_VAL) for k, v in outs.items())
    worst_g = max(margin("d " + k, v, g64[k], ops_ref.MFMA_GRAD) for k, v in grads.items())
    print(f"worst margins: values {worst_v:.2e}, gradients {worst_g:.2e}")


def test_two_launches_are_bitwise_equal(case, first):
    outs, grads = first
    outs2, grads2 = launch(case)
    for k in outs:
        assert torch.equal(outs[k], outs2[k]), k
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), "d " + k


def test_destinations_without_in_edges_and_sources_without_out_edges(case, first):
    outs, grads = first
    deg_in = torch.bincount(case.ei[1], minlength=N)
    assert bool((outs["x1"].cpu()[deg_in == 0] == 0).all()), "destinations without in-edges are exactly 0"
    assert torch.isfinite(grads["x"]).all() and torch.isfinite(outs["out"]).all()
