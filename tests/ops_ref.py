"""float64 references of the fp32 actor and critic ops (geometry_rl_amd.ops), written from the formulas in include/grl_hip.h and the
oracle (oracle/equivariant.py, oracle/trpl.py, oracle/graph.py) -- plain torch with autograd, no GPU needed, no kernel library.
tests/test_ops_ref_cpu.py pins every function to the oracle; tests/test_gpu_actor_ops.py holds the HIP kernels against them.

The functions run in whatever dtype and on whatever device their inputs have: float64 on the CPU is the reference, float64 on the GPU
the reference of the large cases, float32 on the CPU the yardstick the bars of the plain-FMA kernels are derived from (``BARS``)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import equivariant as eq

# Bars, each a fraction of the tensor's OWN scale (its largest reference entry): (forward values, gradients).
# MFMA ops (split-bf16 products): the project's bars for that chain (tests/test_gpu_attention_ops.py, tests/test_gpu_ops.py).
# Plain fp32 FMA ops: 8 x the worst error of the fp32 torch CPU evaluation of the function below against its float64 evaluation on the
# same inputs, rounded up to one significant digit, never above OLD_BARS -- tests/test_ops_ref_cpu.py prints the table and checks them.
MFMA_VAL, MFMA_GRAD = 1e-4, 2e-4
OLD_BARS = {"fiber_conv": (1e-4, 2e-4), "lift": (1e-4, 2e-4), "fiber_basis": (1e-4, 2e-4), "readout": (1e-4, 2e-4),
            "deepsets": (2e-5, 1e-4)}   # what tests/test_gpu_ops.py allows (fiber_basis: no per-op test before; the fp32 chain's bars)
BARS = {"fiber_conv": (9e-7, 4e-6), "lift": (2e-6, 6e-6), "fiber_basis": (4e-6, 7e-6), "readout": (5e-6, 2e-5), "deepsets": (1e-5, 4e-5)}


def round_up_1(x: float) -> float:
    """x rounded up to one significant digit."""
    if x <= 0:
        return 0.0
    e = int(np.floor(np.log10(x)))
    m = int(np.ceil(x / 10.0 ** e - 1e-9))
    return float(f"{m}e{e}")


def derived_bar(worst_fp32: float, old: float) -> float:
    return min(old, round_up_1(8.0 * worst_fp32))


def rel_err(got, ref) -> float:
    """max|got - ref| / max|ref| (0 for an exact match of an all-zero reference, inf for a miss of one)."""
    got, ref = got.detach().double().to(ref.device), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err, sc = float((got - ref).abs().max()), float(ref.abs().max())
    return err / sc if sc > 0 else (0.0 if err == 0 else float("inf"))


def margin(name, got, ref, bar, scale=None):
    """max|got - ref| / scale <= bar, scale = max|ref| unless given; a reference that is exactly zero must be matched exactly."""
    got, ref = got.detach().double().to(ref.device), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    sc = float(ref.abs().max()) if scale is None and ref.numel() else (scale or 0.0)
    m = err / sc if sc > 0 else (0.0 if err == 0 else float("inf"))
    print(f"  {name}: max|err| {err:.3e}, scale {sc:.3e}, margin {m:.2e} (bar {bar:.0e})")
    assert np.isfinite(err) and m <= bar, f"{name}: {m:.3e} of its scale > {bar:.0e}"
    return m


def scatter_sum(msg, index, n):
    """eq.scatter_sum on the device of ``msg``."""
    return torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype, device=msg.device).index_add_(0, index, msg)


# ------------------------------------------------------------------------------------------------ the ops
def edge_conv(x_src, src, dst, n_dst, grid, pos_s, pos_d, w1, b1, w2, b2, wk, dim=3):
    """x1[d] = sum_{e -> d} Wk(basis_mlp(invariants_e)) * x_src[src(e)]; pos_s [n_src, 3], pos_d [n_dst, 3], grid [16, dim]."""
    ps, pd = pos_s[src][:, :dim], pos_d[dst][:, :dim]
    P = {"b.1.weight": w1, "b.1.bias": b1, "b.3.weight": w2, "b.3.bias": b2}
    kb = eq.basis_mlp(eq.spatial_invariants(grid, ps, pd), P, "b")
    return scatter_sum(F.linear(kb, wk) * x_src[src], dst, n_dst)


def node_mlp(x2, x_dst, gamma, beta, w3, b3, w4, b4, prev=None):
    """out = [prev +] x_dst + W4 GELU(W3 LN(x2) + b3) + b4 (exact GELU, LayerNorm over the 64 channels, eps 1e-5 on the variance)."""
    h = F.layer_norm(x2, (x2.shape[-1],), gamma, beta, 1e-5)
    out = x_dst + F.linear(F.gelu(F.linear(h, w3, b3)), w4, b4)
    return out + prev if prev is not None else out


def fiber_conv(x1, fk, bias):
    """x2[n,p,c] = 1/16 sum_o x1[n,o,c] fk[o,p,c] + bias[c]."""
    return torch.einsum("boc,opc->bpc", x1, fk) / fk.shape[-2] + bias


def lift_encode(scal, vec, grid, w_enc):
    """x[n,o,:] = [scal[n,:] | vec[n,v,:] . grid[o,:]] W_enc^T; scal [N,S], vec [N,V,3], grid [16,dim] (dim 2: the z parts are unused)."""
    n, dim = scal.shape[0], grid.shape[1]
    feat = torch.cat([scal[:, None, :].expand(n, grid.shape[0], scal.shape[1]), torch.einsum("nvd,od->nov", vec[..., :dim], grid)], -1)
    return F.linear(feat, w_enc)


def fiber_poly(grid):
    """The (constant) polynomial features of the grid invariants o_o . o_p: [16,16,3]."""
    return eq.polynomial_features(eq.orientation_invariants(grid), 2)


def fiber_kernels(poly, w1, b1, w2, b2, wfs):
    """Phi = GELU(W2 GELU(W1 poly + b1) + b2), fk_i = Phi Wf_i^T (exact GELU) -> [fk_i [16,16,64]]."""
    phi = F.gelu(F.linear(F.gelu(F.linear(poly, w1, b1)), w2, b2))
    return [F.linear(phi, wf) for wf in wfs]


def readout(lat, grid, wd, bd, ws, bs, init_std, min_std, od, ov):
    """Decoder + orientation pooling + contextual std head -> (mean [N,ov,3], sigma [N,3 ov], hidden [N,64]); grid [16,dim]."""
    from oracle import trpl as otr
    n, dim = lat.shape[0], grid.shape[1]
    mean, hidden = eq.readout(lat, wd, bd, grid, dim, od, ov)
    sigma = otr.std_head(hidden, ws, bs, init_std, min_std, n)
    return mean.reshape(n, ov, 3), sigma, hidden


DEEPSETS_KEYS = ["gnn.mlp_inner.lins.0.weight", "gnn.mlp_inner.lins.0.bias", "gnn.mlp_inner.norms.0.weight", "gnn.mlp_inner.norms.0.bias",
                 "gnn.mlp_inner.lins.1.weight", "gnn.mlp_inner.lins.1.bias", "gnn.mlp_outer.lins.0.weight", "gnn.mlp_outer.lins.0.bias",
                 "gnn.mlp_outer.norms.0.weight", "gnn.mlp_outer.norms.0.bias", "gnn.mlp_outer.lins.1.weight", "gnn.mlp_outer.lins.1.bias",
                 "final.weight", "final.bias"]   # the order of ops.DeepSetsPipeline.PARAM_ORDER


def deepsets_value(x, params, masks=None, want_pre=False):
    """DeepSets critic + value head: x [B,n,d], ``params`` in DEEPSETS_KEYS order -> V [B].  LayerNorm over ALL elements of the tensor
    (biased std, eps added to the std).  ``masks`` = (m1 [B,n,64], m2 [B,64]) bool: the ReLU branches to take instead of the reference's
    own (a pre-activation within rounding distance of 0 may take the other branch in fp32 -- the reference then differentiates the
    branch the kernel took, as tests/test_gpu_attention_ops.py does for its gate network)."""
    w1, b1, g1, be1, w2, b2, w3, b3, g2, be2, w4, b4, wv, bv = params

    def gln(h, g, b):
        mean = h.mean()
        return (h - mean) / ((h - mean).std(unbiased=False) + 1e-5) * g + b

    p1 = gln(F.linear(x, w1, b1), g1, be1)
    y1 = F.relu(p1) if masks is None else p1 * masks[0].to(p1.dtype)
    z = F.linear(y1, w2, b2).sum(dim=1)
    p2 = gln(F.linear(z, w3, b3), g2, be2)
    y2 = F.relu(p2) if masks is None else p2 * masks[1].to(p2.dtype)
    v = F.linear(F.linear(y2, w4, b4), wv, bv).reshape(x.shape[0])
    return (v, p1, p2) if want_pre else v
