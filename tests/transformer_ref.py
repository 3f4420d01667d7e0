"""float64 restatement of the transformer baseline actor's encoder (transformer_vanilla.py:29-36,87-92: torch's post-norm encoder layer,
hidden 64, 2 layers, 2 heads, feed-forward 64, no dropout, no mask, no final norm) and of the post_fc head, written out -- no call into
``nn.TransformerEncoder`` -- with its backward by autograd in float64; the cases and the checker of tests/test_gpu_transformer_ops.py.

Parameter order everywhere (``PARAM_NAMES``): the 28 tensors of ``ops.TransformerEncode`` / geometry_rl_amd/csrc/grl_transformer.h.

The allowance of ``check`` is not a constant: per tensor it is max(4 x the error of the STOCK torch fp32 module on the CPU against the same
float64 values, 8 * 2^-24 * max|ref|).  The factor 4 covers other summation orders (64-term dots, n-term softmax sums, B*n-term
weight-gradient sums); the floor is eight roundings of the tensor's largest entry."""
import math

import torch
import torch.nn as nn

LAYER_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight",
               "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")
PARAM_NAMES = (["embedding.weight", "embedding.bias"] + [f"transformer_encoder.layers.{l}.{k}" for l in range(2) for k in LAYER_NAMES]
               + ["fc_out.lins.0.weight", "fc_out.lins.0.bias"])
MARGIN, FLOOR_ULPS = 4.0, 8.0


def layer_norm(z, g, b, eps=1e-5):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)   # biased
    return (z - mean) / torch.sqrt(var + eps) * g + b


def encode(u, params, m0, G, mistake=None):
    """u [B,n,d_in], params: the 28 tensors (any dtype; float64 for the reference) -> hidden [B*G,64].  ``mistake``: one of the seeded
    errors the checker must notice ("no_scale", "pre_norm", "interleaved_heads"), None for the model itself."""
    We, be = params[0], params[1]
    x = u @ We.T + be
    B, n, _ = x.shape
    for l in range(2):
        Win, bin_, Wo, bo, g1, b1n, W1, b1, W2, b2, g2, b2n = params[2 + 12 * l:14 + 12 * l]
        src = layer_norm(x, g1, b1n) if mistake == "pre_norm" else x
        qkv = src @ Win.T + bin_
        q, k, v = qkv[..., :64], qkv[..., 64:128], qkv[..., 128:]
        heads = []
        for h in range(2):
            sel = slice(h, 64, 2) if mistake == "interleaved_heads" else slice(32 * h, 32 * h + 32)
            s = q[..., sel] @ k[..., sel].transpose(-1, -2)
            if mistake != "no_scale":
                s = s / math.sqrt(32.0)
            heads.append(torch.softmax(s, dim=-1) @ v[..., sel])
        if mistake == "interleaved_heads":
            o = torch.stack(heads, dim=-1).reshape(B, n, 64)
        else:
            o = torch.cat(heads, dim=-1)
        a = o @ Wo.T + bo
        if mistake == "pre_norm":
            y = x + a
            x = y + (torch.relu(layer_norm(y, g2, b2n) @ W1.T + b1) @ W2.T + b2)
        else:
            y = layer_norm(x + a, g1, b1n)
            x = layer_norm(y + (torch.relu(y @ W1.T + b1) @ W2.T + b2), g2, b2n)
    return x[:, m0:m0 + G].reshape(B * G, 64) @ params[26].T + params[27]


def head(hidden, wm, bm, ws, bs, shift, min_std):
    return hidden @ wm.T + bm, torch.nn.functional.softplus(hidden @ ws.T + bs + shift) + min_std


def stock_module(d_in, seed, dtype=torch.float32):
    """The package's stock-torch module (kernels="torch") on the CPU with random parameters: biases and LayerNorm parameters too, so that
    nothing the formulas name is zero or one by construction."""
    from geometry_rl_amd.transformer import TransformerVanilla
    g = torch.Generator().manual_seed(seed)
    m = TransformerVanilla(d_in, 64, num_layers=2, num_heads=2, hidden_dim=64, dropout=0.0)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (0.6 / math.sqrt(p.shape[-1])))
            elif "norm" in k and k.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
    return m.to(dtype)


def module_params(m):
    return m.encoder_parameters()


class Graph:
    """What ``TransformerVanilla.one_step`` reads of a graph batch."""

    def __init__(self, B, m0, G):
        self.batch_size, self.output_mask = B, slice(m0, m0 + G)


VALUE_CASES = ("plain", "logits60", "equal_keys", "zero_variance", "relu_zero")


def apply_value_case(m, case):
    """Edit the module's parameters in place for one of the value cases of the per-op test."""
    L = m.transformer_encoder.layers
    with torch.no_grad():
        if case == "logits60":      # EncoderCase scales the query / key projections to the span (it needs the inputs for that)
            pass
        elif case == "equal_keys":  # k = its bias for every token: uniform weights, every logit of a row ties
            for lyr in L:
                lyr.self_attn.in_proj_weight[64:128].zero_()
        elif case == "zero_variance":   # x_0 constant over the channels and a = 0: the first LayerNorm sees variance 0
            m.embedding.weight.copy_(m.embedding.weight[:1].expand_as(m.embedding.weight).clone())
            m.embedding.bias.fill_(0.25)
            L[0].self_attn.out_proj.weight.zero_()
            L[0].self_attn.out_proj.bias.zero_()
        elif case == "relu_zero":   # hidden unit 5 of both layers: W1 y + b1 is exactly 0, where relu' = 0
            for lyr in L:
                lyr.linear1.weight[5].zero_()
                lyr.linear1.bias[5] = 0.0
        elif case != "plain":
            raise KeyError(case)
    return m


def first_layer_logits(u, params):
    """s_h[i,j] of layer 0, both heads, in float64: [2,B,n,n]."""
    p = [t.detach().double() for t in params[:4]]
    qkv = (u.double() @ p[0].T + p[1]) @ p[2].T + p[3]
    return torch.stack([qkv[..., 32 * h:32 * h + 32] @ qkv[..., 64 + 32 * h:96 + 32 * h].transpose(-1, -2) for h in range(2)]) / math.sqrt(32.0)


class EncoderCase:
    """One shape / value case: inputs, the float64 reference (hidden and the 28 gradients for the cotangent R) and the stock fp32 CPU
    module's values of the same.  Computed once, read by every test that needs it."""

    def __init__(self, B, n, d_in, m0, G, value="plain", seed=0):
        self.B, self.n, self.d_in, self.m0, self.G = B, n, d_in, m0, G
        g = torch.Generator().manual_seed(1000 + seed)
        self.u = torch.randn(B, n, d_in, generator=g)
        self.R = torch.randn(B * G, 64, generator=g)
        self.module = apply_value_case(stock_module(d_in, seed), value)
        if value == "logits60":   # the first layer's logits span +-60: exp overflows (or flushes every other entry) without the row-maximum shift
            with torch.no_grad():
                f = math.sqrt(60.0 / float(first_layer_logits(self.u, module_params(self.module)).abs().max()))
                for lyr in self.module.transformer_encoder.layers:
                    lyr.self_attn.in_proj_weight[:128].mul_(f)
                    lyr.self_attn.in_proj_bias[:128].mul_(f)
        self.params = [p.detach().clone() for p in module_params(self.module)]
        p64 = [p.double().requires_grad_(True) for p in self.params]
        h64 = encode(self.u.double(), p64, m0, G)
        self.ref = {"hidden": h64.detach()}
        for k, gr in zip(PARAM_NAMES, torch.autograd.grad(h64, p64, self.R.double())):
            self.ref["d " + k] = gr
        m = self.module
        m.zero_grad()
        hs = m.one_step(Graph(B, m0, G), self.u)
        hs.backward(self.R)
        self.stock = {"hidden": hs.detach()}
        for k, p in zip(PARAM_NAMES, module_params(m)):
            self.stock["d " + k] = p.grad.detach().clone()


def allowance(ref, stock):
    floor = FLOOR_ULPS * 2.0 ** -24 * float(ref.abs().max())
    return max(MARGIN * float((stock.double() - ref).abs().max()), floor)


def check(name, got, ref, stock):
    """Entry-wise: max|got - ref| <= allowance(ref, stock).  -> (error, allowance, error / the stock module's error)."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{name}: non-finite entries"
    err, allow = float((got - ref).abs().max()), allowance(ref, stock)
    stock_err = float((stock.double() - ref).abs().max())
    assert err <= allow, f"{name}: max error {err:.3e} > allowance {allow:.3e} (stock fp32 error {stock_err:.3e}, max|ref| {float(ref.abs().max()):.3e})"
    return err, allow, err / max(stock_err, FLOOR_ULPS * 2.0 ** -24 * float(ref.abs().max()) / MARGIN, 1e-300)


def check_all(label, got: dict, case: EncoderCase, ratios: dict):
    """Every tensor of ``got`` against the case; the largest error ratio per tensor class is kept in ``ratios``."""
    for k, v in got.items():
        _, _, r = check(f"{label}: {k}", v, case.ref[k], case.stock[k])
        cls = "hidden" if k == "hidden" else ("bias/norm gradient" if case.ref[k].dim() == 1 else "weight gradient")
        ratios[cls] = max(ratios.get(cls, 0.0), r)
