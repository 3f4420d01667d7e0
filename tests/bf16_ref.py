"""Float64 emulation of the plain-bf16 build of the edge / node kernels (entry points ``*_bf16``: csrc/grl_common.h GRL_PREC = 1).

Rounding points, as the GRL_PREC branches of csrc/edge_conv16.hip, csrc/node_mlp16.hip and csrc/node_ops.hip place them:

* latents, messages and the gradients handed between kernels are stored as bf16: the caller rounds the inputs to bf16 first, so the
  reference sees the values the kernels load, and each stored tensor is rounded once (``store``; its backward rounds the incoming
  stored gradient in the same way);
* every MFMA product takes both operands rounded to nearest bf16 (``split_pair`` / ``pack_rn``: no lo halves), accumulates in fp32 --
  here in float64 -- and adds the fp32 bias in the accumulator (``mm``, forward and backward: the backward rounds the incoming gradient
  and reuses the rounded forward operands; the first basis layer's bias gradient is an MFMA column of that rounded gradient too);
* GELU is the build's logistic approximant x sigma(1.5976 x + 0.07056 x^3) with its exact derivative (the GRL_PREC branches of csrc/grl_common.h);
* polynomial features, LayerNorm, the per-edge product K_e * x_src and the softmax stay in fp32 arithmetic (float64 here);
* the fiber convolution and the lift (csrc/node_ops.hip) have no MFMA: fp32 multiply-adds on the values as loaded (bf16 latents widened
  exactly; fk, bias, the node features and the encoder stay fp32), so ``fiber_conv`` / ``lift_encode`` round nothing but their one store;
  their weight gradients are fp32 partial sums of products of bf16-exact gradients (autograd's, in float64 here).

``rounding=False, logistic=False`` turns every rounding off and restores the erf GELU: the functions then reproduce the oracle
(tests/test_bf16_ref_cpu.py pins that to 1e-12)."""
import torch
import torch.nn.functional as F


def bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to nearest bf16 and widen back to the tensor's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def ulp16(t: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 numbers at |t| (8 significant bits): what one rounding to nearest bf16 may move a value by, twice over."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


class _Store(torch.autograd.Function):
    """A tensor written to bf16 memory: rounded once forward; the gradient that comes back is read from bf16 memory too."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _MM(torch.autograd.Function):
    """y = x W^T (+ b) as one bf16 MFMA per product: operands rounded to nearest bf16, wide accumulation; backward the same for
    dx = dy W and dW = dy^T x (the incoming gradient rounded as an MFMA operand).  ``round_db``: the bias gradient rides in the same MFMA
    as a column of ones (the basis network's first layer: edge_conv16.hip "dW1 (| db1) += dZ1^T (phi | 1)"), so it sums the ROUNDED
    gradient; otherwise it is a plain fp32 sum of the unrounded one (db2, the node block's biases)."""

    @staticmethod
    def forward(ctx, x, w, b, round_db):
        xr, wr = bf16(x), bf16(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_b, ctx.round_db = b is not None, round_db
        y = xr @ wr.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = bf16(g)
        dx = gr @ wr
        dw = gr.reshape(-1, gr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1])
        db = (gr if ctx.round_db else g).reshape(-1, g.shape[-1]).sum(0) if ctx.has_b else None
        return dx, dw, db, None


def store(x, rounding=True):
    return _Store.apply(x) if rounding else x


def mm(x, w, b=None, rounding=True, round_db=False):
    return _MM.apply(x, w, b, round_db) if rounding else F.linear(x, w, b)


def gelu_logistic(x):
    """x sigma(1.5976 x + 0.07056 x^3): the build's approximant of the erf GELU (autograd gives its exact derivative)."""
    return x * torch.sigmoid(x * (1.5976 + 0.07056 * x * x))


def gelu(x, logistic=True):
    return gelu_logistic(x) if logistic else F.gelu(x)


def polynomial_features(x, degree=2):
    polys = [x]
    for _ in range(degree):
        polys.append(torch.einsum("...i,...j->...ij", polys[-1], x).flatten(-2, -1))
    return torch.cat(polys, -1)


def basis_mlp(inv, w1, b1, w2, b2, rounding=True, logistic=True):
    """Poly -> Linear -> GELU -> Linear -> GELU of the edge invariants [E,O,2] -> [E,O,64] (oracle.equivariant.basis_mlp)."""
    h = gelu(mm(polynomial_features(inv), w1, b1, rounding, round_db=True), logistic)
    return gelu(mm(h, w2, b2, rounding), logistic)


def spatial_invariants(grid, pos_send, pos_receive):
    rel = (pos_send - pos_receive)[:, None, :]
    ga = grid[None, :, :]
    inv1 = (rel * ga).sum(dim=-1, keepdim=True)
    inv2 = (rel - inv1 * ga).norm(dim=-1, keepdim=True)
    return torch.cat([inv1, inv2], dim=-1)


def edge_kernels(grid, pos_s, pos_d, w1, b1, w2, b2, wk, rounding=True, logistic=True):
    """K_e = Wk basis_mlp(invariants_e) per edge [E,O,64] (pos_s / pos_d: the two ends' positions per edge)."""
    return mm(basis_mlp(spatial_invariants(grid, pos_s, pos_d), w1, b1, w2, b2, rounding, logistic), wk, None, rounding)


def edge_messages(x_src, src, grid, pos_s, pos_d, w1, b1, w2, b2, wk, rounding=True, logistic=True, stored=True):
    """msg[e] = K_e * x_src[src[e]], stored per edge (EdgeMessages).  ``stored=False``: the value before its store rounding."""
    m = edge_kernels(grid, pos_s, pos_d, w1, b1, w2, b2, wk, rounding, logistic) * x_src[src]
    return store(m, rounding and stored)


def edge_conv(x_src, src, dst, n_dst, grid, pos_s, pos_d, w1, b1, w2, b2, wk, rounding=True, logistic=True, stored=True):
    """x1[d] = sum over the in-edges of d of K_e * x_src[src[e]] (EdgeConv): the sum in the wide accumulator, stored once."""
    m = edge_kernels(grid, pos_s, pos_d, w1, b1, w2, b2, wk, rounding, logistic) * x_src[src]
    out = torch.zeros((n_dst,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device).index_add(0, dst, m)
    return store(out, rounding and stored)


def node_mlp(x2, x_dst, gamma, beta, w3, b3, w4, b4, prev=None, rounding=True, logistic=True, stored=True):
    """out = [prev +] x_dst + W4 GELU(W3 LN(x2) + b3) + b4 (NodeMLP), stored once."""
    h = F.layer_norm(x2, (x2.shape[-1],), gamma, beta, 1e-5)
    out = x_dst + mm(gelu(mm(h, w3, b3, rounding), logistic), w4, b4, rounding)
    if prev is not None:
        out = out + prev
    return store(out, rounding and stored)


def fiber_conv(x1, fk, bias, rounding=True, stored=True):
    """x2[n,p,c] = 1/16 sum_o x1[n,o,c] fk[o,p,c] + bias[c] (FiberConv): fp32 arithmetic on the loaded values, stored once."""
    return store(torch.einsum("boc,opc->bpc", x1, fk) / fk.shape[-2] + bias, rounding and stored)


def lift_encode(scal, vec, grid, w_enc, rounding=True, stored=True):
    """x[n,o,:] = [scal[n,:] | vec[n,v,:] . grid[o,:]] W_enc^T (LiftEncode; scal [N,S], vec [N,V,3], grid [16,dim], dim 2: the z parts are
    unused): fp32 arithmetic on fp32 inputs, stored once."""
    n, dim = scal.shape[0], grid.shape[1]
    feat = torch.cat([scal[:, None, :].expand(n, grid.shape[0], scal.shape[1]), torch.einsum("nvd,od->nov", vec[..., :dim], grid)], -1)
    return store(F.linear(feat, w_enc), rounding and stored)


def softmax_aggregate(gate, msg, dst, n_dst):
    """PyG softmax (gate given directly) and the weighted sum: exp(g - max) / (sum + 1e-16), max detached -> x1 [n_dst,...]."""
    idx = dst.reshape(-1, *([1] * (gate.dim() - 1))).expand_as(gate)
    mx = torch.full((n_dst,) + tuple(gate.shape[1:]), -float("inf"), dtype=gate.dtype, device=gate.device)
    mx = mx.scatter_reduce(0, idx, gate.detach(), "amax", include_self=True)
    ex = (gate - mx[dst]).exp()
    den = torch.zeros_like(mx).index_add(0, dst, ex) + 1e-16
    alpha = ex / den[dst]
    x1 = torch.zeros_like(mx).index_add(0, dst, alpha * msg)
    return x1, alpha


def softmax_aggregate_bwd(alpha, msg, x1, dx1, dst):
    """Closed form of the backward: d msg_e = alpha_e dx1,  d gate_e = alpha_e dx1 (msg_e - x1)  (x1 before any store rounding);
    also the magnitude term alpha |dx1| (|msg| + |x1|) that bounds the rounding of d gate's cancelling terms."""
    g = dx1[dst]
    dmsg = alpha * g
    dgate = alpha * g * (msg - x1[dst])
    mag = alpha * g.abs() * (msg.abs() + x1[dst].abs())
    return dmsg, dgate, mag


# ------------------------------------------------------------------------------------------------ cases of the per-op tests
# The fp32 suite's inputs (tests/actor_cases.py) as the bf16 build sees them: every latent-typed input and every upstream gradient rounded
# to bf16 first, the emulation above in place of the oracle's maths, the output BEFORE its store rounding (the tests allow the store's half
# ulp on top of the bar: margin16).  tests/test_gpu_bf16_ops.py feeds them to the kernels; tests/test_bf16_ref_cpu.py evaluates them in
# fp32 and in float64 to measure how far last-bit differences alone move the emulation.
LATENTS = ("x1", "x2", "x_dst", "prev", "x_src", "dres", "x")


def as_bf16_case(case, ref):
    import actor_cases as ac
    inputs = {k: (bf16(v) if k in LATENTS else v) for k, v in case.inputs.items()}
    ups = {k: (bf16(u) if u is not None else None) for k, u in case.ups.items()}
    c = ac.Case(case.name + " (bf16 build)", inputs, case.diff, ref, ups)
    c.meta = getattr(case, "meta", None)
    return c


def fiber_conv_case(n):
    import actor_cases as ac
    return as_bf16_case(ac.fiber_conv_case(n), lambda t: {"x2": fiber_conv(t["x1"], t["fk"], t["bias"], stored=False)})


def lift_case(n, grid_kind, S=3, V=4, tag=0):
    import actor_cases as ac
    return as_bf16_case(ac.lift_case(n, grid_kind, S, V, tag), lambda t: {"x": lift_encode(t["scal"], t["vec"], t["grid"], t["w"], stored=False)})


def lift_multi_case(ns, left_out, S, V, grid_kind):
    """Several node types behind one encoder (LiftEncodeMulti): type i is lift_case(ns[i], ..., tag=i); the first type's encoder is
    everybody's; ``left_out``: index of a type whose output gets no gradient."""
    import actor_cases as ac
    cases = [lift_case(n, grid_kind, S, V, tag=i) for i, n in enumerate(ns)]
    inputs = {"w": cases[0].inputs["w"], "grid": ac.grid_of(grid_kind)}
    for i, c in enumerate(cases):
        inputs[f"scal{i}"], inputs[f"vec{i}"] = c.inputs["scal"], c.inputs["vec"]
    ref = lambda t: {f"x{i}": lift_encode(t[f"scal{i}"], t[f"vec{i}"], t["grid"], t["w"], stored=False) for i in range(len(ns))}
    ups = {f"x{i}": (None if i == left_out else c.ups["x"]) for i, c in enumerate(cases)}
    return ac.Case(f"lift multi {ns} left out {left_out} S{S} V{V} {grid_kind} (bf16 build)", inputs, ["w"], ref, ups)


def node_mlp_case(family, n, use_prev):
    import actor_cases as ac
    ref = lambda t: {"out": node_mlp(t["x2"], t["x_dst"], t["gamma"], t["beta"], t["w3"], t["b3"], t["w4"], t["b4"], t.get("prev"), stored=False)}
    return as_bf16_case(ac.node_mlp_case(family, n, use_prev), ref)


def edge_case(kind, with_dres):
    import actor_cases as ac
    c0 = ac.edge_case(kind, with_dres)
    ei, n_src, n_dst, dim, gk = c0.meta

    def ref(t):
        ps, pd = t["pos_s"][t["src"]][:, :dim], t["pos_d"][t["dst"]][:, :dim]
        out = {"x1": edge_conv(t["x_src"], t["src"], t["dst"], n_dst, t["grid"], ps, pd, t["w1"], t["b1"], t["w2"], t["b2"], t["wk"], stored=False)}
        if with_dres:   # the residual gradient enters as a second, linear use of x_src: d x_src = the convolution's + dres
            out["res"] = (t["x_src"] * t["dres"]).sum().reshape(1)
        return out
    return as_bf16_case(c0, ref)


def conv_block_case(n, E):
    """hepi._conv: x feeds the convolution AND the residual of its own node block.  x1 is STORED between the two kernels (rounded once);
    d x is the sum of both branches (the node block hands d out to the edge backward, which adds it inside its d x_src kernel)."""
    import actor_cases as ac
    g = ac.gen(9, n, E)
    ei = torch.stack([torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)])
    pos = torch.rand(n, 3, generator=g) * 2 - 1
    we = ac.weights(g, [(64, 14), (64,), (64, 64), (64,), (64, 64)])
    wm = [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1] + ac.weights(g, [(256, 64), (256,), (64, 256), (64,)])
    inputs = {"x": torch.randn(n, 16, 64, generator=g), "pos": pos, "grid": ac.grid_of("upper"), "src": ei[0], "dst": ei[1]}
    inputs.update({f"e{i}": w for i, w in enumerate(we)})
    inputs.update({f"m{i}": w for i, w in enumerate(wm)})

    def ref(t):
        x1 = edge_conv(t["x"], t["src"], t["dst"], n, t["grid"], t["pos"][t["src"]], t["pos"][t["dst"]], *[t[f"e{i}"] for i in range(5)], stored=True)
        return {"out": node_mlp(x1, t["x"], *[t[f"m{i}"] for i in range(6)], stored=False)}
    c = ac.Case(f"conv + node block n={n} E={E}", inputs, ["x"] + [f"e{i}" for i in range(5)] + [f"m{i}" for i in range(6)], ref,
                {"out": torch.randn(n, 16, 64, generator=g)})
    c = as_bf16_case(c, ref)
    c.meta = (ei, n)
    return c
