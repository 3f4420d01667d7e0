"""Per-op checks of csrc/transformer_ops.hip: ``ops.TransformerEncode`` (forward and backward) and ``ops.PostFcHead`` against the
float64 restatement of tests/transformer_ref.py, entry-wise, every output and every parameter gradient.  The allowance per tensor is
computed (transformer_ref.check): 4 x the stock torch fp32 module's CPU error against the same float64 values, floored at 8 roundings
of the tensor's largest entry.  The largest (kernel error / stock error) per tensor class is printed."""
import pytest
import torch

import transformer_ref as tr

pytestmark = pytest.mark.gpu

# (B, n, d_in, m0, G): n = 1, 2 (fewer rows than waves), 33 / 65 (one past the 32 / 64 a half-wave / a wave holds), 64, 240 (cloth), 256
# (the LDS plan's limit); the actuator slice at the start, in the middle, at the end.  B > the 256 workgroups: samples go in groups --
# (259, 2): groups of 2 and a last group of 1; (600, 33): groups of 3 (99 rows, attention inside each sample); (259, 130): a group cannot
# hold two samples, so the workgroups' loop wraps
SHAPES = [(1, 1, 1, 0, 1), (3, 2, 13, 0, 1), (3, 2, 13, 1, 1), (1, 33, 15, 32, 1), (3, 33, 15, 0, 4), (3, 64, 13, 30, 4), (1, 65, 15, 61, 4),
          (1, 240, 15, 236, 4), (3, 256, 13, 255, 1), (1, 256, 1, 100, 4), (259, 2, 13, 0, 1), (600, 33, 15, 31, 2), (259, 130, 13, 64, 1)]
RATIOS = {}
_CASES = {}


def case(*key):
    if key not in _CASES:
        B, n, d_in, m0, G = key[:5]   # the seed is a function of the shape alone: a case is the same whichever tests ran before it
        _CASES[key] = tr.EncoderCase(B, n, d_in, m0, G, value=key[5], seed=(131 * B + 17 * n + 7 * d_in + 3 * m0 + G) % 1000)
    return _CASES[key]


def run_hip(c):
    from geometry_rl_amd import ops
    dev = torch.device("cuda:0")
    leaves = [p.to(dev).requires_grad_(True) for p in c.params]
    hidden = ops.TransformerEncode.apply(c.u.to(dev), c.m0, c.G, *leaves)
    hidden.backward(c.R.to(dev))
    torch.cuda.synchronize()
    out = {"hidden": hidden.detach()}
    out.update({"d " + k: p.grad for k, p in zip(tr.PARAM_NAMES, leaves)})
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}-n{}-d{}-m{}-G{}".format(*s))
def test_encoder_shapes(shape):
    c = case(*shape, "plain")
    got = run_hip(c)
    ratios = {}
    tr.check_all(str(shape), got, c, ratios)
    print(f"transformer encoder {shape}: kernel error / stock fp32 error, largest per class: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)
    again = run_hip(c)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two identical calls differ"
    print(f"largest ratios so far: {RATIOS}")


@pytest.mark.parametrize("value", [v for v in tr.VALUE_CASES if v != "plain"])
def test_encoder_value_cases(value):
    c = case(3, 33, 15, 32, 1, value)
    got = run_hip(c)
    ratios = {}
    tr.check_all(value, got, c, ratios)
    print(f"transformer encoder {value}: kernel error / stock fp32 error, largest per class: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    if value == "relu_zero":   # relu'(0) = 0, as torch: the unit's incoming weights get an exactly-zero gradient
        for l in range(2):
            assert float(got[f"d transformer_encoder.layers.{l}.linear1.weight"][5].abs().max()) == 0.0
            assert float(got[f"d transformer_encoder.layers.{l}.linear1.bias"][5].abs()) == 0.0
    if value == "equal_keys":  # uniform weights: the key projection's weights get no gradient but rounding
        assert torch.isfinite(got["hidden"]).all()


def test_too_many_tokens_are_refused_before_any_launch(monkeypatch):
    from geometry_rl_amd import hip, ops
    dev = torch.device("cuda:0")
    c = case(1, 2, 13, 0, 1, "plain")
    ps = [p.to(dev) for p in c.params]
    u = torch.zeros(1, 257, 13, device=dev)
    saved, stats, hidden = torch.zeros(15, 257, 64, device=dev), torch.zeros(2, 257, 6, device=dev), torch.full((1, 64), 7.0, device=dev)
    assert hip.query("grl_transformer_fwd", u, ps, saved, stats, hidden, 1, 257, 13, 0, 1, hip.stream_ptr()) == -2
    assert hip.query("grl_transformer_fwd", u, ps, saved, stats, hidden, 1, 0, 13, 0, 1, hip.stream_ptr()) == -2
    assert hip.query("grl_transformer_fwd", u, ps, saved, stats, hidden, 1, 200, 13, 199, 2, hip.stream_ptr()) == -2   # slice past the end
    assert hip.query("grl_transformer_fwd", u, ps, saved, stats, hidden, 1, 200, 65, 0, 1, hip.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert float(hidden.min()) == 7.0 and float(saved.abs().max()) == 0.0   # nothing ran
    launched = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), real(entry, *a, **k))[1])
    with pytest.raises(NotImplementedError):
        ops.TransformerEncode.apply(u, 0, 1, *ps)
    assert launched == []


def test_the_one_launch_path_times_every_library():
    """``hip.KERNEL_TIMES`` (bench.py's roofline leg) sees a launch of each kernel library, once each: grl_stats_accumulate of the main
    library at n = 1, grl_kq_project_fwd of the attention library at 65 rows (the smallest count whose backward spans two blocks) and
    grl_postfc_head_fwd of the transformer library at one row."""
    from geometry_rl_amd import hip
    dev = torch.device("cuda:0")
    f = lambda *s: torch.zeros(*s, device=dev)
    assert hip.query("grl_kq_bwd_blocks", 65) == 2
    saved = hip.KERNEL_TIMES
    hip.KERNEL_TIMES = {}
    try:
        hip.call("grl_stats_accumulate", f(1), 1, torch.zeros(2, device=dev, dtype=torch.float64))
        hip.call("grl_kq_project_fwd", f(65, 64), f(128, 64), f(128), f(128, 64), f(128), f(65, 128), f(65, 128), 65, rows=65)
        hip.call("grl_postfc_head_fwd", f(1, 64), f(1, 64), f(1), f(1, 64), f(1), 0.5, 1e-5, f(1, 1), f(1, 1), f(1, 1), 1, 1, rows=1)
        summary = hip.kernel_time_summary()
    finally:
        hip.KERNEL_TIMES = saved
    assert sorted(summary) == ["grl_kq_project_fwd", "grl_postfc_head_fwd", "grl_stats_accumulate"]
    assert all(n == 1 and ms >= 0.0 for n, ms in summary.values()), summary


@pytest.mark.parametrize("R,A,contextual", [(1, 1, True), (5, 6, True), (259, 16, True), (70, 6, False)])
def test_postfc_head(R, A, contextual):
    from geometry_rl_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(R + A)
    hidden = torch.randn(R, 64, generator=g)
    hidden[0, :] *= 12.0   # one row deep in softplus' linear branch (x > 20) and one deep in its exponential tail
    if R > 1:
        hidden[1, :] *= -12.0
    wm, bm = torch.randn(A, 64, generator=g) * 0.3, torch.randn(A, generator=g)
    ws = torch.randn(A, 64, generator=g) * 0.3 if contextual else torch.zeros(A, 64)
    bs = torch.randn(A, generator=g)
    Rm, Rs = torch.randn(R, A, generator=g), torch.randn(R, A, generator=g)
    shift, min_std = 0.5413, 1e-5
    names = ["hidden", "wm", "bm", "ws", "bs"]

    def run(tensors, fn, cot):
        leaves = [t.clone().requires_grad_(True) for t in tensors]
        mean, sigma = fn(*leaves)
        torch.autograd.backward([mean, sigma], cot)
        out = {"mean": mean.detach(), "sigma": sigma.detach()}
        out.update({"d " + k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in zip(names, leaves)})
        return out

    base = [hidden, wm, bm, ws, bs]
    ref = run([t.double() for t in base], lambda *a: tr.head(*a, shift, min_std), [Rm.double(), Rs.double()])
    stock = run(base, lambda *a: tr.head(*a, shift, min_std), [Rm, Rs])
    got = run([t.to(dev) for t in base], lambda *a: ops.PostFcHead.apply(*a, shift, min_std), [Rm.to(dev), Rs.to(dev)])
    again = run([t.to(dev) for t in base], lambda *a: ops.PostFcHead.apply(*a, shift, min_std), [Rm.to(dev), Rs.to(dev)])
    worst = 0.0
    for k in ref:
        _, _, r = tr.check(f"post_fc head R={R} A={A}: {k}", got[k], ref[k], stock[k])
        worst = max(worst, r)
        assert torch.equal(got[k], again[k]), k
    print(f"post_fc head R={R} A={A} contextual={contextual}: largest kernel error / stock fp32 error {worst:.2f}")
    with pytest.raises(NotImplementedError):
        ops.PostFcHead.apply(hidden.to(dev), torch.zeros(17, 64, device=dev), torch.zeros(17, device=dev), torch.zeros(17, 64, device=dev),
                             torch.zeros(17, device=dev), shift, min_std)
