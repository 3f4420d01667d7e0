"""Pins tests/train_ops_ref.py, the float64 restatements that tests/test_gpu_train_ops.py checks the training-loop kernels against: Adam (with
clipping and a learning rate that changes between steps) must BE torch.optim.Adam(eps=1e-5) after clip_grad_norm_, GAE must be
oracle.trpl.gae_shifted, VecNorm must be oracle.transforms.vecnorm_update, all in float64 to 1e-12; the kNN brute force must follow its stated
order.  The fp32 allowances are checked against a plain fp32 emulation of the kernels' arithmetic: it must land inside them."""
import numpy as np
import torch

import train_ops_ref as tr
from oracle import transforms as otf
from oracle import trpl as otr


def close(name, a, b, tol=1e-12):
    err = float((a.double() - b.double()).abs().max())
    sc = max(1.0, float(b.double().abs().max()))
    assert err <= tol * sc, (name, err, sc)


def _grads(g, n, steps):
    """Gradients of every kind the GPU test uses: exact zeros, ~1e-5, ordinary, 1e3-1e4."""
    out = []
    for s in range(steps):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        kind = torch.randint(0, 4, (n,), generator=g)
        x = torch.where(kind == 0, torch.zeros_like(x), x)
        x = torch.where(kind == 1, x * 1e-5, x)
        x = torch.where(kind == 3, x * 5e3, x)
        out.append(x)
    return out


def test_adam_is_torch_adam():
    g = torch.Generator().manual_seed(0)
    n = 257
    for betas, max_norm in (((0.9, 0.999), None), ((0.8, 0.99), 10.0), ((0.9, 0.999), 1e5)):
        p0 = torch.randn(n, generator=g, dtype=torch.float64)
        w = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([w], lr=3e-4, betas=betas, eps=1e-5)
        p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for t, gr in enumerate(_grads(g, n, 12), start=1):
            lr = 3e-4 * (1.0 - t / 20)          # annealed between steps, as train.py does
            opt.param_groups[0]["lr"] = lr
            w.grad = gr.clone()
            scale = 1.0
            if max_norm is not None:
                scale = tr.clip_coef(gr, max_norm)
                torch.nn.utils.clip_grad_norm_([w], max_norm)
            opt.step()
            p, m, v = tr.adam(p, gr, m, v, lr, betas[0], betas[1], 1e-5, t, scale)
            close(f"p t={t}", p, w.detach())
            close(f"m t={t}", m, opt.state[w]["exp_avg"])
            close(f"v t={t}", v, opt.state[w]["exp_avg_sq"])


def _adam_f32(p, g, m, v, lr, b1, b2, eps, t, scale):
    """The kernels' Adam arithmetic, operation by operation, in numpy float32, with every multiply-add rounded twice (the kernels fuse
    three of them, grl_common.h adam_element: one rounding fewer each; the allowance must hold either way)."""
    f = np.float32
    p, g, m, v = (x.float().numpy().copy() for x in (p, g, m, v))
    b1, b2, eps, lr, scale = f(b1), f(b2), f(eps), f(lr), f(scale)
    bc1 = f(1) - np.power(b1, f(t), dtype=np.float32)
    bc2s = np.sqrt(f(1) - np.power(b2, f(t), dtype=np.float32))
    gi = g * scale
    mi = b1 * m + (f(1) - b1) * gi
    vi = b2 * v + (f(1) - b2) * gi * gi
    p = p - (lr / bc1) * (mi / (np.sqrt(vi) / bc2s + eps))
    return torch.from_numpy(p), torch.from_numpy(mi), torch.from_numpy(vi)


def test_adam_allowance_covers_fp32_arithmetic():
    g = torch.Generator().manual_seed(1)
    n = 4099
    worst = 0.0
    for betas in ((0.9, 0.999), (0.8, 0.99)):
        b1, b2 = tr.f32(betas[0]), tr.f32(betas[1])
        for t0 in (1, 10 ** 4, 10 ** 6):
            p = torch.randn(n, generator=g).float()
            m, v = torch.zeros(n), torch.zeros(n)
            for s, gr in enumerate(_grads(g, n, 30)):
                t, lr = t0 + s, tr.f32(1e-3 / (1 + s))
                gr = gr.float()
                scale = tr.f32(0.37) if s % 3 == 0 else 1.0
                p1, m1, v1 = _adam_f32(p, gr, m, v, lr, b1, b2, tr.f32(1e-5), t, scale)
                rp, rm, rv = tr.adam(p, gr, m, v, lr, b1, b2, tr.f32(1e-5), t, scale)
                ap, am, av = tr.adam_allowance(p, gr, m, v, lr, b1, b2, tr.f32(1e-5), t, scale)
                for name, a, b, al in (("p", p1, rp, ap), ("m", m1, rm, am), ("v", v1, rv, av)):
                    r = float(((a.double() - b).abs() / al.clamp_min(1e-300)).max())
                    worst = max(worst, r)
                    assert r <= 1.0, (name, t, r)
                p, m, v = p1, m1, v1
    print(f"fp32 Adam emulation: worst error / allowance {worst:.3f}")


def _gae_inputs(g, N, T):
    r = torch.randn(N, T, generator=g)
    V = torch.randn(N, T + 1, generator=g) * 3
    done = torch.rand(N, T, generator=g) < 0.05
    term = torch.rand(N, T, generator=g) < 0.05
    return r, done, term, V


def test_gae_is_gae_shifted():
    g = torch.Generator().manual_seed(2)
    for N, T, gamma, lmbda in ((5, 1, 0.99, 0.95), (7, 130, 0.97, 0.9)):
        r, done, term, V = _gae_inputs(g, N, T)
        done[:, -1] = True
        term[0, :] = ~done[0, :]          # terminated without done somewhere, and done without terminated
        a, t_, _, _ = tr.gae(r, done, term, V, gamma, lmbda)
        ao, to = otr.gae_shifted(r.double(), done, term, V.double(), gamma, lmbda)
        close("adv", a, ao)
        close("target", t_, to)


def test_gae_allowance_covers_fp32_scan():
    g = torch.Generator().manual_seed(3)
    N, T = 33, 300
    r, done, term, V = _gae_inputs(g, N, T)
    r[:4] *= 1e3
    gamma, lmbda = tr.f32(0.99), tr.f32(0.95)
    a, t_, ea, et = tr.gae(r, done, term, V, gamma, lmbda)
    f = np.float32
    rn, Vn = r.numpy(), V.numpy()
    nt, nd = (~term).numpy().astype(np.float32), (~done).numpy().astype(np.float32)
    run = np.zeros(N, np.float32)
    adv = np.zeros((N, T), np.float32)
    for k in range(T - 1, -1, -1):
        delta = rn[:, k] + f(gamma) * nt[:, k] * Vn[:, k + 1] - Vn[:, k]
        run = delta + f(gamma) * f(lmbda) * nd[:, k] * run
        adv[:, k] = run
    tgt = adv + Vn[:, :-1]
    assert float(((torch.from_numpy(adv).double() - a).abs() / ea).max()) <= 1.0
    assert float(((torch.from_numpy(tgt).double() - t_).abs() / et).max()) <= 1.0


def test_vecnorm_is_vecnorm_update():
    g = torch.Generator().manual_seed(4)
    for K, decay in ((3, 0.99999), (7, 0.9)):
        st = otf.VecNormState(K)
        st.sum, st.ssq, st.count = st.sum.double(), st.ssq.double(), st.count.double()
        state = torch.zeros(2 * K + 1, dtype=torch.float64)
        for call in range(4):
            x = torch.randn(50 + call, K, generator=g, dtype=torch.float64) * 2 + 1
            update = call < 3
            y_o = otf.vecnorm_update(x, st, decay, 1e-2, update)
            state, _ = tr.vecnorm_state(x, state, decay, update)
            close("sum", state[:K], st.sum)
            close("ssq", state[K:2 * K], st.ssq)
            close("count", state[2 * K:], st.count)
            y, _ = tr.vecnorm_apply(x, state, 1e-2, -1e9, 1e9)
            close("y", y, y_o)
            y, _ = tr.vecnorm_apply(x, state, 1e-2, -0.5, 0.5)
            close("y clipped", y, otf.clip(y_o, -0.5, 0.5))


def test_knn_order_and_padding():
    # a line of points 0, 1, 2, 4 (+ a duplicate of 1): point 1's neighbours are 4 (distance 0), then 0 and 2 (distance 1: lower index first)
    pos = torch.tensor([[[0., 0, 0], [1, 0, 0], [2, 0, 0], [4, 0, 0], [1, 0, 0], [9, 9, 9]]])
    out = tr.knn(pos, torch.tensor([5]), 3)
    assert out[0, 1].tolist() == [4, 0, 2]
    assert out[0, 3].tolist() == [2, 1, 4]
    assert out[0, 5].tolist() == [-1, -1, -1]                    # padding point
    assert tr.knn(pos, torch.tensor([2]), 3)[0, 0].tolist() == [1, -1, -1]
    assert (tr.knn(pos, torch.tensor([0]), 2) == -1).all()
    # against a stable argsort of the distance matrix on random points
    g = torch.Generator().manual_seed(5)
    p = torch.randint(-3, 4, (2, 40, 3), generator=g).double()
    out = tr.knn(p, None, 8)
    for b in range(2):
        d = torch.cdist(p[b], p[b]) ** 2
        d.fill_diagonal_(float("inf"))
        idx = torch.sort(d, dim=1, stable=True).indices[:, :8]
        assert torch.equal(out[b].long(), idx)
