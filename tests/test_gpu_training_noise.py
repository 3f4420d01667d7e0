"""Training noise on the GPU (rigid_tasks_data.py:178-214, rope_tasks_data.py:168-186, pyg_data/utils.py:13-15): the feature launch adds
counter-based Gaussian noise (Philox4x32-10 + Box-Muller, include/grl_hip.h grl_build_features_noise) whose draw counter lives in device
memory.  Checked against the host restatement (tests/noise_ref.py): exact features per family / layout / numbering, the cloth no-op, the
statistics of the stream, a whole update against the oracle fed the same noise, every recorded form against the step-by-step loop,
reproducibility, the collector and two data-parallel ranks."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import graph as ogr
from noise_ref import add_noise
from updater_cases import DEV, dp_ref, make_rollout, run_loop_and_launches, run_step_modes, spawn_dp

pytestmark = pytest.mark.gpu


def _obs(name, B):
    from geometry_rl_amd import graph, synthetic as syn
    if name == "rigid_g1":
        return ogr.rigid_spec(), graph.rigid_spec(), syn.make_rigid_obs(B, seed=3)
    if name == "rigid_g2":   # no angular and no object velocity: the grippers' zero ang column is noisy, the object's vel / ang stay 0
        kw = dict(G=2, angular_velocity=False, object_velocity=False)
        return ogr.rigid_spec(**kw), graph.rigid_spec(**kw), syn.make_rigid_obs(B, seed=4, **kw)
    if name == "rigid_tiny":   # 1, 2, 3, 32, 5, 4 valid object points: padding dropped from the actor graph
        obs = syn.make_rigid_obs(B, seed=9)
        obs["infos"][:, 0] = torch.tensor([1, 2, 3, 32, 5, 4])[torch.arange(B) % 6].float()
        return ogr.rigid_spec(), graph.rigid_spec(), obs
    if name == "rope":
        return ogr.rope_spec(n_links=20), graph.rope_spec(n_links=20), syn.make_rope_obs(B, n_links=20, seed=6)
    if name == "rope_var":
        return (ogr.rope_spec(n_links=20, variable_length=True), graph.rope_spec(n_links=20, variable_length=True),
                syn.make_rope_obs(B, n_links=20, seed=6, variable_length=True))
    if name == "cloth":
        return ogr.cloth_spec(n_particles=25, E_cloth=40), graph.cloth_spec(n_particles=25, E_cloth=40), syn.make_cloth_obs(B, n_particles=25, E_cloth=40, seed=5)
    raise ValueError(name)


def _natural(hd, out, B, dense):
    """HIP features -> {type: [B * n_per, 3 * n_vec]} in the natural (sample, point) order; rows the actor graph dropped are NaN."""
    topo = hd._cache[B]
    n_types = len(hd.spec.node_types)
    res, off = {}, 0
    for t in hd.node_type_list:
        n_per = topo["n_per"][t]
        if dense:
            res[t] = out[:, off:off + n_per, n_types:].reshape(B * n_per, -1)
            off += n_per
            continue
        v = out[1][t].reshape(out[1][t].shape[0], -1)
        nat = torch.full((B * n_per, v.shape[1]), float("nan"), device=v.device)
        if t == topo["main"]:
            nat[topo["gather_main"]] = v
        else:
            nat.copy_(v)
        res[t] = nat
    return res


def _oracle_clean(o_spec, hd, obs, B):
    split = ogr.split_obs(o_spec, {k: v.float() for k, v in obs.items()})
    topo = {"node_types": list(hd.node_type_list), "edge_index": {}, "batch_size": B}
    return ogr.build_features(o_spec, topo, split, hd.dist_as_pos)[2]


def _hd(spec, layout, dist_as_pos, std=0.01, seed=None, noise=True):
    from geometry_rl_amd import graph
    dense = layout == "dense"
    return graph.HyperData(spec, full_graph_obs=dense, dist_as_pos=dist_as_pos, output_mask_key=None if dense else "grippers",
                           concat_input_vector=dense, training_noise=noise, training_noise_std=std, noise_seed=seed)


@pytest.mark.parametrize("balance", [True, False])
@pytest.mark.parametrize("layout", ["per_type", "dense"])
@pytest.mark.parametrize("dist_as_pos", [True, False])
@pytest.mark.parametrize("name", ["rigid_g1", "rigid_g2", "rigid_tiny", "rope", "rope_var"])
def test_features_equal_the_host_restatement(name, dist_as_pos, layout, balance, monkeypatch):
    from geometry_rl_amd import graph
    monkeypatch.setattr(graph, "BALANCE_NODE_ORDER", balance)
    B = 12
    o_spec, spec, obs = _obs(name, B)
    hd = _hd(spec, layout, dist_as_pos, seed=0x1234_5678_9abc_def0 + B)
    obs_d = [obs[k].to(DEV) for k in spec.in_features]
    dense = layout == "dense"
    for it in range(2):   # two successive draws
        seed, draw = hd.noise_state()
        assert draw == it
        out = hd.build_data(*obs_d, train=True)[1]
        got = _natural(hd, out, B, dense)
        clean = _oracle_clean(o_spec, hd, obs, B)
        want, masks = add_noise(spec, clean, B, seed, draw, 0.01, dist_as_pos)
        for t in hd.node_type_list:
            g = got[t].cpu()
            rows = ~torch.isnan(g[:, 0])
            assert rows.any()
            m = torch.from_numpy(masks[t])
            assert masks[t][:3].all()
            err = (g[rows][:, m] - want[t][rows][:, m]).abs().max().item()
            assert err <= 1e-6, (t, err)
            assert torch.equal(g[rows][:, ~m], clean[t][rows][:, ~m]), t   # noise-free slots: bitwise
            if name == "rigid_g2" and t == "object_geometry":
                assert (g[rows][:, 6:] == 0).all()                          # no velocity observation: exactly zero
    assert hd.noise_state()[1] == 2


def test_cloth_is_a_noop():
    B = 6
    o_spec, spec, obs = _obs("cloth", B)
    obs_d = [obs[k].to(DEV) for k in spec.in_features]
    for layout in ("per_type", "dense"):
        a = _hd(spec, layout, True).build_data(*obs_d, train=True)[1]
        b = _hd(spec, layout, True, noise=False).build_data(*obs_d, train=True)[1]
        if layout == "dense":
            assert torch.equal(a, b)
        else:
            for t in a[1]:
                assert torch.equal(a[1][t], b[1][t])


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / (a.std() * b.std()))


def test_noise_statistics():
    B = 4096
    o_spec, spec, obs = _obs("rigid_g1", B)
    obs_d = [obs[k].to(DEV) for k in spec.in_features]
    # the dense layout keeps every padded point: 4096 x (32 object points x 12 + 1 gripper x 9) = 1.6 M noisy elements
    hd = _hd(spec, "dense", False, seed=20261016)
    hc = _hd(spec, "dense", False, noise=False)
    clean = _natural(hc, hc.build_data(*obs_d, train=True)[1], B, True)
    z1 = _natural(hd, hd.build_data(*obs_d, train=True)[1], B, True)
    z2 = _natural(hd, hd.build_data(*obs_d, train=True)[1], B, True)
    samples, comp, slots, succ = [], [], [], []
    for t in hd.node_type_list:
        rows = ~torch.isnan(z1[t][:, 0])
        a = ((z1[t][rows] - clean[t][rows]) / 0.01).double()          # [n, 12]: slots pos, corr, vel, ang (object: all noisy)
        b = ((z2[t][rows] - clean[t][rows]) / 0.01).double()
        noisy = [s for s in range(4) if a[:, 3 * s].abs().max() > 0]
        assert 0 in noisy and 2 in noisy and 3 in noisy
        for s in noisy:
            samples.append(a[:, 3 * s:3 * s + 3].reshape(-1))
            comp += [(a[:, 3 * s], a[:, 3 * s + 1]), (a[:, 3 * s + 1], a[:, 3 * s + 2])]
            succ.append((a[:, 3 * s:3 * s + 3].reshape(-1), b[:, 3 * s:3 * s + 3].reshape(-1)))
        slots.append((a[:, 0], a[:, 6]))
    z = torch.cat(samples)
    n = z.numel()
    assert n > 1_500_000
    mean, std = z.mean().item(), z.std().item()
    c = (z - mean) / std
    skew, kurt = (c ** 3).mean().item(), (c ** 4).mean().item() - 3.0
    zs, _ = torch.sort(z)
    cdf = torch.special.ndtr(zs)
    i = torch.arange(1, n + 1, device=z.device, dtype=torch.float64)
    ks = max((i / n - cdf).max().item(), (cdf - (i - 1) / n).max().item())
    print(f"n {n} mean {mean:.2e} std {std:.5f} skew {skew:.4f} exkurt {kurt:.4f} KS {ks:.2e}")
    assert abs(mean) < 5 / np.sqrt(n) and abs(std - 1) < 5e-3 and abs(skew) < 0.02 and abs(kurt) < 0.02 and ks < 2e-3
    for kind, pairs in (("components", comp), ("slots", slots), ("draws", succ)):
        for x, y in pairs:
            r = _corr(x, y)
            assert abs(r) < 6 / np.sqrt(x.numel()), (kind, r)
    # std scales the noise linearly; train=False is noiseless and leaves the draw
    hd2 = _hd(spec, "dense", False, std=0.02, seed=20261016)
    y = _natural(hd2, hd2.build_data(*obs_d, train=True)[1], B, True)
    for t in hd.node_type_list:
        rows = ~torch.isnan(y[t][:, 0])
        assert ((y[t][rows] - clean[t][rows]) - 2 * (z1[t][rows] - clean[t][rows])).abs().max().item() <= 5e-6
    d0 = hd.noise_state()
    off = _natural(hd, hd.build_data(*obs_d, train=False)[1], B, True)
    assert hd.noise_state() == d0
    for t in hd.node_type_list:
        rows = ~torch.isnan(off[t][:, 0])
        assert torch.equal(off[t][rows], clean[t][rows])


# ---------------------------------------------------------------------------------------------------------- whole update vs the oracle
@pytest.mark.parametrize("name,B", [("rigid_g1", 24), ("empn_g2", 12), ("rope", 8)])
def test_update_matches_the_oracle_with_the_same_noise(name, B, monkeypatch):
    import oracle_cases as oc
    from geometry_rl_amd import agent, synthetic as syn
    o_spec, spec, kw, obs = oc.make_case(name, B)
    pair = oc.build_pair((o_spec, spec, kw), seed=11, d_kw=dict(training_noise=True, training_noise_std=0.01), dev=DEV)
    cfg, oracle, actor, critic, loss = pair.cfg, pair.oracle, pair.actor, pair.critic, pair.loss
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, A, seed=B))
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    hd = actor.hyper_data
    oc.adopt_calibration(pair, batch, device_first=True)   # calibration latches (the weights are replaced by the oracle's clean calibration)
    seed, draw = hd.noise_state()
    assert draw == 1   # (the calibrating pass read draw 0 and left it; its forward consumed it)
    orig = ogr.build_features

    def noisy(spec_, topo, split, dist_as_pos):   # the actor's call (dist_as_pos=True); the critic's HyperData has no noise
        g, s, v = orig(spec_, topo, split, dist_as_pos)
        if dist_as_pos:
            v = add_noise(spec_, v, topo["batch_size"], seed, draw, 0.01, True)[0]
        return g, s, v
    monkeypatch.setattr(ogr, "build_features", noisy)
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm)
    ref, ref_grads = oracle.update(batch)
    upd.gflat.zero_()
    out = loss(dbatch)
    (out["loss_objective"] + out["loss_entropy"] + out["loss_trust_region"]).backward()
    out["loss_critic"].backward()
    assert hd.noise_state() == (seed, draw + 1)
    oc.check("loc", out["loc"], ref["loc"])
    oc.check("state_value", out["state_value"], ref["state_value"])
    for k in oc.LOSS_KEYS:
        oc.check(k, out[k], ref[k])
    bad, scales = oc.gradients_off_scale(actor, critic, ref_grads)
    assert not bad, bad
    hd.set_noise_state(seed, draw)   # the real step from the same draw
    upd.step(dbatch)
    assert hd.noise_state() == (seed, draw + 1)
    bad = oc.first_step_params_off(actor, critic, oracle, cfg, ref_grads, scales)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- recorded forms = the loop
def _noisy_rollout(N, T, seed, noise_seed=None):
    """(the calibrating forward consumes draw 0)"""
    seeded = None if noise_seed is None else (lambda actor, *_: actor.hyper_data.set_noise_state(noise_seed, 0))
    return make_rollout(N, T, seed, after_build=seeded, training_noise=True)


@contextlib.contextmanager
def _draws(r, n):
    d0 = r.actor.hyper_data.noise_state()
    yield d0
    assert r.actor.hyper_data.noise_state() == (d0[0], d0[1] + n)


@pytest.mark.parametrize("form", ["unrolled", "per_step"])
def test_run_minibatches_equals_the_step_loop(form):
    N, T = 8, 10
    res = run_loop_and_launches(lambda: _noisy_rollout(N, T, seed=33), form, N=N, T=T, ppo_epochs=2, driver_seed=9, unroll=4, keys=(),
                                per_mode=lambda mode, r, upd: _draws(r, 2 * T))   # one draw per update
    for a, b in zip(res["loop"][:3], res["launches"][:3]):
        assert torch.equal(a, b), (a - b).abs().max().item()


def test_replays_draw_fresh_noise_like_eager_steps_and_lanes_equal_one_stream():
    k = 4
    d0 = {}

    @contextlib.contextmanager
    def draws(mode, r, upd):
        d0[mode] = r.actor.hyper_data.noise_state()
        with contextlib.nullcontext() if mode == "frozen" else _draws(r, k):
            yield

    def freeze(mode, r):
        if mode == "frozen":   # the same draw every step: another update
            r.actor.hyper_data.set_noise_state(*d0[mode])

    res = run_step_modes(lambda: _noisy_rollout(8, 2, seed=41), ("eager", "graph", "one_stream", "frozen"), k, (),
                         lambda mode: dict(use_graph=mode != "eager", overlap_critic=mode != "one_stream"), before_step=freeze, per_mode=draws)
    res = {mode: snap[0] for mode, snap in res.items()}
    e_graph = (res["graph"] - res["eager"]).abs().max().item()
    e_lanes = (res["graph"] - res["one_stream"]).abs().max().item()
    e_frozen = (res["graph"] - res["frozen"]).abs().max().item()
    print(f"graph vs eager {e_graph:.3e}, lanes vs one stream {e_lanes:.3e}, fresh vs frozen noise {e_frozen:.3e}")
    assert e_graph <= 1e-7 and e_lanes <= 1e-6 and e_frozen > 1e-6


def test_reproducible_with_the_same_seed():
    from geometry_rl_amd import agent
    N, T = 8, 3
    res = []
    for noise_seed in (None, None, 77):
        r = _noisy_rollout(N, T, seed=51, noise_seed=noise_seed)
        upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=True)
        for t in range(T):
            b = {kk: v[:, t].contiguous() for kk, v in r.data.items()}
            upd.step(b)
        res.append(upd.flat.detach().clone())
    assert torch.equal(res[0], res[1])
    assert not torch.equal(res[0], res[2])


def test_collector_draws_fresh_noise_per_replay():
    from geometry_rl_amd.rollout import PolicyActor
    N, T = 8, 3
    outs = {}
    for use_graph in (False, True):
        r = _noisy_rollout(N, T, seed=61)
        pa = PolicyActor(r.actor, r.spec, use_graph=use_graph, deterministic=True)
        obs = {k: r.data[k][:, 0].contiguous() for k in r.spec.in_features}
        with _draws(r, 4):
            outs[use_graph] = [pa(obs)["loc"].clone() for _ in range(4)]
        ev = PolicyActor(r.actor, r.spec, use_graph=use_graph, deterministic=True, train=False)
        with _draws(r, 0):   # evaluation draws nothing
            quiet = [ev(obs)["loc"].clone() for _ in range(3)]
        assert torch.equal(quiet[0], quiet[1]) and torch.equal(quiet[0], quiet[2])
    for a, b in zip(outs[False], outs[True]):
        assert (a - b).abs().max().item() <= 1e-6
    assert not torch.equal(outs[True][1], outs[True][2]) and not torch.equal(outs[True][2], outs[True][3])


# ---------------------------------------------------------------------------------------------------------- data parallel
@contextlib.contextmanager
def _report_noise_state(case, upd, shard, rank, ret):
    yield
    torch.cuda.synchronize()
    ret[f"noise{rank}"] = case.actor.hyper_data.noise_state()


def test_data_parallel_ranks_draw_their_own_noise():
    """The natural order: no calibrating forward in front of the first update."""
    ret = spawn_dp(dp_ref(16, cfg_kw=dict(training_noise=True), calibrate_first=False), 2, use_graph=False, n_steps=2, keys=(), updater_kw={},
                   extra=(__name__, "_report_noise_state"))
    (s0, f0), (s1, f1) = ((ret[f"noise{r}"], ret[r][1]) for r in range(2))
    print("rank noise states", s0, s1)
    assert s0[0] != s1[0] and s0[1] == s1[1]
    assert torch.equal(f0, f1)
