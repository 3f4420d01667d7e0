"""The shared checkers of the update-vs-oracle GPU tests (tests/oracle_cases.py, tests/updater_cases.py) still NOTICE what they are for --
shown without a device: the oracle alone runs K = 2 updates of the small rigid case, stand-ins for the updater (``flat``, ``exp_avg``,
``exp_avg_sq``) and for the device's actor and critic (parameters that are views into ``flat``) are laid out from the oracle's own
parameters and Adam state, and then
  * no checker reports anything on the oracle's own numbers;
  * one tensor off by twice what its rule allows (exp_avg by 2 M_TOL and exp_avg_sq by 2 V_TOL of its scale, a parameter by twice its
    bound, a gradient by 2 G_TOL of its scale), or holding a NaN, is reported, and only that tensor.
Also: ``obs_of`` draws what the direct ``synthetic.make_*_obs`` calls draw."""
import types

import pytest
import torch

import oracle_cases as oc
from oracle_cases import CRITIC, M_TOL, V_TOL
from parity_util import G_TOL, adam_first_step_bound, adam_first_step_bound_elem, grad_scales
from updater_cases import merge_grad_scales, moments_and_params_after

B, K = 4, 2
ACTOR_T = "_pre_std.weight"     # the actor tensor that gets perturbed (the critic's: its first)


class _Net:
    """What the checkers read of a device module: named_parameters()."""

    def __init__(self, named):
        self.named = named

    def named_parameters(self):
        return iter(self.named)


def _stand_ins(actor_p, critic_p, moments=None):
    """(updater, actor, critic) stand-ins from the oracle's parameter dicts: one flat vector, the parameters views into it; ``moments``
    {id(oracle parameter): Adam state} fills exp_avg / exp_avg_sq at the same offsets."""
    src = [(k, p) for k, p in actor_p.items() if p.requires_grad] + [(CRITIC + k, p) for k, p in critic_p.items()]
    flat = torch.cat([p.detach().reshape(-1) for _, p in src]).clone()
    upd = types.SimpleNamespace(flat=flat, exp_avg=torch.zeros_like(flat), exp_avg_sq=torch.zeros_like(flat))
    named, o = [], 0
    for k, p in src:
        n = p.numel()
        named.append((k, torch.nn.Parameter(flat[o:o + n].view(p.shape))))
        st = {} if moments is None else moments.get(id(p), {})
        if "exp_avg" in st:
            upd.exp_avg[o:o + n] = st["exp_avg"].reshape(-1)
            upd.exp_avg_sq[o:o + n] = st["exp_avg_sq"].reshape(-1)
        o += n
    n_actor = sum(1 for k, _ in src if not k.startswith(CRITIC))
    return upd, _Net(named[:n_actor]), _Net(named[n_actor:])


@pytest.fixture(scope="module")
def run():
    from geometry_rl_amd import synthetic as syn
    oc.cap_oracle_threads()
    o_spec, _, kw, _ = oc.make_case("rigid_g1", B)
    o_cfg, _, _, oracle = oc.make_oracle(o_spec, kw, 21)
    batches = []
    for i in range(K):
        b = dict(oc.obs_of("rigid_g1", B, 30 + i))
        b.update(syn.make_ppo_fields(B, 6, seed=40 + i))
        batches.append(b)
    with torch.no_grad():
        oracle.actor_forward({k: batches[0][k] for k in o_spec.in_features}, calibrate=True)
    g_scale, first = None, None
    for b in batches:
        _, ref_grads = oracle.update(b)
        g_scale = merge_grad_scales(g_scale, ref_grads)
        if first is None:   # the state behind Adam's first step, kept for the one-update checkers
            first = types.SimpleNamespace(actor={k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in oracle.actor.items()},
                                          critic={k: v.detach().clone().requires_grad_(True) for k, v in oracle.critic.items()}, grads=ref_grads)
    return types.SimpleNamespace(oracle=oracle, cfg=o_cfg, g_scale=g_scale, first=first)


def _after_k(run):
    o = run.oracle
    moments = {id(p): s for optim in (o.actor_optim, o.critic_optim) for p, s in optim.state.items()}
    return _stand_ins(o.actor, o.critic, moments)


def _entry(upd, net, name):
    """(offset of the tensor's first entry in flat, the tensor's parameter)"""
    p = dict(net.named_parameters())[name]
    return (p.data_ptr() - upd.flat.data_ptr()) // 4, p


def _targets(run):
    return ("actor", ACTOR_T, ACTOR_T), ("critic", next(iter(run.oracle.critic)), CRITIC + next(iter(run.oracle.critic)))


def test_k_updates_checker_passes_the_oracle_and_reports_each_miss(run):
    o, cfg = run.oracle, run.cfg
    check = lambda upd, actor, critic: moments_and_params_after(upd, actor, critic, o, cfg, run.g_scale, K, M_TOL, V_TOL)[0]
    assert check(*_after_k(run)) == []
    for net_name, kk, k in _targets(run):
        ref_p = (o.actor if net_name == "actor" else o.critic)[kk]
        optim = o.actor_optim if net_name == "actor" else o.critic_optim
        all_states = {n: optim.state[p] for n, p in (o.actor if net_name == "actor" else o.critic).items() if p in optim.state}
        m_sc = grad_scales({n: s["exp_avg"] for n, s in all_states.items()})[kk]
        v_sc = grad_scales({n: s["exp_avg_sq"] for n, s in all_states.items()})[kk]
        allowed_p = K * adam_first_step_bound(cfg.lr, 1e-5, run.g_scale[net_name].get(kk, 0.0), cfg.clip_grad_norm, p_ref=ref_p)
        for what, delta in (("exp_avg", 2 * M_TOL * m_sc), ("exp_avg_sq", 2 * V_TOL * v_sc), ("flat", 2 * allowed_p), ("exp_avg", float("nan")),
                            ("flat", float("nan"))):
            upd, actor, critic = _after_k(run)
            i, _ = _entry(upd, actor if net_name == "actor" else critic, k)
            getattr(upd, what)[i] += delta
            bad = check(upd, actor, critic)
            assert [b[:2] for b in bad] == [(net_name, kk)], (net_name, kk, what, delta, bad)
        # ... and just inside every rule nothing is reported (the perturbation, not the tensor, is what was noticed)
        upd, actor, critic = _after_k(run)
        i, _ = _entry(upd, actor if net_name == "actor" else critic, k)
        upd.exp_avg[i] += 0.5 * M_TOL * m_sc
        upd.exp_avg_sq[i] += 0.5 * V_TOL * v_sc
        upd.flat[i] += 0.5 * allowed_p
        assert check(upd, actor, critic) == []


def _after_one(run):
    f = run.first
    upd, actor, critic = _stand_ins(f.actor, f.critic)
    for k, p in actor.named_parameters():
        p.grad = f.grads["actor"][k].clone() if k in f.grads["actor"] else None
    for k, p in critic.named_parameters():
        p.grad = f.grads["critic"][k[len(CRITIC):]].clone()
    return upd, actor, critic


def test_gradient_checker_passes_the_oracle_and_reports_each_miss(run):
    f = run.first
    _, actor, critic = _after_one(run)
    bad, scales = oc.gradients_off_scale(actor, critic, f.grads)
    assert bad == [] and scales == {net: grad_scales(f.grads[net]) for net in ("actor", "critic")}
    for net_name, kk, k in _targets(run):
        for delta in (2 * G_TOL * scales[net_name][kk], float("nan")):
            _, actor, critic = _after_one(run)
            dict((actor if net_name == "actor" else critic).named_parameters())[k].grad.reshape(-1)[0] += delta
            bad, _ = oc.gradients_off_scale(actor, critic, f.grads)
            assert [b[:2] for b in bad] == [(net_name, kk)], (net_name, kk, delta, bad)
        _, actor, critic = _after_one(run)
        dict((actor if net_name == "actor" else critic).named_parameters())[k].grad.reshape(-1)[0] += 0.5 * G_TOL * scales[net_name][kk]
        assert oc.gradients_off_scale(actor, critic, f.grads)[0] == []
    # a miss in the critic is not looked for where only the actor's gradients are asked about
    _, actor, critic = _after_one(run)
    next(iter(critic.named_parameters()))[1].grad.reshape(-1)[0] = float("nan")
    assert oc.gradients_off_scale(actor, critic, f.grads, nets=("actor",))[0] == []


def test_first_step_checker_passes_the_oracle_and_reports_each_miss(run):
    f, cfg = run.first, run.cfg
    scales = {net: grad_scales(f.grads[net]) for net in ("actor", "critic")}
    check = lambda actor, critic: oc.first_step_params_off(actor, critic, f, cfg, f.grads, scales)
    assert not cfg.clip_grad_norm     # (the entry-wise bound is the one in force)
    _, actor, critic = _after_one(run)
    assert check(actor, critic) == []
    for net_name, kk, k in _targets(run):
        ref_p = getattr(f, net_name)[kk]
        allowed = adam_first_step_bound_elem(cfg.lr, 1e-5, f.grads[net_name][kk], scales[net_name][kk], p_ref=ref_p).reshape(-1)
        for factor in (2.0, float("nan")):
            upd, actor, critic = _after_one(run)
            i, _ = _entry(upd, actor if net_name == "actor" else critic, k)
            upd.flat[i] += factor * float(allowed[0])
            bad = check(actor, critic)
            assert [b[:2] for b in bad] == [(net_name, kk)], (net_name, kk, factor, bad)
        upd, actor, critic = _after_one(run)
        i, _ = _entry(upd, actor if net_name == "actor" else critic, k)
        upd.flat[i] += 0.5 * float(allowed[0])
        assert check(actor, critic) == []


@pytest.mark.parametrize("name", ["rigid_g1", "cloth", "cloth_full", "empn_g2"])
def test_obs_of_draws_what_the_direct_calls_draw(name):
    from geometry_rl_amd import synthetic as syn
    n, seed = 3, 37
    want = {"rigid_g1": lambda: syn.make_rigid_obs(n, seed=seed),
            "cloth": lambda: syn.make_cloth_obs(n, n_particles=25, E_cloth=40, seed=seed),
            "cloth_full": lambda: syn.make_cloth_obs(n, seed=seed),
            "empn_g2": lambda: syn.make_rigid_obs(n, G=2, angular_velocity=False, object_velocity=False, seed=seed)}[name]()
    got = oc.obs_of(name, n, seed)
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
