"""Shared scaffolding of the GPU tests that hold the device's policy update against the CPU oracle (oracle/step.py and the objectives'
oracle agents): the cases, the pair of agents built from one seed with identical parameters, the calibration both sides continue from,
K updates on both sides, and the two one-update checks (gradients against their own scale, parameters after Adam's first step).  The
K-update checks themselves are ``merge_grad_scales`` / ``moments_and_params_after`` (tests/updater_cases.py).  TEST INFRASTRUCTURE ONLY, a
plain module like tests/updater_cases.py and tests/trpl_cases.py.  Builders and runners compare NOTHING; the checkers print every margin
and return the tensors that miss their rule: every assertion, with its tolerance, stays in the test that owns it.  That the checkers
notice what they are for is shown without a device in tests/test_oracle_cases_cpu.py."""
from collections import namedtuple

import numpy as np
import torch

from oracle import graph as ogr, step as ost
from parity_util import G_TOL, adam_first_step_bound, adam_first_step_bound_elem, grad_error, grad_scales, param_excess
from updater_cases import merge_grad_scales

TOL = 1e-4
LOSS_KEYS = ["loss_objective", "loss_trust_region", "loss_entropy", "loss_critic", "ESS", "kl", "constraint", "mean_constraint",
             "mean_constraint_max", "cov_constraint", "cov_constraint_max", "entropy", "entropy_diff"]
M_TOL, V_TOL = 5e-4, 1e-3     # K updates: exp_avg, exp_avg_sq of every tensor, of its own largest reference entry (test_gpu_multistep_oracle.py)
CRITIC = "_network1."         # what the device's critic puts in front of the oracle's critic parameter names

Pair = namedtuple("Pair", "o_spec spec o_cfg cfg oracle actor critic proj loss")


def cap_oracle_threads():
    """The oracle's small CPU ops only slow down with more intra-op threads than this."""
    torch.set_num_threads(min(16, torch.get_num_threads()))


def check(name, got, ref, tol=TOL):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = max(1.0, ref.abs().max().item()) if ref.numel() else 1.0
    print(f"{name}: max|err|={err:.3e} ref_max={ref.abs().max().item() if ref.numel() else 0:.3e}")
    assert np.isfinite(err) and err <= tol * scale, f"{name}: err {err:.3e} > {tol * scale:.3e}"


# ------------------------------------------------------------------------------------------------------------- cases
def make_case(name, B):
    """-> (the oracle's spec, the device's spec, AgentConfig keywords of both sides, one observation set)"""
    from geometry_rl_amd import graph, synthetic as syn
    if name == "rigid_g1":
        o_spec, spec = ogr.rigid_spec(), graph.rigid_spec()
        kw = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
        obs = syn.make_rigid_obs(B, seed=3)
    elif name in ("rigid_tiny", "rigid_one"):
        # edge cases of the ragged graph: samples with 1, 2 and 3 valid object points (fewer than the k = 3 neighbours kNN asks
        # for: missing neighbours give no edge; a 1-point sample has no internal edge at all), next to a full 32-point sample;
        # "rigid_one": a single frame (the advantage is not normalised for a batch of one, trpl.py:248)
        o_spec, spec = ogr.rigid_spec(), graph.rigid_spec()
        kw = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
        obs = syn.make_rigid_obs(B, seed=9)
        P = 32
        counts = torch.tensor([1, 2, 3, 32, 5, 4])[torch.arange(B) % 6] if name == "rigid_tiny" else torch.tensor([7])
        valid = (torch.arange(P)[None, :] < counts[:, None]).float()[..., None]
        pos = obs["position_vectors"].clone()
        G = 1
        gen = torch.Generator().manual_seed(99)
        for blk in range(2):  # object points, target points: fresh distinct positions (coincident points = kNN ties), then padding
            sl = slice(3 * G + blk * 3 * P, 3 * G + (blk + 1) * 3 * P)
            pos[:, sl] = ((torch.rand(B, P, 3, generator=gen) * 2 - 1) * valid).reshape(B, -1)
        obs["position_vectors"] = pos
        obs["infos"][:, 0] = counts.float()
    elif name == "rigid_g2":
        o_spec = ogr.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        kw = dict()
        obs = syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=4)
    elif name == "empn_g2":
        o_spec = ogr.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        kw = dict(model="empn")
        obs = syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=8)
    elif name == "rigid_attn":   # FiberBundleConv(aggr="AttentionalAggregation") in every round (hepi_attention.yaml)
        o_spec = ogr.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        kw = dict(aggr="AttentionalAggregation")
        obs = syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=14)
    elif name in ("rigid_frob", "rigid_w2"):   # the other two projection layers (frob_projection_layer.py, w2_projection_layer.py)
        o_spec = ogr.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
        kw = dict(proj_type=name.split("_")[1], trust_region_coeff=2.0)
        obs = syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=12)
    elif name == "cloth":
        o_spec, spec = ogr.cloth_spec(n_particles=25, E_cloth=40), graph.cloth_spec(n_particles=25, E_cloth=40)
        kw = dict(trust_region_coeff=4.0, cov_bound=0.001)
        obs = syn.make_cloth_obs(B, n_particles=25, E_cloth=40, seed=5)
    elif name == "rope":
        o_spec, spec = ogr.rope_spec(n_links=20), graph.rope_spec(n_links=20)
        kw = dict(dim=2, clip_grad_norm=True)
        obs = syn.make_rope_obs(B, n_links=20, seed=6)
    return o_spec, spec, kw, obs


def obs_of(name, B, seed):
    """One observation set of the K-update tests' cases: rigid_g1, cloth (25 particles), cloth_full (225 particles, 10 hole points,
    4 grippers: SURVEY.md 8(d), config 3), empn_g2 (the two-gripper rigid spec, positions only)."""
    from geometry_rl_amd import synthetic as syn
    if name == "rigid_g1":
        return syn.make_rigid_obs(B, seed=seed)
    if name == "cloth":
        return syn.make_cloth_obs(B, n_particles=25, E_cloth=40, seed=seed)
    if name == "cloth_full":
        return syn.make_cloth_obs(B, seed=seed)
    assert name == "empn_g2", name
    return syn.make_rigid_obs(B, G=2, angular_velocity=False, object_velocity=False, seed=seed)


def load_params(module, params, dev):
    sd = module.state_dict()
    for k, v in params.items():
        assert k in sd, k
        assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
    missing = [k for k in sd if k not in params and not k.endswith("callibrated")]
    assert not missing, missing
    module.load_state_dict({k: v.to(dev) for k, v in params.items()}, strict=False)


# ------------------------------------------------------------------------------------------------------------- the pair
def make_oracle(o_spec, o_kw, seed, oracle_cls=ost.OracleAgent):
    """-> (the oracle's AgentConfig, the actor's and the critic's initial parameters, the oracle agent built from them)"""
    o_cfg = ost.AgentConfig(**o_kw)
    a_par, c_par = ost.init_agent_params(o_spec, o_cfg, seed=seed)
    return o_cfg, a_par, c_par, oracle_cls(o_spec, o_cfg, a_par, c_par)


def make_device(spec, cfg, a_par, c_par, dev):
    """-> build_agent's (actor, critic, proj, loss) holding the oracle's initial parameters"""
    from geometry_rl_amd import agent
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev)
    load_params(actor, a_par, dev)
    load_params(critic, {CRITIC + k: v for k, v in c_par.items()}, dev)
    return actor, critic, proj, loss


def build_pair(case, B=None, *, seed, o_kw=(), d_kw=(), oracle_cls=ost.OracleAgent, dev="cuda:0"):
    """Both sides of ``case`` -- a name of make_case, or (o_spec, spec, kw) -- from the parameters of one seed.  ``o_kw`` / ``d_kw``: what the
    oracle's / the device's AgentConfig gets on top of the case's keywords."""
    from geometry_rl_amd import agent
    o_spec, spec, kw = make_case(case, B)[:3] if isinstance(case, str) else case
    cfg = agent.AgentConfig(**dict(kw, **dict(d_kw)))
    o_cfg, a_par, c_par, oracle = make_oracle(o_spec, dict(kw, **dict(o_kw)), seed, oracle_cls)
    return Pair(o_spec, spec, o_cfg, cfg, oracle, *make_device(spec, cfg, a_par, c_par, torch.device(dev)))


def adopt_calibration(pair, obs=None, *, weights=None, device_first=False):
    """The first training call: the oracle's calibrating forward on ``obs`` (a host batch), then its calibrated weights on the device actor,
    which is told that it is calibrated -- both sides continue from bit-identical weights.  ``weights``: a snapshot of the oracle's
    calibrated actor taken earlier, copied instead of calibrating here.  ``device_first``: the device runs its own calibrating forward on
    ``obs`` before its weights are replaced (it latches its flags itself) -> its own calibrated kernels, on the host."""
    actor, own = pair.actor, None
    dev = next(actor.parameters()).device
    with torch.no_grad():
        if weights is None:
            pair.oracle.actor_forward({k: obs[k] for k in pair.o_spec.in_features}, calibrate=True)
            weights = pair.oracle.actor
        if device_first:
            actor.forward_diag(*[obs[k].to(dev) for k in pair.spec.in_features], train=True)
            own = {k: v.detach().cpu().clone() for k, v in actor.state_dict().items() if "kernel.weight" in k}
    actor.load_state_dict({k: v.detach().to(dev) for k, v in weights.items()}, strict=False)
    if not device_first:
        for mod in actor.modules():
            if hasattr(mod, "callibrated"):
                mod.callibrated.fill_(True)
    actor._calib_checked = True
    return own


# ------------------------------------------------------------------------------------------------------------- K updates
def run_updates(pair, batches, upd, per_step, refs=None):
    """One update per host batch on both sides (``refs``: the oracle's (ref, ref_grads) of every update where it ran ahead);
    ``per_step(i, out, ref)`` after each -> the running gradient scales (merge_grad_scales) for moments_and_params_after."""
    dev, g_scale = upd.flat.device, None
    for i, b in enumerate(batches):
        ref, ref_grads = pair.oracle.update(b) if refs is None else refs[i]
        out = upd.step({k: v.to(dev) for k, v in b.items()})
        g_scale = merge_grad_scales(g_scale, ref_grads)
        per_step(i, out, ref)
    return g_scale


# ------------------------------------------------------------------------------------------------------------- one update
def gradients_off_scale(actor, critic, ref_grads, nets=("actor", "critic")):
    """Every gradient tensor of ``nets`` against its OWN scale (parity_util: G_TOL of the tensor's largest reference entry, no max(1, .)
    floor) -> ([(net, name, error, scale)] of the tensors that miss it, the scales of both networks)."""
    scales = {net: grad_scales(ref_grads[net]) for net in ("actor", "critic")}
    got = {"actor": {k: p.grad for k, p in actor.named_parameters() if k in ref_grads["actor"]},
           "critic": {k[len(CRITIC):]: p.grad for k, p in critic.named_parameters()}}
    bad = []
    for net in nets:
        for k, g in got[net].items():
            e, sc = grad_error(g, ref_grads[net][k]), scales[net][k]
            print(f"grad {net} {k}: err {e:.3e} = {e / sc:.2e} of its scale {sc:.3e}")
            if not (np.isfinite(e) and e <= G_TOL * sc):
                bad.append((net, k, e, sc))
    return bad, scales


def first_step_params_off(actor, critic, oracle, cfg, ref_grads, scales):
    """The parameters after Adam's first step against what the gradient tolerance implies through it: entry-wise from the reference
    gradient (parity_util); with gradient clipping Adam sees rescaled gradients: per tensor -> [(net, name, error, fraction of allowed)]."""
    bad = []
    for net, mod, ref_p, strip in (("actor", actor, oracle.actor, 0), ("critic", critic, oracle.critic, len(CRITIC))):
        for k, p in mod.named_parameters():
            kk = k[strip:]
            if cfg.clip_grad_norm or kk not in ref_grads[net]:
                allowed = adam_first_step_bound(cfg.lr, 1e-5, scales[net].get(kk, 0.0), clip=cfg.clip_grad_norm, p_ref=ref_p[kk])
            else:
                allowed = adam_first_step_bound_elem(cfg.lr, 1e-5, ref_grads[net][kk], scales[net][kk], p_ref=ref_p[kk])
            e, x = grad_error(p, ref_p[kk]), param_excess(p, ref_p[kk], allowed)
            print(f"param {net} {kk}: err {e:.3e} = {x:.2f} of allowed")
            if not (np.isfinite(x) and x <= 1.0):
                bad.append((net, kk, e, x))
    return bad
