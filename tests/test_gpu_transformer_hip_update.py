"""The transformer baseline actor on HIP kernels (AgentConfig(transformer_kernels="hip")) through the policy update: against the CPU
pipeline of tests/test_gpu_transformer_config1.py (the same torch modules on the CPU + the oracle's critic and losses), recorded against
eager, the multi-step forms against the step-by-step loop, two ranks against one, the reference fixture, and the dead parameters."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import klpen_ref
import ppo_ref
import transformer_ref as tr
from oracle import graph as ogr, step as ost, trpl as otr
from geometry_rl_amd import synthetic as syn
from updater_cases import assert_ranks_match, make_rollout, run_loop_and_launches, run_two_ranks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TRPL_KEYS = ["loss_objective", "loss_trust_region", "loss_entropy", "loss_critic", "ESS", "kl", "constraint", "mean_constraint",
             "mean_constraint_max", "cov_constraint", "cov_constraint_max", "entropy", "entropy_diff"]
DP_KEYS = ("loss_objective", "loss_trust_region", "loss_entropy", "loss_critic", "kl", "mean_constraint_max", "ESS")
DEAD = ("cls_token", "transformer_encoder_layer.")


def _agent(kernels="hip", **cfg_kw):
    from geometry_rl_amd import agent, graph
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(model="transformer", output_dim=2, output_dim_vec=2, transformer_kernels=kernels, **cfg_kw)   # A = 6
    torch.manual_seed(3)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
    with torch.no_grad():   # the orthogonal(0.01) heads would leave loc ~ 0: make the comparison see the transformer
        actor._mean.weight.mul_(30.0)
        actor._pre_std.weight.mul_(30.0)
    return spec, cfg, actor, critic, loss


def _batch(B, seed):
    batch = dict(syn.make_rigid_obs(B, seed=seed))
    batch.update(syn.make_ppo_fields(B, 6, seed=seed))
    return batch, {k: v.to(DEV) for k, v in batch.items()}


@pytest.mark.parametrize("algorithm", ["trpl", "ppo", "kl_ppo"])
def test_one_update_matches_cpu_pipeline(algorithm):
    """tests/test_gpu_transformer_config1.py::test_one_update_matches_cpu_pipeline with transformer_kernels="hip": B = 64, the same CPU
    pipeline, the same oracle_cases.check allowances; the recorded-step-capable updater."""
    from geometry_rl_amd import agent
    from oracle_cases import check
    B = 64
    extra = {"trpl": {}, "ppo": dict(algorithm="ppo"), "kl_ppo": dict(algorithm="kl_ppo", dtarg=0.01)}[algorithm]
    spec, cfg, actor, critic, loss = _agent(**extra)
    assert actor.gnn.kernels == "hip" and not actor.stock_torch_gnn
    batch, dbatch = _batch(B, 31)
    o_spec = ogr.rigid_spec()
    c_par = {k[len("_network1."):]: v.detach().cpu().clone() for k, v in critic.state_dict().items()}
    oracle = ost.OracleAgent(o_spec, ost.AgentConfig(), {"_unused": torch.zeros(1)}, c_par)
    gnn_c, mean_c, std_c = copy.deepcopy(actor.gnn).cpu(), copy.deepcopy(actor._mean).cpu(), copy.deepcopy(actor._pre_std).cpu()
    gnn_c.set_kernels("torch")   # the CPU side is the stock torch module with the same parameters
    a_params = list(gnn_c.parameters()) + list(mean_c.parameters()) + list(std_c.parameters())
    a_opt = torch.optim.Adam(a_params, lr=cfg.lr, eps=1e-5)
    a_obs = {"scalars": batch["scalars"], "position_vectors": batch["norm_position_vectors"],
             "velocity_vectors": batch["norm_velocity_vectors"], "norm_position_vectors": batch["norm_position_vectors"],
             "norm_velocity_vectors": batch["norm_velocity_vectors"], "infos": batch["infos"]}
    topo, graph, s, v = oracle._graph(a_obs, full_graph_obs=False, dist_as_pos=True)
    x = ogr.critic_input(topo, s, v)

    class G:
        batch_size, node_types, output_mask_key = B, topo["node_types"], "grippers"
        nodes_per_sample = topo["n_per"]

    hidden = gnn_c.one_step(G(), x)
    loc = mean_c(hidden).reshape(B, -1)
    std = F.softplus(std_c(hidden) + otr.inverse_softplus(torch.tensor(1.0 - 1e-5))) + 1e-5
    var = std.reshape(B, -1) ** 2
    value = oracle.critic_forward({k: batch[k] for k in o_spec.in_features})
    if algorithm == "trpl":
        ref = otr.trpl_loss(loc, var, batch, value, mean_bound=cfg.mean_bound, cov_bound=cfg.cov_bound,
                            trust_region_coeff=cfg.trust_region_coeff, entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef,
                            clip_value=cfg.clip_value, proj_type="kl")
        (ref["loss_objective"] + ref["loss_entropy"] + ref["loss_trust_region"]).backward()
        keys = TRPL_KEYS
    elif algorithm == "ppo":
        ref = ppo_ref.ppo_loss(loc, var, batch, value, clip_epsilon=cfg.clip_epsilon, entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef,
                               clip_value=cfg.clip_value)
        (ref["loss_objective"] + ref["loss_entropy"]).backward()
        keys = ["loss_objective", "loss_entropy", "loss_critic", "ESS", "entropy"]
    else:
        ref = klpen_ref.klpen_loss(loc, var, batch, value, cfg.kl_beta, entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef)
        (ref["loss_objective"] + ref["loss_entropy"]).backward()
        keys = ["loss_objective", "loss_entropy", "loss_critic", "kl", "entropy"]
    ref["loss_critic"].backward()
    a_opt.step()
    oracle.critic_optim.step()
    upd = agent.PolicyUpdater(loss, lr=cfg.lr)
    out = upd.step(dbatch)
    check("loc", out["loc"], loc)
    check("var", out["sigma"] ** 2, var)
    check("state_value", out["state_value"], value)
    for k in keys:
        check(k, out[k], ref[k])
    for (k, p), q in zip(list(actor.gnn.named_parameters()), gnn_c.parameters()):
        check("param gnn." + k, p, q, 2e-5)
    check("param _mean.weight", actor._mean.weight, mean_c.weight, 2e-5)
    check("param _pre_std.weight", actor._pre_std.weight, std_c.weight, 2e-5)
    for k, p in critic.named_parameters():
        check("param " + k, p, oracle.critic[k[len("_network1."):]], 2e-5)


def _three_steps(use_graph, **updater_kw):
    from geometry_rl_amd import agent
    spec, cfg, actor, critic, loss = _agent()
    dead0 = {k: p.detach().clone() for k, p in actor.gnn.named_parameters() if k.startswith(DEAD)}
    assert len(dead0) == 13
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, use_graph=use_graph, **updater_kw)
    outs = []
    for i in range(3):
        out = upd.step(_batch(16, 40 + i)[1])
        outs.append({k: out[k].detach().clone() for k in TRPL_KEYS})
    torch.cuda.synchronize()
    return upd, actor, dead0, outs


def test_recorded_steps_equal_eager_steps_bitwise_and_dead_parameters_stay():
    upd_g, actor_g, dead0, outs_g = _three_steps(True)
    assert upd_g.mode.startswith("graph") and upd_g._program is not None
    upd_e, actor_e, _, outs_e = _three_steps(False)
    assert upd_e.mode.startswith("eager")
    assert torch.equal(upd_g.flat, upd_e.flat)
    for a, b in zip(outs_g, outs_e):
        for k in TRPL_KEYS:
            assert torch.equal(a[k], b[k]), k
    for actor in (actor_g, actor_e):   # cls_token and the template layer: no gradient on the stock path, none here -- not one bit moves
        for k, p in actor.gnn.named_parameters():
            if k.startswith(DEAD):
                assert torch.equal(p.detach(), dead0[k]), k
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    moved = [k for k, p in actor_g.gnn.named_parameters() if not k.startswith(DEAD)]
    assert len(moved) == 28


def test_recorded_steps_with_annealing_and_stats():
    """The schedule tables and the running statistics ride in the recorded program of this actor as in the others'."""
    kw = dict(anneal_lr=True, total_network_updates=10, track_stats=True)
    upd_g, _, _, outs_g = _three_steps(True, **kw)
    upd_e, _, _, outs_e = _three_steps(False, **kw)
    assert upd_g.mode.startswith("graph") and upd_g._program is not None
    assert torch.equal(upd_g.flat, upd_e.flat)
    assert torch.equal(upd_g.stats_actor, upd_e.stats_actor) and float(upd_g.stats_actor[14]) == 3.0


@pytest.mark.parametrize("form", ["unrolled", "per_step"])
def test_run_minibatches_equals_the_step_loop_bitwise(form):
    """2 epochs x 4 minibatches of 16 frames: ``run_minibatches`` in both recorded forms against the loop of ``step_from``."""
    N, T = 16, 4
    res = run_loop_and_launches(lambda: make_rollout(N, T, seed=33, model="transformer", transformer_kernels="hip"), form, N=N, T=T,
                                ppo_epochs=2, driver_seed=9, unroll=4, keys=TRPL_KEYS)
    for a, b in zip(res["loop"][:3], res["launches"][:3]):   # parameters and both Adam moments
        assert torch.equal(a, b)
    for k in TRPL_KEYS:
        assert torch.equal(res["loop"][3][-1][k], res["launches"][3][-1][k]), k


def test_module_flipped_between_kernels_agrees_within_the_per_op_allowance():
    """The A/B a user would run: one actor, ``set_kernels`` flipped, the same observations."""
    spec, cfg, actor, critic, loss = _agent()
    batch, dbatch = _batch(16, 5)
    obs = [dbatch[k] for k in loss.in_features]
    with torch.no_grad():
        loc_h, sig_h = actor.forward_diag(*obs, train=False)
        actor.gnn.set_kernels("torch")
        loc_t, sig_t = actor.forward_diag(*obs, train=False)
        actor.gnn.set_kernels("hip")
        # float64 values of the same: the torch modules in double on the CPU
        graph, u = actor.hyper_data.build_data(*obs, train=False)
        ps = [p.detach().double().cpu() for p in actor.gnn.encoder_parameters()]
        mask = actor.gnn.output_mask(graph)
        hidden = tr.encode(u.double().cpu(), ps, mask.start, mask.stop - mask.start)
        w = [t.detach().double().cpu() for t in (actor._mean.weight, actor._mean.bias, actor._pre_std.weight, actor._pre_std.bias)]
        loc64, sig64 = tr.head(hidden, *w, float(actor._pre_activation_shift), float(actor.minimal_std))
    B = loc_h.shape[0]
    tr.check("A/B loc", loc_h, loc64.reshape(B, -1), loc_t.cpu())
    tr.check("A/B sigma", sig_h, sig64.reshape(B, -1), sig_t.cpu())


def dp_transformer_case(B, group):
    """updater_cases.dp_case for the transformer actor on HIP kernels (nothing in it is batch-global: no calibration, no new collective)."""
    from updater_cases import dp_case
    return dp_case(B, group, cfg_kw=dict(model="transformer", transformer_kernels="hip"), calibrate_first=False)   # (A = 6: two grippers)


def test_two_ranks_match_single_rank():
    ref = (__name__, "dp_transformer_case", dict(B=16))
    assert_ranks_match(*run_two_ranks(ref, 2, use_graph=False, dp_use_graph=False, n_steps=1, keys=DP_KEYS, updater_kw={}), 2, 1e-5, 2e-6)


def test_reference_fixture_through_the_hip_path(golden_dir):
    from geometry_rl_amd.policy import GNNGaussianPolicyDiag
    from geometry_rl_amd.transformer import TransformerVanilla
    z = np.load(os.path.join(golden_dir, "tier2d_transformer_post_fc.npz"))
    B, P, G = int(z["B"]), int(z["P"]), int(z["G"])
    u_obj, u_grip = torch.from_numpy(z["u_object_geometry"]), torch.from_numpy(z["u_grippers"])
    d = u_obj.shape[1]

    class Graph:
        batch_size = B
        node_types = ["object_geometry", "grippers"]
        nodes_per_sample = {"object_geometry": P, "grippers": G}
        output_mask_key = "grippers"

    class FakeData:
        def build_data(self, *args, train=True):
            return Graph(), torch.cat([u_obj.reshape(B, P, d), u_grip.reshape(B, G, d)], dim=1).to(DEV)

    gnn = TransformerVanilla(input_dim_node=d, output_dim=64, num_layers=2, num_heads=2, hidden_dim=64, dropout=0.0, device=DEV, kernels="hip")
    policy = GNNGaussianPolicyDiag(gnn=gnn, hyper_data=FakeData(), action_dim=6, num_actuators=G, contextual_std=True, post_fc=True)
    sd = {k[len("param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}
    missing, unexpected = policy.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    loc, cov = policy(torch.zeros(B, 1, device=DEV), train=True)
    assert (loc.cpu() - torch.from_numpy(z["loc"])).abs().max() <= 1e-5
    assert (cov.cpu() - torch.from_numpy(z["cov"])).abs().max() <= 1e-5 * float(z["cov"].max())
    (loc * torch.from_numpy(z["w_loc"]).to(DEV)).sum().add((cov.diagonal(dim1=-2, dim2=-1) * torch.from_numpy(z["w_cov"]).to(DEV)).sum()).backward()
    n = 0
    for k, p in policy.named_parameters():
        key = "grad." + k
        if key in z.files:
            ref = torch.from_numpy(z[key])
            assert (p.grad.cpu() - ref).abs().max() <= 2e-5 * max(1.0, float(ref.abs().max())), k
            n += 1
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert n >= 30
