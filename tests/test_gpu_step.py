"""GPU parity of the whole policy-update path against the CPU oracle: actor/critic outputs, every loss-dict entry,
gradients, and the parameters after one Adam step -- on identical parameters and inputs.  Tolerance 1e-4 (north_star) for the values;
every gradient tensor within 2e-4 of ITS OWN largest reference entry and the post-Adam parameters within what that gradient tolerance
implies through Adam's first step (tests/parity_util.py); several consecutive updates: tests/test_gpu_multistep_oracle.py."""
import pytest
import torch

import oracle_cases as oc
from oracle import trpl as otr
from geometry_rl_amd import synthetic as syn
from oracle_cases import LOSS_KEYS, check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,B", [("rigid_g1", 24), ("rigid_g2", 16), ("cloth", 8), ("rope", 8), ("empn_g2", 12),
                                    ("rigid_tiny", 6), ("rigid_one", 1), ("rigid_frob", 12), ("rigid_w2", 12), ("rigid_attn", 12)])
def test_policy_update_step(name, B):
    from geometry_rl_amd import agent
    dev = torch.device("cuda:0")
    o_spec, spec, kw, obs = oc.make_case(name, B)
    pair = oc.build_pair((o_spec, spec, kw), seed=11)
    cfg, oracle, actor, critic, loss = pair.cfg, pair.oracle, pair.actor, pair.critic, pair.loss
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batch = dict(obs)
    batch.update(syn.make_ppo_fields(B, A, seed=B))
    dbatch = {k: v.to(dev) for k, v in batch.items()}

    # --- calibration (first training call) must reproduce the reference re-initialisation
    own = oc.adopt_calibration(pair, batch, device_first=True)
    for k, v in oracle.actor.items():
        if "kernel.weight" in k:
            check("calibrated " + k, own[k], v, 1e-4)
    # (both sides continue from bit-identical, oracle-calibrated weights so that the update comparison below isolates the update itself)

    # --- one full update on both sides
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm)
    ref, ref_grads = oracle.update(batch)
    # capture gradients before Adam by running loss + backward manually on a copy of the step
    upd.gflat.zero_()
    out = loss(dbatch)
    (out["loss_objective"] + out["loss_entropy"] + out["loss_trust_region"]).backward()
    out["loss_critic"].backward()
    check("loc", out["loc"], ref["loc"])
    check("var", out["sigma"] ** 2, ref["var"])
    check("state_value", out["state_value"], ref["state_value"])
    for k in LOSS_KEYS:
        check(k, out[k], ref[k])
    bad, scales = oc.gradients_off_scale(actor, critic, ref_grads)
    assert not bad, bad
    # --- Adam: run the real step from the same starting point (parameters untouched so far)
    upd.step(dbatch)
    bad = oc.first_step_params_off(actor, critic, oracle, cfg, ref_grads, scales)
    assert not bad, bad


def test_gae_scan():
    from geometry_rl_amd import agent
    dev = torch.device("cuda:0")
    for (N, T) in [(5, 37), (130, 128), (64, 200)]:
        d = syn.make_gae_inputs(N, T, seed=N)
        d["terminated"][:, T // 3] = True
        d["done"][:, T // 3] = True
        adv_ref, tgt_ref = otr.gae_shifted(d["reward"], d["done"], d["terminated"], d["values"])
        adv, tgt = agent.gae(d["reward"].to(dev), d["done"].to(dev), d["terminated"].to(dev), d["values"].to(dev))
        check(f"gae adv {N}x{T}", adv, adv_ref, 1e-5)
        check(f"gae target {N}x{T}", tgt, tgt_ref, 1e-5)
