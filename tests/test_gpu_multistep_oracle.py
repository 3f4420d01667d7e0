"""K = 5 CONSECUTIVE policy updates against the CPU oracle.

One Adam step from zero moments moves every parameter by ~lr * sign(g): it pins signs and the Adam kernel, not gradient magnitudes.  From
the second step on the moments are non-zero, the update depends on the RATIO of accumulated gradients, and an error in a gradient's
magnitude shows up in exp_avg, exp_avg_sq and the parameters.  Both sides run five updates on five different minibatches from identical
(oracle-calibrated) parameters; after the fifth:

  * exp_avg      of every parameter tensor within  5e-4 of the tensor's own largest reference entry
  * exp_avg_sq   of every parameter tensor within  1e-3 of the tensor's own largest reference entry   (squares: twice the relative error)
    (floors as for gradients, tests/parity_util.py: a tensor's scale is at least 1e-4 of the largest entry of its network)
  * parameters   within  K * (the first-step bound of parity_util.adam_first_step_bound) -- the trajectories are compared, not re-synchronised:
                 the bound is what a gradient error of 2e-4 per step can accumulate to through Adam

Cases: rigid HEPi B = 64, cloth HEPi B = 16 (25 particles), two-agent EMPN B = 32 -- and, since round 5, the sizes
BASELINE.json names: rigid HEPi at config 2's exact minibatch (B = 1024, P = 32, K = 5: ~15 s of oracle time on the GPU box) and cloth with
225 particles / 10 hole points / 4 grippers at B = 256 (K = 3).  The recorded (hipGraph) step is what runs from the third update on, so the
comparison also covers replayed launches.  Reference semantics: examples/torchrl/train.py:264-316."""
import pytest

import oracle_cases as oc
from geometry_rl_amd import synthetic as syn
from oracle_cases import M_TOL, V_TOL
from updater_cases import moments_and_params_after

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,B,K", [("rigid_g1", 64, 5), ("cloth", 16, 5), ("empn_g2", 32, 5), ("rigid_g1", 1024, 5), ("cloth_full", 256, 3)])
def test_five_updates_match_the_oracle(name, B, K):
    from geometry_rl_amd import agent, graph
    from oracle import graph as ogr
    oc.cap_oracle_threads()
    case = (ogr.cloth_spec(), graph.cloth_spec(), dict(trust_region_coeff=4.0, cov_bound=0.001)) if name == "cloth_full" else name
    pair = oc.build_pair(case, B, seed=21)
    spec, cfg, loss = pair.spec, pair.cfg, pair.loss
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batches = []
    for i in range(K):
        b = dict(oc.obs_of(name, B, 30 + i))
        b.update(syn.make_ppo_fields(B, A, seed=40 + i))
        batches.append(b)
    oc.adopt_calibration(pair, batches[0])   # first training call: calibration on the first minibatch, then identical weights on both sides
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=True)

    def per_step(i, out, ref):
        for k in ("loss_objective", "loss_trust_region", "loss_critic", "kl"):   # the trajectories stay together step by step
            e = abs(float(out[k]) - float(ref[k]))
            assert e <= 1e-4 * max(1.0, abs(float(ref[k]))), (i, k, e)
    g_scale = oc.run_updates(pair, batches, upd, per_step)
    assert upd.mode.startswith("graph") and upd._program is not None
    bad, _ = moments_and_params_after(upd, pair.actor, pair.critic, pair.oracle, cfg, g_scale, K, M_TOL, V_TOL)   # (the rules: updater_cases)
    assert not bad, bad
