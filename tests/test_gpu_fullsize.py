"""BASELINE.json's full size (4096-frame minibatches of configs 2 / 3 / 4 / 5: rigid HEPi, cloth HEPi, two-agent EMPN, variable-length rope
HEPi in the fp32 and the bf16 build) through properties that hold at any size -- the CPU oracle needs minutes per update there, so it
is not the checker:

* the whole policy update is bitwise reproducible (loss dict, flat gradient, post-Adam parameters);
* permuting the frames of the minibatch changes nothing but the summation order (every loss term is a sum over frames, the graphs
  are per frame): loss terms and the flat gradient agree to rounding;
* the sum of the gradients of four 1024-frame shards, each scaled by 1/B_global inside the kernels, equals the full-batch gradient
  (the data-parallel identity of DESIGN.md section 5: the shard statistics are combined exactly where
  the all-reduces sit) -- checked with four gloo ranks sharing cuda:0."""
import contextlib
import os
import sys

import pytest
import torch

from updater_cases import DEV, DPCase, assert_ranks_match, calibrate, spawn_dp

pytestmark = pytest.mark.gpu
B = 4096
KEYS = ("loss_objective", "loss_trust_region", "loss_entropy", "loss_critic", "kl", "ESS", "mean_constraint", "cov_constraint", "entropy")


WORKLOADS = ["rigid_hepi", "cloth_hepi", "rigid2_empn", "rope_hepi_var", "rope_hepi_bf16"]


def _case(wl, group=None):
    """Same seed on every rank: identical replicas, calibrated on the full batch."""
    from geometry_rl_amd import agent, synthetic as syn
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench   # the workload table of the benchmark: the SAME specs / configs / synthetic inputs the reported numbers run on
    spec, cfg, make_obs, _ = bench.workload(wl)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV, group=group)
    batch = dict(make_obs(B, 3, 0))
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=3))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    calibrate(actor, spec, batch)
    return DPCase(spec, cfg, actor, critic, proj, loss, batch)


def _updater_kw(cfg):
    return dict(clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm)


def _one_update(loss, cfg, batch):
    from geometry_rl_amd import agent
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, **_updater_kw(cfg))
    p0 = upd.flat.clone()
    out = upd.step(batch)
    res = ({k: float(out[k]) for k in KEYS}, upd.gflat.clone(), upd.flat.clone())
    upd.flat.copy_(p0)            # parameters back, moments are per updater: the next updater starts from the same state
    return res


@pytest.mark.parametrize("wl", WORKLOADS)
def test_full_size_update_is_reproducible_and_permutation_invariant(wl):
    spec, cfg, actor, critic, _, loss, batch = _case(wl)
    tol_l, tol_g = (2e-5, 1e-4) if cfg.precision == "fp32" else (2e-3, 2e-2)   # bf16 build: another summation order moves bf16 roundings
    l0, g0, p0 = _one_update(loss, cfg, batch)
    l1, g1, p1 = _one_update(loss, cfg, batch)
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1), (int((g0 != g1).sum()), float((g0 - g1).abs().max()), float(g0.abs().max()))
    assert torch.equal(p0, p1)
    assert all(v == v and abs(v) < 1e6 for v in l0.values()) and float(g0.abs().max()) > 0
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(g0.device)
    # the kNN topology is cached per batch size and reused for later batches (reference quirk, rigid_tasks_data.py:254-255): the
    # permuted minibatch needs its own
    actor.hyper_data._cache.clear()
    critic._network1.hyper_data._cache.clear()
    lp, gp, _ = _one_update(loss, cfg, {k: v[perm].contiguous() for k, v in batch.items()})
    for k in KEYS:
        assert abs(lp[k] - l0[k]) <= tol_l * max(1.0, abs(l0[k])), (k, lp[k], l0[k])
    scale = float(g0.abs().max())
    assert float((gp - g0).abs().max()) <= tol_g * scale, float((gp - g0).abs().max()) / scale


@contextlib.contextmanager
def _gradient_from_unchanged_parameters(case, upd, shard, rank, ret):
    """Step 1 eager (builds the shard's topology), step 2 replays the recorded segments, both from the initial parameters."""
    case.actor.hyper_data._cache.clear()
    case.critic._network1.hyper_data._cache.clear()
    p0 = upd.flat.clone()
    yield lambda i: upd.flat.copy_(p0)
    ret[f"gflat{rank}"] = upd.gflat.cpu()


@pytest.mark.parametrize("wl", ["rigid_hepi", "cloth_hepi", "rigid2_empn", "rope_hepi_var"])
def test_full_size_four_shards_match_the_full_minibatch(wl):
    """4 ranks x 1024 frames (all on cuda:0, gloo; second step = hipGraph segments between the collectives) against the 4096-frame
    update: loss terms and the all-reduced flat gradient."""
    case = _case(wl)
    l0, g0, _ = _one_update(case.loss, case.cfg, case.batch)
    ret = spawn_dp((__name__, "_case", dict(wl=wl)), 4, use_graph=True, n_steps=2, keys=KEYS, updater_kw=_updater_kw(case.cfg),
                   extra=(__name__, "_gradient_from_unchanged_parameters"))
    assert_ranks_match(l0, g0.cpu(), {r: (ret[r][0], ret[f"gflat{r}"]) for r in range(4)}, 4, 2e-5, 1e-4 * float(g0.abs().max()))
