"""The whole-iteration comparison (tests/test_gpu_iteration_oracle.py) would NOTICE the wiring mistakes it exists for -- shown on the oracle
alone (no GPU), on the same case (tests/iteration_ref.py), with the oracle's own outputs as every stage's inputs.  For each mutation of the
wiring at least one compared quantity of the stage named moves by at least 10 times that stage's allowance:

    i    done and terminated swapped in the GAE call                                        stage c (advantage, value_target)
    ii   the T+1 column = the last frame's value / = 0 instead of the value of next_last    stage c
    iii  values not shifted (V[t] as the next value)                                         stage c
    iv   minibatch rows t * N + i instead of i * T + t                                       stage e (first step's loss dict)
    v    state_value and value_target swapped in the batch                                   stage e
    vi   the normaliser updating on the final observation                                    stage a (iteration 2)
    vii  episode state not carried into the second rollout                                   stage d

The 10 x is a condition on the INPUTS (rewards, done pattern, value head), checked here; it is no tolerance of the GPU test.  Allowances:
a  2e-5;  c  train_ops_ref.gae's allowance on the values + (1 + gamma) / (1 - gamma lambda) x 1e-4 max(1, max |V|);  d  none (the stage is
compared exactly: any movement counts, the ratio is reported against one unit of the inputs' lattices, 2^-8 for rewards and 1 for counts,
which is the smallest movement the stage can show);  e  1e-4 max(1, |ref|) per loss-dict entry."""
import pytest
import torch

import iteration_ref as ir
import train_ops_ref
from oracle_cases import LOSS_KEYS, cap_oracle_threads

FACTOR = 10.0


@pytest.fixture(scope="module")
def chain():
    cap_oracle_threads()
    return ir.run_oracle_chain()


def _stage_c_allowance(it):
    """Per-frame allowance of advantage and value_target: the fp32 scan's (train_ops_ref.gae) + the propagated value allowance."""
    adv, tgt, ea, et = train_ops_ref.gae(it["reward"], it["done"], it["terminated"], it["V"], train_ops_ref.f32(ir.GAMMA), train_ops_ref.f32(ir.LMBDA))
    prop = ir.value_propagation(ir.tol_of(it["V"]))
    return ea + prop, et + prop


def _stage_c_ratio(it, adv_m, tgt_m):
    aa, at = _stage_c_allowance(it)
    adv, tgt = it["data"]["advantage"].reshape(ir.N, -1).double(), it["data"]["value_target"].reshape(ir.N, -1).double()
    return max(float(((adv_m.double() - adv).abs() / aa).max()), float(((tgt_m.double() - tgt).abs() / at).max()))


def _loss_ratio(ref, mut):
    return max(abs(float(mut[k]) - float(ref[k])) / (ir.TOL * max(1.0, abs(float(ref[k])))) for k in LOSS_KEYS)


def _report(name, ratio):
    print(f"mutation {name}: moves a compared quantity by {ratio:.3g} x its allowance")
    assert ratio >= FACTOR, (name, ratio)


def test_pattern_contains_the_five_situations():
    done, term = ir.pattern()
    assert not bool((term & ~done).any())    # terminated implies done
    sit = ir.situations(done, term)
    print(sit)
    assert all(sit.values()), sit
    assert len(sit) == 5
    # the same five through the environment, which is a pure function of its step counter
    env, again = ir.SyntheticEnv(), ir.SyntheticEnv()
    for s in (3, 0, 3):
        for a, b in zip(env.outcome(s), again.outcome(s)):
            assert torch.equal(a, b)
        o, p = env.raw_obs(s), again.raw_obs(s)
        assert sorted(o) == ["infos", "position_vectors", "scalars", "velocity_vectors"] and all(torch.equal(o[k], p[k]) for k in o)
    r = torch.stack([env.reward(s) for s in range(ir.STEPS)])
    assert float(r.abs().max()) <= 4.0 and float(r.abs().mean()) >= 0.5 and torch.equal(r * 256, (r * 256).round())   # O(1), on the lattice


def test_last_step_bootstraps_only_where_it_is_not_terminated(chain):
    """The pattern survives gae_shifted's conventions: moving the T+1 column moves the last-step advantage of the environment that is DONE
    ONLY there by gamma times as much, and leaves the environment TERMINATED there exactly alone."""
    it = chain[0]
    T = it["T"]
    r, d, tm, V = it["reward"].double(), it["done"], it["terminated"], it["V"].double()
    boot = int(torch.nonzero(d[:, -1] & ~tm[:, -1])[0])
    stop = int(torch.nonzero(tm[:, -1])[0])
    adv, _ = ir.otr.gae_shifted(r, d, tm, V, ir.GAMMA, ir.LMBDA)
    V2 = V.clone()
    V2[:, T] += 1.0
    adv2, _ = ir.otr.gae_shifted(r, d, tm, V2, ir.GAMMA, ir.LMBDA)
    assert abs(float(adv2[boot, -1] - adv[boot, -1]) - ir.GAMMA) <= 1e-12
    assert torch.equal(adv2[stop], adv[stop])
    # and the scan with an explicit next value IS the oracle's
    a3, t3 = ir.gae_from(r, d, tm, V[:, :-1], V[:, 1:])
    assert torch.equal(a3, adv) and torch.equal(t3, adv + V[:, :-1])
    # the chain's buffer holds exactly this scan, rounded to float32
    assert torch.equal(it["data"]["advantage"].reshape(ir.N, T), adv.float())


def test_the_chain_is_on_policy_at_the_first_update_of_each_iteration(chain):
    """With the oracle as both sides the first update of each iteration sees p == q: the condition (f) of the GPU test, on the reference."""
    for it in chain:
        first = it["losses"][0]
        for k in ("kl", "mean_constraint", "cov_constraint"):
            assert abs(float(first[k])) <= ir.TOL, (k, float(first[k]))
        assert abs(float(first["ESS"]) - 1.0) <= ir.TOL
    assert len(chain[0]["losses"]) + len(chain[1]["losses"]) == 5


def test_mutations_of_stage_c_move_the_advantages(chain):
    worst = {"i": 0.0, "ii last frame": 0.0, "ii zero": 0.0, "iii": 0.0}
    for it in chain:
        T = it["T"]
        r, d, tm, V = it["reward"].double(), it["done"], it["terminated"], it["V"].double()
        worst["i"] = max(worst["i"], _stage_c_ratio(it, *ir.otr.gae_shifted(r, tm, d, V, ir.GAMMA, ir.LMBDA)))
        Vl, Vz = V.clone(), V.clone()
        Vl[:, T], Vz[:, T] = V[:, T - 1], 0.0
        worst["ii last frame"] = max(worst["ii last frame"], _stage_c_ratio(it, *ir.otr.gae_shifted(r, d, tm, Vl, ir.GAMMA, ir.LMBDA)))
        worst["ii zero"] = max(worst["ii zero"], _stage_c_ratio(it, *ir.otr.gae_shifted(r, d, tm, Vz, ir.GAMMA, ir.LMBDA)))
        worst["iii"] = max(worst["iii"], _stage_c_ratio(it, *ir.gae_from(r, d, tm, V[:, :-1], V[:, :-1])))
    for name, ratio in worst.items():
        _report(name, ratio)


def test_mutations_of_stage_e_move_the_first_loss_dict(chain):
    it = chain[0]
    T = it["T"]
    idx = it["idx"][0]
    oracle_keys = list(ir.ogr.rigid_spec().in_features) + list(ir.PPO_KEYS)
    batch = ir.rows(it["data"], idx, oracle_keys)
    ref = ir.loss_at(it["params"], it["topo"], batch)
    for k in LOSS_KEYS:   # (loss_at on the parameters from before the updates reproduces the chain's first update)
        assert abs(float(ref[k]) - float(it["losses"][0][k])) <= 1e-6 * max(1.0, abs(float(ref[k]))), k
    env_i, t = idx // T, idx % T
    assert torch.equal(env_i, torch.arange(ir.N))      # env-aligned: row i of the minibatch is environment i
    wrong = t * ir.N + env_i
    assert not torch.equal(wrong, idx)
    _report("iv", _loss_ratio(ref, ir.loss_at(it["params"], it["topo"], ir.rows(it["data"], wrong, oracle_keys))))
    swapped = dict(batch, state_value=batch["value_target"], value_target=batch["state_value"])
    _report("v", _loss_ratio(ref, ir.loss_at(it["params"], it["topo"], swapped)))


def test_mutation_of_the_normaliser_moves_iteration_two(chain):
    """vi: the frozen call on the final observation of iteration 1 updating the statistics (the frame is then counted twice)."""
    env, st = ir.SyntheticEnv(), ir.new_norm_state()
    T1, T2 = ir.T_ITERS
    for s in range(T1):
        ir.ref_normalise(env.raw_obs(s), st)
    ir.ref_normalise(env.raw_obs(T1), st, update=True)          # (the mutation)
    ratio = 0.0
    for t in range(T2):
        got = ir.ref_normalise(env.raw_obs(T1 + t), st)
        for k in ("norm_position_vectors", "norm_velocity_vectors", "scalars"):
            ratio = max(ratio, float((got[k] - chain[1]["data"][k][:, t]).abs().max()) / ir.NORM_TOL)
    _report("vi", ratio)
    # without the mutation the same loop IS the chain's buffer
    st = ir.new_norm_state()
    for s in range(T1):
        ir.ref_normalise(env.raw_obs(s), st)
    ir.ref_normalise(env.raw_obs(T1), st, update=False)
    assert torch.equal(ir.ref_normalise(env.raw_obs(T1), st)["scalars"], chain[1]["data"]["scalars"][:, 0])


def test_mutation_of_the_episode_state_moves_iteration_two(chain):
    """vii: stage d is compared exactly, so the movement is reported in units of the inputs' lattices (2^-8, 1)."""
    it = chain[1]
    er, sc, sums = ir.ref_episode_stats(it["reward"], it["done"], ir.new_episode_state())   # (the mutation: a fresh state)
    moved_r = float(abs(er.astype("float64") - it["episode_reward"].astype("float64")).max()) * 256
    moved_c = float(abs(sc.astype("int64") - it["step_count"].astype("int64")).max())
    assert sums.tolist() != it["sums"].tolist()
    _report("vii", max(moved_r, moved_c))
    across = int(torch.nonzero(~chain[0]["done"].any(1) & it["done"].any(1))[0])
    assert int(it["step_count"][across, 0]) == ir.T_ITERS[0] + 1      # the carried episode goes on counting
