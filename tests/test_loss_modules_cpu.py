"""The three objectives of the fused loss kernel (TRPLLoss, ClipPPOLoss2, KLPENPPOLoss) behind ONE interface, without a GPU: the base
class, each module's table of report slots, ``out_keys``, ``check_batch`` and its device scalars -- and the argument checks of the five C
entry points of the loss launch, which all return before anything is launched."""
import ctypes

import pytest
import torch

ALGORITHMS = ("trpl", "ppo", "kl_ppo")

# key -> slot of the 14-float report (grl_trpl_report)
TRPL_SLOTS = {"loss_trust_region": 2, "loss_entropy": 3, "ESS": 4, "kl": 5, "mean_constraint": 6, "mean_constraint_max": 7, "cov_constraint": 8,
              "cov_constraint_max": 9, "entropy": 10, "entropy_diff": 11, "loss_objective_value": 12, "constraint": 13}
ENTROPY_SLOTS = {"entropy": 10, "loss_entropy": 3}   # (the two PPO objectives: only with entropy_bonus)
SLOTS = {"trpl": TRPL_SLOTS, "ppo": {"ESS": 4, "loss_objective_value": 12}, "kl_ppo": {"kl": 5, "loss_objective_value": 12}}

TRPL_TAIL = ["ESS", "kl", "constraint", "mean_constraint", "mean_constraint_max", "cov_constraint", "cov_constraint_max", "entropy_diff"]
OUT_KEYS = {   # (entropy_bonus, critic term) -> out_keys
    "trpl": lambda ent, crit: ["loss_objective", "loss_trust_region"] + ["entropy", "loss_entropy"] * ent + ["loss_critic"] * crit + TRPL_TAIL,
    "ppo": lambda ent, crit: ["loss_objective"] + ["entropy", "loss_entropy"] * ent + ["loss_critic"] * crit + ["ESS"],
    "kl_ppo": lambda ent, crit: ["loss_objective", "kl"] + ["entropy", "loss_entropy"] * ent + ["loss_critic"] * crit,
}
NEEDS_OLD = "KLPENPPOLoss needs the old distribution in the minibatch: keys 'loc' and 'var' (or 'covariance_matrix')"


def _loss(algorithm, entropy_bonus=True, critic_coef=1.0):
    from geometry_rl_amd import agent, graph
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, algorithm=algorithm, critic_coef=critic_coef,
                            dtarg=0.01 if algorithm == "kl_ppo" else None)
    torch.manual_seed(0)
    loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")[3]
    loss.entropy_bonus = entropy_bonus
    return loss


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("entropy_bonus", [True, False])
def test_report_slots(algorithm, entropy_bonus):
    from geometry_rl_amd import trpl
    m = _loss(algorithm, entropy_bonus)
    assert m.algorithm == algorithm
    o = torch.arange(14.)
    a_loss, mt = trpl.report_dict(o, m)
    want = dict(SLOTS[algorithm], **(ENTROPY_SLOTS if entropy_bonus and algorithm != "trpl" else {}))
    assert float(a_loss) == 0.0 and {k: int(v) for k, v in mt.items()} == want
    assert {k: int(v) for k, v in trpl.report_dict(o)[1].items()} == TRPL_SLOTS   # (no module: TRPL's table)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("entropy_bonus", [True, False])
@pytest.mark.parametrize("critic_coef", [1, 0])
def test_out_keys(algorithm, entropy_bonus, critic_coef):
    assert _loss(algorithm, entropy_bonus, float(critic_coef)).out_keys == OUT_KEYS[algorithm](int(entropy_bonus), critic_coef)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_one_base_and_its_interface(algorithm):
    from geometry_rl_amd import trpl
    m = _loss(algorithm)
    assert isinstance(m, trpl.FusedLoss) and isinstance(m, trpl._LossBase) and m.world_size == 1
    assert type(m).__mro__[1] is trpl.FusedLoss
    # the report is read again behind the tail launch only where something is launched behind it
    assert m.keeps_report is (algorithm == "kl_ppo")
    assert (type(m).after_report is trpl.FusedLoss.after_report) == (algorithm != "kl_ppo")
    if algorithm != "kl_ppo":
        m.after_report(None)   # (a no-op for the two without an adapt launch)
    scalars = m.device_scalars
    assert list(scalars) == {"trpl": [], "ppo": ["clip_epsilon"], "kl_ppo": ["kl_beta"]}[algorithm]
    assert all(t.numel() == 1 and t.dtype == torch.float32 for t in scalars.values())
    if algorithm == "ppo":
        assert scalars["clip_epsilon"] is m.clip_epsilon
    if algorithm == "kl_ppo":
        assert scalars["kl_beta"] is m.beta


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_check_batch(algorithm):
    m = _loss(algorithm)
    z = torch.zeros(2, 6)
    without = [{}, {"loc": z}, {"var": z}, {"covariance_matrix": z.diag_embed()}]
    for b in without:
        if algorithm == "kl_ppo":
            with pytest.raises(ValueError) as e:
                m.check_batch(b)
            assert str(e.value) == NEEDS_OLD
        else:
            m.check_batch(b)
    m.check_batch({"loc": z, "var": z})
    m.check_batch({"loc": z, "covariance_matrix": z.diag_embed()})


def test_updater_reads_the_scalars_from_the_module():
    """PolicyUpdater's record of the loss module's device storage (a replaced buffer drops the recorded programs) comes from
    ``device_scalars``: no buffer name on its side."""
    from geometry_rl_amd import agent
    for algorithm, names in (("trpl", []), ("ppo", ["clip_epsilon"]), ("kl_ppo", ["kl_beta"])):
        m = _loss(algorithm)
        upd = agent.PolicyUpdater(m, lr=3e-4)
        ptrs = upd._loss_storage()
        assert ptrs == (tuple(t.data_ptr() for t in m.device_scalars.values()) or None) and (ptrs is None) == (not names)


# ---- the argument checks of the five entry points of the loss launch (include/grl_hip.h): raw calls on the built library

_HOST = (ctypes.c_double * 64)()   # a small HOST buffer: the address handed over where an argument must not be NULL
PTR = ctypes.cast(_HOST, ctypes.c_void_p)

# argument names in the order of the C signatures (the stream comes last and is NULL)
TRPL_ARGS = ("cfg", "action_dim", "mean", "sigma", "action", "old_mean", "old_var", "old_logp", "advantage", "value", "old_value", "value_target",
             "dmean", "dsigma", "dvalue", "proj_mean", "proj_var", "adv_stats", "sums", "maxes", "slots", "batch")
PPO_ARGS = ("cfg", "clip_eps", "action_dim", "mean", "sigma", "action", "old_logp", "advantage", "value", "old_value", "value_target", "dmean",
            "dsigma", "dvalue", "adv_stats", "sums", "maxes", "slots", "batch")
KLPEN_ARGS = ("cfg", "beta", "action_dim", "mean", "sigma", "action", "old_mean", "old_var", "old_logp", "advantage", "value", "old_value",
              "value_target", "dmean", "dsigma", "dvalue", "adv_stats", "sums", "maxes", "slots", "batch")
SIGNATURES = {
    "grl_trpl_fwd_bwd": TRPL_ARGS,
    "grl_trpl_fwd_bwd_ent": TRPL_ARGS + ("ent_mode", "ent_beta"),
    "grl_ppo_fwd_bwd": PPO_ARGS,
    "grl_klpen_fwd_bwd": KLPEN_ARGS,
    "grl_trpl_target_terms": ("cfg", "action_dim", "mean", "sigma", "tgt_mean", "tgt_S", "dmean", "dsigma", "sums", "maxes", "slots", "zeros_b",
                              "batch"),
}
# the pointers a case may leave NULL: everything else points at the host buffer unless the case says otherwise
OPTIONAL = ("value", "old_value", "value_target", "dvalue", "proj_mean", "proj_var", "adv_stats", "sums", "maxes")
INTS = {"action_dim": 4, "batch": 4, "ent_mode": 0}

COMMON = [({"action_dim": 0}, -2), ({"action_dim": 17}, -2), ({"batch": 0}, -2), ({"slots": None}, -2)]
GIVEN_VALUE = {"value": PTR, "old_value": PTR, "value_target": PTR, "dvalue": PTR}
CASES = [(name, kw, rc) for name in SIGNATURES for kw, rc in COMMON] + [
    ("grl_trpl_fwd_bwd", {"proj": 3}, -3), ("grl_trpl_fwd_bwd", {"proj": 5}, -3), ("grl_trpl_fwd_bwd", {"proj": 8}, -3),
    ("grl_trpl_fwd_bwd_ent", {"ent_mode": -1}, -2), ("grl_trpl_fwd_bwd_ent", {"ent_mode": 4}, -2), ("grl_trpl_fwd_bwd_ent", {"ent_beta": None}, -2),
    ("grl_ppo_fwd_bwd", {"clip_eps": None}, -2), ("grl_ppo_fwd_bwd", {"mean": None}, -2),
    ("grl_ppo_fwd_bwd", dict(GIVEN_VALUE, dvalue=None), -2),
    ("grl_klpen_fwd_bwd", {"beta": None}, -2), ("grl_klpen_fwd_bwd", {"old_mean": None}, -2),
    ("grl_klpen_fwd_bwd", dict(GIVEN_VALUE, old_value=None), -2),
    ("grl_trpl_target_terms", {"tgt_mean": None}, -2), ("grl_trpl_target_terms", {"zeros_b": None}, -2),
]


@pytest.fixture(scope="module")
def lib():
    from geometry_rl_amd import hip
    return ctypes.CDLL(hip.build(verbose=False))


@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: only where a regressed check can do no more than fail to launch")
@pytest.mark.parametrize("name,kw,rc", CASES, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(CASES)])
def test_entry_points_reject_before_launching(lib, name, kw, rc):
    """Every case differs from an acceptable call in the one argument it names (the pointers a call may omit are NULL, the others point at
    a small host buffer), so the code is that of the check under test; all of them return before the launch."""
    kw = dict(kw)
    if name in ("grl_ppo_fwd_bwd", "grl_klpen_fwd_bwd"):   # cfg6: .., 1 / B_global, B_global, adv_local
        cfg = (ctypes.c_double * 6)(0.0, 1.0, 0.0, 0.25, 4.0, 0.0)
    else:                                                  # cfg9: .., 1 / B_global, B_global, projection type, adv_local
        cfg = (ctypes.c_double * 10)(0.05, 0.0025, 1.0, 0.0, 1.0, 0.0, 0.25, 4.0, float(kw.pop("proj", 0)), 0.0)
    args = []
    for a in SIGNATURES[name]:
        if a == "cfg":
            v = cfg
        elif a in INTS:
            v = ctypes.c_int(kw.get(a, INTS[a]))
        else:
            v = kw.get(a, None if a in OPTIONAL else PTR)
            v = ctypes.c_void_p(0) if v is None else v
        args.append(v)
    assert not set(kw) - set(SIGNATURES[name])
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    assert fn(*args, ctypes.c_void_p(0)) == rc
