"""The recorder of programs (``program.record``) and the entry lists ``PolicyUpdater`` hands it, without a GPU: the recorder is given a
stand-in for ``capture`` that returns its closures, the updater is built on the CPU (its plan builders build closures, they call none)."""
import torch

from geometry_rl_amd.program import Entry, record


class FakeGraph:
    """What the stand-in capture returns: the closures it was given and the pool it was handed; ``pool()`` is a token of its own."""

    def __init__(self, fns, pool):
        self.fns, self.pool_in, self.token = list(fns), pool, object()

    def pool(self):
        return self.token


def _record(entries):
    streams = []

    def fake_capture(fns, pool=None, stream=None):
        streams.append(stream)
        return FakeGraph(fns, pool)
    return record(entries, capture=fake_capture), streams


def test_recorder_groups_runs_per_lane_and_keeps_the_rest():
    ran = []
    f = [lambda i=i: ran.append(i) for i in range(12)]
    host = []
    entries = [Entry("fork", None),
               Entry("run", f[0]), Entry("run", f[1]),                  # two runs of one lane: ONE graph
               Entry("run", f[2], "s"),                                 # a lane change closes the group
               Entry("sum", lambda: None, "s", "a_collective"),         # a collective closes it
               Entry("run", f[3], "s"), Entry("run", f[4], "s"),        # the lane's second graph: the first one's pool
               Entry("run", f[5], "m", None, True),                     # an eager run closes it and is kept
               Entry("run", f[6]),
               Entry("run_host", lambda: host.append("h")),             # host bookkeeping closes it, runs once, is not kept
               Entry("run", f[7]), Entry("run", f[8]),
               Entry("join", None, "m", "the_join")]
    program, streams = _record(entries)
    assert [e.kind for e in program] == ["fork", "graph", "graph", "sum", "graph", "run", "graph", "graph", "join"]
    assert [e.lane for e in program] == ["m", "m", "s", "s", "s", "m", "m", "m", "m"]
    graphs = [e.item for e in program if e.kind == "graph"]
    assert [g.fns for g in graphs] == [[f[0], f[1]], [f[2]], [f[3], f[4]], [f[6]], [f[7], f[8]]]
    assert ran == []                                                    # (the stand-in calls nothing; neither does the recorder)
    m0, s0, s1, m1, m2 = graphs
    assert m0.pool_in is None and s0.pool_in is None                    # the first graph of a lane opens its pool
    assert s1.pool_in is s0.token                                       # the second graph of a lane is handed the first one's pool
    assert m1.pool_in is m0.token and m2.pool_in is m1.token
    m_pools, s_pools = {m0.token, m1.token, m2.token}, {s0.token, s1.token}
    assert {m1.pool_in, m2.pool_in} <= m_pools and {s1.pool_in} <= s_pools   # graphs of different lanes never share a pool
    assert len(set(map(id, streams))) == 1                              # one capture stream for the whole recording
    assert host == ["h"] and all(e.kind != "run_host" for e in program)
    kept = [e for e in program if e.kind != "graph"]
    assert len(kept) == 4 and all(a is b for a, b in zip(kept, [entries[0], entries[4], entries[7], entries[12]]))


def _updater(**kw):
    from geometry_rl_amd import agent, graph
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device="cpu")
    return agent.PolicyUpdater(loss, lr=cfg.lr, **kw)


_Q = [("run", "s", None, None), ("sum", "s", "critic_ln1_fwd_stats", "group"),
      ("run", "s", None, None), ("sum", "s", "critic_ln2_fwd_stats", "group"),
      ("run", "m", None, None), ("sum", "m", "flat_gradient_actor+loss_records", "group"),
      ("run", "s", None, None), ("sum", "s", "critic_ln2_bwd_stats", "group"),
      ("run", "s", None, None), ("sum", "s", "critic_ln1_bwd_stats", "group"),
      ("run", "m", None, None),
      ("run", "s", None, None), ("sum", "s", "flat_gradient_critic", "group"), ("sum", "s", "loss_critic_sum", "group"),
      ("run", "s", None, None),
      ("join", "m", "join_critic_lane", None), ("run_host", "m", None, None)]
OUTLINE = {True: [("fork", "m", None, None)] + _Q,
           False: [("fork", "m", None, None), ("run", "m", None, None), ("sum", "m", "advantage_stats", "group")] + _Q}

OBS = ["scalars", "position_vectors", "velocity_vectors", "norm_position_vectors", "norm_velocity_vectors", "infos"]


def test_outline_and_rollout_keys_are_what_they_were():
    from types import SimpleNamespace
    upd = _updater()
    for published in (True, False):
        assert upd.program_outline(published) == OUTLINE[published]
    for var, data in (("var", {"var": 0, "adv_stats": 0}), ("covariance_matrix", {})):
        a, c, both = upd._rollout_keys(SimpleNamespace(data=data))
        assert a == OBS + ["action", "loc", var, "sample_log_prob", "advantage"]
        assert c == OBS + ["state_value", "value_target"]
        # (adv_stats only with a process group: this updater has none)
        assert both == OBS + ["action", "loc", var, "sample_log_prob", "state_value", "advantage", "value_target"]
    upd.group = object()
    assert upd._rollout_keys(SimpleNamespace(data={"var": 0, "adv_stats": 0}))[2][-2:] == ["value_target", "adv_stats"]
    assert upd._rollout_keys(SimpleNamespace(data={"var": 0}))[2][-1] == "value_target"


def _cpu_buffer(N, T):
    from geometry_rl_amd import synthetic as syn
    from geometry_rl_amd.rollout import RolloutBuffer
    frames = []
    for t in range(T):
        b = dict(syn.make_rigid_obs(N, seed=3 + t))
        b.update(syn.make_ppo_fields(N, 6, seed=3 + t))
        frames.append(b)
    return RolloutBuffer({k: torch.stack([f[k] for f in frames], dim=1) for k in frames[0]})


def test_multi_step_entry_list_shape():
    """Three steps per launch as ONE entry list: per lane and step the gather of index row j and the step; the gate's wait first on the
    critic's lane, only when gated; every step its own state and its own entry of the entropy-bound table."""
    upd = _updater()
    buf = _cpu_buffer(4, 3)
    idx0 = torch.arange(4) * 3
    for gate in (True, False):
        entries, ep = upd._epoch_entries(buf, idx0, 3, gate)
        kinds = [e.kind for e in entries]
        per_step_s = ["critic_gate_wait", "gather", None] if gate else ["gather", None]
        assert kinds == ["fork"] + ["run"] * (6 + 3 * len(per_step_s)) + ["join"] + ["run_host"] * 3
        runs = [e for e in entries if e.kind == "run"]
        assert [(e.lane, e.label) for e in runs] == [("m", "gather"), ("m", None)] * 3 + [("s", lab) for lab in per_step_s] * 3
        assert not any(e.eager for e in runs)
        program, _ = _record([e for e in entries if e.kind != "run_host"])
        assert [(e.kind, e.lane) for e in program] == [("fork", "m"), ("graph", "m"), ("graph", "s"), ("join", "m")]
        assert [len(e.item.fns) for e in program if e.kind == "graph"] == [6, 3 * len(per_step_s)]
        sts = ep["sts"]
        assert len(sts) == 3 and len({id(st) for st in sts}) == 3
        assert [st["beta"].data_ptr() - upd.beta_table.data_ptr() for st in sts] == [0, 8, 16]
        assert ep["idx"].shape == (3, 4) and ep["key"][:3] == (4, 3, False)
