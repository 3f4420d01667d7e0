"""geometry_rl_amd.refconfig without a GPU: (a) the 15 task configs compose to the values their YAML files state; (b) the composition rules
one by one on a tree written to tmp_path; (c) overrides; (d) every key is accounted for; (e) all 15 build on the CPU into what the
hand-written ``agent.build_agent`` twin builds; (f) ``build_agent`` is unchanged with the two new AgentConfig fields at None; (g) the command
line.  CPU builds construct parameter holders only (as tests/test_boundary_factories_cpu.py does): no kernel runs."""
import os
import subprocess
import sys

import pytest
import torch

import refconfig_cases as rcase
from refconfig_cases import CONFIGS, NAMES, TABLE, cfg_name

from geometry_rl_amd import refconfig
from geometry_rl_amd.refconfig import ConfigError, compose


@pytest.fixture(scope="module")
def composed():
    return {n: compose(CONFIGS, cfg_name(n)) for n in NAMES}


def test_the_copied_tree_is_the_whole_tree():
    files = [os.path.join(d, f) for d, _, fs in os.walk(CONFIGS) for f in fs]
    assert len(files) == 43 and all(f.endswith(".yaml") and os.path.getsize(f) <= 8 << 10 for f in files)
    assert sorted(f[:-len("_trpl_cfg.yaml")] for f in os.listdir(CONFIGS) if f.endswith(".yaml")) == NAMES and len(NAMES) == 15


# ------------------------------------------------------------------------------------------------------------- (a) composition
@pytest.mark.parametrize("name", NAMES)
def test_task_config_composes_to_what_its_files_say(composed, name):
    cfg, row = composed[name], TABLE[name]
    algo, obj, proj, optim, pol, val = (cfg["algorithm"],) + tuple(cfg["algorithm"][k] for k in ("objective", "projection", "optim", "policy",
                                                                                                  "value"))
    # common to all
    assert algo["name"] == "trpl"
    assert (proj["proj_type"], proj["scale_prec"], proj["entropy_schedule"], proj["mean_bound"]) == ("kl", True, False, 0.05)
    assert (obj["gamma"], obj["gae_lambda"], obj["ppo_epochs"], obj["clip_value"], obj["clip_epsilon"]) == (0.99, 0.95, 5, 0.2, 0.2)
    assert obj["entropy_bonus"] is True and obj["critic_coef"] == 0.5 and obj["loss_critic_type"] == "l2"
    assert type(optim["lr"]) is float and optim["lr"] == 3e-4 and optim["anneal_lr"] is False
    assert type(pol["minimal_std"]) is float and pol["minimal_std"] == 1e-5
    c_model, c_data = val["pyg_agent"]["model"], val["pyg_agent"]["data"]
    assert c_model["_target_"] == rcase.DEEPSETS
    assert (c_data["base_data"]["full_graph_obs"], c_data["base_data"]["dist_as_pos"]) == (True, False)
    a_model, a_data = pol["pyg_agent"]["model"], pol["pyg_agent"]["data"]
    assert (a_data["base_data"]["full_graph_obs"], a_data["base_data"]["dist_as_pos"]) == (False, True)
    # the table
    assert a_model["_target_"] == row["model"]
    fam = f"geometry_rl.modules.pyg_data.{row['family']}_tasks_data."
    for data in (a_data, c_data):
        assert data["base_data"]["_target_"] == fam + row["family"].capitalize() + "TasksData"
        assert (data["node_type_class"], data["edge_type_class"], data["edge_level_class"]) == (fam + "NodeType", fam + "EdgeType",
                                                                                                fam + "EdgeLevel")
    assert pol["action_dim"] == row["action_dim"]
    assert a_model.get("ponita_dim") == row["ponita_dim"]
    assert (a_model["output_dim"], a_model.get("output_dim_vec")) == row["out"]
    assert a_data["base_data"]["training_noise"] is row["noise"] and a_data["base_data"]["training_noise_std"] == 0.01
    assert c_data["base_data"]["training_noise"] is False
    assert (a_data["input_node_aux_dim"], c_data["input_node_aux_dim"]) == row["aux"]
    assert obj["mini_batch_size"] == row["mini_batch_size"] and obj["clip_grad_norm"] is row["clip_grad_norm"]
    assert proj["cov_bound"] == row["cov_bound"] and proj["trust_region_coeff"] == row["trust_region_coeff"]
    assert obj["entropy_coef"] == row["entropy_coef"]
    assert (cfg["collector"]["frames_per_batch"], cfg["collector"]["total_frames"], cfg["env"]["num_envs"]) == (
        row["frames_per_batch"], row["total_frames"], row["num_envs"])
    assert cfg["collector"]["batch_size"] == row["num_envs"]                       # ${env.num_envs}, typed
    assert a_model.get("only_upper_hemisphere") is row["only_upper_hemisphere"]
    assert a_data["base_data"].get("knn_k") == row["knn_k"] and c_data["base_data"].get("knn_k") == row["knn_k"]
    assert pol["in_features"] == row["actor_in"] and val["in_features"] == row["critic_in"]
    assert pol.get("post_fc") is row["post_fc"]
    assert cfg["experiment_name"] == cfg["env"]["name"] + "_trpl" and cfg["work_dir"] == "${hydra:runtime.cwd}"
    ts = refconfig.train_settings(cfg)
    assert ts.total_network_updates == row["total_network_updates"] and ts.num_mini_batches == row["frames_per_batch"] // row["mini_batch_size"]
    assert (ts.clip_low, ts.clip_high) == (-row["clip"], row["clip"]) and (ts.norm_decay, ts.norm_eps) == (0.99999, 1e-2)
    assert ts.vector_keys == ("position_vectors", "velocity_vectors") and ts.scalar_keys == ("scalars",)
    assert ts.updater_kwargs() == dict(lr=3e-4, clip_grad_norm=row["clip_grad_norm"], max_grad_norm=1.0, anneal_lr=False,
                                       total_network_updates=row["total_network_updates"])
    assert ts.driver_kwargs() == dict(gamma=0.99, lmbda=0.95, ppo_epochs=5, mini_batch_size=row["mini_batch_size"])
    assert ts.normalizer_kwargs()["low"] == -row["clip"]


def test_table_spot_values():
    assert TABLE["rigid_insertion_multi_hepi"]["total_network_updates"] == 100_000
    assert TABLE["rope_closing_hepi"]["total_network_updates"] == 100 * 5 * 200


# ------------------------------------------------------------------------------------------------------------- (b) rules
def _tree(tmp_path, files):
    for rel, text in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    return tmp_path


FOUR = {
    "main.yaml": "defaults:\n  - a: one\n  - _self_\nname: top\nref: ${a.x}\nmixed: v${a.x}_${hydra:job.name}\nkept: ${hydra:x}\n"
                 "lr: 3e-4\nnot1: 1e\nnot2: e5\nnot3: '0x10'\nneg: -1.5E+3\n",
    "a/one.yaml": "defaults:\n  - b: ../../lib/leaf\n  - c: null\n  - d:\n  - base\nx: 7\nwho: one\n",
    "a/base.yaml": "who: base\nfrom_base: 1\n",
    "lib/leaf.yaml": "- k: 1\n- k: 2\n",
}


def test_rules_on_a_four_file_tree(tmp_path):
    cfg = compose(_tree(tmp_path, FOUR), "main")
    assert cfg["a"]["who"] == "one" and cfg["a"]["from_base"] == 1          # own keys last without _self_; a bare entry is the same group
    assert cfg["a"]["b"] == [{"k": 1}, {"k": 2}]                            # relative option at the group's package; list-bodied file
    assert "c" not in cfg["a"] and "d" not in cfg["a"]                      # null option and empty entry skipped
    assert cfg["ref"] == 7 and cfg["mixed"] == "v7_${hydra:job.name}" and cfg["kept"] == "${hydra:x}"
    assert cfg["lr"] == 3e-4 and type(cfg["lr"]) is float and cfg["neg"] == -1500.0
    assert (cfg["not1"], cfg["not2"], cfg["not3"]) == ("1e", "e5", "0x10")


def test_explicit_self_first_and_nested_override(tmp_path):
    files = dict(FOUR)
    files["a/one.yaml"] = "defaults:\n  - _self_\n  - base\n  - b: ../../lib/leaf\nx: 7\nwho: one\n"
    files["lib/other.yaml"] = "z: 1\n"
    files["main.yaml"] = "defaults:\n  - a: one\n  - override a/b: ../../lib/other\n  - _self_\nname: top\n"
    cfg = compose(_tree(tmp_path, files), "main")
    assert cfg["a"]["who"] == "base"                                        # explicit _self_ first: the later file wins
    assert cfg["a"]["b"] == {"z": 1}                                        # override of a nested group
    assert compose(tmp_path, "main", ["a/b=../../lib/leaf"])["a"]["b"] == [{"k": 1}, {"k": 2}]   # the command line beats the file's override
    with pytest.raises(ConfigError, match="nothing.yaml"):
        compose(tmp_path, "main", ["a/b=nothing"])
    with pytest.raises(ConfigError, match="a/q"):
        compose(tmp_path, "main", ["a/q=one"])


def test_projection_kl_ends_with_its_own_keys(composed):
    assert all(c["algorithm"]["projection"]["proj_type"] == "kl" for c in composed.values())


# ------------------------------------------------------------------------------------------------------------- (c) overrides
HEPI_CFG = cfg_name("rigid_insertion_multi_hepi")
_ATT = "../../../pyg_agent/model/hepi_attention"


def test_overrides():
    ppo = compose(CONFIGS, HEPI_CFG, ["algorithm=ppo"])
    assert ppo["algorithm"]["name"] == "ppo" and ppo["algorithm"]["projection"]["proj_type"] == "ppo"
    rows = {k: c for k, c, _, _ in refconfig.explain(ppo)}
    assert all(c == "ignored" for k, c in rows.items() if k.startswith("algorithm.projection."))
    assert rows["algorithm.objective.clip_epsilon"] == "used"
    trpl_rows = {k: c for k, c, _, _ in refconfig.explain(compose(CONFIGS, HEPI_CFG))}
    assert all(c == "used" for k, c in trpl_rows.items() if k.startswith("algorithm.projection."))
    kl = compose(CONFIGS, HEPI_CFG, ["algorithm=kl_ppo"])["algorithm"]["objective"]
    assert (kl["dtarg"], kl["beta"], kl["increment"], kl["decrement"], kl["samples_mc_kl"]) == (0.01, 1.0, 2, 0.5, 1)
    att = compose(CONFIGS, HEPI_CFG, ["algorithm/policy/pyg_agent/model=" + _ATT])["algorithm"]["policy"]["pyg_agent"]["model"]
    assert [p["processor"]["aggr"] for p in att["message_passing"]] == ["AttentionalAggregation"] * 3
    assert att["only_upper_hemisphere"] is True and att["output_dim_vec"] == 2      # the task file's own keys still come last
    empn = compose(CONFIGS, cfg_name("rigid_pushing_multi_empn"), ["algorithm.policy.pyg_agent.model.attention=True"])
    assert empn["algorithm"]["policy"]["pyg_agent"]["model"]["attention"] is True
    dt = compose(CONFIGS, HEPI_CFG, ["algorithm=kl_ppo", "algorithm.objective.dtarg=2e-2"])
    assert dt["algorithm"]["objective"]["dtarg"] == 0.02
    with pytest.raises(ConfigError, match="algorithm.objective.dtrag"):
        compose(CONFIGS, HEPI_CFG, ["algorithm.objective.dtrag=0.02"])
    added = compose(CONFIGS, HEPI_CFG, ["+algorithm.policy.trainable_std=False"])
    assert added["algorithm"]["policy"]["trainable_std"] is False
    with pytest.raises(ConfigError, match="exists already"):
        compose(CONFIGS, HEPI_CFG, ["+algorithm.optim.lr=1e-3"])
    typo = compose(CONFIGS, HEPI_CFG, ["+algorithm.objective.dtrag=0.02"])          # a typo that was ADDED does not pass either
    with pytest.raises(ConfigError, match="unknown key 'algorithm.objective.dtrag'"):
        refconfig.explain(typo)


# ------------------------------------------------------------------------------------------------------------- (d) every key
@pytest.mark.parametrize("name", NAMES)
def test_every_key_is_accounted_for(composed, name):
    cfg = composed[name]
    rows = refconfig.explain(cfg)
    leaves = [k for top in ("algorithm", "collector", "env") for k, _ in refconfig._leaves(cfg[top], top)]
    assert [r[0] for r in rows] == leaves and len(set(leaves)) == len(leaves) > 100
    assert {r[1] for r in rows} == {"used", "fixed", "ignored"} and all(r[3] for r in rows)
    by = {r[0]: r for r in rows}
    assert by["algorithm.policy.hidden_sizes"][1] == "fixed" and by["algorithm.policy.activation"][1] == "ignored"
    assert by["env.warmup_steps"][1] == "ignored" and by["collector.batch_size"][1] == "ignored"
    assert by["algorithm.objective.__target__"][1] == "ignored" and by["algorithm.policy.pyg_agent.model.name"][1] == "ignored"


def test_fixed_keys_refuse_other_values():
    with pytest.raises(ConfigError, match=r"algorithm\.policy\.hidden_sizes"):
        refconfig.explain(compose(CONFIGS, HEPI_CFG, ["algorithm.policy.hidden_sizes=[128, 128]"]))
    with pytest.raises(ConfigError, match=r"algorithm\.objective\.loss_critic_type.*smooth_l1"):
        refconfig.explain(compose(CONFIGS, HEPI_CFG, ["algorithm.objective.loss_critic_type=smooth_l1"]))
    for o in ("algorithm.optim.weight_decay=0.01", "algorithm.policy.shared_critic=True", "algorithm.value.value_type=mlp",
              "algorithm.policy.distribution_class=torchrl.modules.TanhNormal", "algorithm.policy.pyg_agent.model.node_encoder_layers=3"):
        with pytest.raises(ConfigError, match=o.split("=")[0].replace(".", r"\.")):
            refconfig.train_settings(compose(CONFIGS, HEPI_CFG, [o]))


def test_normaliser_settings_must_agree():
    with pytest.raises(ConfigError, match=r"env\.transform\.2"):
        refconfig.train_settings(compose(CONFIGS, HEPI_CFG, ["env.transform.2.decay=0.9"]))


# ------------------------------------------------------------------------------------------------------------- (e) CPU builds
def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", NAMES)
def test_builds_on_cpu_into_the_build_agent_twin(name):
    from geometry_rl_amd import agent, policy, trpl
    row = TABLE[name]
    torch.manual_seed(3)
    cfg, (actor, critic, projection, loss) = rcase.build(name)
    assert isinstance(actor, policy.GNNGaussianPolicyDiag) and isinstance(critic, policy.BaseCritic) and isinstance(loss, trpl.TRPLLoss)
    assert type(projection) is trpl.KLProjectionLayer and projection.cov_bound == row["cov_bound"]
    assert projection.trust_region_coeff == row["trust_region_coeff"] == loss.trust_region_coef
    assert loss.in_features == row["actor_in"] and loss.critic_in_features == row["critic_in"]          # each from its own config key
    assert actor.post_fc is (row["post_fc"] is None) and actor.hyper_data.training_noise is row["noise"]
    assert loss.entropy_coef == row["entropy_coef"] and loss.clip_value == 0.2 and loss.critic_coef == 0.5
    spec = actor.hyper_data.spec
    assert spec.family == row["family"] and actor.num_actuators == spec.num_actuators
    twin_cfg = refconfig.to_agent_config(cfg, spec)
    torch.manual_seed(3)
    t_actor, t_critic, t_proj, t_loss = agent.build_agent(spec, twin_cfg, device="cpu")
    assert _shapes(actor) == _shapes(t_actor) and _shapes(critic) == _shapes(t_critic)
    assert t_loss.in_features == loss.in_features and t_loss.critic_in_features == loss.critic_in_features
    assert (t_proj.mean_bound, t_proj.cov_bound, t_proj.trust_region_coeff, t_proj.proj_code) == (
        projection.mean_bound, projection.cov_bound, projection.trust_region_coeff, projection.proj_code)
    # the reference's re-initialisation of the value net's torch Linears is what GNNVFNet does to ``final`` already
    final = critic._network1.final
    assert float(final.bias.detach().abs().max()) == 0.0 and float(final.weight.detach().norm()) == pytest.approx(0.01, rel=1e-5)


def test_critic_of_the_two_norm_configs_reads_normalised_vectors():
    for name in ("rigid_pushing_multi_transformer", "cloth_hanging_multi_transformer"):
        _, (_, _, _, loss) = rcase.build(name)
        assert loss.critic_in_features[:2] == ["scalars", "norm_position_vectors"]
    _, (_, _, _, loss) = rcase.build("rigid_insertion_multi_transformer")
    assert loss.critic_in_features[:2] == ["scalars", "position_vectors"] and loss.in_features[:2] == ["scalars", "norm_position_vectors"]


def test_rope_closing_clips_gradients():
    ts = refconfig.train_settings((CONFIGS, cfg_name("rope_closing_hepi"), ()))
    assert ts.updater_kwargs()["clip_grad_norm"] is True and (ts.clip_low, ts.clip_high) == (-10.0, 10.0)


def test_other_algorithms_and_refusals_build_or_raise_where_built():
    from geometry_rl_amd import klpen, ppo
    _, (_, _, projection, loss) = rcase.build("rigid_insertion_multi_hepi", ["algorithm=ppo", "algorithm.objective.anneal_clip_epsilon=True"])
    assert projection is None and isinstance(loss, ppo.ClipPPOLoss2) and loss.anneal_clip_epsilon and float(loss.clip_epsilon) == pytest.approx(0.2)
    _, (_, _, projection, loss) = rcase.build("rope_shaping_hepi", ["algorithm=kl_ppo", "algorithm.objective.dtarg=0.02"])
    assert projection is None and isinstance(loss, klpen.KLPENPPOLoss) and (loss.dtarg, loss.increment, loss.decrement) == (0.02, 2.0, 0.5)
    _, (actor, _, _, _) = rcase.build("rigid_insertion_multi_hepi", ["algorithm/policy/pyg_agent/model=" + _ATT])
    assert all(c.attention for r in actor.gnn.processor for _, c in r.items())
    _, (actor, _, projection, loss) = rcase.build("rigid_sliding_multi_hepi", ["algorithm.projection.entropy_schedule=linear"])
    assert loss.entropy_control and projection.entropy_schedule_type == "linear"
    with pytest.raises(ConfigError, match="the GCN / MPNN baseline is not built"):
        rcase.build("rigid_insertion_multi_hepi", ["algorithm/policy/pyg_agent/model=../../../pyg_agent/model/gcn"])
    with pytest.raises(NotImplementedError, match="fp32 kernels only"):
        rcase.build("rigid_pushing_multi_empn", ["algorithm.policy.pyg_agent.model.attention=True"], precision="bf16")
    for proj in ("papi", "ppo"):
        with pytest.raises(NotImplementedError, match="only the TRPL projections"):
            rcase.build("rigid_insertion_multi_hepi", [f"algorithm.projection.proj_type={proj}"])
    with pytest.raises(ConfigError, match="input_node_aux_dim = 5.*hands HEPi 4"):
        rcase.build("rigid_insertion_multi_hepi", ["algorithm.policy.pyg_agent.data.input_node_aux_dim=5"])
    with pytest.raises(ConfigError, match="unknown _target_"):
        rcase.build("rigid_insertion_multi_hepi", ["algorithm.policy.pyg_agent.model._target_=torch.nn.Linear"])
    with pytest.raises(ConfigError, match="contextual_std"):   # AgentConfig cannot say it; build_from_config can
        cfg, _ = rcase.build("rigid_insertion_multi_hepi", ["algorithm.policy.contextual_std=False"])
        refconfig.to_agent_config(cfg, rcase.layout("rigid_insertion_multi_hepi")[0])


# ------------------------------------------------------------------------------------------------------------- (f) build_agent unchanged
# Taken on the PARENT commit (before AgentConfig had actor_in_features / critic_in_features): its geometry_rl_amd package extracted with
# ``git archive``, then torch.manual_seed(1234); build_agent(graph.rigid_spec(), AgentConfig(**kw), device="cpu") and _checksum below.  The
# numbers are sums over ~1e5 float32 parameters in float64: a relative 1e-6 allows every parameter a last-bit difference (the orthogonal
# initialisation runs a QR factorisation, whose rounding may differ between CPUs: 1.5e5 parameters of ~0.05 off by one ulp each move a sum by
# ~2e-6 at most coherent, ~1e-6 relative to the smallest of the three); another draw order or initialisation moves them in the first digits.
PARENT = {
    "hepi": (dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2), (149313, 349.3305830188657, 8280.518933609575, -10.562517018783751)),
    "transformer": (dict(model="transformer", output_dim_vec=2), (95501, 524.5404251107991, 7023.522620467113, -6.108265076569612)),
}


def _checksum(actor, critic):
    flat = torch.cat([v.detach().double().reshape(-1) for m in (actor, critic) for v in m.state_dict().values() if v.is_floating_point()])
    w = torch.cos(torch.arange(flat.numel(), dtype=torch.float64))
    return flat.numel(), float(flat.sum()), float(flat.abs().sum()), float((flat * w).sum())


@pytest.mark.parametrize("kind", sorted(PARENT))
def test_build_agent_is_unchanged_with_the_new_fields_at_none(kind):
    from geometry_rl_amd import agent, graph
    kw, want = PARENT[kind]
    cfg = agent.AgentConfig(**kw)
    assert cfg.actor_in_features is None and cfg.critic_in_features is None
    torch.manual_seed(1234)
    actor, critic, _, loss = agent.build_agent(graph.rigid_spec(), cfg, device="cpu")
    got = _checksum(actor, critic)
    assert got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert g == pytest.approx(w, rel=1e-6)
    spec = graph.rigid_spec()
    assert loss.critic_in_features == spec.in_features
    assert loss.in_features == (spec.in_features if kind == "hepi" else ["scalars"] + ["norm_position_vectors", "norm_velocity_vectors"] * 2
                                + ["infos"])
    _, _, _, loss = agent.build_agent(spec, agent.AgentConfig(critic_in_features=list(loss.in_features), **kw), device="cpu")
    assert loss.critic_in_features == loss.in_features


# ------------------------------------------------------------------------------------------------------------- (g) the command line
_CHILD = """
import runpy, sys
sys.argv = ["refconfig"] + sys.argv[1:]
try:
    runpy.run_module("geometry_rl_amd.refconfig", run_name="__main__")
except SystemExit as e:
    code = e.code
maps = open("/proc/self/maps").read()
print("MAPS-HOLD-KERNEL-LIBRARY:", "libgrl_" in maps)
sys.exit(code)
"""


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=rcase.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", _CHILD, CONFIGS, *args], capture_output=True, text=True, env=env, timeout=300)


def test_command_line_prints_the_table_and_loads_nothing():
    r = _cli(HEPI_CFG)
    assert r.returncode == 0, r.stderr
    assert "algorithm.policy.hidden_sizes" in r.stdout and "fixed" in r.stdout and "TrainSettings.total_network_updates = 100000" in r.stdout
    assert "MAPS-HOLD-KERNEL-LIBRARY: False" in r.stdout


def test_command_line_exits_1_with_the_key_on_a_bad_override():
    r = _cli(HEPI_CFG, "algorithm.objective.dtrag=0.02")
    assert r.returncode == 1 and "algorithm.objective.dtrag" in r.stderr and "MAPS-HOLD-KERNEL-LIBRARY: False" in r.stdout
    r = _cli(HEPI_CFG, "algorithm/policy/pyg_agent/model=../../../pyg_agent/model/gcn")
    assert r.returncode == 1 and "the GCN / MPNN baseline is not built" in r.stderr
