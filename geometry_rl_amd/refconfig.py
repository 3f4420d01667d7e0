"""The reference's Hydra config tree as the way in: compose ``configs/<task>_trpl_cfg.yaml`` without Hydra / OmegaConf (PyYAML only),
account for every key, and build actor, critic, projection and loss through this package's mirrors the way the reference's builder does
(``examples/torchrl/builders/utils_algo_graph.py:208-276`` + ``builders/agent.py:31-78``).

  compose(config_root, name, overrides)       the subset of Hydra >= 1.1 composition the reference's tree uses -> plain dict
  explain(cfg)                                every key under algorithm / collector / env: used | fixed | ignored (+ why); unknown raises
  train_settings(cfg)                         what train.py reads outside the models -> TrainSettings
  build_from_config(cfg, obs dims, names, A)  -> (actor, critic, projection, loss_module)
  to_agent_config(cfg, spec)                  the equivalent hand-written agent.AgentConfig, where it can say the same

``python -m geometry_rl_amd.refconfig <config_root> <name> [overrides...]`` prints the key table and the TrainSettings; it builds nothing
and loads no kernel library.  A copy of the reference's tree is under tests/golden/reference_configs/ (tools/make_golden.py
reference_configs)."""
import copy
import os
import re
import sys
from dataclasses import asdict, dataclass
from typing import Optional, Tuple


class ConfigError(ValueError):
    """A config this package cannot compose, or says something it builds differently."""


# ---------------------------------------------------------------------------------------------------------------- scalars
# OmegaConf reads ``3e-4`` as a float; YAML 1.1 (PyYAML) wants a dot in the mantissa and hands back the string
_FLOAT = re.compile(r"[-+]?(\.[0-9]+|[0-9]+(\.[0-9]*)?)[eE][-+]?[0-9]+")


def _scalar(v):
    return float(v) if isinstance(v, str) and _FLOAT.fullmatch(v) else v


def _scalars(node):
    if isinstance(node, dict):
        return {k: _scalars(v) for k, v in node.items()}
    if isinstance(node, list):
        return [_scalars(v) for v in node]
    return _scalar(node)


def _yaml():
    try:
        import yaml
    except ImportError as e:   # raised by the first compose(), not by importing the package
        raise ImportError("geometry_rl_amd.refconfig reads the reference's configs with PyYAML (import yaml), which is not installed; "
                          "Hydra and OmegaConf are not needed") from e
    return yaml


def _parse_value(text: str):
    return _scalars(_yaml().safe_load(text))


# ---------------------------------------------------------------------------------------------------------------- composition
def _merge(dst: dict, src: dict) -> dict:
    """Dict merges are recursive; lists and scalars replace."""
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = copy.deepcopy(v)
    return dst


def _place(root: dict, package: str, body) -> None:
    """Merge ``body`` at the dotted ``package`` ("" = the root).  A list-bodied file becomes the value there."""
    if not package:
        if not isinstance(body, dict):
            raise ConfigError("the primary config must be a mapping")
        _merge(root, body)
        return
    node, keys = root, package.split(".")
    for k in keys[:-1]:
        if not isinstance(node.get(k), dict):
            node[k] = {}
        node = node[k]
    if isinstance(body, dict) and isinstance(node.get(keys[-1]), dict):
        _merge(node[keys[-1]], body)
    else:
        node[keys[-1]] = copy.deepcopy(body)


class _Composer:
    def __init__(self, root, group_overrides):
        self.root = os.fspath(root)
        self.cli = dict(group_overrides)      # group path -> option, from the command line: wins over a file's ``override`` entries
        self.file_overrides = {}              # group path -> option, from ``override <group>: option`` entries of the defaults lists
        self.chosen = set()                   # group paths that a defaults list selected
        self.parts = []                       # (package, body) in merge order

    def load(self, rel, why):
        path = os.path.join(self.root, rel + ".yaml")
        if not os.path.isfile(path):
            raise ConfigError(f"{why}: no such config file {path}")
        with open(path) as f:
            body = _yaml().safe_load(f)
        return {} if body is None else _scalars(body)

    def option_of(self, group, option):
        if group in self.cli:
            return self.cli[group]
        return self.file_overrides.get(group, option)

    def expand(self, rel, group, why):
        """Place the file ``rel`` (path below the root, no suffix), chosen for the group path ``group`` ("" = the primary file): its
        defaults list in order, its own keys at ``_self_`` or -- where that is absent -- last (Hydra >= 1.1)."""
        body = self.load(rel, why)
        package = group.replace("/", ".")
        if not isinstance(body, dict):
            self.parts.append((package, body))
            return
        body = dict(body)
        defaults = body.pop("defaults", None) or []
        entries = []
        for d in defaults:   # the ``override`` entries first: they replace an option chosen anywhere below, nested groups included
            if isinstance(d, dict):
                (k, v), = d.items()
                if k.startswith("override "):
                    self.file_overrides[k[len("override "):].strip().lstrip("/")] = v
                    continue
            entries.append(d)
        if "_self_" not in entries:
            entries.append("_self_")
        for d in entries:
            if d == "_self_":
                self.parts.append((package, body))
            elif isinstance(d, str):   # a bare name: a file of the same group, merged at the same package
                sibling = os.path.normpath(os.path.join(os.path.dirname(rel), d))
                self.expand(sibling, group, f"defaults entry '{d}' of {rel}.yaml")
            else:
                (k, v), = d.items()
                sub = f"{group}/{k}" if group else k
                self.chosen.add(sub)
                v = self.option_of(sub, v)
                if v is None:   # ``group: null`` and an entry with no value
                    continue
                # a relative option resolves against the GROUP's directory to a file; the package stays the group's
                self.expand(os.path.normpath(os.path.join(sub, str(v))), sub, f"option '{v}' of group '{sub}'")


_INTERP = re.compile(r"\$\{([^${}]+)\}")


def _lookup(root, dotted):
    node = root
    for k in dotted.split("."):
        if isinstance(node, dict) and k in node:
            node = node[k]
        elif isinstance(node, list) and k.isdigit() and int(k) < len(node):
            node = node[int(k)]
        else:
            raise KeyError(dotted)
    return node


def _resolve(root):
    """``${a.b.c}`` against the composed root; ``${resolver:...}`` (hydra:, now:) and a path that does not exist stay as the literal."""
    def value(s, depth=0):
        if depth > 8:
            raise ConfigError(f"interpolation cycle at {s!r}")
        m = _INTERP.fullmatch(s)
        if m and ":" not in m.group(1):   # the whole string is one reference: the value keeps its type
            try:
                v = _lookup(root, m.group(1).strip())
            except KeyError:
                return s
            return value(v, depth + 1) if isinstance(v, str) else copy.deepcopy(v)

        def sub(mm):
            if ":" in mm.group(1):
                return mm.group(0)
            try:
                v = _lookup(root, mm.group(1).strip())
            except KeyError:
                return mm.group(0)
            return str(value(v, depth + 1)) if isinstance(v, str) else str(v)
        return _INTERP.sub(sub, s)

    def walk(node):
        if isinstance(node, dict):
            for k in node:
                node[k] = walk(node[k])
            return node
        if isinstance(node, list):
            return [walk(v) for v in node]
        return value(node) if isinstance(node, str) and "${" in node else node
    return walk(root)


def _set_key(root, dotted, value, add):
    node, keys = root, dotted.split(".")
    for i, k in enumerate(keys[:-1]):
        if isinstance(node, list) and k.isdigit() and int(k) < len(node):
            node = node[int(k)]
        elif isinstance(node, dict) and k in node and isinstance(node[k], (dict, list)):
            node = node[k]
        elif add and isinstance(node, dict) and k not in node:
            node[k] = {}
            node = node[k]
        else:
            raise ConfigError(f"override '{dotted}': no key '{'.'.join(keys[:i + 1])}' in the composed config")
    last = keys[-1]
    if isinstance(node, list):
        if not (last.isdigit() and int(last) < len(node)):
            raise ConfigError(f"override '{dotted}': no entry '{last}' in a list of {len(node)}")
        node[int(last)] = value
        return
    if add and last in node:
        raise ConfigError(f"override '+{dotted}': the key exists already (drop the +)")
    if not add and last not in node:
        raise ConfigError(f"override '{dotted}': no such key in the composed config (a new key needs '+{dotted}=...')")
    node[last] = value


def compose(config_root, name: str, overrides=()) -> dict:
    """The composed config of ``<config_root>/<name>.yaml`` as a plain dict (module docstring).  ``overrides``: Hydra-style strings,
    ``group=option`` (a directory of the tree, or a path with ``/``), ``dotted.key=value`` and ``+dotted.key=value``."""
    root = os.fspath(config_root)
    groups, values = {}, []
    for o in overrides:
        if "=" not in o:
            raise ConfigError(f"override {o!r}: expected key=value")
        key, text = o.split("=", 1)
        key = key.strip()
        add = key.startswith("+")
        key = key.lstrip("+")
        if not add and ("/" in key or ("." not in key and os.path.isdir(os.path.join(root, key)))):
            groups[key.strip("/")] = None if text.strip() in ("null", "") else text.strip()
        else:
            values.append((key, _parse_value(text), add))
    c = _Composer(root, groups)
    c.expand(name[:-5] if name.endswith(".yaml") else name, "", "primary config")
    for g, opt in groups.items():
        if g not in c.chosen:
            raise ConfigError(f"override '{g}={opt}': no defaults list of this config selects the group '{g}'")
    for g, opt in c.file_overrides.items():
        # (hydra/job_logging, hydra/hydra_logging: groups of Hydra's OWN config, which is not in the tree -- nothing here reads them)
        if g not in c.chosen and not g.startswith("hydra/"):
            raise ConfigError(f"'override {g}: {opt}': no defaults list of this config selects the group '{g}'")
    cfg = {}
    for package, body in c.parts:
        _place(cfg, package, body)
    for key, value, add in values:
        _set_key(cfg, key, value, add)
    return _resolve(cfg)


def _as_cfg(cfg) -> dict:
    if isinstance(cfg, dict):
        return cfg
    root, name, *rest = cfg
    return compose(root, name, rest[0] if rest else ())


# ---------------------------------------------------------------------------------------------------------------- the key table
USED, FIXED, IGNORED = "used", "fixed", "ignored"
_REF = "geometry_rl.modules."
_GCN = _REF + "pyg_models.gcn.GCN"
# reference ``_target_`` -> (module of this package, class); None = refused
TARGETS = {
    _REF + "pyg_models.hepi.HEPi": ("hepi", "HEPi"),
    _REF + "pyg_models.ponita.conv.FiberBundleConv": ("hepi", "FiberBundleConv"),
    _REF + "pyg_models.ponita_gcn.PonitaGCN": ("ponita_gcn", "PonitaGCN"),
    _REF + "pyg_models.transformer_vanilla.TransformerVanilla": ("transformer", "TransformerVanilla"),
    _REF + "pyg_models.deepsets.DeepSets": ("policy", "DeepSets"),
    _REF + "pyg_data.rigid_tasks_data.RigidTasksData": ("graph", "RigidTasksData"),
    _REF + "pyg_data.cloth_tasks_data.ClothTasksData": ("graph", "ClothTasksData"),
    _REF + "pyg_data.rope_tasks_data.RopeTasksData": ("graph", "RopeTasksData"),
    _GCN: None,
}
_FAMILY_OF = {_REF + f"pyg_data.{f}_tasks_data.": f for f in ("rigid", "cloth", "rope")}
_TYPE_CLASSES = {"node_type_class": "NodeType", "edge_type_class": "EdgeType", "edge_level_class": "EdgeLevel"}


def _target(name: str):
    """The class of this package that stands for the reference's ``_target_``."""
    if name not in TARGETS:
        raise ConfigError(f"unknown _target_ '{name}': this package mirrors {sorted(t for t, v in TARGETS.items() if v)}")
    if TARGETS[name] is None:
        raise ConfigError("the GCN / MPNN baseline is not built")
    import importlib
    mod, cls = TARGETS[name]
    return getattr(importlib.import_module("." + mod, __package__), cls)


def _family(data_cfg: dict, where: str) -> str:
    t = str(data_cfg.get("base_data", {}).get("_target_"))
    _target(t)
    fam = next((f for p, f in _FAMILY_OF.items() if t.startswith(p)), None)
    if fam is None:
        raise ConfigError(f"{where}.base_data._target_ = {t!r}: not one of the three task data classes")
    for key, cls in _TYPE_CLASSES.items():
        want = next(p for p, f in _FAMILY_OF.items() if f == fam) + cls
        if data_cfg.get(key) != want:
            raise ConfigError(f"{where}.{key} = {data_cfg.get(key)!r}: the data class is {t}, whose types are {want}")
    return fam


_LOGGING = "a name for logging"
_MODEL_KEYS = {
    "HEPi": {
        "_target_": (USED, "the class"), "name": (IGNORED, _LOGGING),
        **{k: (USED, "HEPi(...)") for k in ("latent_dim", "hidden_dim", "output_dim", "output_dim_vec", "num_ori", "degree", "shared_processor",
                                           "concat_global", "num_messages", "ponita_dim", "only_upper_hemisphere")},
        # hepi.HEPi holds ONE bias-free Linear as node encoder and one Linear as decoder, whatever these say; edge attributes are not encoded
        "node_encoder_layers": (FIXED, 2), "edge_encoder_layers": (FIXED, 2), "node_decoder_layers": (FIXED, 2),
        "message_passing.*.code": (USED, "which rounds of the level have a conv"),
        "message_passing.*.processor.*": (USED, "FiberBundleConv(...)"),
    },
    "PonitaGCN": {
        "_target_": (USED, "the class"), "name": (IGNORED, _LOGGING),
        **{k: (USED, "PonitaGCN(...)") for k in ("hidden_dim", "output_dim", "output_dim_vec", "num_layers", "num_ori", "degree",
                                                "widening_factor", "attention", "ponita_dim", "only_upper_hemisphere")},
        "dropout": (IGNORED, "the reference's PonitaGCN takes it and never reads it"),
        "concat_global": (IGNORED, "PonitaGCN has no such argument (the task configs set it for every model)"),
    },
    "TransformerVanilla": {
        "_target_": (USED, "the class"), "name": (IGNORED, _LOGGING),
        **{k: (USED, "TransformerVanilla(...)") for k in ("hidden_dim", "output_dim", "num_heads", "num_layers", "dropout", "concat_global")},
    },
    "DeepSets": {
        "_target_": (USED, "the class"),
        **{k: (USED, "DeepSets(...)") for k in ("hidden_dim", "output_dim", "norm")},
        "concat_global": (IGNORED, "DeepSets has no such argument"),
    },
}
_BASE_DATA = ("_target_", "full_graph_obs", "dist_as_pos", "output_mask_key", "training_noise", "training_noise_std", "concat_input_vector",
              "angular_velocity", "knn_k", "knn_to_actuators_k")
_PROJECTION = ("proj_type", "mean_bound", "cov_bound", "trust_region_coeff", "scale_prec", "entropy_schedule", "target_entropy", "temperature",
               "entropy_eq", "entropy_first")
_ENV_NOTE = "the environment is the caller's"
# pattern (``*`` = one key) -> (class, accepted value | note).  Model keys, the projection block and the transform list: _classify
_KEYS = {
    "algorithm.name": (USED, "trpl | ppo | kl_ppo: which loss, and whether a projection is built"),
    "algorithm.policy.policy_type": (USED, "policy.get_policy_network"),
    "algorithm.policy.distribution_class": (FIXED, "torch.distributions.MultivariateNormal"),
    "algorithm.policy.init": (FIXED, "orthogonal"),
    "algorithm.policy.squash": (FIXED, False),
    "algorithm.policy.shared_critic": (FIXED, False),
    "algorithm.policy.hidden_sizes": (FIXED, [64, 64]),
    "algorithm.policy.out_dim": (FIXED, None),
    "algorithm.policy.activation": (IGNORED, "legacy network: the GNN policy head has no hidden activation"),
    **{f"algorithm.policy.{k}": (USED, "GNNGaussianPolicyDiag(...)") for k in ("minimal_std", "init_std", "contextual_std", "share_action_dim",
                                                                             "post_fc", "trainable_std", "use_tanh_mean")},
    "algorithm.policy.action_dim": (USED, "num_actuators = action width // action_dim"),
    "algorithm.policy.in_features": (USED, "the actor's tensordict keys (loss in_features)"),
    "algorithm.value.value_type": (FIXED, "gnn"),
    "algorithm.value.hidden_sizes": (FIXED, [64, 64]),
    "algorithm.value.activation": (IGNORED, "legacy network: read by the MLP critic only"),
    "algorithm.value.in_features": (USED, "the critic's tensordict keys (loss critic_in_features)"),
    **{f"algorithm.*.pyg_agent.data.base_data.{k}": (USED, "the data class's constructor") for k in _BASE_DATA},
    **{f"algorithm.*.pyg_agent.data.{k}": (USED, "the GNN's type mappings") for k in _TYPE_CLASSES},
    "algorithm.*.pyg_agent.data.input_node_aux_dim": (USED, "input_dim_node = node types + this"),
    "algorithm.*.pyg_agent.data.input_edge_aux_dim": (USED, "input_dim_edge = edge types + this"),
    "algorithm.objective.__target__": (IGNORED, "misspelt _target_ upstream: the builder picks the loss class by algorithm.name"),
    **{f"algorithm.objective.{k}": (USED, "TrainSettings") for k in ("gamma", "gae_lambda", "ppo_epochs", "mini_batch_size", "clip_grad_norm",
                                                                   "max_grad_norm")},
    **{f"algorithm.objective.{k}": (USED, "the loss module (and TrainSettings)") for k in ("clip_epsilon", "anneal_clip_epsilon",
                                                                                          "entropy_bonus")},
    **{f"algorithm.objective.{k}": (USED, "the loss module") for k in ("critic_coef", "entropy_coef", "clip_value", "dtarg", "beta", "increment",
                                                                     "decrement", "samples_mc_kl")},
    "algorithm.objective.loss_critic_type": (FIXED, "l2"),
    "algorithm.optim._target_": (FIXED, "torch.optim.Adam"),
    "algorithm.optim.weight_decay": (FIXED, 0.0),
    "algorithm.optim.lr": (USED, "TrainSettings"),
    "algorithm.optim.anneal_lr": (USED, "TrainSettings"),
    "collector.frames_per_batch": (USED, "TrainSettings"),
    "collector.total_frames": (USED, "TrainSettings"),
    "collector.batch_size": (IGNORED, "= env.num_envs; the collector is the caller's"),
    "env.num_envs": (USED, "TrainSettings"),
    **{f"env.{k}": (IGNORED, _ENV_NOTE) for k in ("name", "seed", "device", "warmup_steps", "eval_type", "extra", "env_info.*", "video",
                                                 "video_length", "video_interval", "video_episode_trigger", "video_dir")},
}
_KEY_RES = [(re.compile(re.escape(p).replace(r"\*", r"[^.]+")), v) for p, v in _KEYS.items()]
_NORMALISERS = {"NDVecNorm": ("in_keys", "out_keys", "shapes", "decay", "eps"), "VecNorm": ("in_keys", "out_keys", "decay", "eps"),
                "ClipTransform": ("low", "high")}


def _leaves(node, prefix):
    """(dotted key, value) of every leaf: mappings and lists of mappings are descended, anything else is a value."""
    if isinstance(node, dict) and node:
        for k, v in node.items():
            yield from _leaves(v, f"{prefix}.{k}" if prefix else str(k))
    elif isinstance(node, list) and node and all(isinstance(v, dict) for v in node):
        for i, v in enumerate(node):
            yield from _leaves(v, f"{prefix}.{i}")
    else:
        yield prefix, node


def _classify(key: str, cfg: dict):
    m = re.fullmatch(r"algorithm\.(policy|value)\.pyg_agent\.model\.(.+)", key)
    if m:
        model = cfg["algorithm"][m.group(1)]["pyg_agent"]["model"]
        table = _MODEL_KEYS[_target(str(model.get("_target_"))).__name__]
        for pat, v in table.items():
            if re.fullmatch(re.escape(pat).replace(r"\*", r"[^.]+"), m.group(2)):
                return v
        return None
    m = re.fullmatch(r"algorithm\.projection\.(.+)", key)
    if m:
        if m.group(1) not in _PROJECTION:
            return None
        if cfg["algorithm"].get("name") != "trpl":
            return IGNORED, "a projection layer is built for algorithm.name == trpl alone"
        return USED, "trpl.get_projection_layer(...)" + (" and the loss's trust_region_coef" if m.group(1) == "trust_region_coeff" else "")
    m = re.fullmatch(r"env\.transform\.(\d+)\.(.+)", key)
    if m:
        entry = cfg["env"]["transform"][int(m.group(1))]
        kind = str(entry.get("_target_", "")).rsplit(".", 1)[-1]
        if m.group(2) == "_target_":
            return (USED, "picks the normaliser's settings") if kind in _NORMALISERS else (IGNORED, "no setting of the normaliser")
        if kind in _NORMALISERS and m.group(2) in _NORMALISERS[kind]:
            return USED, "TrainSettings (ObservationNormalizer)"
        if kind == "ClipTransform" and m.group(2) == "in_keys":
            return IGNORED, "ObservationNormalizer clips every group it writes"
        if kind in ("ReshapeTransform", "FlattenObservation"):
            return IGNORED, "observations arrive flat [B, D]; the kernels read the points of a group themselves"
        return None
    for rx, v in _KEY_RES:
        if rx.fullmatch(key):
            return v
    return None


def explain(cfg) -> list:
    """[(dotted key, "used" | "fixed" | "ignored", value, note)] for every leaf under ``algorithm``, ``collector`` and ``env``.  Raises
    ConfigError for a key in none of the classes, and for a "fixed" key whose value is not the one this package builds."""
    cfg = _as_cfg(cfg)
    rows = []
    for top in ("algorithm", "collector", "env"):
        for key, value in _leaves(cfg.get(top, {}), top):
            c = _classify(key, cfg)
            if c is None:
                raise ConfigError(f"unknown key '{key}' (= {value!r}): nothing in this package reads it, and it is not on the list of keys that "
                                  "are ignored on purpose")
            cls, info = c
            if cls == FIXED:
                if value != info or type(value) is not type(info):
                    raise ConfigError(f"{key} = {value!r}: this package builds {info!r} only")
                info = f"only {info!r} is built"
            rows.append((key, cls, value, info))
    return rows


# ---------------------------------------------------------------------------------------------------------------- train settings
@dataclass(frozen=True)
class TrainSettings:
    """Everything of the config that examples/torchrl/train.py reads outside the models."""
    gamma: float
    gae_lambda: float
    ppo_epochs: int
    mini_batch_size: int
    frames_per_batch: int
    total_frames: int
    num_envs: int
    num_mini_batches: int           # train.py:48: frames_per_batch // mini_batch_size
    total_network_updates: int      # train.py:49-53
    lr: float
    anneal_lr: bool
    clip_grad_norm: bool
    max_grad_norm: float
    anneal_clip_epsilon: bool
    clip_epsilon: Optional[float]   # (kl_ppo's objective has none)
    entropy_bonus: bool
    norm_decay: Optional[float]     # None: the transform list normalises nothing
    norm_eps: Optional[float]
    clip_low: Optional[float]
    clip_high: Optional[float]
    vector_keys: Tuple[str, ...]
    scalar_keys: Tuple[str, ...]

    def updater_kwargs(self) -> dict:
        """The config's share of ``PolicyUpdater(loss, **kw)`` (the keys of agent.updater_kwargs)."""
        return dict(lr=self.lr, clip_grad_norm=self.clip_grad_norm, max_grad_norm=self.max_grad_norm, anneal_lr=self.anneal_lr,
                    total_network_updates=self.total_network_updates)

    def driver_kwargs(self) -> dict:
        """The config's share of ``RolloutDriver(updater, spec, **kw)``."""
        return dict(gamma=self.gamma, lmbda=self.gae_lambda, ppo_epochs=self.ppo_epochs, mini_batch_size=self.mini_batch_size)

    def normalizer_kwargs(self) -> dict:
        """The arguments of ``transforms.ObservationNormalizer`` (device aside)."""
        if self.norm_decay is None or self.clip_low is None:
            raise ConfigError("env.transform holds no VecNorm / NDVecNorm with a ClipTransform: there is no normaliser to configure")
        return dict(vector_keys=self.vector_keys, scalar_keys=self.scalar_keys, decay=self.norm_decay, eps=self.norm_eps, low=self.clip_low,
                    high=self.clip_high)


def train_settings(cfg) -> TrainSettings:
    cfg = _as_cfg(cfg)
    explain(cfg)
    from .updater import total_network_updates
    obj, optim, col = cfg["algorithm"]["objective"], cfg["algorithm"]["optim"], cfg["collector"]
    vec, sca, pairs, clip = [], [], [], None
    for i, t in enumerate(cfg["env"].get("transform") or []):
        kind = str(t.get("_target_", "")).rsplit(".", 1)[-1]
        where = f"env.transform.{i}"
        if kind == "NDVecNorm":
            keys = list(t["in_keys"])
            if list(t.get("out_keys", ["norm_" + k for k in keys])) != ["norm_" + k for k in keys]:
                raise ConfigError(f"{where}.out_keys = {t.get('out_keys')!r}: ObservationNormalizer writes {['norm_' + k for k in keys]!r}")
            if list(t.get("shapes", [3] * len(keys))) != [3] * len(keys):
                raise ConfigError(f"{where}.shapes = {t.get('shapes')!r}: ObservationNormalizer keeps one statistic per axis of 3-vectors, "
                                  f"{[3] * len(keys)!r}")
            vec += keys
            pairs.append((where, t["decay"], t["eps"]))
        elif kind == "VecNorm":
            if "out_keys" in t and list(t["out_keys"]) != list(t["in_keys"]):
                raise ConfigError(f"{where}.out_keys = {t['out_keys']!r}: ObservationNormalizer normalises scalar groups in place")
            sca += list(t["in_keys"])
            pairs.append((where, t["decay"], t["eps"]))
        elif kind == "ClipTransform":
            if clip is not None and clip != (t["low"], t["high"]):
                raise ConfigError(f"{where}: a second ClipTransform with other bounds {t['low']!r} .. {t['high']!r} than {clip!r}; "
                                  "ObservationNormalizer has one pair")
            clip = (t["low"], t["high"])
    for where, decay, eps in pairs[1:]:
        if (decay, eps) != pairs[0][1:]:
            raise ConfigError(f"{where}: decay / eps = {decay!r} / {eps!r} but {pairs[0][0]} has {pairs[0][1]!r} / {pairs[0][2]!r}; "
                              "ObservationNormalizer has one pair")
    fpb, mbs = int(col["frames_per_batch"]), int(obj["mini_batch_size"])
    return TrainSettings(
        gamma=float(obj["gamma"]), gae_lambda=float(obj["gae_lambda"]), ppo_epochs=int(obj["ppo_epochs"]), mini_batch_size=mbs,
        frames_per_batch=fpb, total_frames=int(col["total_frames"]), num_envs=int(cfg["env"]["num_envs"]), num_mini_batches=fpb // mbs,
        total_network_updates=total_network_updates(int(col["total_frames"]), fpb, int(obj["ppo_epochs"]), mbs),
        lr=float(optim["lr"]), anneal_lr=bool(optim["anneal_lr"]), clip_grad_norm=bool(obj["clip_grad_norm"]),
        max_grad_norm=float(obj["max_grad_norm"]), anneal_clip_epsilon=bool(obj.get("anneal_clip_epsilon", False)),
        clip_epsilon=None if "clip_epsilon" not in obj else float(obj["clip_epsilon"]), entropy_bonus=bool(obj.get("entropy_bonus", False)),
        norm_decay=float(pairs[0][1]) if pairs else None, norm_eps=float(pairs[0][2]) if pairs else None,
        clip_low=None if clip is None else float(clip[0]), clip_high=None if clip is None else float(clip[1]),
        vector_keys=tuple(vec), scalar_keys=tuple(sca))


# ---------------------------------------------------------------------------------------------------------------- building
def _instantiate(node: dict, **extra):
    """hydra.utils.instantiate for a mapping with ``_target_``, through the remap table."""
    kw = {k: v for k, v in node.items() if k != "_target_"}
    kw.update(extra)
    return _target(str(node.get("_target_")))(**kw)


def _build_pyg_model(config, input_dim_node, input_dim_edge, node_types, edge_types, edge_levels, device, extra):
    """utils_algo_graph.py:18-58."""
    config = dict(config)
    config.pop("name", None)
    if "message_passing" not in config:
        config["input_dim_node"] = input_dim_node
    else:
        message_passing = []
        for level, message_cfg in enumerate(config.pop("message_passing")):
            message_passing.append([])
            for i in range(config["num_messages"]):   # one fresh conv per (level, active round); shared_processor: HEPi refuses it
                message_passing[level].append(_instantiate(message_cfg["processor"]).to(device) if message_cfg["code"][i] == 1 else None)
        config.update(message_passing=message_passing, input_dim_node=input_dim_node, input_dim_edge=input_dim_edge,
                      node_type_mapping=node_types, edge_type_mapping=edge_types, edge_level_mapping=edge_levels)
    return _instantiate(config, device=device, **extra).to(device)


def _make_pyg_agent(config, where, observation_dim, observation_names, device, extra=None):
    """utils_algo_graph.py:61-95 -> (gnn, base_data)."""
    from . import graph
    data_cfg = config["data"]
    family = _family(data_cfg, where + ".data")
    base_data = _instantiate(data_cfg["base_data"], observation_dim=observation_dim, observation_names=observation_names)
    node_types, edge_types, edge_levels = graph.family_types(family)
    model_cls = _target(str(config["model"].get("_target_"))).__name__
    n_vec = base_data.spec.n_vec
    # what the observation layout gives: HEPi / EMPN embed one norm per vector; the transformer and the critic read the 3 components
    want = n_vec if model_cls in ("HEPi", "PonitaGCN") else 3 * n_vec
    if data_cfg["input_node_aux_dim"] != want:
        raise ConfigError(f"{where}.data.input_node_aux_dim = {data_cfg['input_node_aux_dim']}: the {family} layout hands {model_cls} "
                          f"{want} ({n_vec} vectors per node)")
    input_dim_node = len(node_types) + data_cfg["input_node_aux_dim"]
    input_dim_edge = len(edge_types) + data_cfg["input_edge_aux_dim"]
    extra = dict(extra or {})
    if model_cls not in ("HEPi", "PonitaGCN"):
        extra.pop("precision", None)
    if model_cls != "TransformerVanilla":
        extra.pop("kernels", None)
    if model_cls != "HEPi":
        extra.pop("gate_kernels", None)
    gnn = _build_pyg_model(config["model"], input_dim_node, input_dim_edge, node_types, edge_types, edge_levels, device, extra)
    return gnn, base_data


def _obs_width(observation_dim, key):
    """Width of the observation group ``key`` ([shape per term]; a ``norm_`` group has its raw group's)."""
    terms = observation_dim[key if key in observation_dim else key.replace("norm_", "")]
    return sum(int(d[0]) if hasattr(d, "__len__") else int(d) for d in terms)


def build_from_config(cfg, observation_dim, observation_names, action_dim, *, device="cuda", group=None, precision="fp32",
                      transformer_kernels="torch", attention_gate="torch"):
    """-> (actor GNNGaussianPolicyDiag, critic BaseCritic, projection | None, loss_module): ``make_ppo_models`` (utils_algo_graph.py:208-276)
    and ``AgentBuilder.build`` (builders/agent.py:31-78) on this package's mirrors, step by step.  ``cfg``: a composed dict or
    ``(config_root, name, overrides)``; ``observation_dim`` / ``observation_names``: the observation manager's ``group_obs_term_dim`` /
    ``_group_obs_term_names`` (what graph.spec_from_observation takes); ``action_dim``: the action space's width.  ``precision`` and
    ``transformer_kernels`` / ``attention_gate`` are this package's own switches (agent.AgentConfig), not the config's."""
    import torch
    from . import policy as _policy, trpl as _trpl
    cfg = _as_cfg(cfg)
    ts = train_settings(cfg)   # (runs explain: unknown keys and other values of the fixed keys raise here)
    config = copy.deepcopy(cfg["algorithm"])
    num_outputs = int(action_dim)

    # ---- make_ppo_models:210-215
    config["policy"].pop("distribution_class")   # (fixed: torch.distributions.MultivariateNormal)
    config["policy"].pop("shared_critic")        # (fixed: False)
    critic_type = config["value"].pop("value_type")
    critic_in_features = list(config["value"].pop("in_features"))

    # ---- :226-230 the actor's GNN and data
    policy_pyg = config["policy"].pop("pyg_agent")
    model_cls = _target(str(policy_pyg["model"].get("_target_"))).__name__
    if transformer_kernels not in ("torch", "hip"):
        raise ValueError(f"transformer_kernels: 'torch' or 'hip', got {transformer_kernels!r}")
    if transformer_kernels == "hip" and model_cls != "TransformerVanilla":
        raise NotImplementedError(f"transformer_kernels='hip' is the transformer baseline actor's switch, not {model_cls}'s")
    if transformer_kernels == "hip" and precision != "fp32":
        raise NotImplementedError(f"transformer_kernels='hip' has fp32 kernels only (csrc/transformer_ops.hip): precision='{precision}' is not built")
    if attention_gate != "torch":   # refused here in the switch's own words (HEPi's constructor would refuse the same)
        from .hepi import check_gate_kernels
        check_gate_kernels(attention_gate, "attention_gate=...", precision, model_cls == "HEPi" and any(
            "AttentionalAggregation" in str((m.get("processor") or {}).get("aggr", "")) and any(m.get("code", []))
            for m in policy_pyg["model"].get("message_passing", [])))
    if model_cls == "PonitaGCN":
        from .ponita_gcn import check_attention_group
        check_attention_group(bool(policy_pyg["model"].get("attention", False)), group)
    gnn, hyper_data = _make_pyg_agent(policy_pyg, "algorithm.policy.pyg_agent", observation_dim, observation_names, device,
                                      extra=dict(precision=precision, kernels=transformer_kernels, gate_kernels=attention_gate))

    # ---- :233-243 + _make_probabilistic_actor:123-143
    policy_kwargs = config["policy"]
    actor_in_features = list(policy_kwargs.pop("in_features"))
    policy_kwargs.pop("out_dim")                 # (fixed: null)
    num_actuators = num_outputs // policy_kwargs.pop("action_dim")
    # absent in the transformer configs: the REFERENCE constructor's default applies (abstract_gnn_gaussian_policy.py:37 post_fc=True); this
    # package's GNNGaussianPolicyDiag defaults to False, so the value is always passed
    post_fc = policy_kwargs.pop("post_fc", True)
    if transformer_kernels == "hip":   # tokens per sample: refused here, not in the first step (as agent.build_agent)
        spec = hyper_data.spec
        pv = dict(zip(spec.obs_names["position_vectors"], spec.obs_dims["position_vectors"]))
        gnn.n_tokens = sum(pv[t] // 3 for t in hyper_data.node_type_list)
        gnn.check_tokens(gnn.n_tokens)
    actor = _policy.get_policy_network(proj_type=config["projection"]["proj_type"], squash=False, device=device, dtype=torch.float32,
                                       action_dim=num_outputs, num_actuators=num_actuators, vf_model=None, gnn=gnn, hyper_data=hyper_data,
                                       post_fc=post_fc, **policy_kwargs)
    actor.group = group

    # ---- :244-257
    projection = None
    if config["name"] == "trpl":
        projection = _trpl.get_projection_layer(action_dim=num_outputs, total_train_steps=ts.total_network_updates,
                                                cpu=torch.device(device).type == "cpu", dtype=torch.float32, **config["projection"])

    # ---- :259-274 + _make_value_module:175-198
    c_gnn, c_data = _make_pyg_agent(config["value"].pop("pyg_agent"), "algorithm.value.pyg_agent", observation_dim, observation_names, device)
    value_in_features = sum(_obs_width(observation_dim, k) for k in critic_in_features)
    critic = _policy.get_critic(critic_type=critic_type, dim=value_in_features, gnn=c_gnn, hyper_data=c_data, **config["value"]).to(device)
    # utils_algo_graph.py:195-198 re-initialises every torch.nn.Linear of the value net (orthogonal, gain 0.01, zero bias).  In the reference
    # that is GNNVFNet.final alone -- DeepSets' layers are PyG Linears, which are no torch.nn.Linear -- and policy.GNNVFNet initialises
    # ``final`` exactly so in its constructor, for agent.build_agent as well: nothing is left to do here
    critic._network1.group = group

    # ---- AgentBuilder.build:39-78, + this package's keywords
    obj = cfg["algorithm"]["objective"]
    ours = dict(in_features=actor_in_features, critic_in_features=critic_in_features, group=group)
    if config["name"] == "trpl":
        loss = _trpl.TRPLLoss(actor_network=actor, critic_network=critic, projection=projection, clip_epsilon=obj["clip_epsilon"],
                              loss_critic_type=obj["loss_critic_type"], trust_region_coef=config["projection"]["trust_region_coeff"],
                              entropy_coef=obj["entropy_coef"], entropy_bonus=obj.get("entropy_bonus", False), critic_coef=obj["critic_coef"],
                              clip_value=obj["clip_value"], normalize_advantage=True,
                              entropy_control=bool(config["projection"].get("entropy_schedule")), **ours)
    elif config["name"] == "ppo":
        from .ppo import ClipPPOLoss2
        loss = ClipPPOLoss2(actor_network=actor, critic_network=critic, clip_epsilon=obj["clip_epsilon"],
                            loss_critic_type=obj["loss_critic_type"], entropy_coef=obj["entropy_coef"],
                            entropy_bonus=obj.get("entropy_bonus", False), critic_coef=obj["critic_coef"], clip_value=obj["clip_value"],
                            normalize_advantage=True, anneal_clip_epsilon=bool(obj.get("anneal_clip_epsilon", False)), **ours)
    elif config["name"] == "kl_ppo":
        from .klpen import KLPENPPOLoss
        loss = KLPENPPOLoss(actor_network=actor, critic_network=critic, dtarg=obj["dtarg"], beta=obj["beta"], increment=obj["increment"],
                            decrement=obj["decrement"], samples_mc_kl=obj["samples_mc_kl"], loss_critic_type=obj["loss_critic_type"],
                            entropy_coef=obj["entropy_coef"], critic_coef=obj["critic_coef"], normalize_advantage=True, **ours)
    else:
        raise ConfigError(f"algorithm.name = {config['name']!r}: trpl | ppo | kl_ppo")
    return actor, critic, projection, loss


# ---------------------------------------------------------------------------------------------------------------- AgentConfig
def to_agent_config(cfg, spec):
    """The hand-written form of the config: ``agent.build_agent(spec, to_agent_config(cfg, spec))`` builds the networks and the loss that
    ``build_from_config`` builds.  Raises ConfigError where AgentConfig cannot say what the config says."""
    from .agent import AgentConfig
    cfg = _as_cfg(cfg)
    ts = train_settings(cfg)
    algo = cfg["algorithm"]
    pol, val, obj, proj = algo["policy"], algo["value"], algo["objective"], algo["projection"]
    model, data = pol["pyg_agent"]["model"], pol["pyg_agent"]["data"]["base_data"]
    cls = _target(str(model.get("_target_"))).__name__
    if cls not in ("HEPi", "PonitaGCN", "TransformerVanilla"):
        raise ConfigError(f"AgentConfig.model: hepi | empn | transformer, not {cls}")
    kind = {"HEPi": "hepi", "PonitaGCN": "empn", "TransformerVanilla": "transformer"}[cls]

    def only(key, value, accepted):
        if value != accepted:
            raise ConfigError(f"{key} = {value!r}: agent.build_agent builds {accepted!r} only; AgentConfig cannot say it (use build_from_config)")

    fam = _family(pol["pyg_agent"]["data"], "algorithm.policy.pyg_agent.data")
    only("the actor's task family", fam, spec.family)
    only("the critic's task family", _family(val["pyg_agent"]["data"], "algorithm.value.pyg_agent.data"), spec.family)
    only("algorithm.policy.post_fc", pol.get("post_fc", True), kind == "transformer")
    only("algorithm.policy.contextual_std", pol["contextual_std"], True)
    only("algorithm.policy.share_action_dim", pol["share_action_dim"], True)
    for k in ("trainable_std", "use_tanh_mean"):
        if k in pol:
            only(f"algorithm.policy.{k}", pol[k], k == "trainable_std")
    b = "algorithm.policy.pyg_agent.data.base_data."
    only(b + "full_graph_obs", data.get("full_graph_obs", False), False)
    only(b + "dist_as_pos", data.get("dist_as_pos", False), True)
    only(b + "output_mask_key", data.get("output_mask_key"), spec.actuator)
    only(b + "concat_input_vector", data.get("concat_input_vector", True), kind == "transformer")
    for k, dflt in (("knn_k", 3), ("knn_to_actuators_k", -1), ("angular_velocity", True)):
        if fam == "cloth" and k == "knn_k":
            continue
        only(b + k, data.get(k, dflt), getattr(spec, k))
    cdata = val["pyg_agent"]["data"]["base_data"]
    b = "algorithm.value.pyg_agent.data.base_data."
    only(b + "full_graph_obs", cdata.get("full_graph_obs", False), True)
    only(b + "dist_as_pos", cdata.get("dist_as_pos", False), False)
    only(b + "output_mask_key", cdata.get("output_mask_key"), None)
    only(b + "concat_input_vector", cdata.get("concat_input_vector", True), True)
    only(b + "training_noise", cdata.get("training_noise", False), False)
    only("the critic's model", _target(str(val["pyg_agent"]["model"].get("_target_"))).__name__, "DeepSets")
    kw = {}
    m = "algorithm.policy.pyg_agent.model."
    if kind == "hepi":
        mp = model["message_passing"]
        aggrs = {p["processor"].get("aggr", "add") for p in mp}
        if len(aggrs) != 1:
            raise ConfigError(f"{m}message_passing: processors with different aggr {sorted(aggrs)}; AgentConfig has one")
        for i, p in enumerate(mp):
            want = dict(in_channels=64, out_channels=64, attr_dim=64, groups=64, separable=True, widening_factor=4)
            got = {k: v for k, v in p["processor"].items() if k not in ("_target_", "aggr")}
            only(f"{m}message_passing.{i}.processor", got, want)
        only(m + "num_messages", model["num_messages"], len(mp[0]["code"]))
        kw.update(codes=tuple(tuple(p["code"]) for p in mp), aggr=aggrs.pop())
    if kind in ("hepi", "empn"):
        kw.update(dim=model.get("ponita_dim", 3), num_ori=model["num_ori"], only_upper_hemisphere=model.get("only_upper_hemisphere", False),
                  output_dim=model["output_dim"], output_dim_vec=model["output_dim_vec"])
        only("the action width per actuator (algorithm.policy.action_dim)", pol["action_dim"], 3 * model["output_dim_vec"])
    if kind == "empn":
        kw.update(num_layers=model["num_layers"], attention=bool(model.get("attention", False)))
    if kind == "transformer":
        for k, v in (("num_heads", 2), ("hidden_dim", 64), ("output_dim", 64), ("dropout", 0.0), ("concat_global", False)):
            only(m + k, model.get(k), v)
        kw.update(num_layers=model["num_layers"], output_dim_vec=pol["action_dim"] // 3)
        only("algorithm.policy.action_dim", pol["action_dim"], 3 * kw["output_dim_vec"])
    if algo["name"] == "trpl":
        kw.update(proj_type=proj["proj_type"], scale_prec=proj["scale_prec"], mean_bound=proj["mean_bound"], cov_bound=proj["cov_bound"],
                  trust_region_coeff=proj["trust_region_coeff"], entropy_schedule=proj["entropy_schedule"] or None,
                  target_entropy=proj["target_entropy"], temperature=proj["temperature"], entropy_eq=proj["entropy_eq"],
                  entropy_first=proj["entropy_first"])
    if algo["name"] == "kl_ppo":
        kw.update(dtarg=obj["dtarg"], kl_beta=obj["beta"], kl_increment=obj["increment"], kl_decrement=obj["decrement"])
    else:
        only("algorithm.objective.entropy_bonus", obj.get("entropy_bonus", False), True)
        kw.update(clip_value=obj["clip_value"], clip_epsilon=obj["clip_epsilon"])
    return AgentConfig(model=kind, init_std=pol["init_std"], minimal_std=pol["minimal_std"], entropy_coef=obj["entropy_coef"],
                       critic_coef=obj["critic_coef"], lr=ts.lr, clip_grad_norm=ts.clip_grad_norm, max_grad_norm=ts.max_grad_norm,
                       training_noise=bool(data.get("training_noise", False)), training_noise_std=data.get("training_noise_std", 0.01),
                       algorithm=algo["name"], total_train_steps=ts.total_network_updates, anneal_lr=ts.anneal_lr,
                       anneal_clip_epsilon=ts.anneal_clip_epsilon, actor_in_features=list(pol["in_features"]),
                       critic_in_features=list(val["in_features"]), **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 2:
        print("usage: python -m geometry_rl_amd.refconfig <config_root> <name> [overrides...]", file=sys.stderr)
        return 2
    try:
        cfg = compose(argv[0], argv[1], argv[2:])
        rows = explain(cfg)
        ts = train_settings(cfg)
    except ConfigError as e:
        print(f"ConfigError: {e}", file=sys.stderr)
        return 1
    width = max(len(r[0]) for r in rows)
    for key, cls, value, note in rows:
        print(f"{key:<{width}}  {cls:<7}  {value!r}  # {note}")
    print()
    for k, v in asdict(ts).items():
        print(f"TrainSettings.{k} = {v!r}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
