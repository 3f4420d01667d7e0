"""Wiring of actor, critic, projection and loss for one task config -- the counterpart of
``examples/torchrl/builders/agent.py:14-80`` + ``builders/utils_algo_graph.py:208-276`` without Hydra / the Isaac env object
(observation layout comes from a TaskSpec instead of ``env.observation_manager``).  The policy-update driver that replaces the inner
loop of ``examples/torchrl/train.py:258-316`` is ``updater.PolicyUpdater`` (importable from here as well)."""
from dataclasses import dataclass
from typing import Optional

import torch

from . import hip
from .graph import HyperData, TaskSpec
from .hepi import HEPi, FiberBundleConv
from .policy import BaseCritic, DeepSets, GNNGaussianPolicyDiag, GNNVFNet
from .klpen import KLPENPPOLoss
from .ppo import ClipPPOLoss2
from .trpl import KLProjectionLayer, TRPLLoss
from .program import _no_gc_while_capturing  # noqa: F401  (re-exported)
from .updater import PolicyUpdater  # noqa: F401  (re-exported: the driver lives in updater.py)


@dataclass
class AgentConfig:
    """Values of configs/<task>_hepi_trpl_cfg.yaml that reach the hot path."""
    model: str = "hepi"
    dim: int = 3
    num_ori: int = 16
    only_upper_hemisphere: bool = False
    output_dim: int = 1
    output_dim_vec: int = 1
    num_layers: int = 2
    codes: tuple = ((1, 0), (0, 1), (0, 1))  # configs/algorithm/pyg_agent/model/hepi.yaml:17-48
    init_std: float = 1.0
    minimal_std: float = 1e-5
    mean_bound: float = 0.05
    cov_bound: float = 0.0025
    proj_type: str = "kl"  # kl | frob | w2 | w2_non_com
    scale_prec: bool = True   # False: the Euclidean forms of kl (unchanged) | frob | w2 (the reference CONSTRUCTOR's default; its configs say True)
    trust_region_coeff: float = 1.0
    entropy_coef: float = 0.005
    critic_coef: float = 0.5
    clip_value: float = 0.2
    lr: float = 3e-4
    clip_grad_norm: bool = False
    max_grad_norm: float = 1.0
    aggr: str = "add"         # "AttentionalAggregation": configs/algorithm/pyg_agent/model/hepi_attention.yaml
    precision: str = "fp32"   # "bf16": BASELINE config 5 -- node latents stored as bf16, one bf16 MFMA per dense product, fp32 accumulation
    # model "empn" only: the ``attention`` key of configs/algorithm/pyg_agent/model/ponita_gcn.yaml (key / query attention weights on the
    # messages of every layer, ponita.py:130-137,154-160); fp32, one rank, every layer on the full edge set (ponita_gcn.py)
    attention: bool = False
    # model "transformer" only: "torch" = stock nn.TransformerEncoder + torch heads (eager updates); "hip" = csrc/transformer_ops.hip, the
    # encoder as one launch each way and the post_fc head as one, recorded like the other actors (fp32; transformer.py)
    transformer_kernels: str = "torch"
    # model "hepi" with aggr="AttentionalAggregation" only: "torch" = the gate network of the attention convolutions as torch modules (a
    # library GEMM + ReLU under autograd); "hip" = inside the softmax-aggregation launches (csrc/grl_gate.h, fp32; hepi.py)
    attention_gate: str = "torch"
    # the actor's HyperData only (configs/rigid_pushing_multi_empn_trpl_cfg.yaml:105-106; every upstream critic config keeps it False)
    training_noise: bool = False
    training_noise_std: float = 0.01
    # configs/algorithm/{trpl,ppo,kl_ppo}.yaml: "trpl" (TRPLLoss + projection), "ppo" (ClipPPOLoss2, no projection; objective/default.yaml)
    algorithm: str = "trpl"
    clip_epsilon: float = 0.2
    # configs/algorithm/kl_ppo.yaml + objective/kl_ppo.yaml: "kl_ppo" (KLPENPPOLoss, no projection, no value clipping).  dtarg is a required
    # key of that objective config (builders/agent.py:65-78 reads objective["dtarg"]): None = not given
    dtarg: Optional[float] = None
    kl_beta: float = 1.0
    kl_increment: float = 2.0
    kl_decrement: float = 0.5
    # entropy control of the projection (configs/algorithm/projection/*.yaml: entropy_schedule, target_entropy, temperature, entropy_eq,
    # entropy_first; utils_algo_graph.py:246-253 adds total_train_steps): None / False = off, "linear" | "exp" = the scheduled entropy
    # projection runs inside the fused loss launch (TRPLLoss(entropy_control=True))
    entropy_schedule: Optional[str] = None
    target_entropy: float = 0.0
    temperature: float = 0.5
    entropy_eq: bool = False
    entropy_first: bool = False
    total_train_steps: Optional[int] = None
    # configs/algorithm/optim/default.yaml:5 anneal_lr, objective/default.yaml anneal_clip_epsilon (train.py:263-276): lr and PPO's clip
    # epsilon of update n are base * (1 - n / total_train_steps), per update and inside every recorded program (PolicyUpdater).  The total is
    # total_train_steps, the number the reference's builder hands the projection (= train.py:54-59, updater.total_network_updates).
    # Both False here (the reference's configs say True): the schedule is opt-in, a caller's own anneal_lr loop keeps working
    anneal_lr: bool = False
    anneal_clip_epsilon: bool = False
    # the tensordict keys handed positionally to the actor / the critic (``policy.in_features`` / ``value.in_features`` of a task config).
    # None = the rule below: the family's six (five) groups, the transformer actor with ``norm_`` vectors in the raw slots.  Two configs
    # (rigid_pushing_multi_transformer, cloth_hanging_multi_transformer) hand their CRITIC the normalised vectors too: refconfig.py
    actor_in_features: Optional[list] = None
    critic_in_features: Optional[list] = None


def updater_kwargs(cfg: AgentConfig) -> dict:
    """The keywords of ``PolicyUpdater(loss, **updater_kwargs(cfg))`` that come from the config: the optimiser's settings
    (configs/algorithm/optim/default.yaml) and the per-update schedule's switch and total."""
    return dict(lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, anneal_lr=cfg.anneal_lr,
                total_network_updates=cfg.total_train_steps)


def build_agent(spec: TaskSpec, cfg: AgentConfig, device="cuda", group=None):
    """-> (actor GNNGaussianPolicyDiag, critic BaseCritic, projection, loss_module)  (agent.py:31-64).  ``cfg.algorithm == "ppo"``: the
    projection is None and the loss a ClipPPOLoss2 (utils_algo_graph.py:244-257 builds no projection for PPO); ``"kl_ppo"``: the
    projection is None and the loss a KLPENPPOLoss (builders/agent.py:65-78), which needs ``cfg.dtarg``.  ``cfg.anneal_clip_epsilon``
    reaches the PPO loss alone (train.py:272); ``cfg.anneal_lr`` is the updater's: ``PolicyUpdater(loss, **updater_kwargs(cfg))``."""
    if cfg.algorithm not in ("trpl", "ppo", "kl_ppo"):
        raise ValueError(f"algorithm '{cfg.algorithm}': trpl | ppo | kl_ppo")
    if cfg.algorithm == "kl_ppo" and cfg.dtarg is None:
        raise ValueError("algorithm 'kl_ppo' needs dtarg (the target KL of configs/algorithm/objective/kl_ppo.yaml): AgentConfig(dtarg=...)")
    n_in = len(spec.node_types) + spec.n_vec  # utils_algo_graph.py:79
    if cfg.attention and cfg.model != "empn":
        raise ValueError(f"AgentConfig(attention=True) is the EMPN actor's key / query attention (model='empn'), not model '{cfg.model}' "
                         "(HEPi's attention variant is aggr='AttentionalAggregation')")
    if cfg.transformer_kernels not in ("torch", "hip"):
        raise ValueError(f"AgentConfig(transformer_kernels=...): 'torch' or 'hip', got {cfg.transformer_kernels!r}")
    if cfg.transformer_kernels == "hip":
        ref = "configs/algorithm/pyg_agent/model/transformer.yaml"
        if cfg.model != "transformer":
            raise NotImplementedError(f"AgentConfig(transformer_kernels='hip') is the transformer baseline actor's switch ({ref}), not "
                                      f"model '{cfg.model}'")
        if cfg.precision != "fp32":
            raise NotImplementedError(f"AgentConfig(transformer_kernels='hip') has fp32 kernels only (csrc/transformer_ops.hip; {ref} runs in "
                                      f"fp32 and needs no other): precision='{cfg.precision}' is not built")
    from .hepi import check_gate_kernels
    check_gate_kernels(cfg.attention_gate, "AgentConfig(attention_gate=...)", cfg.precision,
                       cfg.model == "hepi" and cfg.aggr == "AttentionalAggregation" and any(c for lvl in cfg.codes for c in lvl))
    if cfg.model == "hepi":
        mp = []  # utils_algo_graph.py:29-47: one fresh conv per (level, active round)
        for lvl in range(len(spec.edge_levels)):
            mp.append([FiberBundleConv(64, 64, 64, groups=64, separable=True, widening_factor=4, aggr=cfg.aggr) if cfg.codes[lvl][k] else None
                       for k in range(len(cfg.codes[lvl]))])
        gnn = HEPi(input_dim_node=n_in, input_dim_edge=len(spec.edge_types) + 4, hidden_dim=64, latent_dim=64,
                   output_dim=cfg.output_dim, output_dim_vec=cfg.output_dim_vec, node_type_mapping=spec.node_types,
                   edge_type_mapping=[tuple(e) for e in spec.edge_types], edge_level_mapping=spec.edge_levels,
                   message_passing=mp, num_messages=len(cfg.codes[0]), device=device, num_ori=cfg.num_ori,
                   ponita_dim=cfg.dim, only_upper_hemisphere=cfg.only_upper_hemisphere, precision=cfg.precision,
                   gate_kernels=cfg.attention_gate)
    elif cfg.model == "transformer":   # BASELINE config 1: stock-torch baseline actor + post_fc head on the same loss / critic / updater
        from .transformer import TransformerVanilla
        gnn = TransformerVanilla(input_dim_node=len(spec.node_types) + 3 * spec.n_vec, output_dim=64, num_layers=cfg.num_layers,
                                 num_heads=2, hidden_dim=64, dropout=0.0, concat_global=False, device=device,
                                 kernels=cfg.transformer_kernels)
    elif cfg.model == "empn":
        from .ponita_gcn import PonitaGCN, check_attention_group
        check_attention_group(cfg.attention, group)
        gnn = PonitaGCN(input_dim_node=n_in, output_dim=cfg.output_dim, output_dim_vec=cfg.output_dim_vec,
                        num_layers=cfg.num_layers, hidden_dim=64, num_ori=cfg.num_ori, ponita_dim=cfg.dim,
                        only_upper_hemisphere=cfg.only_upper_hemisphere, device=device, precision=cfg.precision,
                        attention=cfg.attention)
    else:
        raise ValueError(cfg.model)
    post_fc = cfg.model == "transformer"
    a_data = HyperData(spec, full_graph_obs=False, dist_as_pos=True, output_mask_key=spec.actuator, concat_input_vector=post_fc,
                       training_noise=cfg.training_noise, training_noise_std=cfg.training_noise_std)
    if cfg.transformer_kernels == "hip":   # tokens per sample = the points of the actor graph's node types: refused here, not in the first step
        pv = dict(zip(spec.obs_names["position_vectors"], spec.obs_dims["position_vectors"]))
        gnn.n_tokens = sum(pv[t] // 3 for t in a_data.node_type_list)
        gnn.check_tokens(gnn.n_tokens)
    A = spec.num_actuators * cfg.output_dim_vec * 3
    actor = GNNGaussianPolicyDiag(gnn=gnn, hyper_data=a_data, action_dim=A, num_actuators=spec.num_actuators, init="orthogonal",
                                  hidden_sizes=(64, 64), contextual_std=True, init_std=cfg.init_std, minimal_std=cfg.minimal_std,
                                  share_action_dim=True, post_fc=post_fc)
    actor.group = group
    c_data = HyperData(spec, full_graph_obs=True, dist_as_pos=False, output_mask_key=None, concat_input_vector=True)
    c_gnn = DeepSets(input_dim_node=len(spec.node_types) + 3 * spec.n_vec, output_dim=64, hidden_dim=64, device=device)
    critic = BaseCritic(GNNVFNet(gnn=c_gnn, hyper_data=c_data))
    critic._network1.group = group
    # config 1 hands its actor the NORMALISED vectors in the raw-vector slots (configs/rigid_insertion_multi_transformer_trpl_cfg.yaml:88-94)
    a_in = [k if k.startswith("norm_") or "vectors" not in k else "norm_" + k for k in spec.in_features] if post_fc else spec.in_features
    if cfg.actor_in_features is not None:
        a_in = list(cfg.actor_in_features)
    c_in = spec.in_features if cfg.critic_in_features is None else list(cfg.critic_in_features)
    if cfg.algorithm == "ppo":   # builders/agent.py:53-64
        loss = ClipPPOLoss2(actor, critic, clip_epsilon=cfg.clip_epsilon, entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef,
                            clip_value=cfg.clip_value, loss_critic_type="l2", normalize_advantage=True, in_features=a_in,
                            critic_in_features=c_in, group=group, anneal_clip_epsilon=cfg.anneal_clip_epsilon)
        return actor, critic, None, loss
    if cfg.algorithm == "kl_ppo":  # builders/agent.py:65-78 (no clip_value: torchrl's class clips no value)
        loss = KLPENPPOLoss(actor, critic, dtarg=cfg.dtarg, beta=cfg.kl_beta, increment=cfg.kl_increment, decrement=cfg.kl_decrement,
                            entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef, loss_critic_type="l2", normalize_advantage=True,
                            in_features=a_in, critic_in_features=c_in, group=group)
        return actor, critic, None, loss
    projection = KLProjectionLayer(proj_type=cfg.proj_type, mean_bound=cfg.mean_bound, cov_bound=cfg.cov_bound,
                                   trust_region_coeff=cfg.trust_region_coeff, scale_prec=cfg.scale_prec, entropy_schedule=cfg.entropy_schedule or False,
                                   action_dim=A, total_train_steps=cfg.total_train_steps, target_entropy=cfg.target_entropy,
                                   temperature=cfg.temperature, entropy_eq=cfg.entropy_eq, entropy_first=cfg.entropy_first)
    loss = TRPLLoss(actor, critic, projection=projection, entropy_coef=cfg.entropy_coef, critic_coef=cfg.critic_coef,
                    clip_value=cfg.clip_value, loss_critic_type="l2", normalize_advantage=True, in_features=a_in,
                    critic_in_features=c_in, group=group, entropy_control=bool(cfg.entropy_schedule))
    return actor, critic, projection, loss


def gae(reward, done, terminated, values, gamma=0.99, lmbda=0.95):
    """Shifted GAE (train.py:134-140,249-251): reward/done/terminated [N,T], values [N,T+1] -> advantage, value_target [N,T]."""
    hip.check_f32(reward, values)
    N, T = reward.shape
    adv = torch.empty_like(reward)
    tgt = torch.empty_like(reward)
    hip.call("grl_gae_scan", reward.contiguous(), done.to(torch.uint8).contiguous(), terminated.to(torch.uint8).contiguous(),
             values.contiguous(), adv, tgt, N, T, gamma, lmbda)
    return adv, tgt


# ---------------------------------------------------------------------------------------------------- checkpoints
# train.py:336-368 saves {"env", "actor": actor.state_dict(), "critic": critic.state_dict(), "reward"} where ``actor`` is torchrl's
# ProbabilisticActor(TensorDictModule(policy)) -- a TensorDictSequential whose first entry wraps the policy -- and ``critic`` is
# ValueOperator(BaseCritic) (utils_algo_graph.py:146-158,200-203).  The wrappers only add key prefixes.
ACTOR_PREFIX = "module.0.module."
CRITIC_PREFIX = "module."


def _strip(sd, prefix):
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


def load_reference_checkpoint(ckpt, actor, critic=None, strict=True, trust=False):
    """Load a reference ``model_checkpoint_*.pth`` (path or the loaded dict) into the HIP-backed actor / critic (play.py:194-205).
    Parameter names are identical (PyG ModuleDict key mangling and the ``callibrated`` buffers included); returns ckpt["reward"].

    The file is read with ``weights_only=True`` (tensors and plain containers only).  The reference also pickles ``env.state_dict()``
    into the same file (train.py:343-351), which may hold arbitrary objects: if the safe load fails, pass ``trust=True`` to fall back
    to a full unpickle -- only for files you produced yourself, unpickling executes code.

    Note on parity of a loaded policy: the KL covariance projection used when training continues here is validated against this
    repository's KKT restatement (ITPAL's source is not in the reference checkout), see DESIGN.md section 2."""
    if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
        try:
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
        except Exception as e:
            if not trust:
                raise RuntimeError(f"{ckpt!r} cannot be read with weights_only=True ({type(e).__name__}: {e}); pass trust=True to "
                                   "unpickle it fully (executes code from the file)") from e
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    actor.load_state_dict(_strip(ckpt["actor"], ACTOR_PREFIX), strict=strict)
    if critic is not None and "critic" in ckpt:
        critic.load_state_dict(_strip(ckpt["critic"], CRITIC_PREFIX), strict=strict)
    return ckpt.get("reward")


def reference_checkpoint(actor, critic, reward=0.0, env_state=None):
    """The dict train.py:343-351 writes, so the reference's play.py can load a policy trained here."""
    return {"env": env_state if env_state is not None else {},
            "actor": {ACTOR_PREFIX + k: v.detach().cpu().clone() for k, v in actor.state_dict().items()},
            "critic": {CRITIC_PREFIX + k: v.detach().cpu().clone() for k, v in critic.state_dict().items()},
            "reward": reward}
