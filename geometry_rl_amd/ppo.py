"""Clipped PPO objective on the fused HIP kernel -- drop-in for
``geometry_rl/algorithms/trust_region_projections/objectives/ppo.py`` (ClipPPOLoss2, the loss of ``algorithm=ppo``).

ClipPPOLoss2 subclasses torchrl 0.3.1's ``ClipPPOLoss`` and replaces only ``loss_critic`` (the clipped value loss of
objectives/utils.py:_clip_value_loss, line for line the TRPL one).  The objective is torchrl's ``ClipPPOLoss.forward``; torchrl is not
a dependency of this package, so it is restated here (UNPINNED: no fixture from the reference checks it; tests/ppo_ref.py is the
float64 restatement the kernel is tested against):

    adv  = (adv - mean) / std.clamp_min(1e-6)                      (normalize_advantage, numel > 1; unbiased std)
    lw   = log N(action; loc, diag(sigma^2)) - sample_log_prob
    gain = min(exp(lw) adv, exp(clamp(lw, log1p(-eps), log1p(eps))) adv)
    loss_objective = -mean(gain);  entropy = mean(MVN entropy);  loss_entropy = -entropy_coef * entropy  (entropy_bonus)
    loss_critic = critic_coef * mean(clipped l2);  ESS = exp(2 lse(lw) - lse(2 lw)) / B

Everything -- objective, entropy, value loss, ESS and the analytic gradients -- comes out of ONE launch of ``grl_ppo_fwd_bwd``: the
fused TRPL kernel in its PPO mode (no projection, no trust-region terms), so every recorded program of ``agent.PolicyUpdater`` runs it.

``clip_epsilon`` is a registered float32 buffer on the policy's device, and the kernel reads it from device memory when it runs: an
annealed epsilon written in place (train.py:272-274, ``loss_module.clip_epsilon.copy_(eps * alpha)``) takes effect at the next step
or replay of a recorded step, with nothing recorded again.  Within one launch of several minibatch steps (``run_minibatches``) it is
constant, as the learning rate is."""
import torch

from . import ops
from .trpl import LossDict, _as_batch, _LossBase, _run_trpl, _TensorDict, _unwrap


def ppo_launch(m, loc, sigma, value, batch, adv_stats, sums=None, maxes=None, defer_fold=False, adv_local=False):
    """The PPO counterpart of trpl.trpl_launch (which dispatches here): one launch of the fused kernel on detached inputs ->
    (sums, maxes, dloc, dsigma, dvalue); the slots and sums have the TRPL layout (trust-region / KL columns zero)."""
    B = loc.shape[0]
    return ops.ppo_fwd_bwd(loc.detach(), sigma.detach(), batch, value.detach() if value is not None else None,
                           clip_epsilon=m.clip_epsilon, entropy_coef=m.entropy_coef if m.entropy_bonus else 0.0,
                           critic_coef=m.critic_coef, clip_value=float(m.clip_value) if m.clip_value is not None else 0.0,
                           global_batch=B * m.world_size, adv_stats=adv_stats, sums=sums, maxes=maxes, defer_fold=defer_fold,
                           adv_local=adv_local)


def report_dict(o, m):
    """The 14-float report (grl_trpl_report / grl_fold_adam_report / the record reports) as PPO's (actor loss, metrics dict of views):
    the keys ClipPPOLoss.forward sets besides loss_objective and loss_critic."""
    mt = {"ESS": o[4], "loss_objective_value": o[12]}
    if m.entropy_bonus:
        mt.update(entropy=o[10], loss_entropy=o[3])
    return o[0], mt


class ClipPPOLoss2(_LossBase):
    """objectives/ppo.py ClipPPOLoss2 (reference signature).  ``actor_network`` is a GNNGaussianPolicyDiag (or a ProbabilisticActor
    wrapping one), ``critic_network`` a BaseCritic (or a ValueOperator around one).  ``forward(tensordict)`` returns, like TRPLLoss, a
    TensorDict when ``tensordict`` is installed, else a :class:`trpl.LossDict`, with the keys of ClipPPOLoss.forward: loss_objective,
    loss_critic, ESS, and entropy / loss_entropy when ``entropy_bonus``.  As in TRPLLoss, the VALUE of ``loss_objective`` is the
    objective and its GRADIENT is that of the whole actor loss, so train.py's ``actor_loss = loss_objective + loss_entropy`` backward
    gives the reference's gradient.  ``samples_mc_entropy`` and ``gamma`` are accepted and unused (the entropy of the diagonal Gaussian
    is analytic; the advantage comes with the batch); ``separate_losses`` changes nothing here (actor and critic share no parameter).
    With torchrl importable the class is a ``torchrl.objectives.LossModule``."""
    algorithm = "ppo"

    def __init__(self, actor_network=None, critic_network=None, *, clip_epsilon=0.2, entropy_bonus=True, samples_mc_entropy=1,
                 entropy_coef=0.01, critic_coef=1.0, loss_critic_type="smooth_l1", normalize_advantage=True, gamma=None,
                 separate_losses=False, clip_value=None, in_features=None, group=None, critic_in_features=None, **kwargs):
        super().__init__()
        if loss_critic_type != "l2":
            raise NotImplementedError("loss_critic_type: only l2 is built (configs/algorithm/objective/default.yaml passes l2; the "
                                      "reference's default smooth_l1 is not)")
        actor_network = _unwrap(actor_network, "forward_diag")
        critic_network = _unwrap(critic_network, "_network1")
        self.actor_network, self.critic_network = actor_network, critic_network
        dev = next((p.device for p in actor_network.parameters()), torch.device("cpu"))
        self.register_buffer("clip_epsilon", torch.tensor(float(clip_epsilon), dtype=torch.float32, device=dev))
        self.entropy_bonus, self.entropy_coef, self.critic_coef = bool(entropy_bonus), float(entropy_coef), float(critic_coef)
        self.samples_mc_entropy, self.gamma, self.separate_losses = samples_mc_entropy, gamma, separate_losses
        self.normalize_advantage, self.clip_value = normalize_advantage, clip_value
        self.in_features = list(in_features or actor_network.hyper_data.spec.in_features)
        self.critic_in_features = list(critic_in_features or self.in_features)
        self.group = group
        self._global_steps = 0

    @property
    def world_size(self):
        if self.group is None:
            return 1
        import torch.distributed as dist
        return dist.get_world_size(self.group)

    @property
    def out_keys(self):   # torchrl 0.3.1 ClipPPOLoss.out_keys
        keys = ["loss_objective"]
        if self.entropy_bonus:
            keys += ["entropy", "loss_entropy"]
        if self.critic_coef:
            keys.append("loss_critic")
        return keys + ["ESS"]

    def forward(self, tensordict):
        b = _as_batch(tensordict, self.in_features + self.critic_in_features)
        loc, sigma = self.actor_network.forward_diag(*[b[k] for k in self.in_features], train=True)
        value = self.critic_network(*[b[k] for k in self.critic_in_features]) if self.critic_coef else None
        actor, critic, mt = _run_trpl(self, loc, sigma, value, b)
        out = {"loss_objective": actor - mt["loss_entropy"] if self.entropy_bonus else actor}   # value = objective; gradient = d(actor loss)
        if self.entropy_bonus:
            out.update(entropy=mt["entropy"], loss_entropy=mt["loss_entropy"])
        if self.critic_coef:
            out["loss_critic"] = critic
        out["ESS"] = mt["ESS"]
        if _TensorDict is not None:
            td = _TensorDict(out, [])
            td.__dict__["_grl_outputs"] = {"loc": loc, "sigma": sigma, "state_value": value}
            return td
        out.update(loc=loc, sigma=sigma, state_value=value)
        return LossDict(out)
