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
or replay of a recorded step, with nothing recorded again.  ``anneal_clip_epsilon=True`` makes that schedule the updater's: a
``PolicyUpdater`` that knows its total number of updates gives EVERY update -- also each of the steps inside one ``run_minibatches``
launch -- its own ``base_clip_epsilon * (1 - n / total)`` from a device table it fills in front of the program, and leaves the last one
in ``clip_epsilon``.  Without it the buffer is the caller's, and constant within a launch of several steps."""
import torch

from . import ops
from .trpl import FusedLoss, _as_batch, _LossBase, _run_trpl   # (_LossBase: torchrl's LossModule when importable)


class ClipPPOLoss2(FusedLoss):
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
                 separate_losses=False, clip_value=None, in_features=None, group=None, critic_in_features=None,
                 anneal_clip_epsilon=False, **kwargs):
        if loss_critic_type != "l2":
            raise NotImplementedError("loss_critic_type: only l2 is built (configs/algorithm/objective/default.yaml passes l2; the "
                                      "reference's default smooth_l1 is not)")
        super().__init__(actor_network, critic_network, entropy_bonus=entropy_bonus, entropy_coef=entropy_coef, critic_coef=critic_coef,
                         normalize_advantage=normalize_advantage, in_features=in_features, critic_in_features=critic_in_features,
                         group=group)
        dev = next((p.device for p in self.actor_network.parameters()), torch.device("cpu"))
        self.register_buffer("clip_epsilon", torch.tensor(float(clip_epsilon), dtype=torch.float32, device=dev))
        self.samples_mc_entropy, self.gamma, self.separate_losses, self.clip_value = samples_mc_entropy, gamma, separate_losses, clip_value
        # train.py:272-274: clip_epsilon = base * (1 - n / total) before every update -- applied by PolicyUpdater, which counts the updates
        self.anneal_clip_epsilon, self.base_clip_epsilon = bool(anneal_clip_epsilon), float(clip_epsilon)

    @property
    def device_scalars(self):
        return {"clip_epsilon": self.clip_epsilon}

    @property
    def out_keys(self):   # torchrl 0.3.1 ClipPPOLoss.out_keys
        keys = ["loss_objective"]
        if self.entropy_bonus:
            keys += ["entropy", "loss_entropy"]
        if self.critic_coef:
            keys.append("loss_critic")
        return keys + ["ESS"]

    def launch(self, loc, sigma, value, batch, adv_stats, *, sums=None, maxes=None, defer_fold=False, adv_local=False, beta=None, eps=None):
        """FusedLoss.launch in the kernel's PPO mode (no projection: the trust-region / KL columns are zero).  ``eps``: the device
        float32[1] this launch reads its clip epsilon from (an annealing updater's entry for the step; default: ``clip_epsilon``)."""
        args, kw = self._launch_args(loc, sigma, value, batch, adv_stats, sums, maxes, defer_fold, adv_local)
        return ops.ppo_fwd_bwd(*args, clip_epsilon=eps if eps is not None else self.clip_epsilon, **kw)

    def report_dict(self, o):
        """The keys ClipPPOLoss.forward sets besides loss_objective and loss_critic."""
        mt = {"ESS": o[4], "loss_objective_value": o[12]}
        if self.entropy_bonus:
            mt.update(entropy=o[10], loss_entropy=o[3])
        return o[0], mt

    def forward(self, tensordict):
        b = _as_batch(tensordict, self.in_features + self.critic_in_features)
        loc, sigma, value = self._networks(b)
        actor, critic, mt = _run_trpl(self, loc, sigma, value, b)
        return self._loss_output(self._ppo_out(actor, critic, mt, last=("ESS",)), loc, sigma, value)
