"""Float64-capable autograd restatement of the clipped PPO objective (TEST INFRASTRUCTURE ONLY).

``ClipPPOLoss2`` (reference objectives/ppo.py) subclasses torchrl 0.3.1's ``ClipPPOLoss`` and overrides only ``loss_critic`` (the clipped
value loss, objectives/utils.py:_clip_value_loss -- the TRPL one, oracle.trpl.clipped_value_loss).  Its objective is torchrl 0.3.1
``torchrl/objectives/ppo.py``: ``ClipPPOLoss._clip_bounds`` = (log1p(-clip_epsilon), log1p(clip_epsilon)) and ``ClipPPOLoss.forward``:

    advantage = (advantage - advantage.mean()) / advantage.std().clamp_min(1e-6)      (normalize_advantage and numel > 1)
    log_weight, dist = self._log_weight(tensordict)                                  (log_prob(action) - sample_log_prob)
    ess = (2 * lw.logsumexp(0) - (2 * lw).logsumexp(0)).exp();  ESS = ess.mean() / batch
    gain1 = log_weight.exp() * advantage
    gain2 = log_weight.clamp(*self._clip_bounds).exp() * advantage
    gain = torch.stack([gain1, gain2], -1).min(dim=-1)[0];  loss_objective = -gain.mean()
    entropy = dist.entropy();  td_out["entropy"] = entropy.mean().detach();  loss_entropy = -entropy_coef * entropy.mean()
    loss_critic = self.loss_critic(tensordict).mean()

torchrl is not installed where this project is built or tested, so the lines above are a RESTATEMENT, UNPINNED: no fixture produced by
the reference checks them (as for GAE and VecNorm).  Everything else is built from the pinned oracle pieces."""
from typing import Dict

import torch

from oracle import step as ost
from oracle import trpl as otr


def ppo_loss(loc, var, batch: Dict[str, torch.Tensor], state_value, *, clip_epsilon, entropy_coef, critic_coef, clip_value=0.2,
             normalize_advantage=True, entropy_bonus=True, adv_stats=None) -> Dict[str, torch.Tensor]:
    """loc [B,A], var [B,A] (covariance diagonal of the CURRENT policy, no projection); ``batch`` holds action, sample_log_prob,
    advantage, value_target, state_value (old).  ``adv_stats`` = (mean, unbiased std) overrides the in-batch statistics."""
    adv = batch["advantage"].reshape(-1)
    if normalize_advantage and adv.numel() > 1:
        if adv_stats is None:
            a_loc, a_scale = adv.mean(), adv.std().clamp_min(1e-6)
        else:
            a_loc, a_scale = adv_stats
        adv = (adv - a_loc) / a_scale
    lw = otr.mvn_diag_log_prob(batch["action"], loc, var) - batch["sample_log_prob"].reshape(-1)
    with torch.no_grad():
        ess = (2 * lw.logsumexp(0) - (2 * lw).logsumexp(0)).exp() / lw.shape[0]
    eps = torch.as_tensor(clip_epsilon, dtype=lw.dtype)
    lo, hi = torch.log1p(-eps), torch.log1p(eps)
    gain1 = lw.exp() * adv
    gain2 = lw.clamp(lo, hi).exp() * adv
    gain = torch.stack([gain1, gain2], -1).min(dim=-1)[0]
    out = {"loss_objective": -gain.mean(), "ESS": ess, "lw": lw.detach()}
    ent = otr.mvn_diag_entropy(var)
    if entropy_bonus:
        out["entropy"] = ent.mean().detach()
        out["loss_entropy"] = -entropy_coef * ent.mean()
    else:
        out["loss_entropy"] = torch.zeros((), dtype=loc.dtype)
    if state_value is not None:
        out["loss_critic"] = (critic_coef * otr.clipped_value_loss(state_value.reshape(-1), batch["state_value"].reshape(-1),
                                                                   batch["value_target"].reshape(-1), clip_value)).mean()
    return out


class PPOOracleAgent(ost.OracleAgent):
    """oracle.step.OracleAgent with PPO's loss and update (train.py:279-316 with algorithm=ppo: actor_loss = loss_objective +
    loss_entropy, no trust-region term)."""

    clip_epsilon = 0.2
    entropy_bonus = True

    def loss(self, batch: Dict[str, torch.Tensor], adv_stats=None, stats_fn=None):
        c = self.cfg
        b = {k: (v.to(self.dtype) if v.is_floating_point() else v) for k, v in batch.items()}
        obs = {k: b[k] for k in self.spec.in_features}
        loc, var = self.actor_forward(obs)
        value = self.critic_forward(obs, stats_fn)
        out = ppo_loss(loc, var, b, value, clip_epsilon=self.clip_epsilon, entropy_coef=c.entropy_coef, critic_coef=c.critic_coef,
                       clip_value=c.clip_value, entropy_bonus=self.entropy_bonus, adv_stats=adv_stats)
        out["loc"], out["var"], out["state_value"] = loc, var, value
        return out

    def update(self, batch):
        out = self.loss(batch)
        (out["loss_objective"] + out["loss_entropy"]).backward()
        out["loss_critic"].backward()
        grads = {"actor": {k: v.grad.clone() for k, v in self.actor.items() if v.grad is not None},
                 "critic": {k: v.grad.clone() for k, v in self.critic.items() if v.grad is not None}}
        if self.cfg.clip_grad_norm:
            torch.nn.utils.clip_grad_norm_(self._actor_leaves(), self.cfg.max_grad_norm)
            torch.nn.utils.clip_grad_norm_(list(self.critic.values()), self.cfg.max_grad_norm)
        self.actor_optim.step()
        self.critic_optim.step()
        self.actor_optim.zero_grad()
        self.critic_optim.zero_grad()
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, grads
