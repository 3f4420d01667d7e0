"""Float64-capable autograd restatement of the adaptive KL-penalty PPO objective (TEST INFRASTRUCTURE ONLY).

``algorithm=kl_ppo`` of the reference (examples/torchrl/builders/agent.py:65-78, configs/algorithm/objective/kl_ppo.yaml) is torchrl's
``KLPENPPOLoss``.  torchrl 0.3.1 ``torchrl/objectives/ppo.py`` ``KLPENPPOLoss.forward``:

    advantage = (advantage - advantage.mean()) / advantage.std().clamp_min(1e-6)      (normalize_advantage and numel > 1)
    log_weight, dist = self._log_weight(tensordict)                                  (log_prob(action) - sample_log_prob)
    neg_loss = log_weight.exp() * advantage
    previous_dist = self.actor.build_dist_from_params(tensordict)                    (the minibatch's stored loc / covariance)
    current_dist = self.actor.get_dist(tensordict_copy)
    kl = torch.distributions.kl.kl_divergence(previous_dist, current_dist)           OLD || NEW
    neg_loss = neg_loss - self.beta * kl
    if kl.mean() > self.dtarg * 1.5: self.beta.data *= self.increment
    elif kl.mean() < self.dtarg / 1.5: self.beta.data *= self.decrement
    td_out = {"loss_objective": -neg_loss.mean(), "kl": kl.detach().mean()}
    entropy = dist.entropy();  td_out["entropy"] = entropy.mean().detach();  loss_entropy = -entropy_coef * entropy.mean()
    loss_critic = self.loss_critic(tensordict).mean()                                 (PPOLoss.loss_critic: distance_loss, NO clipping)

torchrl is not installed where this project is built or tested, so the lines above are a RESTATEMENT, UNPINNED: no fixture produced by
the reference checks them.  One point is deliberately NOT restated: torchrl multiplies ``self.beta.data`` before ``backward()``, so its
autograd graph probably uses the new beta for the KL term's gradient; here value and gradient use the beta the step started with (the
package's documented, unverified difference).  Everything else is built from the pinned oracle pieces."""
from typing import Dict

import torch

from oracle import step as ost
from oracle import trpl as otr


def kl_old_new(old_loc, old_var, loc, var):
    """KL(N(old_loc, diag(old_var)) || N(loc, diag(var))) per frame, from the pinned putils.py:34-67 restatement (oracle.trpl.gaussian_kl
    takes "std" matrices: the square roots of the variances)."""
    mean_part, cov_part = otr.gaussian_kl((old_loc, old_var.sqrt()), (loc, var.sqrt()))
    return mean_part + cov_part


def klpen_loss(loc, var, batch: Dict[str, torch.Tensor], state_value, beta, *, entropy_coef, critic_coef, normalize_advantage=True,
               entropy_bonus=True, adv_stats=None) -> Dict[str, torch.Tensor]:
    """loc [B,A], var [B,A] (covariance diagonal of the CURRENT policy); ``batch`` holds action, loc, var (old), sample_log_prob,
    advantage, value_target.  ``beta``: a float, or a 0-d tensor WITH requires_grad to see the gradient's dependence on it."""
    adv = batch["advantage"].reshape(-1)
    if normalize_advantage and adv.numel() > 1:
        if adv_stats is None:
            a_loc, a_scale = adv.mean(), adv.std().clamp_min(1e-6)
        else:
            a_loc, a_scale = adv_stats
        adv = (adv - a_loc) / a_scale
    B = loc.shape[0]
    lw = otr.mvn_diag_log_prob(batch["action"].reshape(B, -1), loc, var) - batch["sample_log_prob"].reshape(-1)
    kl_f = kl_old_new(batch["loc"].reshape(B, -1), batch["var"].reshape(B, -1), loc, var)
    out = {"loss_objective": (-lw.exp() * adv + beta * kl_f).mean(), "kl": kl_f.detach().mean(), "kl_f": kl_f.detach(), "lw": lw.detach()}
    ent = otr.mvn_diag_entropy(var)
    if entropy_bonus:
        out["entropy"] = ent.mean().detach()
        out["loss_entropy"] = -entropy_coef * ent.mean()
    else:
        out["loss_entropy"] = torch.zeros((), dtype=loc.dtype)
    if state_value is not None:
        out["loss_critic"] = (critic_coef * otr.clipped_value_loss(state_value.reshape(-1), None, batch["value_target"].reshape(-1), 0.0)).mean()
    return out


def thresholds(dtarg):
    """(1.5 dtarg, dtarg / 1.5) formed in double and rounded to float32: what a float32 mean is compared with."""
    return (float(torch.tensor(float(dtarg) * 1.5, dtype=torch.float64).float()), float(torch.tensor(float(dtarg) / 1.5, dtype=torch.float64).float()))


def adapt_beta(beta: float, kl_mean, dtarg: float, inc: float, dec: float) -> float:
    """The new beta: x inc where the float32 mean KL exceeds 1.5 dtarg, x dec where it is below dtarg / 1.5 (both strict)."""
    hi, lo = thresholds(dtarg)
    kl = float(torch.as_tensor(kl_mean).float())
    b = torch.tensor(float(beta), dtype=torch.float32)
    if kl > hi:
        b = b * torch.tensor(float(inc), dtype=torch.float32)
    elif kl < lo:
        b = b * torch.tensor(float(dec), dtype=torch.float32)
    return float(b)


class KLPenOracleAgent(ost.OracleAgent):
    """oracle.step.OracleAgent with the KL-penalty loss and update (train.py:279-316 with algorithm=kl_ppo: actor_loss = loss_objective +
    loss_entropy); ``beta`` is carried across ``update()`` calls, ``betas`` / ``kls`` record the value each update started with and the
    mean KL it reported."""

    dtarg, beta, increment, decrement = 0.01, 1.0, 2.0, 0.5
    entropy_bonus = True

    def loss(self, batch: Dict[str, torch.Tensor], adv_stats=None, stats_fn=None):
        c = self.cfg
        b = {k: (v.to(self.dtype) if v.is_floating_point() else v) for k, v in batch.items()}
        obs = {k: b[k] for k in self.spec.in_features}
        loc, var = self.actor_forward(obs)
        value = self.critic_forward(obs, stats_fn)
        out = klpen_loss(loc, var, b, value, self.beta, entropy_coef=c.entropy_coef, critic_coef=c.critic_coef,
                         entropy_bonus=self.entropy_bonus, adv_stats=adv_stats)
        out["loc"], out["var"], out["state_value"] = loc, var, value
        return out

    def update(self, batch):
        out = self.loss(batch)
        out["beta"] = self.beta                    # the value this step's loss AND gradient used
        self.beta = adapt_beta(self.beta, out["kl"], self.dtarg, self.increment, self.decrement)
        out["beta_next"] = self.beta
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
