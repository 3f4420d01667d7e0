"""Adaptive KL-penalty PPO objective on the fused HIP kernel -- the loss of ``algorithm=kl_ppo`` (examples/torchrl/builders/agent.py:65-78
with configs/algorithm/objective/kl_ppo.yaml), i.e. torchrl's ``KLPENPPOLoss``.

torchrl is not a dependency of this package, so ``KLPENPPOLoss.forward`` of torchrl 0.3.1 is restated here (UNPINNED: no fixture from the
reference checks it; tests/klpen_ref.py is the float64 restatement the kernel is tested against).  On the diagonal Gaussian policy, with
S = sigma^2 the new variance and (mo, So) the minibatch's stored ``loc`` / ``var``:

    adv  = (adv - mean) / std.clamp_min(1e-6)                      (normalize_advantage, numel > 1; unbiased std)
    lw   = log N(action; loc, diag(S)) - sample_log_prob
    kl_f = KL(N(mo, diag(So)) || N(loc, diag(S)))                  OLD || NEW, analytic:
           1/2 sum_i [So_i / S_i + (loc_i - mo_i)^2 / S_i - 1 + log S_i - log So_i]
    loss_objective = mean(-exp(lw) adv + beta kl_f)                (no clipping of the ratio);  kl = mean(kl_f), detached
    entropy = mean(MVN entropy);  loss_entropy = -entropy_coef * entropy  (entropy_bonus)
    loss_critic = critic_coef * mean((V - R)^2)                    (plain l2: torchrl 0.3.1's PPOLoss.loss_critic clips nothing)
    then:  kl > 1.5 dtarg -> beta *= increment;  kl < dtarg / 1.5 -> beta *= decrement;  else unchanged

Everything but the last line comes out of ONE launch of ``grl_klpen_fwd_bwd`` (the fused loss kernel in its KL-penalty mode); the last line
is one single-thread launch behind the step's report (``grl_klpen_adapt``).  ``beta`` is a registered float32 buffer on the policy's
device: the loss launch reads it from device memory, the adapt launch rewrites it there, so a recorded step -- and each of the steps
inside one ``run_minibatches`` launch -- sees the value the step before it left, with nothing recorded again and nothing read back.

A step's value AND gradient use the beta in force when the step starts.  torchrl writes ``self.beta.data *= ...`` before ``backward()``,
so its autograd graph probably differentiates the KL term with the NEW beta; that could not be verified without torchrl and is not
reproduced (it would put a global reduction between the forward and the backward of the loss launch): a known, unverified difference
(DESIGN.md finding 73)."""
import torch

from . import ops
from .trpl import LossDict, _as_batch, _LossBase, _run_trpl, _TensorDict, _unwrap


def klpen_launch(m, loc, sigma, value, batch, adv_stats, sums=None, maxes=None, defer_fold=False, adv_local=False):
    """The KL-penalty counterpart of trpl.trpl_launch (which dispatches here): one launch of the fused kernel on detached inputs ->
    (sums, maxes, dloc, dsigma, dvalue); the slots and sums have the TRPL layout (column 11 = sum of the per-frame KL, trust-region
    columns zero)."""
    B = loc.shape[0]
    if "loc" not in batch or ("var" not in batch and "covariance_matrix" not in batch):
        raise ValueError("KLPENPPOLoss needs the old distribution in the minibatch: keys 'loc' and 'var' (or 'covariance_matrix')")
    if "var" not in batch:
        batch = dict(batch, var=batch["covariance_matrix"].diagonal(dim1=-2, dim2=-1).contiguous())
    return ops.klpen_fwd_bwd(loc.detach(), sigma.detach(), batch, value.detach() if value is not None else None, beta=m.beta,
                             entropy_coef=m.entropy_coef if m.entropy_bonus else 0.0, critic_coef=m.critic_coef, clip_value=0.0,
                             global_batch=B * m.world_size, adv_stats=adv_stats, sums=sums, maxes=maxes, defer_fold=defer_fold,
                             adv_local=adv_local)


def klpen_adapt(m, out14):
    """The penalty weight's update from a step's 14-float report, on the current stream (ops.klpen_adapt)."""
    ops.klpen_adapt(out14, m.beta, m.dtarg, m.increment, m.decrement)


def report_dict(o, m):
    """The 14-float report (grl_trpl_report / grl_fold_adam_report / the record reports) as (actor loss, metrics dict of views): the keys
    KLPENPPOLoss.forward sets besides loss_objective and loss_critic.  No ESS: torchrl's class computes none."""
    mt = {"kl": o[5], "loss_objective_value": o[12]}
    if m.entropy_bonus:
        mt.update(entropy=o[10], loss_entropy=o[3])
    return o[0], mt


class KLPENPPOLoss(_LossBase):
    """torchrl 0.3.1 ``KLPENPPOLoss`` (signature of the reference builder's call).  ``actor_network`` is a GNNGaussianPolicyDiag (or a
    ProbabilisticActor wrapping one), ``critic_network`` a BaseCritic (or a ValueOperator around one).  ``forward(tensordict)`` runs the
    loss launch, the report and the beta update ONCE, like torchrl's forward, and returns a TensorDict when ``tensordict`` is installed,
    else a :class:`trpl.LossDict`, with loss_objective, kl, loss_critic, and entropy / loss_entropy when ``entropy_bonus``.  As in
    ClipPPOLoss2, the VALUE of ``loss_objective`` is the objective and its GRADIENT that of the whole actor loss, so train.py's
    ``actor_loss = loss_objective + loss_entropy`` backward gives the restated gradient.  ``samples_mc_kl`` is accepted and unused (the
    KL of two diagonal Gaussians is analytic), as are ``samples_mc_entropy`` and ``gamma``; ``separate_losses`` changes nothing here.
    ``beta`` is a float32 buffer (it travels in ``state_dict``); write it in place (``loss.beta.fill_(x)``) to set it.  With torchrl
    importable the class is a ``torchrl.objectives.LossModule``."""
    algorithm = "kl_ppo"
    clip_value = None   # (torchrl 0.3.1's PPOLoss.loss_critic has no value clipping)

    def __init__(self, actor_network=None, critic_network=None, *, dtarg=0.01, beta=1.0, increment=2, decrement=0.5, samples_mc_kl=1,
                 entropy_bonus=True, samples_mc_entropy=1, entropy_coef=0.01, critic_coef=1.0, loss_critic_type="smooth_l1",
                 normalize_advantage=True, gamma=None, separate_losses=False, in_features=None, group=None, critic_in_features=None,
                 **kwargs):
        super().__init__()
        if loss_critic_type != "l2":
            raise NotImplementedError("loss_critic_type: only l2 is built (configs/algorithm/objective/kl_ppo.yaml passes l2; the "
                                      "reference's default smooth_l1 is not)")
        if increment < 1.0:
            raise ValueError(f"increment should be >= 1.0 in KLPENPPOLoss, got {increment:4.4f}")
        if decrement > 1.0:
            raise ValueError(f"decrement should be <= 1.0 in KLPENPPOLoss, got {decrement:4.4f}")
        actor_network = _unwrap(actor_network, "forward_diag")
        critic_network = _unwrap(critic_network, "_network1")
        self.actor_network, self.critic_network = actor_network, critic_network
        dev = next((p.device for p in actor_network.parameters()), torch.device("cpu"))
        self.register_buffer("beta", torch.tensor(float(beta), dtype=torch.float32, device=dev))
        self.dtarg, self.increment, self.decrement = float(dtarg), float(increment), float(decrement)
        self.samples_mc_kl = samples_mc_kl
        self.entropy_bonus, self.entropy_coef, self.critic_coef = bool(entropy_bonus), float(entropy_coef), float(critic_coef)
        self.samples_mc_entropy, self.gamma, self.separate_losses = samples_mc_entropy, gamma, separate_losses
        self.normalize_advantage = normalize_advantage
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
    def out_keys(self):   # torchrl 0.3.1 KLPENPPOLoss.forward's keys
        keys = ["loss_objective", "kl"]
        if self.entropy_bonus:
            keys += ["entropy", "loss_entropy"]
        if self.critic_coef:
            keys.append("loss_critic")
        return keys

    def forward(self, tensordict):
        b = _as_batch(tensordict, self.in_features + self.critic_in_features)
        if "loc" not in b or ("var" not in b and "covariance_matrix" not in b):
            raise ValueError("KLPENPPOLoss needs the old distribution in the minibatch: keys 'loc' and 'var' (or 'covariance_matrix')")
        loc, sigma = self.actor_network.forward_diag(*[b[k] for k in self.in_features], train=True)
        value = self.critic_network(*[b[k] for k in self.critic_in_features]) if self.critic_coef else None
        o14 = torch.empty(14, device=loc.device, dtype=torch.float32)
        actor, critic, mt = _run_trpl(self, loc, sigma, value, b, out=o14)
        with torch.no_grad():
            klpen_adapt(self, o14)   # (behind the report: the launch above has read the old beta)
        out = {"loss_objective": actor - mt["loss_entropy"] if self.entropy_bonus else actor, "kl": mt["kl"]}
        if self.entropy_bonus:
            out.update(entropy=mt["entropy"], loss_entropy=mt["loss_entropy"])
        if self.critic_coef:
            out["loss_critic"] = critic
        if _TensorDict is not None:
            td = _TensorDict(out, [])
            td.__dict__["_grl_outputs"] = {"loc": loc, "sigma": sigma, "state_value": value}
            return td
        out.update(loc=loc, sigma=sigma, state_value=value)
        return LossDict(out)
