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
from .trpl import FusedLoss, _as_batch, _run_trpl


class KLPENPPOLoss(FusedLoss):
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
    keeps_report = True   # (after_report reads the step's mean KL from it)

    def __init__(self, actor_network=None, critic_network=None, *, dtarg=0.01, beta=1.0, increment=2, decrement=0.5, samples_mc_kl=1,
                 entropy_bonus=True, samples_mc_entropy=1, entropy_coef=0.01, critic_coef=1.0, loss_critic_type="smooth_l1",
                 normalize_advantage=True, gamma=None, separate_losses=False, in_features=None, group=None, critic_in_features=None,
                 **kwargs):
        if loss_critic_type != "l2":
            raise NotImplementedError("loss_critic_type: only l2 is built (configs/algorithm/objective/kl_ppo.yaml passes l2; the "
                                      "reference's default smooth_l1 is not)")
        if increment < 1.0:
            raise ValueError(f"increment should be >= 1.0 in KLPENPPOLoss, got {increment:4.4f}")
        if decrement > 1.0:
            raise ValueError(f"decrement should be <= 1.0 in KLPENPPOLoss, got {decrement:4.4f}")
        super().__init__(actor_network, critic_network, entropy_bonus=entropy_bonus, entropy_coef=entropy_coef, critic_coef=critic_coef,
                         normalize_advantage=normalize_advantage, in_features=in_features, critic_in_features=critic_in_features,
                         group=group)
        dev = next((p.device for p in self.actor_network.parameters()), torch.device("cpu"))
        self.register_buffer("beta", torch.tensor(float(beta), dtype=torch.float32, device=dev))
        self.dtarg, self.increment, self.decrement = float(dtarg), float(increment), float(decrement)
        self.samples_mc_kl = samples_mc_kl
        self.samples_mc_entropy, self.gamma, self.separate_losses = samples_mc_entropy, gamma, separate_losses

    @property
    def device_scalars(self):
        return {"kl_beta": self.beta}

    @property
    def out_keys(self):   # torchrl 0.3.1 KLPENPPOLoss.forward's keys
        keys = ["loss_objective", "kl"]
        if self.entropy_bonus:
            keys += ["entropy", "loss_entropy"]
        if self.critic_coef:
            keys.append("loss_critic")
        return keys

    def check_batch(self, b):
        if "loc" not in b or ("var" not in b and "covariance_matrix" not in b):
            raise ValueError("KLPENPPOLoss needs the old distribution in the minibatch: keys 'loc' and 'var' (or 'covariance_matrix')")

    def launch(self, loc, sigma, value, batch, adv_stats, *, sums=None, maxes=None, defer_fold=False, adv_local=False, beta=None, eps=None):
        """FusedLoss.launch in the kernel's KL-penalty mode (column 11 = sum of the per-frame KL, trust-region columns zero)."""
        self.check_batch(batch)
        if "var" not in batch:
            batch = dict(batch, var=batch["covariance_matrix"].diagonal(dim1=-2, dim2=-1).contiguous())
        args, kw = self._launch_args(loc, sigma, value, batch, adv_stats, sums, maxes, defer_fold, adv_local)
        return ops.klpen_fwd_bwd(*args, beta=self.beta, **kw)

    def after_report(self, o14):
        """The penalty weight's update from a step's 14-float report, on the current stream (ops.klpen_adapt)."""
        ops.klpen_adapt(o14, self.beta, self.dtarg, self.increment, self.decrement)

    def report_dict(self, o):
        """The keys KLPENPPOLoss.forward sets besides loss_objective and loss_critic.  No ESS: torchrl's class computes none."""
        mt = {"kl": o[5], "loss_objective_value": o[12]}
        if self.entropy_bonus:
            mt.update(entropy=o[10], loss_entropy=o[3])
        return o[0], mt

    def forward(self, tensordict):
        b = _as_batch(tensordict, self.in_features + self.critic_in_features)
        self.check_batch(b)
        loc, sigma, value = self._networks(b)
        o14 = torch.empty(14, device=loc.device, dtype=torch.float32)
        actor, critic, mt = _run_trpl(self, loc, sigma, value, b, out=o14)
        with torch.no_grad():
            self.after_report(o14)   # (behind the report: the launch above has read the old beta)
        return self._loss_output(self._ppo_out(actor, critic, mt, first=("kl",)), loc, sigma, value)
