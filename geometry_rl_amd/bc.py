"""Behaviour cloning: the supervised actor update of ``examples/torchrl/behavior_cloning.py:76-129`` -- the reference's second training
loop, the pre-training half of its "clone, then fine-tune with TRPL" workflow -- on the package's own kernels.

    BCLoss          the objective: the actor's mean against a demonstrated action on the fused loss kernel (its modes 8 / 9);
    BCUpdater       one update = actor forward, loss launch, actor backward, fold, [clip,] Adam on the actor alone, report -- eager or
                    recorded, one program per minibatch size;
    BehaviorCloner  the driver over a recorded rollout: the reference's 80/20 split, its shuffled minibatches, per-epoch mean loss.

What is NOT here is the reference's evaluation (``AgentBuilder.eval_model``, behavior_cloning.py:131-137): it steps the simulator.  The
driver reports the objective on the held-out fifth of the demonstrations instead.  ``BCUpdater`` is a ``flat.FlatUpdater`` like
``PolicyUpdater`` (layout, overwrite rule, Adam, static inputs, checkpoint share: flat.py), ``BehaviorCloner`` draws with
``RolloutDriver``'s sampler (rollout.py); ``BCUpdater.release()`` hands the cloned actor over to a ``PolicyUpdater``."""
from typing import Dict, Optional

import torch

from . import hip, ops
from .flat import FlatUpdater, _job_arrays, cpu
from .program import Entry, record
from .rollout import RolloutBuffer, check_sampling, env_aligned_rows, seeded_generator
from .trpl import LossDict, _as_batch, _InjectGrad, _LossBase, _TensorDict, _unwrap

OBJECTIVES = ("mse", "nll")


class BCLoss(_LossBase):
    """The loss of behavior_cloning.py:101,113-119 as a module: ``loss_fn(td_out["action"], data["action"])`` with ``nn.MSELoss``.

    RESTATED and UNPINNED (torchrl is not a dependency of this package): the reference's ``actor`` is a ProbabilisticActor called in
    train mode outside any ``set_exploration_type``; with torchrl 0.3.1's default interaction type its ``action`` output is the MODE of
    the distribution, i.e. ``loc`` -- the regression target of the mean, the std head takes no part.  That is objective ``"mse"``.

    ``"nll"`` is not in the reference: the negative log-likelihood of the demonstrated action under N(loc, diag(sigma^2)).  After MSE
    cloning the std head has never seen a gradient and sits at ``init_std``, and the trust region of the TRPL fine-tuning that follows is
    measured against that std; the likelihood clones mean and std together.

    ``actor_network``: any actor ``build_agent`` or ``refconfig.build_from_config`` returns (or a ProbabilisticActor around one).
    ``forward(batch)`` takes a mapping / TensorDict with the actor's observation groups and ``action`` and returns ``loss_bc`` (it carries
    the gradient: value and d loss / d (loc, sigma) come from ONE launch of the fused loss kernel), ``mse`` (nn.MSELoss, in either
    objective), ``nll`` (mean over the frames), ``entropy`` (of the policy, mean) and ``max_sq_err`` (the largest per-frame sum of squared
    errors) -- means over the minibatch."""
    algorithm = "bc"
    group = None
    world_size = 1

    def __init__(self, actor_network, objective: str = "mse", in_features=None, group=None):
        if objective not in OBJECTIVES:
            raise ValueError(f"BCLoss(objective=...): 'mse' (the reference's regression) or 'nll', got {objective!r}")
        if group is not None:
            raise NotImplementedError("behaviour cloning runs on one rank: no process group (data parallelism is not built for it)")
        super().__init__()
        self.actor_network = _unwrap(actor_network, "forward_diag")
        self.objective = objective
        self.in_features = list(in_features or self.actor_network.hyper_data.spec.in_features)

    @property
    def out_keys(self):
        return ["loss_bc", "mse", "nll", "entropy", "max_sq_err"]

    def launch(self, loc, sigma, action, *, sums=None, maxes=None, defer_fold=False):
        """One launch of the fused kernel in this objective's mode on detached inputs -> (sums, maxes, dloc, dsigma); ``defer_fold``: see
        ops.trpl_fwd_bwd."""
        return ops.bc_fwd_bwd(loc.detach(), sigma.detach(), action, mode=self.objective, global_batch=loc.shape[0], sums=sums, maxes=maxes,
                              defer_fold=defer_fold)

    @staticmethod
    def report_dict(o14):
        """The 14-float report (grl_trpl_report and its kin; include/grl_hip.h, modes 8 / 9) under this module's keys, as views."""
        return {"loss_bc": o14[0], "mse": o14[1], "nll": o14[5], "entropy": o14[10], "max_sq_err": o14[7]}

    def forward(self, tensordict):
        b = _as_batch(tensordict, self.in_features)
        loc, sigma = self.actor_network.forward_diag(*[b[k] for k in self.in_features], train=True)
        with torch.no_grad():
            sums, maxes, dloc, dsigma = self.launch(loc, sigma, b["action"])
            o14 = torch.empty(14, device=loc.device, dtype=torch.float32)
            hip.call("grl_trpl_loss_values", sums, maxes, 0.0, o14)
        out = self.report_dict(o14)
        out["loss_bc"] = _InjectGrad.apply(out["loss_bc"], 2, loc, sigma, dloc, dsigma)
        extra = {"loc": loc, "sigma": sigma}
        if _TensorDict is not None:
            td = _TensorDict(out, [])
            td.__dict__["_grl_outputs"] = extra
            return td
        return LossDict(out, **extra)


class BCUpdater(FlatUpdater):
    """One behaviour-cloning update of a ``BCLoss``: behavior_cloning.py:96-99,113-123 -- ``torch.optim.Adam(actor.parameters(), lr=5e-4)``
    with torch's defaults (NB ``eps=1e-8``, not the RL loop's 1e-5), zero_grad, backward, step -- on the ACTOR's trainable parameters alone.

    The layout is ``FlatUpdater``'s: parameters, gradients and both moments are flat fp32 buffers, every parameter starts 16-byte aligned,
    and ``p.data`` / ``p.grad`` are views of them.  One step, in order: ``forward_diag(train=True)`` (calibration on the first call, training
    noise as in the RL step; the step count rides on the feature launch), the loss launch with its fold deferred, ``autograd.backward``,
    then the tail -- the queued gradient folds, Adam with the step count in device memory and the report as ONE launch
    (``ops.fold_adam_report``) where the folds overwrite and nothing is clipped; else the fold launch (overwrite under
    ``flat.fold_overwrite``, accumulate into the zeroed buffer otherwise), ``grl_clip_coef``, ``grl_adam_step_dev`` and the report -- and one
    ``grl_stats_accumulate`` that adds the report to running fp64 sums (``stats_reset`` / ``stats_read``: means without a host
    synchronisation per step).  Every launch is an existing entry point; the loss launch is grl_trpl_fwd_bwd in mode 8 / 9.

    ``use_graph=True``: the first step of a minibatch size runs eagerly (topology, calibration, the overwrite check), from the second on
    the step is ONE single-stream hipGraph per size on static inputs, kept per size (a short last minibatch has its own).  ``step_from``
    gathers the rows by one launch (grl_gather_rows_many) straight into the static inputs.  The stock-torch transformer actor runs
    eagerly.  ``release()`` ends the updater: the parameters become ordinary tensors again (values kept), so a
    ``PolicyUpdater`` built afterwards on the same actor lays them out anew and finds the cloned values."""

    def __init__(self, loss: BCLoss, lr=5e-4, eps=1e-8, betas=(0.9, 0.999), clip_grad_norm=False, max_grad_norm=1.0, use_graph=True,
                 group=None):
        if group is not None or getattr(loss, "group", None) is not None:
            raise NotImplementedError("BCUpdater runs on one rank: no process group (data parallelism is not built for behaviour cloning)")
        self.loss_module = loss
        actor = loss.actor_network
        self.eps, self.betas, self.clip, self.max_norm = float(eps), tuple(betas), bool(clip_grad_norm), float(max_grad_norm)
        super().__init__(actor, [[p for p in actor.parameters() if p.requires_grad]], lr, use_graph)
        self.stats = torch.zeros(15, device=self.flat.device, dtype=torch.float64)   # running sums of the 14 report values + the number of updates
        self._programs = {}   # minibatch size -> (program, static inputs, state)
        self._released = False

    def join_lanes(self):
        """Nothing to join: the program has one lane, the caller's stream (PolicyUpdater's method, for tools that time either updater)."""

    def _keys(self):
        return list(dict.fromkeys(list(self.loss_module.in_features) + ["action"]))

    # ---- the running means of the reported values
    def stats_reset(self):
        self.stats.zero_()

    def stats_read(self) -> Dict[str, float]:
        """The fp64 means of the reported values over the updates since ``stats_reset()`` as Python floats, and ``"updates"``, their
        number.  Synchronises ONCE (one small device-to-host copy)."""
        a = self.stats.cpu()
        n = int(a[14])
        out = {"updates": n}
        if n:
            out.update({k: float(v) for k, v in self.loss_module.report_dict(a[:14] / n).items()})
        return out

    # ---- the step's program: one "run" entry on the caller's stream (one hipGraph when recorded) and the host's output dict
    def _tail(self, fold_, o14):
        """Fold + [clip +] Adam + report behind the backward: one launch where that is possible, the separate entry points otherwise."""
        n = self.flat.numel()
        ow = self._fold_overwrite
        report = dict(slots=fold_.slots, batch=fold_.batch, sums=fold_.sums, maxes=fold_.maxes, ent_coef=0.0, out14=o14)
        if not self.clip and ow and ops.fold_adam_report(ow, self._tail_args(0, n, self.lr_dev, self.step_dev), report):
            return
        ops.flush_deferred_grads(overwrite=ow)
        # (behavior_cloning.py clips nothing; the option is PolicyUpdater's, with a workspace of this step's own)
        sq = torch.empty(1, device=self.flat.device, dtype=torch.float64) if self.clip else None
        self._adam(0, n, lr=self.lr_dev, step_dev=self.step_dev, sq=sq)
        hip.call("grl_trpl_report", fold_.slots, fold_.batch, fold_.sums, fold_.maxes, 0.0, o14)

    def _plan(self, batch, st):
        m, actor = self.loss_module, self.loss_module.actor_network
        hd = actor.hyper_data

        def run():
            if not self._fold_overwrite:
                self.gflat.zero_()
            obs = [batch[k] for k in m.in_features]
            zw = torch.empty(13, device=self.flat.device, dtype=torch.float64)   # loss sums (12) | maxes (2 x u32)
            with ops.deferred_folds():   # the leaf-gradient folds of the backward are queued and executed by the tail
                with self._count_rides(hd):
                    loc, sigma = actor.forward_diag(*obs, train=True)
                with torch.no_grad():
                    fold_, _mx, dloc, dsigma = m.launch(loc, sigma, batch["action"], sums=zw[:12], maxes=zw[12:13].view(torch.int32),
                                                        defer_fold=True)
                ops.actor_backward([loc, sigma], [dloc, dsigma])
                with torch.no_grad():
                    o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32)
                    self._tail(fold_, o14)
            hip.call("grl_stats_accumulate", o14, 14, self.stats)
            st.update(o14=o14, loc=loc.detach(), sigma=sigma.detach())

        def finish():   # host only: the output dict of views (recorded once, valid for every replay)
            st["out"] = dict(m.report_dict(st["o14"]), loc=st["loc"], sigma=st["sigma"])

        return [Entry("run", run), Entry("run_host", finish)]

    def _compile(self, batch, B):
        m = self.loss_module
        m.actor_network.hyper_data.check_topology(*[batch[k] for k in m.in_features])   # one sync, before anything is captured
        static = {k: batch[k].clone() for k in self._keys()}
        st = {}
        self._programs[B] = (record(self._plan(static, st)), static, st)

    def _check(self, batch):
        if self._released:
            raise RuntimeError("this BCUpdater was released: its parameters are ordinary tensors again; build a new one")
        missing = [k for k in self._keys() if k not in batch]
        if missing:
            raise KeyError(f"the minibatch lacks {missing}: behaviour cloning reads the actor's observation groups and 'action'")

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """One update on ``batch`` (the actor's observation groups and ``action``, [B, ...]) -> the report: ``loss_bc``, ``mse``, ``nll``,
        ``entropy``, ``max_sq_err`` (device scalars, views of the step's report buffer), ``loc`` and ``sigma``."""
        self._check(batch)
        return self._counted(1, lambda: self._step(batch))

    def _step(self, batch):
        B = int(batch["action"].shape[0])
        if self._eager_first(B):
            st = {}
            self._first_eager(self._plan(batch, st))
            return st["out"]
        if B not in self._programs:
            self._compile(batch, B)
        program, static, st = self._programs[B]
        self._refresh(static, batch, f"the recorded step of {B} frames {{}}")
        self._execute(program)
        return st["out"]

    def step_from(self, buf: RolloutBuffer, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One update on the minibatch made of rows ``idx`` (device int64 [B]) of a device-resident ``RolloutBuffer``.  With a recorded
        step of that size the rows are gathered by ONE launch straight into its static inputs."""
        keys = self._keys()
        B = int(idx.numel())
        if self.use_graph and B in self._programs:
            static = self._programs[B][1]
            jobs = self._gather_jobs(static, buf, keys)
            if jobs is not None:
                hip.call("grl_gather_rows_many", *_job_arrays(jobs), idx, B)
                return self.step(static)
        return self.step(buf.rows(idx, keys))

    def run_minibatches(self, buf: RolloutBuffer, idx_rows) -> Optional[Dict[str, torch.Tensor]]:
        """The updates of consecutive minibatches, ``idx_rows`` [M, B] int64 (or a list of index tensors): the loop of ``step_from``, bit
        for bit (the program has one lane and one graph per step: there is no boundary between two lanes to save).  -> the last report."""
        return self._step_rows(buf, idx_rows)

    @torch.no_grad()
    def evaluate(self, buf: RolloutBuffer, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The objective on rows ``idx`` without an update: no gradient, ``train=False`` (no training noise), nothing written but the
        report -- the same keys as ``step``.  Eager; the cached topology of that size is checked against the rows (one sync)."""
        self._check(buf.data)
        m, actor = self.loss_module, self.loss_module.actor_network
        b = buf.rows(idx, self._keys())
        obs = [b[k] for k in m.in_features]
        was_training = actor.training
        try:
            loc, sigma = actor.forward_diag(*obs, train=False)
        finally:
            actor.train(was_training)
        actor.hyper_data.check_topology(*obs)
        sums, maxes, _, _ = m.launch(loc, sigma, b["action"])
        o14 = torch.empty(14, device=loc.device, dtype=torch.float32)
        hip.call("grl_trpl_loss_values", sums, maxes, 0.0, o14)
        return dict(m.report_dict(o14), loc=loc, sigma=sigma)

    # ---- the whole training state (checkpoint.py), as PolicyUpdater's on the actor alone
    def _saved_hyper(self) -> dict:
        return dict(eps=self.eps, betas=self.betas, clip=self.clip, max_norm=self.max_norm, objective=self.loss_module.objective)

    def state_dict(self) -> dict:
        """Buffers, moments, the ONE step count, the rate, the running sums, the actor's module state (latches, frozen parameters), its
        noise words and position-built topologies: CPU tensors and plain values.  Synchronises once."""
        from . import checkpoint as ck
        if self._released:
            raise RuntimeError("this BCUpdater was released: its buffers no longer hold the actor's parameters")
        actor = self.loss_module.actor_network
        return {"version": ck.VERSION, "layout": ck.layout([("actor.", actor)], self.flat), **self._flat_state(), "hyper": self._saved_hyper(),
                "algorithm": {"loss": type(self.loss_module).__name__, "objective": self.loss_module.objective}, "stats": cpu(self.stats),
                "actor": {k: cpu(v) for k, v in actor.state_dict().items()}, "data": {"actor": ck.data_state(actor.hyper_data)}}

    def load_state_dict(self, sd: dict) -> None:
        """In place (``copy_``; the actor through ``load_state_dict``, which writes through its views of ``flat``); the recorded programs
        stay.  ``steps`` and ``step_dev`` take the one saved count (Adam's bias correction reads the device's).  Raises ValueError before
        anything is written when the layout, the objective, a hyper-parameter or the format version differ."""
        from . import checkpoint as ck
        ck.check_version(sd, "BCUpdater.load_state_dict")
        if self._released:
            raise RuntimeError("this BCUpdater was released: build a new one and load into it")
        actor = self.loss_module.actor_network
        self._check_flat_state(sd, [("actor.", actor)])
        odd = ck.differing(sd["hyper"], self._saved_hyper())
        if odd:
            raise ValueError("the saved run's hyper-parameters differ: " + ", ".join(f"{k} saved {sd['hyper'].get(k)!r}, here "
                             f"{self._saved_hyper().get(k)!r}" for k in odd))
        for bad in (ck.module_mismatch(actor, sd["actor"], "actor"), actor.hyper_data.topology_mismatch(sd["data"]["actor"]["topology"])):
            if bad:
                raise ValueError(bad)
        with torch.no_grad():
            actor.load_state_dict(sd["actor"])
            self._load_flat_state(sd)
            self.stats.copy_(sd["stats"])
            ck.load_data_state(actor.hyper_data, sd["data"]["actor"], self.flat.device)
        self._settle_calibration(actor)

    def release(self):
        """End of the cloning (``FlatUpdater.release``), and the recorded programs are forgotten.  A ``PolicyUpdater`` built afterwards
        on the same actor finds the cloned values."""
        super().release()
        self._programs, self._released = {}, True


class BehaviorCloner:
    """The loop of behavior_cloning.py:76-129 over a recorded rollout ``data`` ([N, T, ...]: the actor's observation groups, as the actor
    consumes them, and ``action``).

    The reference flattens its [N, T] rollout row-major and takes the first 80 % of the rows for training (lines 76-94): a split by
    ENVIRONMENT.  The same here: the first ``int(train_fraction * N)`` environments train, the rest are held out.

    ``sampling="uniform"`` is the reference's ``DataLoader(shuffle=True)``: a fresh permutation of the training rows per epoch, cut into
    minibatches of ``mini_batch_size``, the short last one kept unless ``drop_last``.  It pairs the graph topology cached per batch size
    with rows of other environments, so it is refused for ragged tasks exactly as ``RolloutDriver`` refuses it (``object_num_points`` /
    ``links_num_points`` among the infos) unless ``allow_stale_topology``.  ``"env_aligned"`` (default) is ``RolloutDriver``'s sampler over
    the training environments: per environment a permutation of its T steps, a minibatch = ``mini_batch_size / n_train`` permutation
    columns, so row i of every minibatch belongs to training environment i mod n_train -- what makes rigid tasks and variable-length ropes
    usable.  Every training row is drawn exactly once per epoch in both.

    ``fit`` reports, per epoch, the mean of the minibatch losses (the reference's ``sum(losses) / len(losses)``) and, every ``eval_every``
    epochs, the objective on the HELD-OUT environments.  DEVIATION: the reference measures reward in the simulator at that point
    (``AgentBuilder.eval_model``, lines 131-137); this package has no simulator, the held-out loss stands in for it."""

    def __init__(self, updater: BCUpdater, spec, data: RolloutBuffer, mini_batch_size: int, train_fraction: float = 0.8,
                 sampling: str = "env_aligned", drop_last: bool = False, seed: int = 0, allow_stale_topology: bool = False):
        check_sampling(spec, sampling, allow_stale_topology)
        self.updater, self.spec, self.data = updater, spec, data
        self.N, self.T = data.N, data.T
        self.n_train = int(train_fraction * self.N)   # behavior_cloning.py:81 on the row-major [N, T] rollout
        if not 0 < self.n_train <= self.N:
            raise ValueError(f"train_fraction={train_fraction} of {self.N} environments leaves {self.n_train} to train on")
        self.mini_batch_size = int(mini_batch_size)
        if self.mini_batch_size < 1:
            raise ValueError(f"mini_batch_size={mini_batch_size}")
        if sampling == "env_aligned" and self.mini_batch_size % self.n_train:
            raise ValueError(f"env-aligned sampling needs mini_batch_size ({self.mini_batch_size}) to be a multiple of the number of "
                             f"training environments ({self.n_train} of {self.N})")
        self.sampling, self.drop_last, self.seed, self.gen = sampling, bool(drop_last), seed, None
        self.epochs_done = 0   # epochs fitted so far, over every ``fit`` call (and a resumed run's: state_dict)
        self.device = next(iter(data.data.values())).device

    def train_rows(self) -> torch.Tensor:
        """The training rows of the flattened [N*T] rollout: the first n_train environments, row-major."""
        return torch.arange(self.n_train * self.T, device=self.device)

    def heldout_rows(self) -> torch.Tensor:
        """The held-out rows, time step after time step: row i belongs to held-out environment i mod (N - n_train)."""
        n_hold = self.N - self.n_train
        env = torch.arange(self.n_train, self.N, device=self.device)
        return (env[None, :] * self.T + torch.arange(self.T, device=self.device)[:, None]).reshape(n_hold * self.T)

    def epoch_minibatches(self):
        """The index tensors (int64, into the flattened rollout) of one epoch's minibatches: every training row exactly once, the short
        last minibatch kept unless ``drop_last``."""
        mbs, n, T = self.mini_batch_size, self.n_train, self.T
        self.gen = seeded_generator(self.gen, self.seed, self.device)
        if self.sampling == "uniform":
            perm = torch.randperm(n * T, device=self.device, generator=self.gen)
            out = [perm[i:i + mbs] for i in range(0, n * T, mbs)]
        else:
            k = mbs // n
            idx = env_aligned_rows(n, T, self.gen, self.device)         # [T, n]
            out = [idx[j:j + k].reshape(-1) for j in range(0, T, k)]   # k columns, column after column
        if self.drop_last and out and out[-1].numel() < mbs:
            out.pop()
        return out

    def _settings(self) -> dict:
        return dict(N=self.N, T=self.T, n_train=self.n_train, mini_batch_size=self.mini_batch_size, sampling=self.sampling,
                    drop_last=self.drop_last)

    def state_dict(self) -> dict:
        """The shuffling generator (or its seed while nothing was drawn), the train / held-out split and the number of epochs fitted."""
        from . import checkpoint as ck
        return {"version": ck.VERSION, "settings": self._settings(), "epochs": int(self.epochs_done),
                "generator": ck.generator_state(self.gen, self.seed)}

    def load_state_dict(self, sd: dict) -> None:
        from . import checkpoint as ck
        ck.check_version(sd, "BehaviorCloner.load_state_dict")
        odd = ck.differing(sd["settings"], self._settings())
        if odd:
            raise ValueError(f"the saved cloner's data or split differ at {odd}: saved {sd['settings']}, here {self._settings()}")
        self.gen, self.seed = ck.restore_generator(sd["generator"], self.device)
        self.epochs_done = int(sd["epochs"])

    def evaluate(self) -> Dict[str, float]:
        """The report on the held-out environments as Python floats (synchronises); {} when nothing is held out."""
        if self.n_train == self.N:
            return {}
        out = self.updater.evaluate(self.data, self.heldout_rows())
        return {k: float(out[k]) for k in self.updater.loss_module.out_keys}

    def fit(self, epochs: int, eval_every: int = 10) -> Dict[str, object]:
        """``epochs`` passes over the training rows -> {"loss": [per-epoch mean of the minibatch losses], "train": [per-epoch means of the
        whole report], "eval": {epoch: held-out report}}.  The means come from the updater's fp64 running sums in device memory: ONE host
        synchronisation per epoch, none per step.  The held-out report follows the reference's schedule (``epoch > 0 and epoch %
        eval_every == 0``, line 131; 0 = never) -- there it is the simulator's reward, here the objective on the held-out rows."""
        upd = self.updater
        hist = {"loss": [], "train": [], "eval": {}}
        for epoch in range(int(epochs)):
            upd.stats_reset()
            upd.run_minibatches(self.data, self.epoch_minibatches())
            means = upd.stats_read()   # (the epoch's synchronisation)
            hist["loss"].append(means.get("loss_bc"))
            hist["train"].append(means)
            self.epochs_done += 1
            if eval_every and epoch > 0 and epoch % eval_every == 0:
                hist["eval"][epoch] = self.evaluate()
        return hist
