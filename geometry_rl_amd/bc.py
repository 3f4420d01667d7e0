"""Behaviour cloning: the supervised actor update of ``examples/torchrl/behavior_cloning.py:76-129`` -- the reference's second training
loop, the pre-training half of its "clone, then fine-tune with TRPL" workflow -- on the package's own kernels.

    BCLoss          the objective: the actor's mean against a demonstrated action on the fused loss kernel (its modes 8 / 9);
    BCUpdater       one update = actor forward, loss launch, actor backward, fold, [clip,] Adam on the actor alone, report -- eager or
                    recorded, one program per minibatch size;
    BehaviorCloner  the driver over a recorded rollout: the reference's 80/20 split, its shuffled minibatches, per-epoch mean loss.

What is NOT here is the reference's evaluation (``AgentBuilder.eval_model``, behavior_cloning.py:131-137): it steps the simulator.  The
driver reports the objective on the held-out fifth of the demonstrations instead.  ``PolicyUpdater``, ``RolloutDriver`` and
``build_agent`` are untouched; ``BCUpdater.release()`` hands the cloned actor over to a ``PolicyUpdater``."""
from typing import Dict, Optional

import torch

from . import hip, ops
from .program import Entry, execute, record
from .rollout import RolloutBuffer
from .trpl import LossDict, _as_batch, _InjectGrad, _LossBase, _TensorDict, _unwrap
from .updater import _job_arrays

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


def fold_overwrite(actor) -> bool:
    """PolicyUpdater's rule for writing (not accumulating) the leaf gradients with the one fold launch: every leaf gradient of the pass
    comes through the fold queue -- not with a post_fc (transformer) actor, whose unused parameters no fold ever writes, nor with an
    attention gate that runs as torch modules (torch's AccumulateGrad adds into .grad)."""
    gnn = getattr(actor, "gnn", None)
    return (not getattr(actor, "post_fc", False)
            and not any(getattr(mod, "attention", False) and getattr(mod, "gate_kernels", "torch") == "torch"
                        for mod in (gnn.modules() if gnn is not None else [])))


class BCUpdater:
    """One behaviour-cloning update of a ``BCLoss``: behavior_cloning.py:96-99,113-123 -- ``torch.optim.Adam(actor.parameters(), lr=5e-4)``
    with torch's defaults (NB ``eps=1e-8``, not the RL loop's 1e-5), zero_grad, backward, step -- on the ACTOR's trainable parameters alone.

    Layout as PolicyUpdater's: parameters, gradients and both moments are flat fp32 buffers, every parameter starts 16-byte aligned, and
    ``p.data`` / ``p.grad`` are views of them.  One step, in order: ``forward_diag(train=True)`` (calibration on the first call, training
    noise as in the RL step; the step count rides on the feature launch), the loss launch with its fold deferred, ``autograd.backward``,
    then the tail -- the queued gradient folds, Adam with the step count in device memory and the report as ONE launch
    (``ops.fold_adam_report``) where the folds overwrite and nothing is clipped; else the fold launch (overwrite under PolicyUpdater's
    rule, accumulate into the zeroed buffer otherwise), ``grl_clip_coef``, ``grl_adam_step_dev`` and the report -- and one
    ``grl_stats_accumulate`` that adds the report to running fp64 sums (``stats_reset`` / ``stats_read``: means without a host
    synchronisation per step).  Every launch is an existing entry point; the loss launch is grl_trpl_fwd_bwd in mode 8 / 9.

    ``use_graph=True``: the first step of a minibatch size runs eagerly (topology, calibration, the overwrite check), from the second on
    the step is ONE single-stream hipGraph per size on static inputs, kept per size (a short last minibatch has its own).  ``step_from``
    gathers the rows by one launch (grl_gather_rows_many) straight into the static inputs.  The stock-torch transformer actor runs
    eagerly, as in PolicyUpdater.  ``release()`` ends the updater: the parameters become ordinary tensors again (values kept), so a
    ``PolicyUpdater`` built afterwards on the same actor lays them out anew and finds the cloned values."""

    def __init__(self, loss: BCLoss, lr=5e-4, eps=1e-8, betas=(0.9, 0.999), clip_grad_norm=False, max_grad_norm=1.0, use_graph=True,
                 group=None):
        if group is not None or getattr(loss, "group", None) is not None:
            raise NotImplementedError("BCUpdater runs on one rank: no process group (data parallelism is not built for behaviour cloning)")
        self.loss_module = loss
        actor = loss.actor_network
        self.eps, self.betas, self.clip, self.max_norm = float(eps), tuple(betas), bool(clip_grad_norm), float(max_grad_norm)
        self.params = [p for p in actor.parameters() if p.requires_grad]
        pad4 = lambda k: (k + 3) & ~3   # every parameter starts 16-byte aligned (vector loads in the weight-staging prologues)
        n = sum(pad4(p.numel()) for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        self.gflat = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            p.grad = self.gflat[off:off + k].view_as(p)
            off += pad4(k)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.steps = 0
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32)   # optimizer step, device side (graph replays)
        self.lr_dev = torch.full((1,), float(lr), device=dev, dtype=torch.float32)   # read by the recorded Adam launches
        self._lr = float(lr)
        self.stats = torch.zeros(15, device=dev, dtype=torch.float64)   # running sums of the 14 report values + the number of updates
        self.use_graph = bool(use_graph)
        self.mode = "graph" if use_graph else "eager"
        if use_graph and getattr(actor, "stock_torch_gnn", False):   # torch's own launches are not capture-safe (PolicyUpdater does the same)
            self.use_graph, self.mode = False, "eager (stock-torch transformer actor: not recorded)"
        self._programs, self._eager_sizes = {}, set()   # minibatch size -> (program, static inputs, state)
        self._fold_overwrite = fold_overwrite(actor)
        self._overwrite_checked = not self._fold_overwrite
        self._released = False

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        if float(value) != self._lr:
            self._lr = float(value)
            self.lr_dev.fill_(self._lr)

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
        adam = dict(grads=self.gflat, params=self.flat, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr_dev=self.lr_dev, betas=self.betas,
                    eps=self.eps, step_dev=self.step_dev)
        report = dict(slots=fold_.slots, batch=fold_.batch, sums=fold_.sums, maxes=fold_.maxes, ent_coef=0.0, out14=o14)
        if not self.clip and ow and ops.fold_adam_report(ow, adam, report):
            return
        ops.flush_deferred_grads(overwrite=ow)
        coef = None
        if self.clip:   # behavior_cloning.py clips nothing; the option is PolicyUpdater's (train.py:308-310)
            sq = torch.empty(1, device=self.flat.device, dtype=torch.float64)
            coef = torch.empty(1, device=self.flat.device, dtype=torch.float32)
            hip.call("grl_clip_coef", self.gflat, n, self.max_norm, sq, coef)
        hip.call("grl_adam_step_dev", self.flat, self.gflat, self.exp_avg, self.exp_avg_sq, n, self.lr_dev, *self.betas, self.eps, self.step_dev,
                 coef, 1.0)
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
                hd.bump_next = self.step_dev   # the step count rides on the actor's feature launch
                loc, sigma = actor.forward_diag(*obs, train=True)
                assert hd.bump_next is None, "the actor's feature launch did not take the step count"
                with torch.no_grad():
                    fold_, _mx, dloc, dsigma = m.launch(loc, sigma, batch["action"], sums=zw[:12], maxes=zw[12:13].view(torch.int32),
                                                        defer_fold=True)
                ops.TAIL_PRE = {} if ops.FUSE_TAIL_PRE else None   # (lift and fiber-basis backward share one launch: PolicyUpdater._actor_head)
                try:
                    torch.autograd.backward([loc, sigma], [dloc, dsigma])
                    ops.flush_tail_pre()
                finally:
                    ops.TAIL_PRE = None
                with torch.no_grad():
                    o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32)
                    self._tail(fold_, o14)
            hip.call("grl_stats_accumulate", o14, 14, self.stats)
            st.update(o14=o14, loc=loc.detach(), sigma=sigma.detach())

        def finish():   # host only: the output dict of views (recorded once, valid for every replay)
            st["out"] = dict(m.report_dict(st["o14"]), loc=st["loc"], sigma=st["sigma"])

        return [Entry("run", run), Entry("run_host", finish)]

    @staticmethod
    def _do(e: Entry):
        if e.kind == "graph":
            e.item.replay()
        else:
            e.item()

    def _execute(self, program):
        execute(program, self._do, lambda: None, lambda label: None)

    def _eager(self, batch):
        st, hooks, torch_fed = {}, [], []
        if not self._overwrite_checked:   # overwrite mode: no leaf gradient may arrive through torch's AccumulateGrad (PolicyUpdater._step)
            hooks = [p.register_hook(lambda g, i=i: torch_fed.append(i) if g is not None else None) for i, p in enumerate(self.params)]
        try:
            self._execute(self._plan(batch, st))
        finally:
            for h in hooks:
                h.remove()
        if hooks:
            self._overwrite_checked = True
            if torch_fed:
                raise RuntimeError(f"{len(set(torch_fed))} parameter(s) received their gradient from torch autograd instead of the fold queue "
                                   "while BCUpdater runs in overwrite mode (their .grad is never zeroed): this model must be added to the "
                                   "exceptions of bc.fold_overwrite")
        return st["out"]

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
        B = int(batch["action"].shape[0])
        self.steps += 1
        try:
            if not self.use_graph or B not in self._eager_sizes:   # the first step of a size always runs eagerly
                self._eager_sizes.add(B)
                return self._eager(batch)
            if B not in self._programs:
                self._compile(batch, B)
            program, static, st = self._programs[B]
            jobs = []
            for k, v in static.items():
                src = batch[k]
                if src is v:
                    continue
                if src.shape != v.shape:
                    raise ValueError(f"minibatch tensor '{k}' has shape {tuple(src.shape)}, the recorded step of {B} frames {tuple(v.shape)}")
                if src.dtype != v.dtype or not src.is_contiguous() or src.device != v.device:
                    v.copy_(src)
                else:
                    jobs.append((v.data_ptr(), src.data_ptr(), v.numel() * v.element_size()))
            for i in range(0, len(jobs), 24):
                hip.call("grl_copy_many", *_job_arrays(jobs[i:i + 24]))
            self._execute(program)
            return st["out"]
        except BaseException:
            self.steps -= 1
            raise

    def step_from(self, buf: RolloutBuffer, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One update on the minibatch made of rows ``idx`` (device int64 [B]) of a device-resident ``RolloutBuffer``.  With a recorded
        step of that size the rows are gathered by ONE launch straight into its static inputs."""
        keys = self._keys()
        B = int(idx.numel())
        if self.use_graph and B in self._programs:
            static = self._programs[B][1]
            src = [buf.flat(k) for k in keys]
            if all(static[k].dtype == v.dtype and static[k][0].numel() == v.shape[1] for k, v in zip(keys, src)):
                jobs = [(static[k].data_ptr(), v.data_ptr(), v.shape[1] * v.element_size()) for k, v in zip(keys, src)]
                hip.call("grl_gather_rows_many", *_job_arrays(jobs), idx, B)
                return self.step(static)
        return self.step(buf.rows(idx, keys))

    def run_minibatches(self, buf: RolloutBuffer, idx_rows) -> Optional[Dict[str, torch.Tensor]]:
        """The updates of consecutive minibatches, ``idx_rows`` [M, B] int64 (or a list of index tensors): the loop of ``step_from``, bit
        for bit (the program has one lane and one graph per step: there is no boundary between two lanes to save).  -> the last report."""
        out = None
        for r in idx_rows:
            out = self.step_from(buf, r)
        return out

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
        if self.flat.is_cuda:
            torch.cuda.current_stream().synchronize()
        if int(self.step_dev) != self.steps:
            raise RuntimeError(f"the device-side step count is {int(self.step_dev)}, the host's {self.steps}: an update failed while it was "
                               "issued; this state cannot be resumed bit for bit")
        cpu = lambda t: t.detach().cpu().clone()
        return {"version": ck.VERSION, "layout": ck.layout([("actor.", actor)], self.flat), "flat": cpu(self.flat), "exp_avg": cpu(self.exp_avg),
                "exp_avg_sq": cpu(self.exp_avg_sq), "steps": int(self.steps), "lr": self._lr, "hyper": self._saved_hyper(),
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
        if sd["layout"] != ck.layout([("actor.", actor)], self.flat) or sd["flat"].numel() != self.flat.numel():
            raise ValueError(f"the saved parameter layout is not this updater's ({len(sd['layout'])} parameters, {sd['flat'].numel()} floats "
                             f"against {len(self.params)}, {self.flat.numel()})")
        odd = ck.differing(sd["hyper"], self._saved_hyper())
        if odd:
            raise ValueError("the saved run's hyper-parameters differ: " + ", ".join(f"{k} saved {sd['hyper'].get(k)!r}, here "
                             f"{self._saved_hyper().get(k)!r}" for k in odd))
        for bad in (ck.module_mismatch(actor, sd["actor"], "actor"), actor.hyper_data.topology_mismatch(sd["data"]["actor"]["topology"])):
            if bad:
                raise ValueError(bad)
        with torch.no_grad():
            actor.load_state_dict(sd["actor"])
            self.flat.copy_(sd["flat"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            self.steps = int(sd["steps"])
            self.step_dev.fill_(self.steps)
            self._lr = float(sd["lr"])
            self.lr_dev.fill_(self._lr)
            self.stats.copy_(sd["stats"])
            ck.load_data_state(actor.hyper_data, sd["data"]["actor"], self.flat.device)
        if not ck.settle_calibration(actor):
            self._eager_sizes = set()   # (saved before the first training forward: the next step calibrates, which no capture allows)

    def release(self):
        """End of the cloning: every parameter becomes an ordinary tensor again (its values kept, its ``.grad`` dropped) and the recorded
        programs are forgotten.  A ``PolicyUpdater`` built afterwards on the same actor finds the cloned values."""
        for p in self.params:
            p.data = p.data.clone()
            p.grad = None
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
        if sampling not in ("env_aligned", "uniform"):
            raise ValueError(sampling)
        infos = (getattr(spec, "obs_names", None) or {}).get("infos", ())
        ragged = any(n in infos for n in ("object_num_points", "links_num_points"))
        if sampling == "uniform" and ragged and not allow_stale_topology:
            raise ValueError("uniform sampling pairs the topology cached per batch size with rows of other environments; this task has "
                             "ragged per-sample point counts (object_num_points / links_num_points): pass allow_stale_topology=True to "
                             "reproduce the reference quirk")
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

    def _generator(self):
        if self.gen is None:
            self.gen = torch.Generator(device=self.device)
            self.gen.manual_seed(self.seed)
        return self.gen

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
        if self.sampling == "uniform":
            perm = torch.randperm(n * T, device=self.device, generator=self._generator())
            out = [perm[i:i + mbs] for i in range(0, n * T, mbs)]
        else:
            k = mbs // n
            perm = torch.argsort(torch.rand(n, T, device=self.device, generator=self._generator()), dim=1)   # per environment, of its time steps
            idx = (torch.arange(n, device=self.device)[:, None] * T + perm).t().contiguous()                 # [T, n]
            out = [idx[j:j + k].reshape(-1) for j in range(0, T, k)]                                          # k columns, column after column
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
