"""The policy-update driver that replaces the inner loop of ``examples/torchrl/train.py:258-316``: ``PolicyUpdater`` lays one update out
as a program of ``Entry`` objects and runs it eagerly or recorded into hipGraphs (program.py records and issues programs).  The flat
layout, the overwrite rule of the gradient fold, Adam on a slice, the static inputs and the flat part of a training state are
``flat.FlatUpdater``'s, shared with behaviour cloning (bc.py); the programs, the lanes and the schedules are here."""
import contextlib
import os
from typing import Dict, Optional

import torch

from . import hip, ops
from .flat import FlatUpdater, _job_arrays, cpu
from .program import Entry, capture, execute, record  # noqa: F401  (capture: re-exported, the collector-side actor's name for it)

_CRITIC_GROUPS = {}   # (id of the actor lane's process group, its ranks) -> the critic lane's communicator


def annealed(base: float, n: int, total: int) -> float:
    """train.py:263-274: the linearly annealed value of update ``n`` (the count of updates BEFORE it) out of ``total``,
    ``base * (1 - n / total)`` in float64.  Stored into a float32 tensor it is rounded once, which is what ``lr_dev.fill_(x)`` and
    ``clip_epsilon.copy_(x)`` do with the same Python float."""
    return base * (1.0 - n / float(total))


def total_network_updates(total_frames: int, frames_per_batch: int, ppo_epochs: int, mini_batch_size: int) -> int:
    """train.py:54-59: iterations x epochs x minibatches per epoch, each an integer division."""
    return (total_frames // frames_per_batch) * ppo_epochs * (frames_per_batch // mini_batch_size)


class PolicyUpdater(FlatUpdater):
    """One policy-update step of a TRPLLoss, a ClipPPOLoss2 or a KLPENPPOLoss = loss forward, actor + critic backward, optional clip_grad_norm_ per network, two Adam(lr,
    eps=1e-5) steps (train.py:279-316).  Parameters of both networks live in ONE flat fp32 buffer (gradients likewise), so a
    data-parallel run needs a single RCCL all-reduce of the gradient per step and Adam is a single kernel per optimizer.

    The step is laid out as an explicit program (``_plan``) of device-only segments, each free of host synchronisation, so with
    ``use_graph=True`` they are recorded once into hipGraphs (torch.cuda.CUDAGraph) and replayed -- the ~3 ms of per-step launch
    overhead disappears, which is what strong scaling over 8 GPUs needs (512 frames per GPU are < 1 ms of device time).  One program per
    case (``_plan_one_stream`` / ``_plan_lanes`` / ``_plan_dp``): see the comment above ``_plan``.

    ``loss_module`` is a TRPLLoss, a ClipPPOLoss2 or a KLPENPPOLoss: every program runs each (the fused loss kernel is the launch that
    differs; the KL-penalty loss adds ONE single-thread launch per step, below).
    PPO's ``clip_epsilon`` buffer is read from device memory by that launch, so an in-place write (``loss.clip_epsilon.copy_(eps)``)
    takes effect at the next step or replay without recording again; written by the host like this it is constant within one
    ``run_minibatches`` launch of several steps, like ``lr`` (the per-update schedule below moves both inside a launch).  Replacing the
    buffer by another tensor drops the recorded program (it is recorded again).
    KLPENPPOLoss's ``beta`` buffer is device data in both directions: the loss launch reads it, and every program runs the adapt launch
    (``grl_klpen_adapt``) exactly once per step on the actor's lane, behind whichever tail wrote the step's report and ahead of the next
    step's loss launch -- the next step, also the next of the steps inside one ``run_minibatches`` launch, sees the adapted value with
    nothing read back.  Data parallel it follows the tail behind the collective: every rank adapts on the GLOBAL mean KL, so beta stays
    bitwise equal across the ranks.  An in-place host write (``loss.beta.fill_(x)``) takes effect at the next step or replay.

    ``track_stats=True``: every program ends each lane with one more small launch (``grl_stats_accumulate``) that adds the values the
    update reports to running fp64 sums in device memory -- ``stats_read()`` returns their means over all updates since ``stats_reset()``
    (what train.py:294,320 logs as ``train/<key>``) without a host synchronisation per step; the updates themselves are unchanged.  False
    (default): nothing is allocated and every program is what it is without the argument.

    ``anneal_lr=True`` with ``total_network_updates`` (train.py:54-59; ``total_network_updates()`` of this module), and a
    ``ClipPPOLoss2(anneal_clip_epsilon=True)``: the schedule of train.py:263-276 per UPDATE, inside every program.  Update ``n`` (the count
    of updates before it, what ``_global_steps`` gets) runs with ``annealed(base, n, total)``: ``_schedule_prepare`` writes the values of the
    updates a program is about to run into ``sched_table`` by ONE launch in front of it, and the Adam launches of BOTH lanes and the PPO
    loss launch of step j read entry j where they read ``lr_dev`` / ``clip_epsilon`` otherwise -- no launch inside a step is added or
    changed.  An entry is written once per program and read-only while it runs, so the critic's Adam of step j reads step j's rate
    wherever the actor's lane is; every rank forms the values from the same count, so they are bitwise equal across ranks.  ``lr``
    then returns the rate of the last issued update and SETS the schedule's base rate (data of the next fill: nothing is recorded
    again); ``loss.clip_epsilon`` is left at the last issued update's epsilon by the same launch.  An update with ``n >= total`` raises
    ValueError before anything is enqueued (the reference would run a non-positive rate).  Default False: nothing is allocated, every
    program is what it is without the arguments."""

    SCHED_SLOTS = 32   # steps per program the schedule table has entries for ((lr, epsilon) pairs: one grl_write_floats launch)

    def __init__(self, loss_module, lr=3e-4, eps=1e-5, betas=(0.9, 0.999), clip_grad_norm=False, max_grad_norm=1.0,
                 group=None, use_graph=False, overlap_critic=True, allow_eager_fallback=False, force_dp_plan=False,
                 critic_after_first_conv=True, track_stats=False, anneal_lr=False, total_network_updates=None):
        self.loss_module, self.group = loss_module, group
        self.overlap_critic = overlap_critic   # one rank: False = everything on the caller's stream (_plan_one_stream)
        self.force_dp_plan = force_dp_plan     # a process group of ONE rank runs the data-parallel program (bench.py --dp-plan)
        # one rank, two lanes: the critic's lane starts when the actor's FIRST edge convolution has finished (a launch of the lane waits on a
        # flag that the actor's lane sets to the step count behind that launch: _plan_lanes).  Beside that launch the critic's kernels cost it
        # 60-90 us at 4096 frames (DESIGN.md finding 42); beside the HBM-bound kernels that follow they cost less: -1.6 % on the step (finding
        # 55).  True: the size table of _gate_for; False: never gated; "edge0": always gated.
        if not (isinstance(critic_after_first_conv, bool) or critic_after_first_conv == "edge0"):
            raise ValueError(f"critic_after_first_conv={critic_after_first_conv!r}: True (size table) | False | \"edge0\"")
        self.critic_after_first_conv = critic_after_first_conv
        self.epoch_unroll = 8   # minibatch steps per recorded launch of run_minibatches
        # data parallel: gate the critic's lane behind the actor's first edge convolution from this shard size on (0: never).  One-rank RCCL
        # group, alternating on one box (profiles/r06_ab_dp_gate.txt): -4.1 % at 4096 frames per rank, -2 % at 2048, -1.3 % at 1024, 0 at 512
        self.dp_gate_from_frames = int(os.environ.get("GRL_DP_GATE_FROM", "1024"))
        self.epoch_unroll_max_gated_frames = 64   # run_minibatches: the gated multi-step launch up to this many work-frames ...
        self.epoch_gated_from_frames = 3072       # ... and the gated per-step program from here on
        # which recorded form run_minibatches takes above 64 work-frames is measured once per size (_tune_form); False: the table
        self.autotune_form = True
        self.form_by_size, self.form_times = {}, {}

        self.allow_eager_fallback = allow_eager_fallback   # False: a failed hipGraph capture raises instead of degrading silently
        self._hyper = dict(eps=eps, betas=tuple(betas), clip=clip_grad_norm, max_norm=max_grad_norm)
        if group is not None:
            import torch.distributed as dist
            self.rank, n_ranks = dist.get_rank(group), dist.get_world_size(group)
        else:
            self.rank, n_ranks = 0, 1
        # the flat gradient has room IN FRONT of it for the ranks' loss records ([world][14] (hi, lo) float pairs, grl_trpl_fold_record_pairs):
        # data parallel, ``gbuf[:rec + n_actor]`` is ONE all-reduce -- the records ride on the actor's gradient slice
        nets = (loss_module.actor_network, loss_module.critic_network)
        super().__init__(nets[0], [[p for p in net.parameters() if p.requires_grad] for net in nets], lr, use_graph, record_floats=28 * n_ranks)
        dev = self.flat.device
        self.step_dev_c = torch.zeros(1, device=dev, dtype=torch.int32)  # the same count kept by the critic's lane
        self.lane_flag = torch.zeros(1, device=dev, dtype=torch.int32)   # step count of the last "first edge convolution finished" signal
        # entropy bounds, device side (TRPL with entropy control): one entry per step of a launch.  The fused loss launch of step j of a
        # launch reads entry j; the host fills the entries stream-ordered in front of the launch (_entropy_prepare), so recorded programs
        # replay a moving bound unchanged -- the bound is data, like lr_dev
        self.BETA_SLOTS = 64
        self.beta_table = torch.zeros(self.BETA_SLOTS, device=dev, dtype=torch.float64)
        # the per-update schedule (class docstring): entry j of sched_table = (lr, clip epsilon) of step j of the program about to run.
        # ``_lr`` is then the rate of the last issued update, ``_base_lr`` the rate the schedule starts from
        self.anneals_lr = bool(anneal_lr)
        self.anneals_eps = bool(getattr(loss_module, "anneal_clip_epsilon", False))
        self.total_network_updates = None if total_network_updates is None else int(total_network_updates)
        if (self.anneals_lr or self.anneals_eps) and (self.total_network_updates is None or self.total_network_updates < 1):
            raise ValueError("anneal_lr=True / a loss module with anneal_clip_epsilon=True need total_network_updates >= 1 (train.py:54-59: "
                             f"updater.total_network_updates(...)), got {total_network_updates!r}")
        self._base_lr = float(lr)
        self.sched_table = (torch.zeros(2 * self.SCHED_SLOTS, device=dev, dtype=torch.float32)
                            if (self.anneals_lr or self.anneals_eps) else None)
        # running sums of the reported values (track_stats): the actor lane's 14 report values + the number of updates, the critic lane's
        # loss + its count; each lane adds to its own, so the lanes still share nothing
        self.track_stats = bool(track_stats)
        self.stats_actor = torch.zeros(15, device=dev, dtype=torch.float64) if self.track_stats else None
        self.stats_critic = torch.zeros(2, device=dev, dtype=torch.float64) if self.track_stats else None
        self._stats_one_stream = False   # the running program is _plan_one_stream: its report carries the critic loss
        self._drop_recordings()                    # (nothing is recorded yet: _program, _static, _epoch)
        self._cstream = None                       # the critic lane's stream, made when a program first needs it (_critic_stream)
        self._loss_ptr = self._loss_storage()      # (_check_loss_storage)
        self._calib_synced = False                 # (_check_calibrated)
        gnn = getattr(loss_module.actor_network, "gnn", None)
        if gnn is not None and hasattr(gnn, "ponita"):   # EMPN key / query attention: one rank only (ponita_gcn.check_attention_group)
            from .ponita_gcn import check_attention_group
            check_attention_group(getattr(gnn, "attention", False), group)
        # the critic's lane reduces on a communicator of its own (_plan_dp).  dist.new_group is collective over the WHOLE default group
        # and must be entered by every rank in the same order: ``group`` therefore has to span WORLD (asserted), and a failure propagates
        # -- ranks that disagree on which communicator carries the critic's collectives would deadlock in the first step.
        # GRL_DP_ONE_COMM=1 (the documented fallback, README "switches"): both lanes on ``group``.
        self.group_c = None
        if group is not None and os.environ.get("GRL_DP_ONE_COMM", "0") == "0":
            import torch.distributed as dist
            ranks = dist.get_process_group_ranks(group)
            if len(ranks) != dist.get_world_size():
                raise ValueError("PolicyUpdater(group=...) must span the default process group (dist.new_group for the critic's lane is "
                                 "collective over WORLD); set GRL_DP_ONE_COMM=1 to run both lanes on a sub-group's own communicator")
            # ONE extra communicator per process group, shared by every updater built on it (a communicator per updater was
            # never destroyed -- the data-parallel tests leaked one each)
            key = (id(group), tuple(ranks))
            if key not in _CRITIC_GROUPS:
                _CRITIC_GROUPS[key] = dist.new_group(ranks=ranks)
            self.group_c = _CRITIC_GROUPS[key]
        # GRL_DP_ONESHOT=1: the actor lane's one collective (gradient slice + loss records) as a one-shot all-reduce over hipIpc-mapped peer
        # buffers (geometry_rl_amd/oneshot.py) instead of RCCL.  OFF by default: tested with stand-in ranks on one GPU only
        # (tests/test_gpu_oneshot.py); DESIGN.md section 5 has the switch-on criterion for a real node.
        self._oneshot = None
        if group is not None and n_ranks > 1 and os.environ.get("GRL_DP_ONESHOT", "0") == "1" and self.flat.is_cuda:
            import torch.distributed as dist
            if dist.get_backend(group) == "nccl":
                from . import oneshot
                self._oneshot = oneshot.ipc_rank(group, self.gbuf[:self._rec + self.n_actor])
        if group is not None:
            self.sync_replicas()
        # data parallel: every rank's actor draws its training noise from a stream of its own (the rank folded into the key)
        hd = getattr(loss_module.actor_network, "hyper_data", None)
        if hd is not None and self.rank:
            hd.fold_noise_rank(self.rank)

    # ---- hyper-parameters.  ``lr`` lives in device memory (no re-recording); the others are baked into recorded launches as
    #      scalars, so changing one drops the recorded program (it is re-recorded by the next step)
    def _schedule_takes_lr(self, value: float) -> bool:
        if self.anneals_lr:   # the schedule's base rate: data of the next fill (_schedule_prepare), no recorded launch reads it
            self._base_lr = value
        return self.anneals_lr

    def _set_hyper(self, key, value):
        if self._hyper[key] != value:
            self._hyper[key] = value
            self._drop_recordings()   # recorded launches carry the old scalar

    eps = property(lambda self: self._hyper["eps"], lambda self, v: self._set_hyper("eps", v))
    betas = property(lambda self: self._hyper["betas"], lambda self, v: self._set_hyper("betas", tuple(v)))
    clip = property(lambda self: self._hyper["clip"], lambda self, v: self._set_hyper("clip", bool(v)))
    max_norm = property(lambda self: self._hyper["max_norm"], lambda self, v: self._set_hyper("max_norm", float(v)))

    def _drop_recordings(self):
        """Forget the recorded step (with its static inputs) and the recorded multi-step launch: the next step / launch records again."""
        self._program, self._static, self._epoch = None, None, None

    def _loss_storage(self):
        """Device storage the recorded launches read from (and, KL-penalty PPO's beta, write to) the loss module itself
        (``loss_module.device_scalars``); None where the module has none."""
        return tuple(t.data_ptr() for t in self.loss_module.device_scalars.values()) or None

    def _check_loss_storage(self):
        """A loss buffer REPLACED by another tensor (not written in place) drops the recorded programs: they read the old storage."""
        ptr = self._loss_storage()
        if ptr != self._loss_ptr:
            self._drop_recordings()
        self._loss_ptr = ptr

    def _entropy_prepare(self, batch, n_steps: int = 1):
        """TRPL with entropy control: latch the layer's initial entropy at the first update (from ``batch``; data parallel: the global
        mean, one all-reduce, outside every recorded program) and write the bounds of updates ``steps .. steps + n_steps - 1`` into the
        table's first entries on the current stream.  No synchronisation once the initial entropy is known."""
        from .trpl import entropy_active, latch_initial_entropy
        m = self.loss_module
        if not entropy_active(m):
            return
        if m.projection.initial_entropy is None:
            b = batch
            if b is None or ("var" not in b and "covariance_matrix" not in b):
                raise ValueError("the first update with entropy control needs the old distribution (loc, var) in the minibatch")
            latch_initial_entropy(m, b)
        if n_steps > self.BETA_SLOTS:
            raise ValueError(f"{n_steps} steps per launch with entropy control: the bound table has {self.BETA_SLOTS} entries")
        ops.write_doubles(self.beta_table, m.projection.entropy_bounds(range(self.steps, self.steps + n_steps)))

    def _schedule_check(self, n_steps: int = 1):
        """The per-update schedule ends with update ``total - 1``: refuse the next ``n_steps`` updates on the host where one lies behind it
        (train.py would run it at a rate <= 0) -- before the step count moves and before anything is enqueued."""
        if self.sched_table is not None and self.steps + n_steps > self.total_network_updates:
            raise ValueError(f"update {max(self.steps, self.total_network_updates)} of a schedule over total_network_updates = "
                             f"{self.total_network_updates}: the annealed learning rate / clip epsilon would be <= 0")

    def _schedule_prepare(self, n_steps: int = 1):
        """The per-update schedule: the (lr, clip epsilon) of updates ``steps .. steps + n_steps - 1`` into the table's first entries, and the
        last epsilon into the loss module's own buffer, by ONE launch on the current stream in front of the program (the program before it
        has joined its lanes into this stream, so nothing still reads the entries).  Formed on the host in float64 from the update count alone
        -- every rank writes the same bits -- and rounded once to float32 on the way."""
        if self.sched_table is None:
            return
        if n_steps > self.SCHED_SLOTS:
            raise ValueError(f"{n_steps} steps per launch with a per-update schedule: the table has {self.SCHED_SLOTS} entries")
        m, total, vals = self.loss_module, self.total_network_updates, []
        for n in range(self.steps, self.steps + n_steps):
            vals += [annealed(self._base_lr, n, total) if self.anneals_lr else self._lr,
                     annealed(m.base_clip_epsilon, n, total) if self.anneals_eps else 0.0]
        ops.write_floats(self.sched_table, vals, m.clip_epsilon if self.anneals_eps else None, 2 * n_steps - 1)
        if self.anneals_lr:
            self._lr = vals[-2]

    def _sched_slots(self, j: int) -> dict:
        """What step ``j`` of a program reads instead of ``lr_dev`` / the loss module's ``clip_epsilon``: its entries of the schedule table
        (a step's ``st["lr"]`` / ``st["eps"]``; empty without a schedule)."""
        out = {}
        if self.anneals_lr:
            out["lr"] = self.sched_table[2 * j:2 * j + 1]
        if self.anneals_eps:
            out["eps"] = self.sched_table[2 * j + 1:2 * j + 2]
        return out

    # ---- the means of the reported values over many updates (track_stats=True)
    def _stats_add(self, src, acc):
        """``acc[:n] += src``, ``acc[n] += 1`` on the current stream: the last launch of a lane (no-op without track_stats)."""
        if self.track_stats:
            hip.call("grl_stats_accumulate", src, src.numel(), acc)

    def stats_reset(self):
        """Zero the running sums (on the caller's stream: every program joins the critic's lane at its end)."""
        if not self.track_stats:
            raise RuntimeError("PolicyUpdater(track_stats=True) keeps the running sums; this updater was built without them")
        self.stats_actor.zero_()
        self.stats_critic.zero_()

    def stats_read(self) -> Dict[str, float]:
        """The fp64 means of every reported value over the updates since ``stats_reset()`` as Python floats, under the loss module's own
        key names (``loss_objective``, ``loss_critic``, then the keys of the loss module's ``report_dict``), and ``"updates"``,
        their number.  Joins the critic's lane and synchronises ONCE (two small device-to-host copies)."""
        from .trpl import report_critic
        if not self.track_stats:
            raise RuntimeError("PolicyUpdater(track_stats=True) keeps the running sums; this updater was built without them")
        self.join_lanes()
        a, c = self.stats_actor.cpu(), self.stats_critic.cpu()
        n, n_c = int(a[14]), int(c[1])
        if self._stats_one_stream and n_c == 0:
            n_c = n   # (one stream: the critic loss rides in the actor lane's report)
            critic_sum = report_critic(a)
        else:
            critic_sum = c[0]
        if n != n_c:
            raise RuntimeError(f"the actor's lane counted {n} updates, the critic's {n_c}: the running sums do not belong to one sequence")
        out = {"updates": n}
        if n:
            _, mt = self.loss_module.report_dict(a[:14] / n)
            mt = {k: float(v) for k, v in mt.items()}
            out.update(loss_objective=mt.pop("loss_objective_value"), loss_critic=float(critic_sum / n), **mt)
        return out

    def anneal_lr(self, base_lr: float, iteration: int, total_iterations: int) -> float:
        """train.py:264-271: ``alpha = 1 - i / total; lr = base_lr * alpha`` for both optimisers, written by the host for the updates that
        follow (an updater built with ``anneal_lr=True`` follows the schedule per update by itself: this call is not for it)."""
        if self.anneals_lr:
            raise RuntimeError("PolicyUpdater(anneal_lr=True) anneals the rate per update itself; set ``lr`` to change the schedule's base rate")
        self.lr = annealed(base_lr, iteration, total_iterations)
        return self.lr

    def sync_replicas(self):
        """Data parallel: every replica takes rank 0's parameters AND its ``callibrated`` latches (the data-dependent
        re-initialisation of conv.py:104-105 is rank-local arithmetic on rank-local data; replicas must not each run their own)."""
        if self.group is None:
            return
        import torch.distributed as dist
        src = dist.get_global_rank(self.group, 0) if hasattr(dist, "get_global_rank") else 0
        dist.broadcast(self.flat, src=src, group=self.group)
        actor = self.loss_module.actor_network
        flags = [b for n, b in actor.named_buffers() if n.endswith("callibrated")]
        if flags:
            t = torch.stack([f.to(torch.uint8) for f in flags]).to(self.flat.device)
            dist.broadcast(t, src=src, group=self.group)
            for f, v in zip(flags, t):
                f.fill_(bool(v))
        actor._calib_checked = False   # re-inspect the latches on the next training forward

    # ---- the step's programs: lists of ``Entry``.  There is exactly one program per case:
    #        _plan_one_stream  one rank, everything on the caller's stream (overlap_critic=False: the per-kernel timing leg of bench.py, and
    #                          the form every other program must agree with);
    #        _plan_lanes       one rank (default): two lanes that never meet inside a step, ONE single-stream hipGraph each;
    #        _plan_dp          several ranks (or force_dp_plan): the same two lanes with the collectives between their graph segments.
    def _plan(self, batch: Dict[str, torch.Tensor], st: dict):
        m = self.loss_module
        if not m.critic_coef:
            raise NotImplementedError("PolicyUpdater expects the critic term (critic_coef > 0 in every TRPL config)")
        one_rank = m.world_size == 1 and not (self.group is not None and self.force_dp_plan)
        st.update(self._sched_slots(0))   # (a per-update schedule: one step per program, its first entries)
        if one_rank and not self.overlap_critic:
            return self._plan_one_stream(batch, st)
        if one_rank:
            return self._plan_lanes(batch, st)
        return self._plan_dp(batch, st)

    def _critic_leaves(self):
        vf = self.loss_module.critic_network._network1
        ia, ib = vf.gnn.mlp_inner, vf.gnn.mlp_outer
        return (ia.lins[0].weight, ia.lins[0].bias, ia.norms[0].weight, ia.norms[0].bias, ia.lins[1].weight, ia.lins[1].bias,
                ib.lins[0].weight, ib.lins[0].bias, ib.norms[0].weight, ib.norms[0].bias, ib.lins[1].weight, ib.lins[1].bias,
                vf.final.weight, vf.final.bias)

    def _adam_of(self, st, lo, hi, i_, step_dev=None):
        """``_adam`` over [lo, hi) with the step's own rate (a per-update schedule); i_: 0 actor, 1 critic (the slot of the step's clip workspace)."""
        self._adam(lo, hi, lr=st.get("lr", self.lr_dev), step_dev=self.step_dev if step_dev is None else step_dev, sq=st["zw"][23 + i_:24 + i_])

    def _prep(self, batch, st, zero=None):
        """Inputs of a step: the batch with its variance diagonal, the two networks' observation lists, the fp64 workspace
        ((8 unused) | advantage sums (2) | loss sums (12) | maxes (2 x u32) | clip (2); every slot is WRITTEN by its producer).  ``zero``:
        the slice of the flat gradient THIS lane owns -- zeroed here when the folds accumulate (no overwrite mode)."""
        m = self.loss_module
        if not self._fold_overwrite and zero is not None:
            zero.zero_()
        b = dict(batch)
        m.check_batch(b)
        if "var" not in b:
            b["var"] = b["covariance_matrix"].diagonal(dim1=-2, dim2=-1).contiguous()
        st["b"] = b
        st["obs"] = [b[k] for k in m.in_features]
        # (a multi-step launch hands the actor's lane ITS rollout tensors only: where the actor reads other observation groups than the
        # critic -- the transformer actor's normalised vectors -- the critic's list is the critic lane's business, built from its own batch)
        st["cobs"] = [b[k] for k in m.critic_in_features] if all(k in b for k in m.critic_in_features) else None
        st["zw"] = torch.empty(26, device=self.flat.device, dtype=torch.float64)
        st.setdefault("beta", self.beta_table[0:1])   # (entropy control: the bound this step's loss launch reads; _epoch_entries sets entry j)

    def _actor_head(self, st, adv, adv_local):
        """Actor forward + fused loss kernel (actor terms only) + actor backward; -> the loss kernel's fold handle.  The caller has armed the
        fold queue (ops.deferred_folds): the leaf-gradient folds of this backward are queued and executed by one launch at the lane's end."""
        m, actor = self.loss_module, self.loss_module.actor_network
        zw = st["zw"]
        sums, maxes = zw[10:22], zw[22:23].view(torch.int32)
        loc, sigma = actor.forward_diag(*st["obs"], train=True)
        with torch.no_grad():
            fold_, _mx, dloc, dsigma, _ = m.launch(loc, sigma, None, st["b"], adv, sums=sums, maxes=maxes, defer_fold=True,
                                                   adv_local=adv_local, beta=st["beta"], eps=st.get("eps"))
        st.update(loc=loc.detach(), sigma=sigma.detach())
        ops.actor_backward([loc, sigma], [dloc, dsigma])
        return fold_

    @staticmethod
    def _finish(st):
        """Host only: the output dict of views (recorded once, valid for every replay)."""
        a_loss, mt = st.pop("lv_main")
        mt = dict(mt)
        out = {"loss_objective": mt.pop("loss_objective_value"), "loss_critic": st.pop("c_loss"), "loc": st["loc"], "sigma": st["sigma"],
               "state_value": st["value"].unsqueeze(-1)}
        out.update(mt)
        st["out"] = out

    def _plan_one_stream(self, batch, st):
        """One rank, one stream: critic forward, actor forward, the fused loss kernel WITH the value terms, both backward passes, one fold,
        the optimizer step(s), reported values -- four closures on the caller's stream (one hipGraph when recorded)."""
        from .trpl import adv_stats_local, loss_values
        m = self.loss_module
        actor, vf = m.actor_network, m.critic_network._network1
        leaves = self._critic_leaves()
        ow = self._fold_overwrite
        self._stats_one_stream = True

        def s0():  # critic features, first critic stage, advantage statistics
            self._prep(batch, st, zero=self.gflat)
            with torch.no_grad():
                vf.train(True)
                _, x = vf.hyper_data.build_data(*st["cobs"], train=True)
                st["pipe"] = ops.DeepSetsPipeline(x, leaves, 1)
                st["pipe"].fwd1()
                st["adv"] = None
                if m.normalize_advantage and x.shape[0] > 1:
                    st["adv"] = st["zw"][8:10]
                    adv_stats_local(m, st["b"], st["adv"])

        def s1():
            st["pipe"].fwd2()

        def s2():  # value head, actor forward, fused TRPL kernel, actor backward, the critic's backward stages, ONE fold for both networks
            pipe = st["pipe"]
            with ops.deferred_folds():
                value = pipe.fwd3()
                loc, sigma = actor.forward_diag(*st["obs"], train=True)
                with torch.no_grad():
                    zw = st["zw"]
                    sums, maxes, dloc, dsigma, dvalue = m.launch(loc, sigma, value, st["b"], st["adv"], sums=zw[10:22],
                                                                 maxes=zw[22:23].view(torch.int32), beta=st["beta"], eps=st.get("eps"))
                torch.autograd.backward([loc, sigma], [dloc, dsigma])
                with torch.no_grad():
                    pipe.bwd3(dvalue)
                    pipe.bwd2()
                    grads = pipe.bwd1(leaves)
                assert all(g is None for g in grads), "critic parameters must own .grad views of the flat buffer"
                ops.flush_deferred_grads(overwrite=ow)
            st.update(loc=loc.detach(), sigma=sigma.detach(), value=value, sums=sums, maxes=maxes)

        def s3():  # optimizers + reported values (train.py:308-316, trpl.py:280-321)
            with torch.no_grad():
                self.step_dev.add_(1)
                na, n = self.n_actor, self.flat.numel()
                # the two optimizers of train.py:120-127 have identical hyper-parameters and schedules: without per-network gradient
                # clipping their two Adam steps are ONE launch over the flat buffer (element-wise: the same numbers)
                for i_, (lo, hi) in enumerate(((0, na), (na, n)) if self.clip else ((0, n),)):
                    self._adam_of(st, lo, hi, i_)
                o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32) if (self.track_stats or m.keeps_report) else None
                a_loss, c_loss, mt = loss_values(m, st["sums"], st["maxes"], out=o14)
                st["lv_main"], st["c_loss"] = (a_loss, mt), c_loss
                m.after_report(o14)
                self._stats_add(o14, self.stats_actor)   # (one call: the report carries the critic loss)

        return [Entry("run", s0), Entry("run", s1), Entry("run", s2), Entry("run", s3), Entry("run_host", lambda: self._finish(st))]

    def _signal_lane(self):
        """lane_flag[0] = step_dev[0] on the current stream (one tiny launch): the critic's lane may start this step."""
        hip.call("grl_copy_many", *_job_arrays([(self.lane_flag.data_ptr(), self.step_dev.data_ptr(), 4)]))

    @contextlib.contextmanager
    def _actor_lane_head(self, gate: bool):
        """Around the actor lane's forward + backward: the step count rides on the lane's first launch (grl_build_features_bump) and, ``gate``,
        the critic's lane is signalled right behind the actor's first edge convolution -- by the fiber convolution launched behind it, which
        writes the flag when it starts (ops.FiberConv, ops.SIGNAL_IN_KERNEL), or else by a copy launch of its own."""
        hd = self.loss_module.actor_network.hyper_data
        with self._count_rides(hd):
            if gate:
                def signal():
                    if hd.bump_next is not None:   # the step count has not been advanced yet (a calibrating pass in front of the step's own
                        return False               # forward): not this edge convolution
                    if ops.SIGNAL_IN_KERNEL:
                        ops.PENDING_SIGNAL = (self.lane_flag, self.step_dev)
                    else:
                        self._signal_lane()
                    return True
                ops.AFTER_EDGE_HOOK = signal
            try:
                yield
            finally:
                ops.AFTER_EDGE_HOOK = None
                unsent, ops.PENDING_SIGNAL = ops.PENDING_SIGNAL, None
            if unsent is not None:   # (no fiber convolution followed the edge convolution: send the signal by itself)
                self._signal_lane()

    def _critic_wait(self):
        """A gated critic lane's first launch: waits until the actor's lane has signalled THIS step (flag >= the lane's finished steps + 1)."""
        hip.call("grl_wait_flag_ge", self.lane_flag, self.step_dev_c, 1, 200000)

    def _critic_stages(self, cb, st, world):
        """The critic lane's stages as closures (fwd1, fwd2, fwd3, bwd2, bwd1), each free of host synchronisation: between two of them the
        whole-tensor LayerNorm sums are summed over the ranks (_plan_dp places the collectives; one rank runs the stages back to back).
        ``cb``: the batch the lane reads -- straight from it, the lane depends on nothing the actor's lane prepares, so it can be enqueued
        first (a gated lane puts ``_critic_wait`` in front of them).  The caller arms the fold queue around bwd1 (the only stage that emits
        leaf gradients) and appends its tail."""
        from .trpl import value_loss
        m = self.loss_module
        vf = m.critic_network._network1
        leaves = self._critic_leaves()
        na = self.n_actor

        @torch.no_grad()
        def fwd1():
            if not self._fold_overwrite:
                self.gflat[na:].zero_()   # on THIS lane, in front of its folds (never from the actor's lane)
            vf.train(True)
            _, x = vf.hyper_data.build_data(*[cb[k] for k in m.critic_in_features], train=True, bump=self.step_dev_c)   # (+ the lane's step count)
            st["pipe"] = ops.DeepSetsPipeline(x, leaves, world)
            st["pipe"].fwd1()

        @torch.no_grad()
        def fwd2():
            st["pipe"].fwd2()

        @torch.no_grad()
        def fwd3():   # value head, the lane's OWN loss, last stage backward
            st["value"] = st["pipe"].fwd3()
            # (c_loss: this rank's mean, the reported value on one rank; vl: the fp64 (sum, mean over the global batch) _plan_dp all-reduces)
            dvalue, st["c_loss"], st["vl"] = value_loss(m, st["value"], cb)
            st["pipe"].bwd3(dvalue)

        @torch.no_grad()
        def bwd2():
            st["pipe"].bwd2()

        @torch.no_grad()
        def bwd1():
            grads = st["pipe"].bwd1(leaves)
            assert all(g is None for g in grads), "critic parameters must own .grad views of the flat buffer"

        return fwd1, fwd2, fwd3, bwd2, bwd1

    def _plan_lanes(self, batch, st):
        """One rank as a two-lane PROGRAM of single-stream graphs.  This HIP runtime replays a captured graph with two branches through
        the host (hipGraphLaunch returned after 2/3 of the DEVICE time of a forked step; tools/ubench/graph_branches.py) and every
        cross-branch edge costs a 6-11 us gap; a graph boundary on a lane costs ~15 us as well.  So each lane is ONE graph and the lanes
        never meet inside a step (DESIGN.md findings 37, 38):
          actor's lane : features, lift, convolutions, read-out, fused loss kernel (actor terms only; the batch's advantage statistics are
                         summed inside it), backward, then ONE tail launch: fold + Adam over the actor's slice + reported values;
          critic's lane: features, the three forward stages, its OWN loss (clipped value loss: elementwise in the frame), the three
                         backward stages, tail: fold + Adam over the critic's slice.
        Actor and critic share no parameter and no intermediate (train.py:279-316 runs two backward passes and two optimizers); the lanes
        are forked at the step's start and joined at its end.  Each lane zeroes ITS OWN slice of the flat gradient when the folds
        accumulate (attention gate: torch's AccumulateGrad adds into .grad)."""
        # Gate the critic's lane behind the actor's first edge convolution?  It pays where the critic then finishes inside the actor's FORWARD
        # (its kernels cost the one-wave-per-SIMD backward launches far more than the forward ones: gated at the forward's END the step is 6 %
        # slower): measured on rigid HEPi +1.1 % at 4096 frames, +3 % at 512, +1 % at 32, 0 at 2048, -1.5 % at 1024, where a forward of
        # 0.35 ms is too short for it (profiles/r05_ab_critic_gate.txt, r05_ab_critic_gate_points.txt).  True (default) = that table.
        frames = next(int(v.shape[0]) for v in batch.values() if torch.is_tensor(v))
        actor_lane, critic_lane = self._lane_entries(batch, batch, st, self._gate_for(frames))
        return [Entry("fork", None), *actor_lane, *critic_lane, Entry("join", None), Entry("run_host", lambda: self._finish(st))]

    def _lane_entries(self, batch, cbatch, st, gate):
        """The lanes of ``_plan_lanes`` as "run" entries -> (the actor's, reading ``batch``; the critic's, reading ``cbatch``: the gate's wait
        when ``gate``, then the stages with the tail).  The multi-step launch puts each lane's gather in front of the lane's step."""
        from .trpl import report_values
        m = self.loss_module
        ow = self._fold_overwrite
        na, n_all = self.n_actor, self.flat.numel()
        # the one-launch tail needs every leaf gradient of the lane in the fold queue (overwrite mode) and no clipping (which needs the
        # finished gradient norm before Adam)
        fuse_tail = not self.clip and ow
        self._stats_one_stream = False

        def main_all():
            self._prep(batch, st, zero=self.gflat[:na])
            with ops.deferred_folds():   # the leaf-gradient folds of the backward are queued and executed by the tail
                with self._actor_lane_head(gate):
                    fold_ = self._actor_head(st, None, bool(m.normalize_advantage and st["obs"][0].shape[0] > 1))
                with torch.no_grad():
                    done, o14 = False, None
                    if fuse_tail:   # fold + Adam + reported values: ONE launch at the lane's end (ops.fold_adam_report)
                        o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32)
                        ent = m.entropy_coef if m.entropy_bonus else 0.0
                        # (gated: the lane's closing signal -- see below -- rides on this launch)
                        done = ops.fold_adam_report(ow, self._tail_args(0, na, st.get("lr", self.lr_dev), self.step_dev),
                                                    dict(slots=fold_.slots, batch=fold_.batch, sums=fold_.sums, maxes=fold_.maxes,
                                                         ent_coef=ent, out14=o14), signal=(self.lane_flag, self.step_dev) if (gate and ops.SIGNAL_IN_KERNEL) else None)
                        if done:
                            a_loss, mt = m.report_dict(o14)
                    if not done:
                        ops.flush_deferred_grads(overwrite=ow)
                        self._adam_of(st, 0, na, 0)
                        keep = self.track_stats or m.keeps_report   # (the report is read again behind this launch)
                        if keep and o14 is None:
                            o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32)
                        a_loss, _c, mt = report_values(m, fold_.slots, fold_.batch, fold_.sums, fold_.maxes, out=o14 if keep else None)
            if gate and not (done and ops.SIGNAL_IN_KERNEL):   # ... and once more at the lane's end, whatever happened above (an actor without an edge convolution; a
                self._signal_lane()                            # signal that carried a stale count): the critic's lane can be late, it can never be stuck
            m.after_report(o14)                                # (KL-penalty PPO: beta for the NEXT step, from this step's report)
            self._stats_add(o14, self.stats_actor)             # (track_stats: the lane's last launch, whichever tail wrote the report)
            st.update(sums=fold_.sums, maxes=fold_.maxes, lv_main=(a_loss, mt))

        stages = self._critic_stages(cbatch, st, 1)

        def critic_all():
            with ops.deferred_folds(), torch.no_grad():
                for stage in stages:
                    stage()
                if not (fuse_tail and ops.fold_adam_report(ow, self._tail_args(na, n_all, st.get("lr", self.lr_dev), self.step_dev_c))):
                    ops.flush_deferred_grads(overwrite=ow)
                    self._adam_of(st, na, n_all, 1, self.step_dev_c)
                self._stats_add(st["c_loss"], self.stats_critic)

        wait = [Entry("run", self._critic_wait, "s", "critic_gate_wait")] if gate else []
        return [Entry("run", main_all)], [*wait, Entry("run", critic_all, "s")]

    def _plan_dp(self, batch, st):
        """Several ranks: the same two lanes, graph segments between the collectives (which stay eager torch.distributed calls).
          actor's lane : [features ... forward, fused loss kernel (actor terms), backward, fold, this rank's loss record] -> ONE all-reduce:
                         the ACTOR's slice of the flat gradient with the ranks' loss records riding in front of it -> [Adam, reported values];
                         the advantage statistics come from the rollout driver (one all-reduce per EPOCH, ``adv_stats`` column) or, for a
                         bare ``step(batch)``, from one more graph + collective at the head of the lane;
          critic's lane: its four LayerNorm-statistic reductions, its own loss, the all-reduce of ITS slice and of its loss sum, its Adam --
                         on a communicator of its own (``group_c``; collectives of one communicator execute in issue order on one internal
                         stream: a critic reduction waiting for a critic kernel must not hold back the actor's gradient all-reduce issued
                         behind it).  GRL_DP_ONE_COMM=1: both lanes on ``group`` (the documented fallback; same results).
        Every rank enqueues the SAME sequence of collectives per communicator, in the order of this list (host order = enqueue order);
        tests/test_dp_program_order.py checks that property of the program itself."""
        from .trpl import adv_stats_local
        m = self.loss_module
        world = m.world_size
        ow = self._fold_overwrite
        na, n_all = self.n_actor, self.flat.numel()
        S = "s"
        # ``adv_stats`` in the batch ([B, 2] fp64, every row = the GLOBAL (sum, sum of squares) of this minibatch's advantages:
        # rollout.RolloutDriver.publish_advantage_stats): the statistics kernel, its all-reduce and the graph boundary behind it leave
        # the actor's lane -- two graphs and one collective on its path.
        published = m.normalize_advantage and "adv_stats" in batch
        self._stats_one_stream = False

        def p_stats():
            self._prep(batch, st, zero=self.gflat[:na])
            st["adv"] = None
            if published:
                st["adv"] = batch["adv_stats"][0]
            elif m.normalize_advantage and st["obs"][0].shape[0] * world > 1:
                with torch.no_grad():
                    st["adv"] = st["zw"][8:10]
                    adv_stats_local(m, st["b"], st["adv"])

        # Large shards: the critic's lane waits (a launch of its own, grl_wait_flag_ge) until the actor's first edge convolution has finished --
        # beside that launch the critic's kernels cost it 60-170 us at 4096 frames (finding 42; DESIGN round 6).  The wait starts with the step
        # and ends inside the actor's forward: it is never resident during a backward launch.  GRL_DP_GATE_FROM frames (0 = never).
        frames_local = next((int(v.shape[0]) for v in batch.values() if torch.is_tensor(v)), 0)
        gate_dp = bool(self.dp_gate_from_frames) and self._work_frames(frames_local) >= self.dp_gate_from_frames   # (work-normalised, see _work_frames)

        def p_main():
            if published:
                p_stats()
            with ops.deferred_folds():   # the leaf-gradient folds of the backward are queued and executed with the loss record, below
                with self._actor_lane_head(gate_dp):
                    fold_ = self._actor_head(st, st["adv"], False)
                if gate_dp:   # ... and once more at the end of the segment: the critic's lane can be late, never stuck (its wait is bounded as well)
                    self._signal_lane()
                st.update(sums=fold_.sums, maxes=fold_.maxes)
                with torch.no_grad():
                    # this rank's loss sums / maxes as ONE record of float pairs in front of the flat gradient (own row, zeros in the
                    # others): the SUM all-reduce of the actor's slice delivers every rank's record -- no collective of their own.  The
                    # record and the fold of the slabs come from ONE launch (both only feed that all-reduce)
                    if not ops.fold_record_pairs(ow, fold_.slots, fold_.batch, self.rank, world, self.gbuf[:self._rec]):
                        hip.call("grl_trpl_fold_record_pairs", fold_.slots, fold_.batch, self.rank, world, self.gbuf[:self._rec])
                        ops.flush_deferred_grads(overwrite=ow)

        # (the reported values live in ONE buffer per recorded program: the tail may run as an eager launch behind the collective, below)
        o14 = torch.empty(14, device=self.flat.device, dtype=torch.float32)
        st["lv_main"] = m.report_dict(o14)

        def p_tail():   # behind the lane's collective: Adam on the reduced gradient, reported values of the delivered records
            with torch.no_grad():
                ent = m.entropy_coef if m.entropy_bonus else 0.0
                if self.clip:   # (the clip coefficient needs the reduced gradient's norm first: the separate launches)
                    self._adam_of(st, 0, na, 0)
                    hip.call("grl_trpl_report_record_pairs", self.gbuf[:self._rec], world, st["sums"], st["maxes"], ent, o14)
                else:           # Adam on the reduced slice + the reported values of the delivered records: ONE launch
                    hip.call("grl_adam_report_record_pairs", self.flat[:na], self.gflat[:na], self.exp_avg[:na], self.exp_avg_sq[:na], na,
                             st.get("lr", self.lr_dev), *self.betas, self.eps, self.step_dev,
                             self.gbuf[:self._rec], world, st["sums"], st["maxes"], ent, o14)
                m.after_report(o14)                      # (KL-penalty PPO: every rank adapts on the GLOBAL mean KL -- beta stays equal across the ranks)
                self._stats_add(o14, self.stats_actor)   # (the GLOBAL values: every rank adds the same numbers, no collective)

        q_fwd1, q_fwd2, q_fwd3, q_bwd2, bwd1 = self._critic_stages(batch, st, world)
        q_wait = [Entry("run", self._critic_wait, S, "critic_gate_wait")] if gate_dp else []

        def q_bwd1():
            with ops.deferred_folds(), torch.no_grad():   # the critic's slabs are folded here, on its lane, into its slice of the flat gradient
                bwd1()
                ops.flush_deferred_grads(overwrite=ow)

        def q_tail():
            with torch.no_grad():
                self._adam_of(st, na, n_all, 1, self.step_dev_c)
                st["c_loss"] = st["vl"][1].float()   # (the all-reduced sum of the ranks' shares, already divided by B_global)
                self._stats_add(st["c_loss"], self.stats_critic)

        # (host order = enqueue order: the critic's segments are interleaved so that its lane is fed early; each lane's own order is what
        #  the device sees.  p_stats comes first when present: it also prepares the step's inputs for both lanes.)
        head_ = [] if published else [Entry("run", p_stats), Entry("sum", lambda: st["adv"], "m", "advantage_stats")]
        # p_tail without clipping is ONE launch, cheaper issued eagerly than replayed as a one-node graph (a graph launch behind a collective
        # costs ~13 us of lane time, an eager kernel launch ~4; -1.5 % at 512 frames per rank)
        return [Entry("fork", None), *head_,
                *q_wait, Entry("run", q_fwd1, S), Entry("sum", lambda: st["pipe"].stats1, S, "critic_ln1_fwd_stats"),
                Entry("run", q_fwd2, S), Entry("sum", lambda: st["pipe"].stats2, S, "critic_ln2_fwd_stats"),
                Entry("run", p_main),
                Entry("sum", lambda: self.gbuf[:self._rec + na], "m", "flat_gradient_actor+loss_records"),
                Entry("run", q_fwd3, S), Entry("sum", lambda: st["pipe"].bst2, S, "critic_ln2_bwd_stats"),
                Entry("run", q_bwd2, S), Entry("sum", lambda: st["pipe"].bst1, S, "critic_ln1_bwd_stats"),
                Entry("run", p_tail, eager=not self.clip),
                Entry("run", q_bwd1, S), Entry("sum", lambda: self.gflat[na:], S, "flat_gradient_critic"),
                Entry("sum", lambda: st["vl"], S, "loss_critic_sum"),
                Entry("run", q_tail, S),
                Entry("join", None, "m", "join_critic_lane"), Entry("run_host", lambda: self._finish(st))]

    def program_outline(self, published: bool = True):
        """The data-parallel program as data, without running anything: [(kind, lane, label, communicator)] in HOST (enqueue) order, where
        communicator is "group" / "group_c" for collectives and None otherwise.  ``published``: the minibatch carries the epoch's advantage
        statistics (rollout.RolloutDriver.publish_advantage_stats) -- otherwise the lane starts with one more graph and collective.
        Needs no GPU (the closures are built, not called): tests/test_dp_program_order.py checks on four gloo ranks that every rank
        enqueues the same sequence per communicator and that the program has no dependency cycle across communicators -- the property the
        device-side RCCL run of two concurrently driven communicators rests on."""
        out = []
        for e in self._plan_dp({"adv_stats": None} if published else {}, {}):
            comm = None
            if e.kind == "sum":
                comm = "group_c" if (e.lane == "s" and self.group_c is not None) else "group"
            out.append((e.kind, e.lane, e.label, comm))
        return out

    def _critic_stream(self):
        if self._cstream is None:
            # the LOWEST priority the device offers: the critic's small launches take the compute units the actor's kernels leave (heads,
            # tails, the latency-bound loss kernel) instead of displacing their workgroups (DESIGN.md finding 33)
            prio = 0
            if hasattr(torch.cuda.Stream, "priority_range"):
                try:
                    prio = max(torch.cuda.Stream.priority_range())
                except Exception:
                    prio = 0
            self._cstream = torch.cuda.Stream(priority=prio)
        return self._cstream

    # ``collective_log``: None, or {} to record -- per label a list of (start event, end event, payload bytes) on the lane's stream: how long
    # the lane was held by each collective (wait for the other ranks + transfer).  Read with ``collective_summary()``.
    collective_log = None

    def _log_span(self, label, nbytes=0):
        """Context manager: HIP events on the current stream around a collective / cross-lane wait when the log is on."""
        if self.collective_log is None or label is None:
            return contextlib.nullcontext()
        @contextlib.contextmanager
        def span():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            yield
            e1.record()
            self.collective_log.setdefault(label, []).append((e0, e1, nbytes))
        return span()

    def collective_summary(self, n_steps: int):
        """{label: {per_step, mean_ms, max_ms, bytes}} from the recorded events (synchronises)."""
        torch.cuda.synchronize()
        out = {}
        for label, recs in (self.collective_log or {}).items():
            ms = [a.elapsed_time(b) for a, b, _ in recs]
            out[label] = {"per_step": len(recs) / max(1, n_steps), "mean_ms": sum(ms) / len(ms), "max_ms": max(ms), "bytes": recs[0][2]}
        return out

    def all_reduce_sum(self, t, label=None, lane="m"):
        """The collective of the programs: "sum" all-reduce of ``t`` on the lane's communicator (the critic's lane: ``group_c``)."""
        import torch.distributed as dist
        if t is None:
            return
        group = self.group_c if (lane == "s" and self.group_c is not None) else self.group
        with self._log_span(label or "sum", t.numel() * t.element_size()):
            if self._oneshot is not None and lane == "m" and t.data_ptr() == self._oneshot.payload.data_ptr() and t.numel() == self._oneshot.n:
                self._oneshot.all_reduce()   # (GRL_DP_ONESHOT=1: in place, on this lane's stream; every rank enqueues it at this point of the program)
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def _check_topology(self, batch, cbatch):
        """One sync, before anything is captured: the cached topology fits the minibatch the actor's (``batch``) and the critic's lane read."""
        m = self.loss_module
        m.actor_network.hyper_data.check_topology(*[batch[k] for k in m.in_features])
        m.critic_network._network1.hyper_data.check_topology(*[cbatch[k] for k in m.critic_in_features])

    def _compile(self, batch):
        """Record the step's program on static copies of the minibatch (adjacent "run" entries of a lane share one hipGraph)."""
        self._check_topology(batch, batch)
        self._static = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        st = self._st = {}
        self._program = record(self._plan(self._static, st))

    def step_from(self, buf, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One update on the minibatch made of rows ``idx`` (device int64 [B]) of a device-resident ``rollout.RolloutBuffer``.
        With recorded graphs the rows are gathered by ONE launch straight into the static input buffers."""
        self._schedule_check()   # (in front of the gather as well: nothing is enqueued for a refused update)
        keys = self._rollout_keys(buf)[2]
        jobs = None
        # (recorded without a key that is gathered now, e.g. adv_stats: the plain minibatch makes the step record again)
        if self.use_graph and self._program is not None and int(idx.numel()) == self._static[keys[0]].shape[0] and all(k in self._static for k in keys):
            jobs = self._gather_jobs(self._static, buf, keys)
        if jobs is None:
            return self.step(buf.rows(idx, keys))
        hip.call("grl_gather_rows_many", *_job_arrays(jobs), idx, idx.numel())
        return self.step(self._static)

    # ---- several minibatch steps per launch (round 6).  A shard-sized step is ~35 dependent launches of 5-15 us; what it pays on top of
    #      them is the boundary of every replay (~13 us between two graph launches on a stream, ~7 us between the eager minibatch gather
    #      and the graph behind it) and, at 32 frames, the host's ~0.1 ms of enqueue work per step.  The minibatches of an epoch are known
    #      when it starts (train.py:258-261 iterates a sampler without replacement), so ``unroll`` consecutive steps are recorded into ONE
    #      graph per lane: the gathers ride inside (fixed rows of a static index matrix), each lane gathers ITS inputs into buffers of its
    #      own (the lanes share nothing, so no join between the steps of a launch), the critic's gate is a launch of its lane.
    def _epoch_ok(self) -> bool:
        m = self.loss_module
        return bool(self.use_graph and m.world_size == 1 and not (self.group is not None and self.force_dp_plan) and self.overlap_critic
                    and m.critic_coef and self.epoch_unroll > 1)

    def _rollout_keys(self, buf):
        """-> (the rollout tensors the actor's lane reads, the critic's, their union in ``step_from``'s gather order + the epoch's published
        advantage statistics (rollout.RolloutDriver) where a data-parallel run has them)."""
        m = self.loss_module
        var = "var" if "var" in buf.data else "covariance_matrix"
        lane_of = {"action": "m", "loc": "m", var: "m", "sample_log_prob": "m", "state_value": "s", "advantage": "m", "value_target": "s"}
        a = list(dict.fromkeys(list(m.in_features) + [k for k, lane in lane_of.items() if lane == "m"]))
        c = list(dict.fromkeys(list(m.critic_in_features) + [k for k, lane in lane_of.items() if lane == "s"]))
        both = list(dict.fromkeys(list(m.in_features) + list(m.critic_in_features) + list(lane_of)))
        if "adv_stats" in buf.data and self.group is not None:
            both.append("adv_stats")
        return a, c, both

    def _epoch_key(self, buf, B, U):
        """What a recorded multi-step launch depends on: its sizes and the rollout tensors its gathers read (RolloutDriver.compute_advantages
        REPLACES the buffer's state_value / advantage / value_target, so the next rollout through the same buffer object records again)."""
        ka, kc, _ = self._rollout_keys(buf)
        # (four entries: bench.py reads key[1] as the steps per launch and key[2] as the flag of the retired cursor form, now always False)
        return (B, U, False, tuple(buf.flat(k).data_ptr() for k in ka + kc))

    def _epoch_entries(self, buf, idx0, U, gate):
        """``U`` consecutive steps as ONE program (recorded: one graph per lane): step j gathers the FIXED row j of a static [U, B] index
        matrix (filled per launch) into its lane's own inputs.  -> (entries, what ``_epoch`` keeps of them); nothing is launched."""
        B = int(idx0.numel())
        ka, kc, _ = self._rollout_keys(buf)
        sa, sc = buf.rows(idx0, ka), buf.rows(idx0, kc)      # static inputs, one private set per lane
        idx_static = torch.zeros(U, B, device=idx0.device, dtype=torch.int64)
        src = {k: buf.flat(k) for k in ka + kc}   # (held by the recording: its gathers read these storages)
        ga, gc = _job_arrays(self._gather_jobs(sa, buf, ka)), _job_arrays(self._gather_jobs(sc, buf, kc))   # (rows of ``buf`` itself: they fit)

        def gather(args, j, lane):
            row = idx_static[j]
            return Entry("run", lambda: hip.call("grl_gather_rows_many", *args, row, B), lane, "gather")
        sts, mains, critics = [], [], []
        for j in range(U):
            st = {"beta": self.beta_table[j:j + 1], **self._sched_slots(j)}   # (entropy control, per-update schedule: step j of a launch reads ITS entries)
            actor_lane, (*wait, critic_all) = self._lane_entries(sa, sc, st, bool(gate))
            mains += [gather(ga, j, "m"), *actor_lane]
            critics += [*wait, gather(gc, j, "s"), critic_all]   # (behind the lane's gate, in front of its features)
            sts.append(st)
        entries = [Entry("fork", None), *mains, *critics, Entry("join", None),
                   *[Entry("run_host", lambda st=st: self._finish(st)) for st in sts]]
        return entries, dict(key=self._epoch_key(buf, B, U), idx=idx_static, sts=sts, keep=(sa, sc, src))

    def _launch_epoch(self, buf, rows, key, gate):
        """``rows`` [U, B] (device int64): U steps as ONE recorded launch per lane, recorded first when ``key`` (_epoch_key) is not the
        recording's.  Returns the loss dict of the last step; ``self.last_outs`` holds those of all U."""
        U = int(rows.shape[0])
        def issue():
            if self._epoch is None or self._epoch["key"] != key:
                entries, ep = self._epoch_entries(buf, rows[0], U, gate)
                self._check_topology(*ep["keep"][:2])
                self._epoch = dict(ep, program=record(entries))
            self._epoch["idx"].copy_(rows)
            self._execute(self._epoch["program"])
        self._advance(None, U, issue)   # (the first update of a size has run eagerly: no initial entropy is latched here)
        self.last_outs = [st["out"] for st in self._epoch["sts"]]
        return self.last_outs[-1]

    # The size thresholds of the lane policy (_gate_for, run_minibatches) were measured on rigid_insertion_multi HEPi, whose compact graph has
    # this many edges per frame (kNN + task edges); every other workload is placed on that scale by ITS edge count -- the edge kernels are
    # 60 % of every step, so a cloth minibatch of 512 frames is "a rigid minibatch of ~1900 frames" to the policy, not a small one
    POLICY_EDGES_PER_FRAME = 64

    def _work_frames(self, frames: int) -> int:
        """``frames`` of this workload on the scale the lane policy was measured on: the cached topology's edges / POLICY_EDGES_PER_FRAME
        (the topology of a size exists once its first, eager step has run; before that the frame count itself)."""
        hd = getattr(self.loss_module.actor_network, "hyper_data", None)
        topo = hd._cache.get(frames) if hd is not None else None
        if not topo or not topo.get("edges"):
            return frames
        return max(1, round(sum(es.n_edges for es in topo["edges"].values()) / self.POLICY_EDGES_PER_FRAME))

    def _gate_for(self, frames: int) -> bool:
        """Is the critic's lane gated behind the actor's first edge convolution at this minibatch size?  (see _plan_lanes)"""
        mode = self.critic_after_first_conv
        return bool(mode) and (isinstance(mode, str) or not (768 <= self._work_frames(frames) < 2048))

    def run_minibatches(self, buf, idx_rows: torch.Tensor, unroll: Optional[int] = None):
        """The updates of consecutive minibatches: ``idx_rows`` [M, B] int64 (device), row j = the rollout rows of minibatch j (what
        ``rollout.RolloutDriver.epoch_minibatches`` hands out).  One rank with recorded lanes takes one of two recorded forms:
          * ``unroll`` steps per launch where the critic's lane is not gated, or the launches are smaller than the chip (<= 64 frames):
            no boundary at all between the steps of a launch (-3 % at 32 frames, -1.5 % at 1024);
          * the per-step program (a loop of ``step_from``) where the lane IS gated: a gate waiting inside a multi-step launch is a resident
            wave during the previous step's one-wave-per-SIMD backward kernels, which then find 255 free compute units for 256 workgroups
            (+10 % at 512 frames, +20 % at 4096: DESIGN.md, round 6).
        Otherwise, and for the first (eager) step of a size and the remainder, a loop of ``step_from``.  Returns the loss dict of the last
        step; ``self.last_outs`` holds the dicts of the last launch's steps."""
        M, B = int(idx_rows.shape[0]), int(idx_rows.shape[1])
        U = int(unroll or self.epoch_unroll)
        self._check_loss_storage()
        out, j = None, 0
        if not self._epoch_ok() or U <= 1:
            return self._step_rows(buf, idx_rows)
        while j < M and B not in self._eager_sizes:     # the first step of a size runs eagerly (topology, calibration, checks)
            out = self.step_from(buf, idx_rows[j])
            j += 1
        # Which form?  Measured on rigid HEPi (profiles/r06_ab_ungated_unroll.txt, r06_ab_unroll.txt): several steps per launch with the critic's
        # lane UNGATED (it runs ahead inside the launch; the lanes share nothing) beats the gated per-step program up to 2048 frames
        # (-3.7 % at 128, -1.2 % at 256 / 512, -2 % at 2048) and loses to it at 4096 (+1.7 %), where the critic's 0.25 ms of kernels beside
        # the wrong launches cost more than the boundaries of a 3 ms step; with the gate INSIDE a multi-step launch it loses everywhere
        # above 64 frames (a resident waiting wave during the previous step's one-wave-per-SIMD backward kernels).
        Bw = self._work_frames(B)   # (the thresholds are on the scale of the workload they were measured on)
        gate_here = self._gate_for(B) and (Bw <= self.epoch_unroll_max_gated_frames or Bw >= self.epoch_gated_from_frames)
        # That table is ONE workload's; on the others the better of the two forms differs by 1-2 % either way (cloth and rope
        # prefer the gated per-step program at 512 frames, the two-agent EMPN the multi-step launch: profiles/r06_ab_policy.txt).  Both forms
        # give bitwise the same update, so above 64 work-frames the choice is MEASURED once per size on the running program (_tune_form:
        # alternating blocks of U steps of each, HIP events) whenever a call brings enough minibatches; until then the table decides.
        form = self.form_by_size.get(B)
        if form is None and self.autotune_form and Bw > self.epoch_unroll_max_gated_frames and M - j >= self.tune_minibatches(U):
            j, out = self._tune_form(buf, idx_rows, j, U)
            form = self.form_by_size[B]
        if form is None:
            form = "per_step" if gate_here and Bw > self.epoch_unroll_max_gated_frames else "unrolled"
        elif form == "unrolled":
            gate_here = False   # (the measured multi-step launch is the ungated one)
        if form == "unrolled" and M - j >= U:
            key = self._epoch_key(buf, B, U)
            while M - j >= U:
                out = self._launch_epoch(buf, idx_rows[j:j + U], key, gate_here)
                j += U
        return self._step_rows(buf, idx_rows[j:], out)

    TUNE_ROUNDS = 2   # alternating blocks per form in _tune_form

    def tune_minibatches(self, U: Optional[int] = None) -> int:
        """Minibatches one measurement of the two recorded forms consumes (they are ordinary updates, in order)."""
        U = int(U or self.epoch_unroll)
        return U + 3 + 2 * self.TUNE_ROUNDS * U

    def _tune_form(self, buf, idx_rows, j, U):
        """Measure, on the running program, which recorded form is faster at this minibatch size: ``U`` steps per launch with the critic's lane
        ungated, or one step per launch with the lane gated as ``_gate_for`` says.  Both are recorded and replayed once, then TUNE_ROUNDS
        alternating blocks of U steps of each are timed with HIP events on the caller's stream (both lanes joined at every block boundary);
        ONE host synchronisation at the end.  Every step is an ordinary update of the next minibatch, and the two forms produce bitwise the
        same update (tests/test_gpu_rollout.py), so the measurement changes nothing but the time.  -> (next j, last loss dict)."""
        B = int(idx_rows.shape[1])
        main = torch.cuda.current_stream()
        key = self._epoch_key(buf, B, U)

        def unrolled(rows):
            return self._launch_epoch(buf, rows, key, False)

        out = unrolled(idx_rows[j:j + U]); j += U          # records (and runs) the multi-step launch
        out = self._step_rows(buf, idx_rows[j:j + 3]); j += 3          # records the per-step program, first replays
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * self.TUNE_ROUNDS + 1)]
        self.join_lanes()
        ev[0].record(main)
        for r in range(self.TUNE_ROUNDS):
            out = unrolled(idx_rows[j:j + U]); j += U
            self.join_lanes()
            ev[2 * r + 1].record(main)
            out = self._step_rows(buf, idx_rows[j:j + U]); j += U
            self.join_lanes()
            ev[2 * r + 2].record(main)
        ev[-1].synchronize()
        t_u = min(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(self.TUNE_ROUNDS)) / U
        t_p = min(ev[2 * r + 1].elapsed_time(ev[2 * r + 2]) for r in range(self.TUNE_ROUNDS)) / U
        self.form_by_size[B] = "unrolled" if t_u <= t_p else "per_step"
        self.form_times[B] = {"unrolled_ms_per_step": t_u, "per_step_ms_per_step": t_p, "steps_per_block": U, "blocks_per_form": self.TUNE_ROUNDS}
        return j, out

    def reset_graph(self):
        """Drop the recorded step (next step re-records): needed when the minibatch size changes."""
        self._drop_recordings()
        self._eager_sizes, self.form_by_size, self.form_times = set(), {}, {}

    # ---- the whole training state (checkpoint.py): what makes update n + 1 what it is, most of it outside the modules' state_dict()
    def _algorithm(self) -> dict:
        """The objective as plain values: the loss class, the projection's type and flags (a state is loaded into the same algorithm only)."""
        m = self.loss_module
        proj = getattr(m, "projection", None)
        out = {"loss": type(m).__name__, "projection": None}
        if proj is not None:
            out.update(projection=proj.proj_type, scale_prec=proj.scale_prec, entropy_schedule=proj.entropy_schedule_type,
                       entropy_eq=proj.entropy_eq, entropy_first=proj.entropy_first, entropy_control=bool(getattr(m, "entropy_control", False)))
        return out

    def _saved_hyper(self) -> dict:
        return dict(self._hyper, anneals_lr=self.anneals_lr, anneals_eps=self.anneals_eps, total_network_updates=self.total_network_updates,
                    track_stats=self.track_stats)

    def _named_groups(self) -> list:
        return [("actor.", self.loss_module.actor_network), ("critic.", self.loss_module.critic_network)]

    def _data_objects(self) -> dict:
        """The ``HyperData`` of either network: each keeps noise words and cached topologies."""
        m = self.loss_module
        hds = {"actor": getattr(m.actor_network, "hyper_data", None),
               "critic": getattr(getattr(m.critic_network, "_network1", None), "hyper_data", None)}
        return {k: hd for k, hd in hds.items() if hd is not None}

    def state_dict(self) -> dict:
        """Everything the next update depends on, as CPU tensors and plain Python values (``checkpoint.save`` writes it; INTEGRATION.md
        "Saving and resuming a run" lists it).  Joins the lanes and synchronises once; call it between any two ``step`` / ``run_minibatches`` calls.
        The step count is ONE number, the host's: a state whose device-side count differs (an update that raised while it was issued) is
        refused, it cannot be continued bit for bit."""
        from . import checkpoint as ck
        m = self.loss_module
        self.join_lanes()
        flat_state = self._flat_state()   # (the synchronisation, and the refusal)
        proj = getattr(m, "projection", None)
        ent = getattr(proj, "initial_entropy", None)
        return {
            "version": ck.VERSION, "layout": ck.layout(self._named_groups(), self.flat), "n_actor": int(self.n_actor),
            **flat_state, "base_lr": self._base_lr,
            "hyper": self._saved_hyper(), "algorithm": self._algorithm(),
            "device_scalars": {k: cpu(t) for k, t in m.device_scalars.items()},
            "initial_entropy": None if ent is None else cpu(torch.as_tensor(ent)),
            "stats": {"actor": cpu(self.stats_actor), "critic": cpu(self.stats_critic), "one_stream": bool(self._stats_one_stream)} if self.track_stats else None,
            "actor": {k: cpu(v) for k, v in m.actor_network.state_dict().items()},
            "critic": {k: cpu(v) for k, v in m.critic_network.state_dict().items()},
            "data": {k: ck.data_state(hd) for k, hd in self._data_objects().items()},
            "rank": int(self.rank), "world": int(m.world_size),
            "form_by_size": {int(k): str(v) for k, v in self.form_by_size.items()},
        }

    def load_state_dict(self, sd: dict) -> None:
        """Continue the run ``sd`` (``state_dict()``) was taken from: every value is restored IN PLACE, into the storage the recorded programs
        read (``copy_``; the modules through ``load_state_dict``, which writes through their views of ``flat``), stream-ordered on the
        caller's stream behind a join of the lanes.  Nothing recorded is dropped -- ``_program``, ``_static`` and ``_epoch`` stay the
        objects they were -- and the next update is bit for bit the one the saved run would have issued.

        The one saved step count goes to ``steps``, ``step_dev``, ``step_dev_c`` and ``lane_flag`` alike.  They must never disagree: the
        recorded Adam launches take their bias correction from ``step_dev`` (actor) and ``step_dev_c`` (critic), a gated critic lane waits
        until ``lane_flag`` -- which the actor's lane sets to ``step_dev`` -- reaches ``step_dev_c + 1``, and the host forms the entropy
        bounds and the (lr, clip epsilon) table from ``steps``.  A critic count ahead of the actor's leaves the gate waiting for a signal
        that does not come (``_advance`` explains the same for the host's count); one behind it releases the lane early and gives the two
        networks different bias corrections; a host count apart from the device's schedules other rates than Adam's step belongs to.

        Raises ValueError BEFORE anything is written when the layout fingerprint, the algorithm, a hyper-parameter, ``rank`` / ``world`` or
        the format version differ from this updater's: a resumed run with other settings is another run.  Change settings after loading,
        through the properties.  ``form_by_size`` is advisory: taken only while this updater has measured nothing itself."""
        from . import checkpoint as ck
        m = self.loss_module
        ck.check_version(sd, "PolicyUpdater.load_state_dict")
        self._check_flat_state(sd, self._named_groups())
        if sd["n_actor"] != self.n_actor:
            raise ValueError(f"the saved parameter layout is not this updater's (n_actor {sd['n_actor']} against {self.n_actor})")
        if sd["algorithm"] != self._algorithm():
            raise ValueError(f"the saved run's algorithm differs at {ck.differing(sd['algorithm'], self._algorithm())}: saved {sd['algorithm']}, "
                             f"this updater {self._algorithm()}")
        odd = ck.differing(sd["hyper"], self._saved_hyper())
        if odd:
            raise ValueError("the saved run's hyper-parameters differ: " + ", ".join(f"{k} saved {sd['hyper'].get(k)!r}, here "
                             f"{self._saved_hyper().get(k)!r}" for k in odd) + " (load into an updater built alike, then change the setting)")
        if (sd["rank"], sd["world"]) != (self.rank, m.world_size):
            raise ValueError(f"the state is rank {sd['rank']} of {sd['world']}, this updater rank {self.rank} of {m.world_size}: every rank "
                             "loads its own file, under the world size it was saved with")
        if set(sd["device_scalars"]) != set(m.device_scalars) or set(sd["data"]) != set(self._data_objects()):
            raise ValueError(f"the saved loss scalars {sorted(sd['device_scalars'])} / data objects {sorted(sd['data'])} are not this updater's")
        for bad in (ck.module_mismatch(m.actor_network, sd["actor"], "actor"), ck.module_mismatch(m.critic_network, sd["critic"], "critic"),
                    *[hd.topology_mismatch(sd["data"][k]["topology"]) for k, hd in self._data_objects().items()]):
            if bad:
                raise ValueError(bad)
        # ---- nothing above has written; everything below writes in place
        self.join_lanes()
        dev = self.flat.device
        with torch.no_grad():
            m.actor_network.load_state_dict(sd["actor"])    # (through the views of ``flat``; the policy re-inspects its latches: they are saved true)
            m.critic_network.load_state_dict(sd["critic"])
            self._load_flat_state(sd)
            m._global_steps = self.steps
            for t in (self.step_dev_c, self.lane_flag):
                t.fill_(self.steps)
            self._base_lr = float(sd["base_lr"])
            for name, t in m.device_scalars.items():
                t.copy_(sd["device_scalars"][name])
            proj = getattr(m, "projection", None)
            if proj is not None:
                ent = sd["initial_entropy"]
                proj.initial_entropy = None if ent is None else ent.to(dev)
                proj._init_host_src = proj._init_host = None   # (the cached host copy belongs to the value that was there)
            if self.track_stats:
                self.stats_actor.copy_(sd["stats"]["actor"])
                self.stats_critic.copy_(sd["stats"]["critic"])
                self._stats_one_stream = bool(sd["stats"]["one_stream"])
            for name, hd in self._data_objects().items():
                ck.load_data_state(hd, sd["data"][name], dev)
        self._calib_synced = True   # (the latches and the kernels are the saved run's: no replica calibrates again)
        self._settle_calibration(m.actor_network)
        if not self.form_by_size:
            self.form_by_size = dict(sd["form_by_size"])

    def _check_calibrated(self):
        """Data parallel: the first training forward of a fresh actor re-initialises the conv kernels from rank-local data
        (conv.py:104-105).  Let it happen once, on every rank, BEFORE the first update, then adopt rank 0's result -- otherwise each
        replica would rescale its own weights (views of ``flat``) and the replicas would diverge for good."""
        # (the latch FIRST: ``hasattr(gnn, "calibrated")`` evaluates the property, which reads the per-conv flags from the device -- until
        #  round 4 every data-parallel step paid a device synchronisation here and the host never ran ahead of the device)
        if self.group is None or self._calib_synced:
            return None
        actor = self.loss_module.actor_network
        gnn = getattr(actor, "gnn", None)
        if gnn is None or not hasattr(gnn, "calibrated"):
            return None
        self._calib_synced = True
        return not gnn.calibrated   # True: this rank's actor still has to calibrate -> the caller syncs afterwards

    def _advance(self, batch, n, issue):
        """The bookkeeping around ``n`` updates that ``issue()`` enqueues: the loss module's count, the entropy bounds of the updates (from
        ``batch`` the initial entropy, at the first one), their learning rates and clip epsilons under a per-update schedule, the host's
        step count -- taken back when issuing raised.  -> what ``issue`` returns."""
        self._schedule_check(n)
        self.loss_module._global_steps = self.steps
        self._entropy_prepare(batch, n)
        lr_before = self._lr
        self._schedule_prepare(n)
        try:
            # ``_counted`` takes the count back when issuing raised.  The critic lane's gate waits until the DEVICE-side step count (advanced by
            # the actor's feature launch) reaches the HOST's: a step that raised before that launch was enqueued must not leave the host ahead
            # for good -- the next step's wait would never be satisfied and the process would hang on the device instead of raising (ADVICE
            # r5).  After a failure the host count is at most the device's: the gate may then release early, it can never be stuck.
            return self._counted(n, issue)
        except BaseException:
            self._lr = lr_before   # (a per-update schedule: the rate of the last update that WAS issued)
            raise

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if self._check_calibrated():
            actor, m = self.loss_module.actor_network, self.loss_module
            with torch.no_grad():
                actor.forward_diag(*[batch[k] for k in m.in_features], train=True)   # calibrates on this rank's shard
            self.sync_replicas()                                                       # ... and rank 0's factors win everywhere
        return self._advance(batch, 1, lambda: self._step(batch))

    def _step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        B = next(v.shape[0] for v in batch.values() if torch.is_tensor(v))
        self._check_loss_storage()
        if self._eager_first(B):
            st = {}
            self._first_eager(self._plan(batch, st))
            return st["out"]
        if self._program is not None and (any(self._static[k].shape != batch[k].shape for k in self._static if k in batch)
                                          or ("adv_stats" in batch) != ("adv_stats" in self._static)):
            self.reset_graph()                      # another minibatch size (or the published advantage statistics appeared /
            self._eager_sizes.add(B)                # disappeared: a different data-parallel plan): record again for it
        if self._program is None:
            try:
                self._compile(batch)
            except Exception as e:
                torch.cuda.synchronize()
                if not self.allow_eager_fallback:
                    raise RuntimeError(
                        f"hipGraph capture of the policy-update step failed ({type(e).__name__}: {e}).  Pass use_graph=False, or "
                        "allow_eager_fallback=True to continue with eager launches (several times slower for small minibatches).") from e
                import sys
                print(f"[geometry_rl_amd] hipGraph capture failed ({type(e).__name__}: {e}); continuing with eager launches "
                      "(allow_eager_fallback=True)", file=sys.stderr)
                self.use_graph, self._program, self._static, self.mode = False, None, None, "eager (graph capture failed)"
                return self._step(batch)
        self._refresh(self._static, batch, "the recorded step was captured for {}: call PolicyUpdater.reset_graph() before changing the "
                      "minibatch size")
        self._execute(self._program)
        return self._st["out"]

    def _execute(self, program):
        """Issue a program, eager or recorded (program.execute): lane "s" is the critic's stream, every entry goes through ``_do``."""
        execute(program, self._do, self._critic_stream, self._log_span)

    def join_lanes(self):
        """The caller's stream waits for the critic's stream, if there is one (for callers that read or time both lanes' work)."""
        if self._cstream is not None:
            torch.cuda.current_stream().wait_stream(self._cstream)

    def _do(self, e: Entry):
        """Issue one entry on the current stream (tools that time entries wrap this method); "sum" is the programs' one collective."""
        if e.kind == "sum":
            self.all_reduce_sum(e.item(), e.label, e.lane)
        else:
            super()._do(e)
