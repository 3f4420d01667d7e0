"""``FlatUpdater``: what ``PolicyUpdater`` (updater.py) and ``BCUpdater`` (bc.py) share around the actor's lane, once -- the flat fp32
layout of parameters, gradients and moments, the rule for when the one fold launch may overwrite the leaf gradients and its check on the
first eager step, ``[clip +] Adam`` on a slice, the static inputs of a recorded step, the eager-first / step-count bookkeeping and the
flat part of a training state.  Which programs a step is made of, and how many are kept, is each subclass's own business."""
import contextlib
import ctypes

import torch

from . import hip
from .program import Entry, execute


def _job_arrays(jobs):
    """[(destination pointer, source pointer, bytes)] as the three C arrays and the count that grl_copy_many / grl_gather_rows_many take."""
    n = len(jobs)
    return ((ctypes.c_void_p * n)(*[j[0] for j in jobs]), (ctypes.c_void_p * n)(*[j[1] for j in jobs]),
            (ctypes.c_longlong * n)(*[j[2] for j in jobs]), n)


cpu = lambda t: t.detach().cpu().clone()   # a tensor as a training state keeps it


def fold_overwrite(actor) -> bool:
    """May the one fold launch at the end of the backward pass WRITE the leaf gradients (ops.flush_deferred_grads(overwrite=True)) instead
    of accumulating into a zeroed buffer (no per-step zeroing launch)?  Only while EVERY leaf gradient of the step comes through the fold
    queue: not with a post_fc (transformer) actor, stock or on HIP kernels (``cls_token`` and the template encoder layer take no part in
    the forward, no fold ever writes their gradients: they stay the zeros of the buffer), nor with an attention gate that runs as torch
    modules (torch's AccumulateGrad adds into .grad; gate_kernels="hip" hands the gate's gradients to the queue like every other)."""
    gnn = getattr(actor, "gnn", None)
    return (not getattr(actor, "post_fc", False)
            and not any(getattr(mod, "attention", False) and getattr(mod, "gate_kernels", "torch") == "torch"
                        for mod in (gnn.modules() if gnn is not None else [])))


class FlatUpdater:
    """Base of the updaters.  A subclass provides ``clip`` / ``max_norm`` / ``betas`` / ``eps`` (attributes or properties) and calls
    ``__init__`` with its actor and its parameter groups."""

    def __init__(self, actor, param_groups, lr, use_graph, record_floats=0):
        self._lay_out(param_groups, lr, record_floats)
        self.use_graph = bool(use_graph)
        self.mode = "graph" if use_graph else "eager"   # what actually runs (bench.py reports it)
        if use_graph and getattr(actor, "stock_torch_gnn", False):
            # config 1's baseline actor with kernels="torch" is a stock torch.nn.TransformerEncoder: torch's own launches (rocBLAS / hipBLASLt
            # workspaces) are not capture-safe on this stack; it is the reference's CPU-sized plumbing case, not a throughput path
            self.use_graph, self.mode = False, "eager (stock-torch transformer actor: not recorded)"
        self._eager_sizes = set()   # minibatch sizes whose first, eager step has run (_eager_first)
        self._fold_overwrite = fold_overwrite(actor)
        self._overwrite_checked = not self._fold_overwrite

    # ---- layout
    def _lay_out(self, param_groups, lr, record_floats=0):
        """Parameters (``param_groups``: lists, one after the other; ``n_actor``: the padded size of the first), gradients (``gflat``, in ``gbuf``
        behind ``record_floats`` floats of room) and moments as flat fp32 buffers with ``p.data`` / ``p.grad`` as views; the step count, the rate."""
        self.params = [p for g in param_groups for p in g]
        pad4 = lambda k: (k + 3) & ~3   # every parameter starts 16-byte aligned (vector loads in the weight-staging prologues)
        self.n_actor = sum(pad4(p.numel()) for p in param_groups[0])
        n = sum(pad4(p.numel()) for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        self._rec = int(record_floats)
        self.gbuf = torch.zeros(self._rec + n, device=dev, dtype=torch.float32)
        self.gflat = self.gbuf[self._rec:]
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
        # learning rate, device side: the recorded Adam launches read it, so a rate the host writes (train.py:264-271) takes effect under replay
        self.lr_dev = torch.full((1,), float(lr), device=dev, dtype=torch.float32)
        self._lr = float(lr)

    def release(self):
        """End of this updater: every parameter becomes an ordinary tensor again (its values kept, its ``.grad`` dropped).  An updater built
        afterwards on the same modules lays them out anew and finds the values."""
        for p in self.params:
            p.data = p.data.clone()
            p.grad = None

    # ---- ``lr`` lives in device memory: setting it records nothing again
    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        if not self._schedule_takes_lr(float(value)) and float(value) != self._lr:
            self._lr = float(value)
            self.lr_dev.fill_(self._lr)

    def _schedule_takes_lr(self, value: float) -> bool:
        """Hook of the setter: True where a per-update schedule of the subclass has taken ``value`` (as its base rate)."""
        return False

    # ---- the actor's lane
    @contextlib.contextmanager
    def _count_rides(self, hyper_data):
        """Around the actor's forward: the step count rides on its feature launch (grl_build_features_bump)."""
        hyper_data.bump_next = self.step_dev
        yield
        assert hyper_data.bump_next is None, "the actor's feature launch did not take the step count"

    def _adam(self, lo, hi, *, lr, step_dev, sq):
        """One optimizer's step over its slice [lo, hi) of the flat buffers (train.py:308-316); ``lr`` / ``step_dev``: the device scalars the
        launch reads; ``sq``: the fp64 scalar grl_clip_coef leaves the squared gradient norm in (read only with ``clip``)."""
        coef = None
        if self.clip:   # train.py:308-310
            coef = torch.empty(1, device=self.flat.device, dtype=torch.float32)
            hip.call("grl_clip_coef", self.gflat[lo:hi], hi - lo, self.max_norm, sq, coef)
        hip.call("grl_adam_step_dev", self.flat[lo:hi], self.gflat[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], hi - lo, lr,
                 *self.betas, self.eps, step_dev, coef, 1.0)

    def _tail_args(self, lo, hi, lr, step_dev):
        """The Adam part of the one-launch tail (ops.fold_adam_report) over the slice [lo, hi)."""
        return dict(grads=self.gflat[lo:hi], params=self.flat[lo:hi], exp_avg=self.exp_avg[lo:hi], exp_avg_sq=self.exp_avg_sq[lo:hi],
                    lr_dev=lr, betas=self.betas, eps=self.eps, step_dev=step_dev)

    # ---- static inputs of a recorded step
    @staticmethod
    def _refresh(static, batch, what):
        """Copy the minibatch into the static inputs the recorded graphs read, 24 tensors per launch; ``what``: the ValueError's size hint."""
        jobs = []
        for k, v in static.items():
            src = batch[k]
            if src is v:
                continue
            if src.shape != v.shape:
                raise ValueError(f"minibatch tensor '{k}' has shape {tuple(src.shape)}, " + what.format(tuple(v.shape)))
            if src.dtype != v.dtype or not src.is_contiguous() or src.device != v.device:
                v.copy_(src)  # host-resident / strided / other dtype: the ordinary path
            else:
                jobs.append((v.data_ptr(), src.data_ptr(), v.numel() * v.element_size()))
        for i in range(0, len(jobs), 24):
            hip.call("grl_copy_many", *_job_arrays(jobs[i:i + 24]))

    @staticmethod
    def _gather_jobs(static, buf, keys):
        """The jobs of one grl_gather_rows_many launch, rows of the rollout's tensors ``keys`` into ``static``; None where one does not fit."""
        src = [buf.flat(k) for k in keys]
        if any(static[k].dtype != v.dtype or static[k][0].numel() != v.shape[1] for k, v in zip(keys, src)):
            return None
        return [(static[k].data_ptr(), v.data_ptr(), v.shape[1] * v.element_size()) for k, v in zip(keys, src)]

    def _step_rows(self, buf, rows, out=None):
        """``step_from`` on the rows of ``rows`` [M, B], in order -> the last step's report (``out`` where M = 0)."""
        for r in rows:
            out = self.step_from(buf, r)
        return out

    # ---- issuing
    def _do(self, e: Entry):
        """Issue one entry on the current stream (tools that time entries wrap this method)."""
        if e.kind == "graph":
            e.item.replay()
        else:   # "run", "run_host"
            e.item()

    def _execute(self, program):
        """Issue a program, eager or recorded (program.execute), on the caller's stream: every entry goes through ``_do``."""
        execute(program, self._do, lambda: None, lambda label: None)

    def _eager_first(self, B: int) -> bool:
        """Is this step of ``B`` frames issued eagerly?  The first of a size always: it builds the cached topology, calibrates, is checked."""
        eager = not (self.use_graph and B in self._eager_sizes)
        self._eager_sizes.add(B)
        return eager

    def _first_eager(self, plan):
        """Issue the eager program ``plan``, the first time with the overwrite-coverage check around it: overwrite mode is only right while
        NO leaf gradient arrives through torch's AccumulateGrad, which would add into a never-zeroed .grad.  A hook on a leaf fires exactly
        for such a gradient (ops' backward functions hand None to autograd for the leaves whose slabs they queue)."""
        hooks, torch_fed = [], []
        if not self._overwrite_checked:
            hooks = [p.register_hook(lambda g, i=i: torch_fed.append(i) if g is not None else None) for i, p in enumerate(self.params)]
        try:
            self._execute(plan)
        finally:
            for h in hooks:
                h.remove()
        if hooks:
            self._overwrite_checked = True
            if torch_fed:
                raise RuntimeError(f"{len(set(torch_fed))} parameter(s) received their gradient from torch autograd instead of the fold queue "
                                   f"while {type(self).__name__} runs in overwrite mode (their .grad is never zeroed): this model must be "
                                   "added to the exceptions of flat.fold_overwrite")

    def _counted(self, n, issue):
        """``issue()`` enqueues ``n`` updates: the host's step count advances in front of it and is taken back when issuing raised."""
        self.steps += n
        try:
            return issue()
        except BaseException:
            self.steps -= n
            raise

    # ---- the flat part of a training state (checkpoint.py); each subclass adds its own keys around it
    def _flat_state(self) -> dict:
        """Buffers, moments, the ONE step count (a device-side count that differs is refused) and the rate, on the CPU.  Synchronises once."""
        if self.flat.is_cuda:
            torch.cuda.current_stream().synchronize()
        if int(self.step_dev) != self.steps:
            raise RuntimeError(f"the device-side step count is {int(self.step_dev)}, the host's {self.steps}: an update failed while it was "
                               "issued; this state cannot be resumed bit for bit")
        return {"flat": cpu(self.flat), "exp_avg": cpu(self.exp_avg), "exp_avg_sq": cpu(self.exp_avg_sq), "steps": int(self.steps), "lr": self._lr}

    def _check_flat_state(self, sd, named_groups):
        """ValueError where the saved layout is not the one of ``named_groups`` ([(prefix, module)], checkpoint.layout) here; writes nothing."""
        from . import checkpoint as ck
        mine = ck.layout(named_groups, self.flat)
        if sd["layout"] != mine or sd["flat"].numel() != self.flat.numel():
            odd = [a[0] for a, b in zip(sd["layout"], mine) if a != b][:3]
            raise ValueError(f"the saved parameter layout is not this updater's ({len(sd['layout'])} parameters, {sd['flat'].numel()} floats "
                             f"against {len(mine)}, {self.flat.numel()}; first differences {odd})")

    def _load_flat_state(self, sd):
        """In place, under the caller's ``no_grad``; ``steps`` and ``step_dev`` take the ONE saved count (Adam's bias correction reads the device's)."""
        self.flat.copy_(sd["flat"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.steps = int(sd["steps"])
        self.step_dev.fill_(self.steps)
        self._lr = float(sd["lr"])
        self.lr_dev.fill_(self._lr)

    def _settle_calibration(self, actor):
        """The tail of a load: saved before the first training forward, the next step calibrates, which no capture allows: it runs eagerly."""
        from . import checkpoint as ck
        if not ck.settle_calibration(actor):
            self._eager_sizes = set()
