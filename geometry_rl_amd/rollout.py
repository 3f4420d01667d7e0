"""The once-per-rollout part of the training loop around the policy update (examples/torchrl/train.py:249-316):

    values over the [N, T+1] frames  ->  shifted GAE  ->  ppo_epochs x (N*T / mini_batch) minibatch updates, each minibatch
    drawn WITHOUT replacement.

The reference keeps the rollout in a CPU ``LazyTensorStorage`` and moves every minibatch to the device (train.py:120,128,261);
here the rollout stays resident in HBM (4096 x 128 rigid frames are 1.6 GB) and a minibatch is assembled by ONE gather launch
(``grl_gather_rows_many``) straight into the static input buffers of the recorded update step.

Sampling (``RolloutDriver(mini_batch_size=, sampling=)``), always without replacement, every frame exactly once per epoch:

* ``"env_aligned"`` (default): per environment a random permutation of its T time steps; a minibatch of ``k * N`` frames
  (``mini_batch_size`` must be a multiple of the number of environments N; k = 1 for rigid / rope whose configs set
  mini_batch_size = num_envs, k = 2 for cloth: configs/cloth_hanging_multi_hepi_trpl_cfg.yaml:40,125) takes k permutation columns,
  laid out column after column, so row i of EVERY minibatch belongs to environment i mod N.  That is what the graph topology
  cached per batch size assumes (rigid_tasks_data.py:254-255: valid point counts and kNN edges are those of the first batch of
  that size).  DEVIATION from the reference, which draws uniformly from the flattened N*T frames (SamplerWithoutReplacement,
  train.py:128) and therefore pairs its cached placeholders with rows of other environments -- harmless only when all
  environments share one topology.
* ``"uniform"``: the reference's sampler -- a random permutation of the N*T frames cut into minibatches of ``mini_batch_size``
  (last one dropped if short: the recorded step has one size).  Allowed for task families whose topology does not depend on the
  row (cloth: fully connected hole boundary, fixed sizes); for rigid (ragged point counts) it raises unless
  ``allow_stale_topology=True`` reproduces the reference quirk knowingly."""
from typing import Dict, Iterator, Optional

import torch

from . import agent as _agent, checkpoint as _ckpt, hip as _hip, updater as _updater
from .program import capture

PPO_KEYS = ("action", "loc", "var", "sample_log_prob", "state_value", "advantage", "value_target")


class RolloutBuffer:
    """Device-resident rollout: every tensor is [N, T, ...]; ``flat(k)`` views it as rows [N*T, width]."""

    def __init__(self, data: Dict[str, torch.Tensor]):
        some = next(iter(data.values()))
        self.N, self.T = some.shape[0], some.shape[1]
        self.data = {k: v.contiguous() for k, v in data.items()}
        for k, v in self.data.items():
            if v.shape[:2] != (self.N, self.T):
                raise ValueError(f"{k}: expected leading dims [{self.N}, {self.T}], got {tuple(v.shape)}")

    def flat(self, k: str) -> torch.Tensor:
        v = self.data[k]
        return v.reshape(self.N * self.T, -1)

    def rows(self, idx: torch.Tensor, keys) -> Dict[str, torch.Tensor]:
        """Plain (allocating) minibatch: rows ``idx`` of the given keys."""
        return {k: self.flat(k).index_select(0, idx) for k in keys}


def explained_variance(value: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``train/explained_variance`` (train.py:142,325: torchmetrics ``ExplainedVariance()`` on ``state_value`` against ``value_target``)
    of a rollout's [N, T(, 1)] float32 tensors -> device float32[2]: [0] what the metric returns for [N, T, 1] inputs -- it reduces over
    dimension 0, one score 1 - Var(target - value) / Var(target) per time step, and averages the scores uniformly; a zero denominator
    scores 1 where the numerator is 0 too and 0 otherwise -- and [1] the same score over all N*T frames at once.  torchmetrics is not a
    dependency of this package: the semantics is RESTATED and UNPINNED (no fixture from the reference checks it; tests/stats_ref.py is the
    float64 restatement the kernel is tested against).  Two launches, no synchronisation."""
    _hip.check_f32(value, target)
    N, T = int(value.shape[0]), int(value.shape[1])
    if value.numel() != N * T or target.numel() != N * T:
        raise ValueError(f"expected [N, T] or [N, T, 1] tensors, got {tuple(value.shape)} and {tuple(target.shape)}")
    nbytes = _hip.query("grl_explained_variance_scratch_bytes", N, T)
    if nbytes < 0:
        raise ValueError(f"grl_explained_variance does not take a rollout of {N} x {T} frames")
    scratch = torch.empty(nbytes, device=value.device, dtype=torch.uint8)
    out = torch.empty(2, device=value.device, dtype=torch.float32)
    _hip.call("grl_explained_variance", value.contiguous(), target.contiguous(), N, T, scratch, out)
    return out


class EpisodeStats:
    """torchrl's collector-side ``RewardSum`` and ``StepCounter`` transforms, which every reference config lists
    (configs/rigid_insertion_multi_hepi_trpl_cfg.yaml:74-76), for N environments on the device.  ``scan(reward, done)`` takes a rollout's
    [N, T(, 1)] reward (float32) and done (bool) and returns ``episode_reward`` (the running return: a float32 sum, one add per step) and
    ``step_count`` (the running length) per frame; the frame behind a ``done`` frame starts from 0, and the running values are carried in
    ``ret_state`` / ``len_state`` from one call to the next (episodes continue across rollouts).  ``sums`` (device fp64[3]) holds the last
    scan's (sum of episode_reward, sum of step_count, number) over its done frames: what train.py:238-246 logs as ``train/reward`` and
    ``train/episode_length``.  RESTATED and UNPINNED: torchrl is not a dependency and no fixture from the reference checks it
    (tests/stats_ref.py is the restatement the kernel is tested against)."""

    def __init__(self, N: int, device="cuda"):
        self.N = int(N)
        self.ret_state = torch.zeros(self.N, device=device, dtype=torch.float32)
        self.len_state = torch.zeros(self.N, device=device, dtype=torch.int32)
        self.sums = torch.zeros(3, device=device, dtype=torch.float64)

    def scan(self, reward: torch.Tensor, done: torch.Tensor):
        _hip.check_f32(reward)
        N, T = int(reward.shape[0]), int(reward.shape[1])
        if N != self.N or reward.numel() != N * T or done.numel() != N * T:
            raise ValueError(f"expected [{self.N}, T] or [{self.N}, T, 1] tensors, got {tuple(reward.shape)} and {tuple(done.shape)}")
        episode_reward = torch.empty(reward.shape, device=reward.device, dtype=torch.float32)
        step_count = torch.empty(reward.shape, device=reward.device, dtype=torch.int32)
        _hip.call("grl_episode_scan", reward.contiguous(), done.to(torch.uint8).contiguous(), self.ret_state, self.len_state,
                  episode_reward, step_count, self.sums, N, T)
        return episode_reward, step_count

    def state_dict(self) -> dict:
        """The running return and length of every environment and the last scan's sums (episodes continue across rollouts, and across a
        resumed run): CPU tensors."""
        return {"version": _ckpt.VERSION, "N": self.N, "ret_state": self.ret_state.detach().cpu().clone(),
                "len_state": self.len_state.detach().cpu().clone(), "sums": self.sums.detach().cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        _ckpt.check_version(sd, "EpisodeStats.load_state_dict")
        if sd["N"] != self.N:
            raise ValueError(f"the saved episode statistics are those of {sd['N']} environments, these of {self.N}")
        self.ret_state.copy_(sd["ret_state"])
        self.len_state.copy_(sd["len_state"])
        self.sums.copy_(sd["sums"])


# ---- the sampler without replacement (train.py:128,258), shared by RolloutDriver and bc.BehaviorCloner
def check_sampling(spec, sampling: str, allow_stale_topology: bool) -> None:
    """ValueError for an unknown sampler, and for the uniform one on a ragged task unless ``allow_stale_topology``."""
    if sampling not in ("env_aligned", "uniform"):
        raise ValueError(sampling)
    # raggedness, not the task family, is what makes the cached topology wrong for rows of other environments: rigid tasks carry a
    # per-sample object_num_points, variable-length ropes a per-sample links_num_points (padded nodes are dropped by the CACHED counts)
    infos = (getattr(spec, "obs_names", None) or {}).get("infos", ())
    ragged = any(n in infos for n in ("object_num_points", "links_num_points"))
    if sampling == "uniform" and ragged and not allow_stale_topology:
        raise ValueError("uniform sampling pairs the topology cached per batch size with rows of other environments; this task has "
                         "ragged per-sample point counts (object_num_points / links_num_points): pass allow_stale_topology=True to "
                         "reproduce the reference quirk")


def seeded_generator(gen: Optional[torch.Generator], seed: int, device) -> torch.Generator:
    """``gen``, or while nothing has been drawn yet (None) a new generator on ``device`` seeded with ``seed``."""
    return gen if gen is not None else torch.Generator(device=device).manual_seed(seed)


def env_aligned_rows(n: int, T: int, gen: torch.Generator, device) -> torch.Tensor:
    """[T, n] int64 row indices into the flattened [n*T] rollout of ``n`` environments: column i of every row belongs to environment i."""
    perm = torch.argsort(torch.rand(n, T, device=device, generator=gen), dim=1)       # per-environment permutation of time
    return (torch.arange(n, device=device)[:, None] * T + perm).t().contiguous()


class RolloutDriver:
    def __init__(self, updater: "_updater.PolicyUpdater", spec, gamma: float = 0.99, lmbda: float = 0.95, ppo_epochs: int = 5,
                 seed: int = 0, mini_batch_size: Optional[int] = None, sampling: str = "env_aligned",
                 allow_stale_topology: bool = False):
        self.updater, self.spec = updater, spec
        self.gamma, self.lmbda, self.ppo_epochs = gamma, lmbda, ppo_epochs
        self.gen = None
        self.seed = seed
        self.mini_batch_size = mini_batch_size   # None: one frame per environment (= num_envs)
        check_sampling(spec, sampling, allow_stale_topology)
        self.sampling = sampling

    def _settings(self) -> dict:
        return dict(gamma=self.gamma, lmbda=self.lmbda, ppo_epochs=self.ppo_epochs, mini_batch_size=self.mini_batch_size, sampling=self.sampling)

    def state_dict(self) -> dict:
        """The sampler's generator -- wherever in its sequence it stands, also between two launches of an epoch -- or the seed while no
        minibatch has been drawn yet; the settings ride along and are compared on loading."""
        return {"version": _ckpt.VERSION, "settings": self._settings(), "generator": _ckpt.generator_state(self.gen, self.seed)}

    def load_state_dict(self, sd: dict) -> None:
        _ckpt.check_version(sd, "RolloutDriver.load_state_dict")
        odd = _ckpt.differing(sd["settings"], self._settings())
        if odd:
            raise ValueError(f"the saved driver's settings differ at {odd}: saved {sd['settings']}, here {self._settings()}")
        self.gen, self.seed = _ckpt.restore_generator(sd["generator"], self.updater.flat.device)

    # ---- train.py:134-140,249-251: critic over the T+1 frames of every environment, then the shifted GAE scan
    @torch.no_grad()
    def compute_advantages(self, buf: RolloutBuffer, next_last: Dict[str, torch.Tensor]) -> None:
        """``next_last``: observation groups of the frame after the last one, [N, 1, width].  Writes ``state_value``,
        ``advantage`` and ``value_target`` [N, T, 1] into the buffer."""
        critic = self.updater.loss_module.critic_network
        N, T = buf.N, buf.T
        vals = torch.empty(N, T + 1, device=buf.data["reward"].device, dtype=torch.float32)
        # all T frames of every environment as ONE time-batched critic call (policy.GNNVFNet._values_time_batched: the time steps are groups
        # of one launch set, statistics per step; data parallel: the per-step statistics of a chunk travel in one all-reduce per LayerNorm
        # stage -- two collectives per chunk, where the looped form issued two per time step), the frame after the last one as a second call
        vals[:, :T] = critic(*[buf.data[k] for k in self.spec.in_features], train=False).reshape(N, T)
        vals[:, T:] = critic(*[next_last[k] for k in self.spec.in_features], train=False).reshape(N, 1)
        adv, tgt = _agent.gae(buf.data["reward"].reshape(N, T), buf.data["done"].reshape(N, T), buf.data["terminated"].reshape(N, T),
                              vals, self.gamma, self.lmbda)
        buf.data["state_value"] = vals[:, :T].reshape(N, T, 1).contiguous()
        buf.data["advantage"] = adv.reshape(N, T, 1)
        buf.data["value_target"] = tgt.reshape(N, T, 1)

    def epoch_indices(self, N: int, T: int, device) -> torch.Tensor:
        """[T, N] int64 row indices into the flattened [N*T] rollout: row j = minibatch j."""
        self.gen = seeded_generator(self.gen, self.seed, device)
        return env_aligned_rows(N, T, self.gen, device)

    def epoch_minibatches(self, N: int, T: int, device):
        """List of int64 index tensors into the flattened [N*T] rollout, one per minibatch of this epoch."""
        mbs = self.mini_batch_size or N
        if self.sampling == "uniform":
            self.gen = seeded_generator(self.gen, self.seed, device)
            perm = torch.randperm(N * T, device=device, generator=self.gen)
            return [perm[i:i + mbs] for i in range(0, N * T - mbs + 1, mbs)]
        if mbs % N:
            raise ValueError(f"env-aligned sampling needs mini_batch_size ({mbs}) to be a multiple of the number of environments ({N})")
        k = mbs // N
        idx = self.epoch_indices(N, T, device)                    # [T, N]
        return [idx[j:j + k].reshape(-1) for j in range(0, T - k + 1, k)]   # k columns, column after column

    def publish_advantage_stats(self, buf: RolloutBuffer, idxs) -> None:
        """Data parallel: the batch normalisation of the advantages (trpl.py:248-252) needs the (sum, sum of squares) over ALL ranks'
        shares of a minibatch.  The minibatches of an epoch are known when it starts, so their statistics are reduced by ONE all-reduce
        per epoch ([n_minibatches, 2] fp64) instead of one per update, and written next to the advantages as a per-frame column
        ``adv_stats`` (every frame carries its minibatch's global sums): the update's row gather brings them along and the fused loss
        kernel reads row 0 -- no statistics kernel, no collective and no graph boundary for them inside the update
        (``PolicyUpdater._plan``).  Rebuilt at every epoch (the sampler reshuffles)."""
        upd = self.updater
        if upd.group is None or not upd.loss_module.normalize_advantage:
            return
        idx = torch.stack([i.reshape(-1) for i in idxs])                           # [n_mb, frames per rank]
        a = buf.flat("advantage").reshape(-1).double()[idx]
        s = torch.stack([a.sum(1), (a * a).sum(1)], dim=1).contiguous()
        upd.all_reduce_sum(s, "advantage_stats_epoch")
        if "adv_stats" not in buf.data:
            buf.data["adv_stats"] = torch.zeros(buf.N, buf.T, 2, device=s.device, dtype=torch.float64)
        buf.flat("adv_stats")[idx.reshape(-1)] = s.repeat_interleave(idx.shape[1], dim=0)

    def epochs(self, buf: RolloutBuffer) -> Iterator[list]:
        """Per PPO epoch the list of its minibatches' index tensors, their advantage statistics published (data parallel)."""
        dev = next(iter(buf.data.values())).device
        for _ in range(self.ppo_epochs):
            idxs = self.epoch_minibatches(buf.N, buf.T, dev)
            self.publish_advantage_stats(buf, idxs)
            yield idxs

    def minibatches(self, buf: RolloutBuffer) -> Iterator[torch.Tensor]:
        for idxs in self.epochs(buf):
            yield from idxs

    def run(self, buf: RolloutBuffer, next_last: Optional[Dict[str, torch.Tensor]] = None):
        """One rollout pass: [GAE] + ppo_epochs * T policy updates.  Returns the loss dict of the last update."""
        if next_last is not None:
            self.compute_advantages(buf, next_last)
        if self.updater.track_stats:
            self.updater.stats_reset()   # (the means iteration_log reports are those of THIS pass)
        out = None
        for idxs in self.epochs(buf):
            if idxs:   # one call per epoch (epoch_minibatches cuts one size): one rank with recorded lanes takes several steps per launch
                out = self.updater.run_minibatches(buf, torch.stack([i.reshape(-1) for i in idxs]))
        return out

    def iteration_log(self, buf: RolloutBuffer, episode_stats: Optional["EpisodeStats"] = None) -> Dict[str, float]:
        """The ``log_info`` of one training iteration (train.py:237-246, 318-333) after ``run``, as Python floats: ``train/<key>`` = the mean
        of every reported loss term over the pass's ppo_epochs x minibatches updates (``PolicyUpdater(track_stats=True).stats_read()``),
        ``train/explained_variance`` (+ ``_flat``: over all frames at once) of the buffer's state_value against value_target, ``train/lr``,
        ``train/clip_epsilon`` (PPO), ``train/kl_beta`` (KL-penalty PPO: the penalty weight the pass left behind), and ``train/reward`` / ``train/episode_length`` when ``episode_stats`` (the one ``collect`` scanned this
        rollout with) saw at least one finished episode -- omitted otherwise, as in train.py:239.  The host-side timing keys are the
        caller's.  Everything is enqueued first; the host then waits ONCE per call, not once per step."""
        upd = self.updater
        ev = explained_variance(buf.data["state_value"], buf.data["value_target"])
        means = upd.stats_read()                                   # (the synchronisation)
        log = {f"train/{k}": v for k, v in means.items() if k != "updates"}
        ev = ev.tolist()
        log.update({"train/explained_variance": ev[0], "train/explained_variance_flat": ev[1], "train/lr": upd.lr})
        log.update({f"train/{name}": float(t) for name, t in upd.loss_module.device_scalars.items()})
        if episode_stats is not None:
            ret, length, n = episode_stats.sums.tolist()
            if n > 0:
                log.update({"train/reward": ret / n, "train/episode_length": length / n})
        return log


class PolicyActor:
    """Collector-side actor: ``ProbabilisticActor(TensorDictModule(policy, in_keys, ["loc", "covariance_matrix"]),
    distribution_class=MultivariateNormal, return_log_prob=True, default_interaction_type=RANDOM)`` of
    examples/torchrl/builders/utils_algo_graph.py:146-158 -- one no-grad policy pass per environment step (train.py:114-123) with the
    same forward kernels as the update, followed by the sampling kernel.  ``__call__(obs)`` returns the keys the collector writes
    into the rollout: ``loc``, ``var`` (the diagonal of covariance_matrix), ``action``, ``sample_log_prob``.

    ``use_graph``: after the first call (which builds the cached topology and, on a fresh policy, calibrates the convolutions --
    the collector calls the module with its default ``train=True``, gnn_gaussian_policy_diag.py:65) the pass is recorded into a
    hipGraph and replayed on static input buffers.

    ``train``: the pass's ``train`` flag (True, as the collector's default call).  With the policy's training noise on, every pass -- every
    replay -- draws a fresh noise set from the actor's generator; ``train=False`` (evaluation) is noiseless."""

    def __init__(self, policy, spec, use_graph: bool = True, seed: int = 0, deterministic: bool = False, train: bool = True):
        self.policy, self.spec, self.use_graph, self.deterministic = policy, spec, use_graph, deterministic
        self.train = bool(train)
        self.gen, self.seed = None, seed
        self._graph, self._static, self._out, self._calls = None, None, None, 0
        self._resumed = False   # load_state_dict: the next call runs eagerly, like a first call (it may be the process's first)

    def state_dict(self) -> dict:
        """The sampling generator and the number of calls.  The policy's own state (weights, latches, noise words, topologies) is the
        updater's part of a training state."""
        return {"version": _ckpt.VERSION, "deterministic": bool(self.deterministic), "calls": int(self._calls),
                "generator": _ckpt.generator_state(self.gen, self.seed)}

    def load_state_dict(self, sd: dict) -> None:
        """Drops the one recorded graph and takes a NEW generator at the saved state (a generator that is registered with a capture is not
        reliably reseated).  The next call runs eagerly, as a first call does -- in a fresh process it IS the first: the latches are read,
        a missing topology is built, the noise words are made, none of which a capture allows -- and the call after it records again.
        Eager and replayed passes launch the same kernels on the same draws: the samples are those of the run that was not interrupted."""
        _ckpt.check_version(sd, "PolicyActor.load_state_dict")
        if sd["deterministic"] != bool(self.deterministic):
            raise ValueError(f"the saved actor was deterministic={sd['deterministic']}, this one is deterministic={self.deterministic}")
        dev = next(self.policy.parameters()).device
        self.gen, self.seed = _ckpt.restore_generator(sd["generator"], dev)
        self._graph, self._static, self._out = None, None, None
        self._calls, self._resumed = int(sd["calls"]), True

    def _pass(self, obs):
        loc, sigma = self.policy.forward_diag(*[obs[k] for k in self.spec.in_features], train=self.train)
        B, A = loc.shape
        eps = torch.zeros_like(loc) if self.deterministic else torch.randn(loc.shape, device=loc.device, dtype=loc.dtype, generator=self.gen)
        action, var = torch.empty_like(loc), torch.empty_like(loc)
        logp = torch.empty(B, device=loc.device, dtype=torch.float32)
        _hip.call("grl_gaussian_sample", loc.contiguous(), sigma.contiguous(), eps, action, logp, var, B, A)
        return {"loc": loc, "var": var, "action": action, "sample_log_prob": logp}

    @torch.no_grad()
    def __call__(self, obs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        dev = obs[self.spec.in_features[0]].device
        if self.gen is None and not self.deterministic:
            self.gen = torch.Generator(device=dev)
            self.gen.manual_seed(self.seed)
        self._calls += 1
        resumed, self._resumed = self._resumed, False
        if not self.use_graph or self._calls == 1 or resumed:
            return self._pass(obs)
        if self._graph is None:
            self._static = {k: obs[k].clone() for k in self.spec.in_features}

            def record():
                self._out = self._pass(self._static)
            self._graph = capture([record], generator=self.gen)
        for k in self.spec.in_features:
            self._static[k].copy_(obs[k])
        self._graph.replay()
        return self._out


def collect(env_step, first_obs: Dict[str, torch.Tensor], actor: PolicyActor, T: int, normalizer=None, episode_stats=None):
    """The data-collection half of one training iteration (train.py:114-123, 232-247) with everything on the device: for T steps the
    (optionally normalised) observation goes through the collector-side actor, the action into ``env_step(action) -> (next raw
    observation groups, reward [N], done [N] bool, terminated [N] bool)``; the frames are stacked into a ``RolloutBuffer`` [N, T, ...].
    Returns ``(buffer, next_last)`` as ``RolloutDriver.run`` takes them (``next_last``: the observation after the last step, [N, 1, width]).
    ``episode_stats``: an ``EpisodeStats`` -- its scan runs once over the stacked rollout and the buffer gains ``episode_reward`` and
    ``step_count`` [N, T, 1] (the collector-side RewardSum / StepCounter transforms)."""
    raw = first_obs
    frames = []
    for _ in range(T):
        obs = normalizer(raw) if normalizer is not None else raw
        out = actor(obs)
        rec = {k: v.clone() for k, v in obs.items()}
        rec.update({k: out[k].clone() for k in ("loc", "var", "action", "sample_log_prob")})
        raw, reward, done, terminated = env_step(out["action"])
        rec.update(reward=reward.reshape(-1, 1).float(), done=done.reshape(-1, 1), terminated=terminated.reshape(-1, 1))
        frames.append(rec)
    last = normalizer(raw, update=False) if normalizer is not None else raw
    data = {k: torch.stack([f[k] for f in frames], dim=1) for k in frames[0]}
    if episode_stats is not None:
        data["episode_reward"], data["step_count"] = episode_stats.scan(data["reward"], data["done"])
    return RolloutBuffer(data), {k: v.unsqueeze(1) for k, v in last.items()}
