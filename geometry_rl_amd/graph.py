"""Batched hetero point-cloud graphs for the HIP actor/critic: the MI355X-side counterpart of
``geometry_rl/modules/pyg_data/{base,rigid_tasks,cloth_tasks,rope_tasks}_data.py``.

Differences from the reference that do not change any output:
  * no PyG containers: a :class:`GraphBatch` is plain device tensors -- per node type a compact node list, per edge
    type an :class:`~geometry_rl_amd.ops.EdgeSet` (CSR by destination and by source, int32);
  * zero-padded object points (reference orbit/tasks/common/utils.py:193-211) are dropped from the ACTOR graph: they have
    no edges (rigid_tasks_data.py:285-287,313-319), so their latents never reach the actuator read-out.  The critic
    (DeepSets) still sees every padded point, exactly like the reference (deepsets.py:44-51);
  * edge attributes (HeteroCartesian/HeteroDistance, transforms.py:122-163) are not materialised: no model on the hot
    path reads them.
The topology is built once per batch size and reused for every later batch of that size, like the reference cache
(rigid_tasks_data.py:254-255).
"""
from dataclasses import dataclass, field, fields
from typing import Dict, List, Optional, Tuple

import torch

from . import hip, ops

EdgeType = Tuple[str, str, str]


@dataclass
class TaskSpec:
    family: str
    node_types: List[str]
    edge_types: List[EdgeType]
    edge_levels: List[str]
    obs_names: Dict[str, List[str]]
    obs_dims: Dict[str, List[int]]
    num_actuators: int
    knn_k: int = 3
    angular_velocity: bool = True
    n_vec: int = 4
    in_features: List[str] = field(default_factory=list)
    knn_to_actuators_k: int = -1   # > 0: task edges only from the k points nearest to each actuator (rigid_tasks_data.py:303-311)

    @property
    def actuator(self) -> str:
        return "grippers"


_IN6 = ["scalars", "position_vectors", "velocity_vectors", "norm_position_vectors", "norm_velocity_vectors", "infos"]


def rigid_spec(P=32, G=1, E_mesh=180, angular_velocity=True, object_velocity=True) -> TaskSpec:
    """rigid_tasks_data.py:21-48 + rigid_tasks/config/common_cfg/observations_cfg.py:143-192,254-273."""
    vel = ["grippers"] + (["grippers_angular"] if angular_velocity else [])
    if object_velocity:
        vel += ["object_geometry"] + (["object_geometry_angular"] if angular_velocity else [])
    return TaskSpec(
        "rigid", ["object_geometry", "grippers", "target_geometry"],
        [("object_geometry", "internal", "object_geometry"), ("grippers", "agent", "grippers"),
         ("object_geometry", "task", "grippers")], ["internal", "task", "agent"],
        {"scalars": ["object_target_distances"], "position_vectors": ["grippers", "object_geometry", "target_geometry"],
         "velocity_vectors": vel, "infos": ["object_num_points", "object_geometry_edges", "object_num_edges"]},
        {"scalars": [1], "position_vectors": [3 * G, 3 * P, 3 * P],
         "velocity_vectors": [3 * G if n.startswith("grippers") else 3 for n in vel], "infos": [1, 2 * E_mesh, 1]},
        G, angular_velocity=angular_velocity, n_vec=4, in_features=list(_IN6))


def cloth_spec(n_particles=225, n_hole=10, G=4, E_cloth=600) -> TaskSpec:
    """cloth_tasks_data.py:19-47 + cloth_tasks/config/common_cfg/observations_cfg.py:150-193."""
    return TaskSpec(
        "cloth", ["particles", "grippers", "hole_boundary", "target_hook"],
        [("hole_boundary", "internal", "hole_boundary"), ("grippers", "agent", "grippers"),
         ("hole_boundary", "task", "grippers")], ["internal", "task", "agent"],
        {"scalars": ["hole_target_distances", "cloth_edges_length"],
         "position_vectors": ["grippers", "particles", "init_particles", "hole_boundary", "target_hook"],
         "velocity_vectors": ["grippers", "particles"]},
        {"scalars": [n_hole, E_cloth], "position_vectors": [3 * G, 3 * n_particles, 3 * n_particles, 3 * n_hole, 3],
         "velocity_vectors": [3 * G, 3 * n_particles]},
        G, n_vec=3, in_features=_IN6[:5])


def rope_spec(n_links=80, G=2, variable_length=False) -> TaskSpec:
    """rope_tasks_data.py:21-46 + rope_tasks/config/common_cfg/observations_cfg.py:131-160.

    ``variable_length`` (BASELINE config 5; not in the reference, which requires equal rope sizes within a batch,
    rope_tasks_data.py:127): an extra ``infos`` group carries ``links_num_points`` [B,1]; links / target points beyond that count are
    zero padding, treated exactly like the rigid tasks' padded object points -- no edges, dropped from the actor graph, still summed by
    the DeepSets critic.  No reference fixture can pin this form (tests/golden/tier3_*: the reference's rope builder connects all links);
    it is held to its oracle tests alone."""
    spec = _rope_spec(n_links, G)
    if variable_length:
        spec.obs_names["infos"], spec.obs_dims["infos"] = ["links_num_points"], [1]
        spec.in_features = list(_IN6)
    return spec


def _rope_spec(n_links=80, G=2) -> TaskSpec:
    return TaskSpec(
        "rope", ["links", "grippers", "target_geometry"],
        [("links", "internal", "links"), ("grippers", "agent", "grippers"), ("links", "task", "grippers")],
        ["internal", "task", "agent"],
        {"scalars": ["links_target_distances"], "position_vectors": ["grippers", "links", "target_geometry"],
         "velocity_vectors": ["grippers", "links"]},
        {"scalars": [1], "position_vectors": [3 * G, 3 * n_links, 3 * n_links], "velocity_vectors": [3 * G, 3 * n_links]},
        G, n_vec=3, in_features=_IN6[:5])


@dataclass
class GraphBatch:
    """What ``build_data`` hands to ``gnn.one_step`` (the reference passes a PyG HeteroData batch)."""
    batch_size: int
    node_types: List[str]
    num_nodes: Dict[str, int]
    pos: Dict[str, torch.Tensor]  # raw positions [N_t, 3] (invariants use un-normalised positions, hepi.py:148-149)
    edges: Dict[EdgeType, "ops.EdgeSet"]
    output_mask_key: Optional[str]
    nodes_per_sample: Dict[str, int]
    compact: bool  # True: padded points removed (actor graph)
    # the per-type position / vector / one-hot tensors are views of ONE buffer each, node types in ``all_order`` (the read-out type last):
    # a homogeneous model (EMPN: ponita_gcn.py:73-83 flattens the hetero batch into one graph) reads them without a concatenation
    all_order: Optional[List[str]] = None
    pos_all: Optional[torch.Tensor] = None      # [N_all, 3]
    vec_all: Optional[torch.Tensor] = None      # [N_all, n_vec, 3]
    scalar_all: Optional[torch.Tensor] = None   # [N_all, n_types] (one-hot node type)
    # The compact numbering of the main node type is an implementation choice (balanced_node_order renumbers it for the edge backward's load
    # balance): natural_id[t][i] = the node's index in the NATURAL order (sample after sample, valid points in their order), None = identity.
    natural_id: Optional[Dict[str, torch.Tensor]] = None

    def natural(self, node_type: str, ids: torch.Tensor) -> torch.Tensor:
        """Node ids of ``node_type`` in the natural numbering (what the reference's batched graph uses)."""
        m = (self.natural_id or {}).get(node_type)
        return ids if m is None else m.to(ids.device)[ids.long()]

    @property
    def edge_types(self):
        return list(self.edges.keys())


_MASK64 = (1 << 64) - 1


def _signed64(x: int) -> int:
    x &= _MASK64
    return x - (1 << 64) if x >> 63 else x


def _mix64(x: int) -> int:
    """splitmix64's finaliser: a 64-bit seed from a small integer."""
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


BALANCE_NODE_ORDER = True   # module attribute, not environment: tests flip it


def balanced_node_order(src: torch.Tensor, n_nodes: int, slots: int, group: int = 8):
    """A renumbering of ``n_nodes`` nodes with out-edges ``src`` (node id per edge) and node boundaries ``split`` [slots + 1] of the NEW order
    such that slot s = nodes split[s] .. split[s+1] carries ~E / slots edges.  The natural order is cut into windows of ``group`` slots'
    worth of edges (contiguous: a window is a few neighbouring frames, neighbours stay near each other in memory); inside a window the nodes
    are dealt to its ``group`` slots largest out-degree first, each to the least loaded slot (ties: the lower slot) -- longest-processing-time
    packing; nodes without out-edges go round-robin.  -> (new_of_old int64 [n_nodes], split int32 [slots + 1]), both on the CPU; a pure
    function of its arguments."""
    import heapq
    deg = torch.bincount(src.reshape(-1).cpu(), minlength=n_nodes).tolist()
    E = sum(deg)
    n_groups = max(1, slots // group)
    per_group = E / n_groups
    new_of_old = [0] * n_nodes
    split = [0]
    nxt, node, cum = 0, 0, 0
    for g in range(n_groups):
        n_bins = group if g < n_groups - 1 else slots - group * (n_groups - 1)
        first = node
        if g == n_groups - 1:
            node = n_nodes
        else:
            while node < n_nodes and cum + deg[node] <= (g + 1) * per_group + 1e-9:
                cum += deg[node]
                node += 1
        members = list(range(first, node))
        bins = [[] for _ in range(n_bins)]
        heap = [(0, b) for b in range(n_bins)]
        rr = 0
        for n_ in sorted(members, key=lambda i: (-deg[i], i)):
            if deg[n_] == 0:
                bins[rr % n_bins].append(n_)
                rr += 1
                continue
            load, b = heapq.heappop(heap)
            bins[b].append(n_)
            heapq.heappush(heap, (load + deg[n_], b))
        for bin_ in bins:
            for n_ in sorted(bin_):          # (natural order inside a slot: neighbouring rows stay neighbours)
                new_of_old[n_] = nxt
                nxt += 1
            split.append(nxt)
    assert nxt == n_nodes and len(split) == slots + 1
    return torch.tensor(new_of_old, dtype=torch.int64), torch.tensor(split, dtype=torch.int32)


class HyperData:
    """Mirror of RigidTasksData / ClothTasksData / RopeTasksData (constructor kwargs of rigid_tasks_data.py:53-67).

    ``build_data(*obs, train)`` returns ``(graph, input_vector)`` with ``input_vector`` either
    ``(scalar_dict, vector_dict)`` (concat_input_vector=False, actor) or the dense critic input ``[B, n_all, d]``
    (concat_input_vector=True; the reference returns the per-type dict that DeepSets concatenates, deepsets.py:41-49)."""

    def __init__(self, spec: TaskSpec, *, full_graph_obs=False, dist_as_pos=False, output_mask_key=None, training_noise=False,
                 training_noise_std=1e-2, concat_input_vector=True, drop_padding=True, noise_seed=None, **ignored):
        self.spec = spec
        # training noise (rigid_tasks_data.py:178-214, rope_tasks_data.py:168-186): N(0, std^2) on the input vectors of every build_data with
        # train=True, drawn on the device by the feature launch itself (csrc/grl_feat.h) -- see _noise_words for which slots.  cloth: the flag
        # is accepted and changes nothing, as upstream (cloth_tasks_data.py adds no noise).  DELIBERATE DEVIATION: upstream adds the noise in
        # place (``pos_vec += ...``), which writes into the caller's observation tensor where a reshape is a view (a group of one term); the
        # kernel never writes its inputs.
        self.training_noise, self.training_noise_std = bool(training_noise), float(training_noise_std)
        self._noise_on = self.training_noise and spec.family != "cloth"
        if noise_seed is None:   # from torch's initial seed (torch.manual_seed before construction reproduces a run; no draw is consumed)
            noise_seed = _mix64(torch.initial_seed() ^ (int(dist_as_pos) << 1 | int(concat_input_vector) << 2 | int(full_graph_obs) << 3))
        self._noise_host = (int(noise_seed) & _MASK64, 0)   # (seed, draw) until the device state exists
        self._noise_dev = None        # device int64[4] = uint64 {seed, draw, ticket, unused}, allocated by the first noisy build_data
        self._noise_advance = True    # False: the launches read the draw and leave it (policy.GNNGaussianPolicyDiag's calibrating pass)
        self._noise_rank = None
        self.full_graph_obs = full_graph_obs
        self.dist_as_pos = dist_as_pos
        self._output_mask_key = output_mask_key
        self.concat_input_vector = concat_input_vector
        self.drop_padding = drop_padding and not concat_input_vector
        fam = spec.family
        if fam == "rigid":
            self.node_type_list = [t for t in spec.node_types if t != "target_geometry"]
        elif fam == "cloth":
            keep = [t for t in spec.node_types if t != "target_hook"]
            self.node_type_list = keep if full_graph_obs else [t for t in keep if t != "particles"]
        else:
            self.node_type_list = list(spec.node_types)
        self._cache = {}
        self.bump_next = None   # one-shot: a device int32[1] the NEXT build_data's feature launch advances by one (PolicyUpdater: step count)
        self.check_topology_always = False   # debugging: True = every eager build_data re-validates the cached topology (one device sync each)

    # ---- training noise: the device-side generator state {seed, draw}
    def _noise_state_tensor(self, dev) -> torch.Tensor:
        if self._noise_dev is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HyperData: the noise state must exist before a capture (run one eager build_data with train=True first)")
            seed, draw = self._noise_host
            self._noise_dev = torch.tensor([_signed64(seed), _signed64(draw), 0, 0], dtype=torch.int64, device=dev)
        return self._noise_dev

    def noise_state(self):
        """(seed, draw) of the training-noise generator: the next noisy feature launch draws with these (one device sync)."""
        if self._noise_dev is None:
            return self._noise_host
        seed, draw = self._noise_dev[:2].tolist()
        return seed & _MASK64, draw & _MASK64

    def set_noise_state(self, seed: int, draw: int = 0) -> None:
        """Put the generator at (seed, draw): stream-ordered behind the work already enqueued (one host-to-device copy)."""
        self._noise_host = (int(seed) & _MASK64, int(draw) & _MASK64)
        if self._noise_dev is not None:
            self._noise_dev.copy_(torch.tensor([_signed64(self._noise_host[0]), _signed64(self._noise_host[1]), 0, 0], dtype=torch.int64))

    def fold_noise_rank(self, rank: int) -> None:
        """Data parallel: rank r > 0 draws from its own stream (key = mix(seed, r)); rank 0 keeps the key.  Applied once per HyperData."""
        if not rank or self._noise_rank is not None:
            return
        self._noise_rank = rank
        seed, draw = self.noise_state()
        self.set_noise_state(_mix64(seed ^ _mix64(rank)), draw)

    def share_noise(self, other: "HyperData", advance: bool) -> None:
        """Draw from ``other``'s generator state (same device words); ``advance`` False: this object's launches only read the draw."""
        self._noise_on = other._noise_on
        self.training_noise, self.training_noise_std = other.training_noise, other.training_noise_std
        self._noise_host, self._noise_dev, self._noise_advance = other._noise_host, other._noise_dev, advance

    def _noise_words(self, t, n_t, B):
        """Noise word per vector slot of node type t (include/grl_hip.h grl_build_features_noise), the rules of rigid_tasks_data.py:178-214 /
        rope_tasks_data.py:168-186: the position always; ``corr`` only for the type that has a target (with dist_as_pos its value is computed
        from the NOISY position: the position's noise is added as well); ``vel`` / ``ang`` only for types with a velocity observation --
        ``ang`` even without an angular velocity (upstream adds noise to its zeros); everything else stays exact."""
        spec = self.spec
        has_vel = t in spec.obs_names["velocity_vectors"]
        terms = self._feature_terms(t, n_t)
        head = (spec.node_types.index(t) << 24) | (spec.n_vec << 16) | (B << 32)
        words = []
        for v, (ta, _tb) in enumerate(terms):
            if v == 0:
                on, pos_too = True, False
            elif v == 1:
                on, pos_too = ta is not None, ta is not None and self.dist_as_pos
            else:
                on, pos_too = has_vel, False
            words.append(_signed64(head | (v << 8) | (2 if pos_too else 0) | 1) if on else 0)
        return words

    # ---- cached topology: invariant and guards
    def reset_cache(self):
        """Forget the cached topologies.  INVARIANT of the cache (the reference's, rigid_tasks_data.py:254-255, keyed on the batch
        size alone): every later batch of a cached size has the same per-row point counts -- and is expected to have the same
        neighbourhoods -- as the batch the topology was built from, i.e. row i of every minibatch of that size belongs to the
        same environment (``rollout.RolloutDriver`` samples env-aligned for exactly this reason).  Call this before feeding a batch
        of a cached size that breaks the invariant (another env set, shuffled rows, another data-parallel shard offset)."""
        self._cache.clear()

    # ---- cached topology as training state (checkpoint.py).  The kNN neighbourhoods of a size are those of the FIRST batch of that size (the
    #      invariant above): a run continued in a fresh process would build them from whichever minibatch it meets first, and every later
    #      update would walk other edges than the run that was never interrupted.
    def _topology_reads_positions(self) -> bool:
        """Does a cached topology depend on more than the per-row point counts?  Not for a dense (critic) object, which builds no edges, nor
        for cloth's fully connected hole boundary without nearest-point task edges: those rebuild bit for bit from any env-aligned batch."""
        if self.concat_input_vector:
            return False
        return self.spec.family != "cloth" or getattr(self.spec, "knn_to_actuators_k", -1) > 0

    def topology_state(self) -> dict:
        """{batch size: the cached topology as CPU tensors and plain values} of every size whose topology was built from a batch's
        positions ({} where none is: ``_topology_reads_positions``).  What ``build_data`` derives lazily (``all_order`` ...) is left out."""
        if not self._topology_reads_positions():
            return {}
        cpu = lambda v: v.detach().cpu() if torch.is_tensor(v) else v
        out = {}
        for B, topo in self._cache.items():
            edges = {self.spec.edge_types.index(et): {f.name: cpu(getattr(es, f.name)) for f in fields(es)} for et, es in topo["edges"].items()}
            nat = topo.get("natural_id")
            out[int(B)] = dict(n_per=dict(topo["n_per"]), main=topo["main"], gather_main=cpu(topo["gather_main"]), n_main=int(topo["n_main"]),
                               edges=edges, G=int(topo["G"]), n_valid=cpu(topo["n_valid"]), permuted=bool(topo.get("permuted", False)),
                               natural_id=None if nat is None else cpu(nat[topo["main"]]))
        return out

    def topology_mismatch(self, state: dict) -> Optional[str]:
        """A saved topology against the one already cached for its size: None where none is cached or they are the same edges; else what
        differs.  A cached topology is never replaced (recorded programs read its arrays): ``reset_cache()`` first."""
        for B, s in state.items():
            topo = self._cache.get(int(B))
            if topo is None:
                continue
            same = (torch.equal(topo["gather_main"].cpu(), s["gather_main"])
                    and {self.spec.edge_types.index(et) for et in topo["edges"]} == set(s["edges"])
                    and all(torch.equal(es.src_d.cpu(), s["edges"][self.spec.edge_types.index(et)]["src_d"])
                            and torch.equal(es.rowptr_d.cpu(), s["edges"][self.spec.edge_types.index(et)]["rowptr_d"])
                            for et, es in topo["edges"].items()))
            if not same:
                return (f"the topology cached for batch size {B} has other nodes or edges than the saved one (it was built from another "
                        "first batch): call reset_cache() on the data object and reset_graph() on the updater before loading")
        return None

    def load_topology_state(self, state: dict, device) -> None:
        """Install the saved topologies of the sizes that have none cached (``topology_mismatch`` has compared the others)."""
        dev = torch.device(device)
        to = lambda v: v.to(dev) if torch.is_tensor(v) else v
        n_types = len(self.spec.node_types)
        for B, s in state.items():
            if int(B) in self._cache:
                continue
            main, n_per = s["main"], dict(s["n_per"])
            edges = {self.spec.edge_types[i]: ops.EdgeSet(**{k: to(v) for k, v in es.items()}) for i, es in s["edges"].items()}
            one_hot = {}
            for t in self.node_type_list:
                oh = torch.zeros(s["n_main"] if t == main else int(B) * n_per[t], n_types, device=dev)
                oh[:, self.spec.node_types.index(t)] = 1
                one_hot[t] = oh
            self._cache[int(B)] = dict(n_per=n_per, main=main, gather_main=to(s["gather_main"]), n_main=s["n_main"], edges=edges, one_hot=one_hot,
                                       G=s["G"], n_valid=to(s["n_valid"]), permuted=s["permuted"],
                                       natural_id=None if s["natural_id"] is None else {main: to(s["natural_id"])})

    def check_topology(self, *args) -> None:
        """Raise if the batch's per-row valid point counts differ from those the cached topology of this batch size was built
        from (padded points are DROPPED from the actor graph according to the cached counts, so a mismatch silently mis-assigns
        nodes).  One device->host sync: called by PolicyUpdater when it records the step, by every eager build when
        ``check_topology_always`` is set, never inside a replayed graph."""
        obs = dict(zip(self.spec.in_features, args))
        B = obs["scalars"].shape[0]
        topo = self._cache.get(B)
        count_name = {"rigid": "object_num_points", "rope": "links_num_points"}.get(self.spec.family)
        if topo is None or count_name not in self.spec.obs_names.get("infos", []):
            return
        names, dims = self.spec.obs_names["infos"], self.spec.obs_dims["infos"]
        off = sum(dims[:names.index(count_name)])
        P = topo["n_per"][topo["main"]]
        now = obs["infos"][:, off].reshape(B).long().clamp(max=P)
        if not torch.equal(now, topo["n_valid"]):
            bad = int((now != topo["n_valid"]).sum())
            raise RuntimeError(f"HyperData: {bad} of {B} rows have a different {count_name} than the batch the cached topology "
                               "of this batch size was built from; call reset_cache() (see its docstring for the invariant)")

    # ---- observation split (rigid_tasks_data.py:93-150)
    def _split(self, obs: Dict[str, torch.Tensor]):
        B = obs["scalars"].shape[0]
        out = {}
        for group, x in obs.items():
            base = group.replace("norm_", "")
            if base not in self.spec.obs_dims:
                continue
            parts = torch.split(x, self.spec.obs_dims[base], dim=1)
            out[group] = {name: (p.reshape(B, -1, 3) if "vectors" in group else p)
                          for name, p in zip(self.spec.obs_names[base], parts)}
        return out

    # ---- topology (cached per batch size)
    def _topology(self, split, B: int, dev):
        key = B
        if key in self._cache:
            return self._cache[key]
        spec = self.spec
        posv = split["position_vectors"]
        n_per = {t: posv[t].shape[1] for t in self.node_type_list}
        G = n_per["grippers"]
        main = spec.edge_types[0][0]  # particle-like node type carrying the internal edges
        P = n_per[main]
        if spec.family == "rigid":
            n_valid = split["infos"]["object_num_points"].reshape(B).long().clamp(max=P)
        elif "links_num_points" in split.get("infos", {}):   # variable-length ropes
            n_valid = split["infos"]["links_num_points"].reshape(B).long().clamp(max=P)
        else:
            n_valid = torch.full((B,), P, dtype=torch.long, device=dev)
        ar = torch.arange(P, device=dev)
        valid = ar[None, :] < n_valid[:, None]  # [B,P]
        if self.drop_padding:
            offset = torch.cumsum(n_valid, 0) - n_valid  # compact id of (b, 0)
            gather_main = torch.nonzero(valid.reshape(-1)).reshape(-1)  # index into [B*P]
        else:
            offset = torch.arange(B, device=dev) * P
            gather_main = torch.arange(B * P, device=dev)
        n_main = int(gather_main.numel())
        b_of = torch.arange(B, device=dev)[:, None].expand(B, P)[valid]  # sample of every valid point
        j_of = ar[None, :].expand(B, P)[valid]
        cid = offset[b_of] + j_of  # compact id of every valid point
        edges = {}
        et_int, et_agent, et_task = spec.edge_types
        need_edges = not self.concat_input_vector  # the DeepSets critic never reads the edges
        # internal edges
        if not need_edges:
            pass
        elif spec.family == "cloth":  # fully connected hole boundary (cloth_tasks_data.py:252-260)
            jj, kk = torch.meshgrid(ar, ar, indexing="ij")
            m = jj != kk
            src = (offset[:, None] + jj[m][None, :]).reshape(-1)
            dst = (offset[:, None] + kk[m][None, :]).reshape(-1)
        else:  # kNN among the valid points (rigid_tasks_data.py:285-287, rope_tasks_data.py:251)
            k = spec.knn_k
            nbr = torch.empty(B, P, k, dtype=torch.int32, device=dev)
            hip.call("grl_knn_topology", posv[main].contiguous().float(), n_valid.int().contiguous(), nbr, B, P, k)
            nb = nbr.long()[valid]  # [n_valid_total, k]
            ok = nb >= 0
            src = (offset[b_of][:, None] + nb)[ok]
            dst = cid[:, None].expand_as(nb)[ok]
        split_s_int = None
        if need_edges and et_int[0] in self.node_type_list and self.drop_padding and BALANCE_NODE_ORDER and spec.family != "cloth" and src.numel():
            # The compact numbering of the main node type is ours to choose (every consumer reads it through gather_main / the edge arrays):
            # renumber the nodes -- inside windows of a few frames -- so that the wave slots of the fused edge backward, which walk CONTIGUOUS
            # node ranges of the source-sorted CSR, carry equal numbers of edges.  kNN out-degrees vary 0 .. 10: cutting the natural order at
            # node boundaries leaves the slowest wave 25 % over the mean at a 512-frame shard (30 passes for 24), and a one-wave-per-SIMD
            # kernel runs as long as its slowest wave (balanced_node_order).  A function of the topology alone: results stay reproducible.
            slots = 4 * hip.query("grl_edge_bwd_blocks", src.numel())
            new_of_old, split_s_int = balanced_node_order(src, n_main, slots)
            new_of_old = new_of_old.to(dev)
            src, dst, cid = new_of_old[src], new_of_old[dst], new_of_old[cid]
            old_of_new = torch.empty_like(new_of_old)
            old_of_new[new_of_old] = torch.arange(n_main, device=dev)
            gather_main = gather_main[old_of_new]
            split_s_int = split_s_int.to(dev)
        else:
            new_of_old = old_of_new = None
        if need_edges and et_int[0] in self.node_type_list:
            edges[et_int] = ops.build_edge_set(torch.stack([src, dst]), n_main, n_main, split_s=split_s_int)
        # agent edges: j != k among the actuators of a sample
        if not need_edges:
            pass
        elif G > 1:
            gj, gk = torch.meshgrid(torch.arange(G, device=dev), torch.arange(G, device=dev), indexing="ij")
            m = gj != gk
            base = (torch.arange(B, device=dev) * G)[:, None]
            edges[et_agent] = ops.build_edge_set(torch.stack([(base + gj[m][None]).reshape(-1), (base + gk[m][None]).reshape(-1)]),
                                                 B * G, B * G)
        else:
            edges[et_agent] = None  # empty edge set: the conv is skipped (hetero_fiber_conv.py:48-49)
        # task edges: every valid point -> every actuator of its sample; with knn_to_actuators_k > 0 only the k valid points
        # nearest to each actuator (rope_tasks_data.py / cloth_tasks_data.py: torch_geometric.nn.knn(points[:n], actuator[None], k).flip(0)).
        # DELIBERATE DEVIATION for family "rigid": the reference's rigid builder computes the same kNN (rigid_tasks_data.py:303-311) but its
        # edge_index assignment sits in the else branch (:319), so with k > 0 it never sets these edges; here all families follow the
        # rope / cloth semantics.  No BASELINE config sets k > 0.
        kta = getattr(spec, "knn_to_actuators_k", -1)
        if need_edges and et_task[0] in self.node_type_list and kta > 0:
            pm, pg = posv[main].float(), posv["grippers"].float()                      # [B,P,3], [B,G,3]
            d2 = ((pm[:, None, :, :] - pg[:, :, None, :]) ** 2).sum(-1)                 # [B,G,P]
            d2 = d2.masked_fill(~valid[:, None, :], float("inf"))
            kk = min(kta, P)
            order = torch.argsort(d2, dim=-1, stable=True)[..., :kk]                    # ties: lower index first
            ok = torch.gather(d2, -1, order) < float("inf")                             # fewer than k valid points: the valid ones only (as PyG knn)
            src = (offset[:, None, None] + order)[ok]
            if new_of_old is not None:
                src = new_of_old[src]
            dst = (torch.arange(B, device=dev)[:, None, None] * G + torch.arange(G, device=dev)[None, :, None]).expand_as(order)[ok]
            edges[et_task] = ops.build_edge_set(torch.stack([src, dst]), n_main, B * G)
        elif need_edges and et_task[0] in self.node_type_list:
            src = cid[:, None].expand(-1, G).reshape(-1)
            dst = (b_of[:, None] * G + torch.arange(G, device=dev)[None, :]).reshape(-1)
            edges[et_task] = ops.build_edge_set(torch.stack([src, dst]), n_main, B * G)
        n_types = len(spec.node_types)
        one_hot = {}
        for t in self.node_type_list:
            n_t = n_main if t == main else B * n_per[t]
            oh = torch.zeros(n_t, n_types, device=dev)
            oh[:, spec.node_types.index(t)] = 1  # transforms.py:52-66
            one_hot[t] = oh
        topo = dict(n_per=n_per, main=main, gather_main=gather_main, n_main=n_main, edges={k: v for k, v in edges.items() if v is not None},
                    one_hot=one_hot, G=G, n_valid=n_valid, permuted=new_of_old is not None,
                    natural_id=({main: old_of_new} if new_of_old is not None else None))
        self._cache[key] = topo
        return topo

    def _slice(self, obs, group, name):
        """(group tensor, row stride, column offset, vectors per sample) of one named observation inside its group."""
        base = group.replace("norm_", "")
        names, dims = self.spec.obs_names[base], self.spec.obs_dims[base]
        i = names.index(name)
        x = obs[group]
        return x, x.shape[1], sum(dims[:i]), dims[i] // 3

    def _feature_terms(self, t, n_t):
        """[(A, B)] per vector slot of node type t, A / B = (group, name) or None; the value is A - B
        (rigid_tasks_data.py:150-250, cloth_tasks_data.py:150-240, rope_tasks_data.py:150-235)."""
        spec = self.spec
        NP, NV = "norm_position_vectors", "norm_velocity_vectors"
        has_vel = lambda name: name in spec.obs_names["velocity_vectors"]
        corr = lambda target: ((NP, t), (NP, target)) if self.dist_as_pos else ((NP, target), None)
        fam = spec.family
        if fam == "rigid":
            c = corr("target_geometry") if t == "object_geometry" else (None, None)
            vel = ((NV, t), None) if has_vel(t) else (None, None)
            ang = ((NV, f"{t}_angular"), None) if (has_vel(t) and spec.angular_velocity) else (None, None)
            return [((NP, t), None), c, vel, ang]
        if fam == "cloth":
            if t == "particles":
                c = corr("init_particles")
            elif t == "hole_boundary":
                c = corr("target_hook")
            else:
                c = (None, None)
            return [((NP, t), None), c, ((NV, t), None) if has_vel(t) else (None, None)]
        c = corr("target_geometry") if t == "links" else (None, None)
        return [((NP, t), None), c, ((NV, t), None) if has_vel(t) else (None, None)]

    def build_data(self, *args, train=True, **kw):
        """rigid_tasks_data.py / base_data.py:45-55.  Positional obs tensors in ``spec.in_features`` order.  All node features
        (and the raw positions) are written by ONE launch of ``grl_build_features``; with ``train`` and training noise on, that launch
        (``grl_build_features_noise``) also adds the noise of the generator's current draw and advances the draw."""
        spec = self.spec
        obs = {k: (v if v.dtype == torch.float32 and v.is_contiguous() else v.float().contiguous())
               for k, v in zip(spec.in_features, args)}
        B = obs["scalars"].shape[0]
        dev = obs["scalars"].device
        with torch.no_grad():
            topo = self._cache.get(B)
            if topo is None:
                topo = self._topology(self._split(obs), B, dev)
            elif self.check_topology_always and not torch.cuda.is_current_stream_capturing():
                self.check_topology(*[obs[k] for k in spec.in_features])
            main, gm = topo["main"], topo["gather_main"]
            full = topo["n_main"] == B * topo["n_per"][main] and not topo.get("permuted", False)   # (identity numbering: no gather needed)
            n_types, n_vec = len(spec.node_types), spec.n_vec
            d = n_types + 3 * n_vec
            n_total = sum(topo["n_per"][t] for t in self.node_type_list)
            dense = self.concat_input_vector
            x_dense = torch.empty(B, n_total, d, device=dev, dtype=torch.float32) if dense else None
            graph_pos, scalar_dict, vector_dict = {}, {}, {}
            words = []
            noisy = train and self._noise_on
            nwords = [] if noisy else None

            def term(tn, n_t):
                if tn is None:
                    return 0, 0, 0, 0
                xg, stride, off, n_src = self._slice(obs, *tn)
                return xg.data_ptr(), stride, off, int(n_src == 1 and n_t > 1)

            row_off = 0
            pos_all = vec_all = None
            if not dense:   # one buffer per quantity, node types in all_order (read-out type last); the per-type tensors are views
                order = topo.get("all_order")
                if order is None:
                    ro = self._output_mask_key
                    order = topo["all_order"] = [t for t in self.node_type_list if t != ro] + ([ro] if ro in self.node_type_list else [])
                    topo["scalar_all"] = torch.cat([topo["one_hot"][t] for t in order], 0).contiguous()
                    o_, offs = 0, {}
                    for t in order:
                        offs[t] = o_
                        o_ += topo["n_main"] if t == main else B * topo["n_per"][t]
                        topo["one_hot"][t] = topo["scalar_all"][offs[t]:o_]
                    topo["all_off"], topo["n_all"] = offs, o_
                pos_all = torch.empty(topo["n_all"], 3, device=dev, dtype=torch.float32)
                vec_all = torch.empty(topo["n_all"], n_vec, 3, device=dev, dtype=torch.float32)
            for t in self.node_type_list:
                n_t = topo["n_per"][t]
                gather = gm.data_ptr() if (t == main and not full) else 0
                n_nodes = topo["n_main"] if t == main else B * n_t
                if not dense:
                    o0 = topo["all_off"][t]
                    graph_pos[t] = pos_all[o0:o0 + n_nodes]
                    vector_dict[t] = vec_all[o0:o0 + n_nodes]
                    scalar_dict[t] = topo["one_hot"][t]
                    pa = term(("position_vectors", t), n_t)
                    words += [graph_pos[t].data_ptr(), pa[0], 0, gather, 3, 0, 0, 0, n_nodes, n_t, pa[1], pa[2], pa[3], 0, 0, 0, -1, 0]
                    if noisy:
                        nwords.append(0)   # (raw positions: geometry, never noisy)
                terms = self._feature_terms(t, n_t)
                assert len(terms) == n_vec
                if noisy:
                    nwords += self._noise_words(t, n_t, B)
                for v, (ta, tb) in enumerate(terms):
                    A, Bt = term(ta, n_t), term(tb, n_t)
                    if dense:
                        out, rs, col, rps, ro = x_dense.data_ptr(), d, n_types + 3 * v, n_total, row_off
                        onehot = spec.node_types.index(t) if v == 0 else -1
                    else:
                        out, rs, col, rps, ro, onehot = vector_dict[t].data_ptr(), 3 * n_vec, 3 * v, 0, 0, -1
                    words += [out, A[0], Bt[0], gather, rs, col, rps, ro, n_nodes, n_t, A[1], A[2], A[3], Bt[1], Bt[2], Bt[3], onehot,
                              n_types]
                row_off += n_t
            n_desc = len(words) // 18
            # kw["bump"]: optional device int32[1] advanced by this launch (PolicyUpdater: the optimizer's step count of the recorded step)
            bump = kw.get("bump")
            if bump is None and self.bump_next is not None:
                bump, self.bump_next = self.bump_next, None
            from . import ops
            # noise: (host noise words, device state, std, advance) -- the draw advances by one per launch, in stream order
            noise = None
            if noisy:
                noise = (nwords, self._noise_state_tensor(dev), self.training_noise_std, int(self._noise_advance))
            if ops.HEAD is not None and ops.HEAD.feat is None:   # rides in the merged head launch of this forward (ops.HeadLaunch)
                ops.HEAD.feat = (words, n_desc, bump, noise)
            elif noise is not None:
                hip.call("grl_build_features_noise", words, n_desc, bump, *noise)
            else:
                hip.call("grl_build_features_bump", words, n_desc, bump)
            self._keepalive = obs  # the launch reads these buffers asynchronously
            graph = GraphBatch(B, list(self.node_type_list), {t: (topo["n_main"] if t == main else B * topo["n_per"][t])
                                                              for t in self.node_type_list}, graph_pos,
                               topo["edges"], self._output_mask_key, topo["n_per"], self.drop_padding,
                               topo.get("all_order"), pos_all, vec_all, topo.get("scalar_all"), topo.get("natural_id"))
            if dense:
                return graph, x_dense
            return graph, (scalar_dict, vector_dict)


# ---------------------------------------------------------------------------------------------------- reference constructors
# The reference builds its data objects from the environment's observation manager (builders/utils_algo_graph.py:79-110):
#   RigidTasksData(observation_dim=env.observation_manager.group_obs_term_dim, observation_names=..._term_names, full_graph_obs=...,
#                  dist_as_pos=..., output_mask_key=..., training_noise=..., concat_input_vector=..., angular_velocity=..., knn_k=...,
#                  knn_to_actuators_k=...)                                   (rigid_tasks_data.py:53-67; cloth :51-62; rope :51-63)
# ``observation_dim``: {group: [shape tuple per term]} (only shape[0] is read, rigid_tasks_data.py:82), ``observation_names``:
# {group: [term name per term]}.  The classes below take exactly those kwargs and derive the TaskSpec from them.
_FAMILY = {
    "rigid": dict(node_types=["object_geometry", "grippers", "target_geometry"], main="object_geometry", n_vec=4,
                  edge_types=[("object_geometry", "internal", "object_geometry"), ("grippers", "agent", "grippers"),
                              ("object_geometry", "task", "grippers")], in_features=list(_IN6)),
    "cloth": dict(node_types=["particles", "grippers", "hole_boundary", "target_hook"], main="hole_boundary", n_vec=3,
                  edge_types=[("hole_boundary", "internal", "hole_boundary"), ("grippers", "agent", "grippers"),
                              ("hole_boundary", "task", "grippers")], in_features=_IN6[:5]),
    "rope": dict(node_types=["links", "grippers", "target_geometry"], main="links", n_vec=3,
                 edge_types=[("links", "internal", "links"), ("grippers", "agent", "grippers"), ("links", "task", "grippers")],
                 in_features=_IN6[:5]),
}


EDGE_LEVELS = ["internal", "task", "agent"]


def family_types(family: str):
    """(node types, edge types, edge levels) of a task family: the members of the reference's ``NodeType`` / ``EdgeType`` / ``EdgeLevel``
    classes of ``pyg_data/<family>_tasks_data.py``, in their order (what the builder hands the GNN as its three mappings,
    builders/utils_algo_graph.py:75-79)."""
    f = _FAMILY[family]
    return list(f["node_types"]), [tuple(e) for e in f["edge_types"]], list(EDGE_LEVELS)


def spec_from_observation(family: str, observation_dim: Dict, observation_names: Dict, *, knn_k: int = 3,
                          knn_to_actuators_k: int = -1, angular_velocity: bool = True) -> TaskSpec:
    """TaskSpec from the observation manager's ``group_obs_term_dim`` / ``group_obs_term_names`` dictionaries."""
    f = _FAMILY[family]
    first = lambda d: int(d[0]) if isinstance(d, (tuple, list, torch.Size)) else int(d)
    dims = {g: [first(d) for d in ds] for g, ds in observation_dim.items() if not g.startswith("norm_")}
    names = {g: list(ns) for g, ns in observation_names.items() if not g.startswith("norm_")}
    for g in names:
        if len(names[g]) != len(dims[g]):
            raise ValueError(f"observation group '{g}': {len(names[g])} names for {len(dims[g])} terms")
    pv = dict(zip(names["position_vectors"], dims["position_vectors"]))
    if "grippers" not in pv or f["main"] not in pv:
        raise ValueError(f"{family}: position_vectors must contain 'grippers' and '{f['main']}' (got {list(pv)})")
    if family == "rigid" and "infos" not in names:
        raise ValueError("rigid tasks need the 'infos' group (object_num_points, rigid_tasks_data.py:270)")
    return TaskSpec(family, list(f["node_types"]), [tuple(e) for e in f["edge_types"]], ["internal", "task", "agent"], names, dims,
                    pv["grippers"] // 3, knn_k=knn_k, angular_velocity=angular_velocity, n_vec=f["n_vec"],
                    in_features=list(f["in_features"]), knn_to_actuators_k=knn_to_actuators_k)


class _RefData(HyperData):
    FAMILY = None

    def __init__(self, observation_dim: Dict, observation_names: Dict, full_graph_obs: bool = False, dist_as_pos: bool = False,
                 output_mask_key: Optional[str] = None, training_noise: bool = False, training_noise_std: float = 1e-2,
                 concat_input_vector: bool = True, angular_velocity: bool = True, knn_k: int = 3, knn_to_actuators_k: int = -1,
                 **kwargs):
        spec = spec_from_observation(self.FAMILY, observation_dim, observation_names, knn_k=knn_k,
                                     knn_to_actuators_k=knn_to_actuators_k, angular_velocity=angular_velocity)
        super().__init__(spec, full_graph_obs=full_graph_obs, dist_as_pos=dist_as_pos, output_mask_key=output_mask_key,
                         training_noise=training_noise, training_noise_std=training_noise_std,
                         concat_input_vector=concat_input_vector, **kwargs)
        self.observation_dim, self.observation_names = spec.obs_dims, spec.obs_names
        self.angular_velocity, self.knn_k, self.knn_to_actuators_k = angular_velocity, knn_k, knn_to_actuators_k


class RigidTasksData(_RefData):
    """geometry_rl/modules/pyg_data/rigid_tasks_data.py:53-91."""
    FAMILY = "rigid"


class ClothTasksData(_RefData):
    """geometry_rl/modules/pyg_data/cloth_tasks_data.py:51-86."""
    FAMILY = "cloth"


class RopeTasksData(_RefData):
    """geometry_rl/modules/pyg_data/rope_tasks_data.py:51-89."""
    FAMILY = "rope"
