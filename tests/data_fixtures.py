"""Readers of the tier3 fixtures (tools/make_golden.py tier3): what the reference's RigidTasksData / ClothTasksData / RopeTasksData
returned from ``build_data`` on recorded observations, and what GNNVFNet -> DeepSets.one_step computed on the critic layout.

Generated under semantic stubs of the PyG containers and neighbour searches (``generated_under_semantic_stubs`` in every file); the
reference's own lines decide everything compared here.

``ModelFixture`` reads the tier2h fixtures (tools/make_golden.py tier2h): the same data classes handed straight to the reference's
PonitaGCN (EMPN) / HEPi ``one_step`` -- padded rigid batches, the 2-D rope, cloth -- with the state dict before and after the calibrating
call, outputs, gradients, and the float64 run of the same model.

Not in any fixture: variable-length ropes (our extension: the reference's rope builder reads no point count), the rigid builder with
knn_to_actuators_k > 0 (upstream never assigns those edges), training noise, PonitaGCN(attention=True), a model on a data class built
with knn_to_actuators_k > 0 (the builders with it are pinned by tier3, the models on full task edges by tier2h)."""
import os

import numpy as np
import torch

CASES = {"rigid_g1": "rigid", "rigid_g2": "rigid", "cloth": "cloth", "rope": "rope", "rope_kta": "rope", "cloth_kta": "cloth"}
MAIN = {"rigid": "object_geometry", "cloth": "hole_boundary", "rope": "links"}
IN_FEATURES = ["scalars", "position_vectors", "velocity_vectors", "norm_position_vectors", "norm_velocity_vectors", "infos"]
ACTOR = dict(full_graph_obs=False, dist_as_pos=True, output_mask_key="grippers", concat_input_vector=False)
CRITIC = dict(full_graph_obs=True, dist_as_pos=False, output_mask_key=None, concat_input_vector=True)
CRITIC_CASES = ("rigid_g1", "cloth")
TIE_GAP = 1e-3


def layouts(case):
    """tag -> constructor keywords of the layouts recorded for ``case``."""
    out = {"actor": ACTOR, "critic": CRITIC}
    if CASES[case] == "cloth":
        out["actor_full"] = dict(ACTOR, full_graph_obs=True)
    return out


# tier2h: data class -> model (case -> task family)
MODEL_CASES = {"empn_rigid_g2_pad": "rigid", "empn_rope_dim2": "rope", "hepi_rigid_g1_pad": "rigid", "hepi_cloth": "cloth"}
HEPI_CODES = [[1, 0], [0, 1], [0, 1]]   # configs/algorithm/pyg_agent/model/hepi.yaml, as tier2b


class Fixture:
    def __init__(self, golden_dir, case, file=None, family=None):
        z = np.load(os.path.join(golden_dir, file or f"tier3_data_{case}.npz"))
        family = family or CASES[case]
        self.case, self.family, self.main = case, family, MAIN[family]
        self.z = {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}
        assert int(self.z["generated_under_semantic_stubs"]) == 1
        self.obs = {k: self.z["obs." + k] for k in IN_FEATURES if "obs." + k in self.z}
        self.observation_names = {k[len("observation_names."):]: [str(n) for n in v] for k, v in self.z.items()
                                  if k.startswith("observation_names.")}
        self.observation_dim = {k[len("observation_dim."):]: [(int(d),) for d in v] for k, v in self.z.items()
                                if k.startswith("observation_dim.")}
        self.kwargs = {k[len("kwarg."):]: int(v) for k, v in self.z.items() if k.startswith("kwarg.")}
        if "angular_velocity" in self.kwargs:
            self.kwargs["angular_velocity"] = bool(self.kwargs["angular_velocity"])
        self.B = self.obs["scalars"].shape[0]

    def args(self):
        return [self.obs[k] for k in IN_FEATURES if k in self.obs]

    def n_per(self, t):
        names, dims = self.observation_names["position_vectors"], self.observation_dim["position_vectors"]
        return dims[names.index(t)][0] // 3

    def n_valid(self):
        """Valid points of the main node type per sample (only the rigid tasks pad)."""
        P = self.n_per(self.main)
        if self.family == "rigid":
            return self.obs["infos"][:, 0].long().clamp(max=P)
        return torch.full((self.B,), P, dtype=torch.long)

    def valid_rows(self, t):
        """Rows of node type ``t`` in the reference's numbering (b * n_per + j) that our actor graph keeps, in natural order."""
        n = self.n_per(t)
        if t != self.main:
            return torch.arange(self.B * n)
        nv = self.n_valid()
        return torch.cat([b * n + torch.arange(int(nv[b])) for b in range(self.B)])

    def node_types(self, tag):
        return [str(t) for t in self.z[f"{tag}.node_types"]]

    def edge_types(self, tag):
        return [tuple(str(e).split("|")) for e in self.z[f"{tag}.edge_types"]]

    def node(self, tag, what, t):
        return self.z[f"{tag}.{what}.{t}"]

    def edge_set(self, tag, et):
        ei = self.z[f"{tag}.edge_index." + "|".join(et)]
        return sorted(zip(ei[0].tolist(), ei[1].tolist()))

    def compact_edge_set(self, tag, et):
        """The reference edge set in natural COMPACT numbering (padded points removed), after asserting that no edge touches padding."""
        maps = []
        for t in (et[0], et[2]):
            rows = self.valid_rows(t)
            m = torch.full((self.B * self.n_per(t),), -1, dtype=torch.long)
            m[rows] = torch.arange(rows.numel())
            maps.append(m)
        out = []
        for s, d in self.edge_set(tag, et):
            cs, cd = int(maps[0][s]), int(maps[1][d])
            assert cs >= 0 and cd >= 0, ("an edge of the reference touches a padded point", et, s, d)
            out.append((cs, cd))
        return sorted(out)

    def critic_dense(self, tag="critic"):
        """[B, n_all, d]: the recorded input_vector_dict, node types in the recorded order (what DeepSets.one_step concatenates;
        tier3_critic.npz pins that line itself)."""
        return torch.cat([self.node(tag, "input_vector", t).reshape(self.B, self.n_per(t), -1) for t in self.node_types(tag)], dim=1)


class ModelFixture(Fixture):
    """tier2h_<case>.npz + tier2h_<case>_grad.npz.  ``init`` / ``cal`` / ``cal64``: the model's whole state dict before the first training
    call, after it, and after it in the float64 run (the files store of ``cal`` / ``cal64`` only the entries that call changed: the
    calibrated kernels and their flags); ``grad``: every parameter gradient under R_out / R_hidden at the calibrated state; ``model``:
    empn (else HEPi), dim, upper, output_dim, output_dim_vec."""

    def __init__(self, golden_dir, case):
        super().__init__(golden_dir, case, f"tier2h_{case}.npz", MODEL_CASES[case])
        pick = lambda p: {k[len(p):]: torch.as_tensor(v) for k, v in self.z.items() if k.startswith(p)}   # (the flags are bool arrays)
        self.model = {k: int(v) for k, v in pick("model.").items()}
        self.init = pick("init.")
        self.changed = sorted(pick("cal."))
        assert self.changed == sorted(pick("cal64.")) and set(self.changed) <= set(self.init)
        self.cal = {**self.init, **pick("cal.")}
        self.cal64 = {**{k: (v.double() if v.dtype.is_floating_point else v) for k, v in self.init.items()}, **pick("cal64.")}
        g = np.load(os.path.join(golden_dir, f"tier2h_{case}_grad.npz"))
        self.grad = {k[len("grad."):]: torch.from_numpy(g[k]) for k in g.files}

    def node_types(self, tag=None):
        return [str(t) for t in self.z["node_types"]]

    def edge_types(self, tag=None):
        return [tuple(str(e).split("|")) for e in self.z["edge_types"]]

    def edge_set(self, tag, et):
        ei = self.z["edge_index." + "|".join(et)]
        return sorted(zip(ei[0].tolist(), ei[1].tolist()))

    def ref_distance(self, key):
        """max |fp32 reference - fp64 reference| of an output ("out", "hidden") or a calibrated tensor ("cal.<name>")."""
        a, b = (self.cal[key[4:]], self.cal64[key[4:]]) if key.startswith("cal.") else (self.z[key], self.z[key + "64"])
        return float((a.double() - b).abs().max())


def tie_gap(points, queries, k, exclude_self):
    """Smallest (d_{k+1} - d_k) / d_k over the queries, Euclidean distances in float64 (inf: fewer than k + 1 candidates)."""
    d = torch.cdist(queries.double(), points.double())
    if exclude_self:
        d.fill_diagonal_(float("inf"))
    if points.shape[0] - int(exclude_self) <= k:
        return float("inf")
    d = d.sort(dim=1).values
    return float(((d[:, k] - d[:, k - 1]) / d[:, k - 1]).min())


def load_critic(golden_dir):
    z = np.load(os.path.join(golden_dir, "tier3_critic.npz"))
    assert int(z["generated_under_semantic_stubs"]) == 1
    return {k: torch.from_numpy(z[k]) for k in z.files}
