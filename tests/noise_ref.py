"""Host restatement of the training noise of the feature launch (include/grl_hip.h grl_build_features_noise): Philox4x32-10 keyed by the
64-bit seed, counter = (element id lo, hi, draw lo, hi), Box-Muller on its four words, three normals per element; and the per-family rules
of which input-vector slots get noise (rigid_tasks_data.py:178-214, rope_tasks_data.py:168-186; cloth: none)."""
import numpy as np
import torch

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32-valued array [..., 4], key: (k0, k1) -> uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # (32 x 32 bits: exact in uint64)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + W0) & _LO, (k1 + W1) & _LO
    return np.stack(c, axis=-1)


def normals(seed: int, draw: int, elem) -> np.ndarray:
    """The three normals of every element id in ``elem`` (int array) at (seed, draw) -> float64 [n, 3]."""
    e = np.asarray(elem, dtype=np.uint64).reshape(-1)
    d = np.uint64(draw)
    ctr = np.stack([e & _LO, e >> np.uint64(32), np.full_like(e, d & _LO), np.full_like(e, d >> np.uint64(32))], axis=-1)
    r = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    s = 2.0 ** -24
    u1 = ((r[:, 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * s
    u2 = (r[:, 1] >> np.uint64(8)).astype(np.float64) * s
    u3 = ((r[:, 2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * s
    u4 = (r[:, 3] >> np.uint64(8)).astype(np.float64) * s
    ra, rb = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    return np.stack([ra * np.cos(2 * np.pi * u2), ra * np.sin(2 * np.pi * u2), rb * np.cos(2 * np.pi * u4)], axis=-1)


def noisy_slots(spec, t, dist_as_pos):
    """[(slot, add the position slot's noise as well)] of node type t that get noise (per family)."""
    if spec.family == "cloth":
        return []
    corr_type = {"rigid": "object_geometry", "rope": "links"}[spec.family]
    out = [(0, False)]
    if t == corr_type:
        out.append((1, bool(dist_as_pos)))
    if t in spec.obs_names["velocity_vectors"]:
        out += [(s, False) for s in range(2, spec.n_vec)]
    return out


def add_noise(spec, vector_dict, B, seed, draw, std, dist_as_pos):
    """vector_dict: {type: [B * n_per, 3 * n_vec]} in the natural (sample, point) order, noise-free (oracle.graph.build_features) ->
    the same with the noise of (seed, draw) added (float32; computed in float64).  Also -> {type: bool mask [3 * n_vec] of noisy columns}."""
    out, masks = {}, {}
    n_slots = spec.n_vec
    for t, v in vector_dict.items():
        ti = spec.node_types.index(t)
        rows = v.shape[0]
        n_per = rows // B
        r = np.arange(rows, dtype=np.uint64)
        b, j = r // np.uint64(n_per), r % np.uint64(n_per)
        e0 = ((np.uint64(ti) * np.uint64(B) + b) * np.uint64(n_per) + j) * np.uint64(n_slots)
        x = v.detach().cpu().double().numpy().copy()
        mask = np.zeros(3 * n_slots, dtype=bool)
        for slot, pos_too in noisy_slots(spec, t, dist_as_pos):
            x[:, 3 * slot:3 * slot + 3] += std * normals(seed, draw, e0 + np.uint64(slot))
            if pos_too:
                x[:, 3 * slot:3 * slot + 3] += std * normals(seed, draw, e0)
            mask[3 * slot:3 * slot + 3] = True
        out[t], masks[t] = torch.from_numpy(x).float(), mask
    return out, masks
