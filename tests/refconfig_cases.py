"""What tests/test_refconfig_cpu.py and tests/test_gpu_refconfig.py share: the copy of the reference's config tree, the 15 task configs, a
table of their values WRITTEN BY READING THE YAML FILES (never by running the loader), and the small observation layouts they are built at."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "tests", "golden", "reference_configs")

_H = "geometry_rl.modules.pyg_models."
HEPI, EMPN, TRANSFORMER = _H + "hepi.HEPi", _H + "ponita_gcn.PonitaGCN", _H + "transformer_vanilla.TransformerVanilla"
DEEPSETS = _H + "deepsets.DeepSets"
_RAW = ["scalars", "position_vectors", "velocity_vectors", "norm_position_vectors", "norm_velocity_vectors"]
_NORM = ["scalars", "norm_position_vectors", "norm_velocity_vectors", "norm_position_vectors", "norm_velocity_vectors"]


def _row(model, family, action_dim, ponita_dim, out, noise, aux, mbs, clip_grad, cov_bound, *, fpb, total, envs, trc, clip, entropy_coef=0.005,
         upper=None, knn_k=3, actor_in=_RAW, critic_in=_RAW, infos=True, post_fc=False):
    tail = ["infos"] if infos else []
    return dict(model=model, family=family, action_dim=action_dim, ponita_dim=ponita_dim, out=out, noise=noise, aux=aux, mini_batch_size=mbs,
                clip_grad_norm=clip_grad, cov_bound=cov_bound, frames_per_batch=fpb, total_frames=total, num_envs=envs,
                trust_region_coeff=trc, clip=clip, entropy_coef=entropy_coef, only_upper_hemisphere=upper, knn_k=knn_k,
                actor_in=list(actor_in) + tail, critic_in=list(critic_in) + tail, post_fc=post_fc,
                total_network_updates=(total // fpb) * 5 * (fpb // mbs))


_CLOTH = dict(fpb=10_000, total=5_000_000, envs=100, trc=4.0, clip=50.0, knn_k=None, infos=False)
_RIGID = dict(fpb=100_000, envs=1000, clip=20.0)
_ROPE = dict(fpb=40_000, envs=200, clip=10.0, infos=False)
# post_fc None: the key is absent (the transformer configs), so the reference constructor's True applies
TABLE = {
    "cloth_hanging_multi_empn": _row(EMPN, "cloth", 3, 3, (1, 1), False, (3, 9), 200, False, 0.001, **_CLOTH),
    "cloth_hanging_multi_hepi": _row(HEPI, "cloth", 3, 3, (1, 1), False, (3, 9), 200, False, 0.001, **_CLOTH),
    "cloth_hanging_multi_transformer": _row(TRANSFORMER, "cloth", 3, None, (64, None), False, (9, 9), 200, False, 0.001, actor_in=_NORM,
                                            critic_in=_NORM, post_fc=None, **_CLOTH),
    "rigid_insertion_multi_empn": _row(EMPN, "rigid", 6, 3, (2, 2), False, (4, 12), 1000, False, 0.0025, total=20_000_000, trc=1.0, upper=True,
                                       **_RIGID),
    "rigid_insertion_multi_hepi": _row(HEPI, "rigid", 6, 3, (2, 2), False, (4, 12), 1000, False, 0.0025, total=20_000_000, trc=1.0, upper=True,
                                       **_RIGID),
    "rigid_insertion_multi_transformer": _row(TRANSFORMER, "rigid", 6, None, (64, None), False, (12, 12), 1000, False, 0.0025,
                                              total=20_000_000, trc=1.0, actor_in=_NORM, post_fc=None, **_RIGID),
    "rigid_insertion_two_agents_multi_empn": _row(EMPN, "rigid", 3, 3, (1, 1), False, (4, 12), 1000, False, 0.0025, total=10_000_000, trc=1.0,
                                                  upper=True, **_RIGID),
    "rigid_insertion_two_agents_multi_hepi": _row(HEPI, "rigid", 3, 3, (1, 1), False, (4, 12), 1000, False, 0.0025, total=10_000_000, trc=1.0,
                                                  upper=True, **_RIGID),
    "rigid_insertion_two_agents_multi_transformer": _row(TRANSFORMER, "rigid", 3, None, (64, None), False, (12, 12), 1000, False, 0.0025,
                                                         total=10_000_000, trc=1.0, actor_in=_NORM, post_fc=None, **_RIGID),
    "rigid_pushing_multi_empn": _row(EMPN, "rigid", 3, 2, (1, 1), True, (4, 12), 1000, False, 0.0025, total=30_000_000, trc=1.0, **_RIGID),
    "rigid_pushing_multi_hepi": _row(HEPI, "rigid", 3, 2, (1, 1), True, (4, 12), 1000, False, 0.0025, total=30_000_000, trc=1.0, **_RIGID),
    "rigid_pushing_multi_transformer": _row(TRANSFORMER, "rigid", 3, None, (64, None), True, (12, 12), 1000, False, 0.0025, total=30_000_000,
                                            trc=1.0, actor_in=_NORM, critic_in=_NORM, post_fc=None, **_RIGID),
    "rigid_sliding_multi_hepi": _row(HEPI, "rigid", 6, 2, (2, 2), False, (4, 12), 1000, False, 0.001, total=20_000_000, trc=4.0,
                                     entropy_coef=0.0005, **_RIGID),
    "rope_closing_hepi": _row(HEPI, "rope", 3, 2, (1, 1), False, (3, 9), 200, True, 0.001, total=4_000_000, trc=4.0, **_ROPE),
    "rope_shaping_hepi": _row(HEPI, "rope", 3, 2, (1, 1), False, (3, 9), 200, True, 0.0025, total=10_000_000, trc=1.0, **_ROPE),
}
NAMES = sorted(TABLE)


def cfg_name(name: str) -> str:
    return name + "_trpl_cfg"


# ---- small layouts: ragged rigid objects (6 .. 12 of 12 points), a cloth whose particles outnumber its hole points, a 12-link rope
def layout(name: str):
    """-> (TaskSpec of the small layout, observation_dim, observation_names, keyword arguments of the matching ``synthetic.make_*_obs``)."""
    from geometry_rl_amd import graph
    if name.startswith("cloth"):
        kw = dict(n_particles=16, n_hole=6, G=2, E_cloth=24)
        spec = graph.cloth_spec(**kw)
    elif name.startswith("rope"):
        kw = dict(n_links=12, G=2)
        spec = graph.rope_spec(**kw)
    elif "two_agents" in name:
        kw = dict(P=12, G=2, E_mesh=20, angular_velocity=False)
        spec = graph.rigid_spec(**kw)
    else:
        kw = dict(P=12, G=1, E_mesh=20)
        spec = graph.rigid_spec(**kw)
    return spec, {g: [(d,) for d in ds] for g, ds in spec.obs_dims.items()}, spec.obs_names, kw


def make_obs(name: str, B: int, seed: int = 0):
    from geometry_rl_amd import synthetic as syn
    spec, _, _, kw = layout(name)
    make = {"cloth": syn.make_cloth_obs, "rope": syn.make_rope_obs, "rigid": syn.make_rigid_obs}[spec.family]
    return make(B, seed=seed, **kw)


def build(name: str, overrides=(), device="cpu", **kw):
    """-> (cfg, (actor, critic, projection, loss)) of the task config at its small layout."""
    from geometry_rl_amd import refconfig
    cfg = refconfig.compose(CONFIGS, cfg_name(name), overrides)
    spec, od, on, _ = layout(name)
    A = spec.num_actuators * cfg["algorithm"]["policy"]["action_dim"]
    return cfg, refconfig.build_from_config(cfg, od, on, A, device=device, **kw)
