"""Training noise without a GPU: the host restatement of the feature launch's generator (tests/noise_ref.py) reproduces the published
Random123 Philox4x32-10 known-answer vectors, its Box-Muller mapping gives standard normals, and the host-side bookkeeping of HyperData
(constructor, seed, noise words) follows the documented rules."""
import numpy as np
import pytest
import torch

from noise_ref import noisy_slots, normals, philox4x32_10


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]
    assert [int(x) for x in got] == list(want)


def test_box_muller_normals_are_standard():
    z = normals(1234, 7, np.arange(200000)).reshape(-1)
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.std() - 1) < 0.01
    assert np.isfinite(z).all()
    # another draw / another seed: another stream
    assert not np.allclose(normals(1234, 8, np.arange(16)), normals(1234, 7, np.arange(16)))
    assert not np.allclose(normals(1235, 7, np.arange(16)), normals(1234, 7, np.arange(16)))


def test_hyperdata_noise_bookkeeping():
    from geometry_rl_amd import graph
    spec = graph.rigid_spec(G=2, angular_velocity=False, object_velocity=False)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    hd = graph.HyperData(spec, dist_as_pos=True, output_mask_key="grippers", concat_input_vector=False, training_noise=True,
                         training_noise_std=0.01)
    assert torch.equal(before, torch.get_rng_state())          # no draw of torch's generator is consumed
    torch.manual_seed(3)
    hd2 = graph.HyperData(spec, dist_as_pos=True, output_mask_key="grippers", concat_input_vector=False, training_noise=True)
    assert hd.noise_state() == hd2.noise_state() and hd.noise_state()[1] == 0
    torch.manual_seed(4)
    assert graph.HyperData(spec, dist_as_pos=True, concat_input_vector=False, training_noise=True).noise_state() != hd.noise_state()
    hd.set_noise_state(99, 5)
    assert hd.noise_state() == (99, 5)
    hd.fold_noise_rank(1)
    seed1 = hd.noise_state()
    assert seed1[0] != 99 and seed1[1] == 5
    hd.fold_noise_rank(1)                                        # (once)
    assert hd.noise_state() == seed1
    # the noise words against the host rules: type, slot, n_slots, B and the two flags
    B = 5
    for t in hd.node_type_list:
        words = hd._noise_words(t, 2, B)
        want = dict(noisy_slots(spec, t, True))
        for slot, w in enumerate(words):
            w &= (1 << 64) - 1
            assert bool(w & 1) == (slot in want), (t, slot)
            if w:
                assert (w >> 8) & 0xff == slot and (w >> 16) & 0xff == spec.n_vec and (w >> 24) & 0xff == spec.node_types.index(t)
                assert w >> 32 == B and bool(w & 2) == want[slot]
    # grippers (velocity observed, no angular velocity): pos, vel and the zero ang column are noisy; the object (no velocity): pos + corr
    assert [s for s, _ in noisy_slots(spec, "grippers", True)] == [0, 2, 3]
    assert noisy_slots(spec, "object_geometry", True) == [(0, False), (1, True)]
    assert noisy_slots(graph.cloth_spec(), "particles", True) == []


def test_factories_accept_training_noise():
    from geometry_rl_amd import agent, graph
    spec = graph.rigid_spec()
    dims = {g: [(d,) for d in ds] for g, ds in spec.obs_dims.items()}
    hd = graph.RigidTasksData(dims, spec.obs_names, full_graph_obs=False, dist_as_pos=True, output_mask_key="grippers",
                              training_noise=True, training_noise_std=0.01, concat_input_vector=False)
    assert hd.training_noise and hd._noise_on and hd.training_noise_std == 0.01
    cs = graph.cloth_spec()
    cd = graph.ClothTasksData({g: [(d,) for d in ds] for g, ds in cs.obs_dims.items()}, cs.obs_names, training_noise=True)
    assert cd.training_noise and not cd._noise_on                 # accepted, no effect (cloth_tasks_data.py adds no noise)
    cfg = agent.AgentConfig(model="empn", training_noise=True)
    assert cfg.training_noise and cfg.training_noise_std == 0.01
