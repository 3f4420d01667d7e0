"""Save and resume under data parallelism: two ranks on cuda:0 over gloo (two processes open at once), TRPL with training noise and the
scheduled entropy bound, each rank on its half of the environments with a training-state file of ITS OWN.  The resumed pair -- rebuilt under
another torch seed, no calibrating forward -- continues bit for bit as the uninterrupted pair; the ranks' parameters stay equal to each
other, their noise keys differ."""
import functools

import pytest
import torch

import resume_cases as rc
from spawn_util import spawn_ranks

pytestmark = pytest.mark.gpu


def test_two_ranks_resume_bit_for_bit(tmp_path):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    spawn_ranks(functools.partial(rc.dp_worker), 2, (2,), (str(tmp_path), ret))
    assert all(r in ret for r in range(2))
    (a0, b0, na0, nb0, fresh0, d0), (a1, b1, na1, nb1, fresh1, d1) = ret[0], ret[1]
    assert not d0 and not d1, "\n".join((d0 + d1)[:20])                       # every step's losses and every snapshot, per rank
    assert torch.equal(a0, b0) and torch.equal(a1, b1)                        # resumed parameters = the uninterrupted pair's
    assert torch.equal(b0, b1)                                                # ... and equal across the ranks
    assert nb0 == na0 and nb1 == na1 and nb0[0] != nb1[0] and nb0[1] == nb1[1] > 0   # the ranks' noise keys differ, their draw counts do not
    assert fresh0[0] != nb0[0] and fresh1[0] != nb1[0], "the rebuilt ranks drew their noise keys from the saved seed: the case shows nothing"
