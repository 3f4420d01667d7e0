"""The kernels of csrc/stats_ops.hip per op, against the float64 restatements of tests/stats_ref.py: the running sums behind the
per-iteration means (grl_stats_accumulate), the explained variance (grl_explained_variance) and the RewardSum / StepCounter scan
(grl_episode_scan).  Inputs are chosen so that the sums and the scan are EXACT in their number formats (equality, not a tolerance); the
explained variance is held to the float32 rounding of its result."""
import numpy as np
import pytest
import torch

import stats_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------- grl_stats_accumulate
@pytest.mark.parametrize("n", [1, 14])
def test_accumulate_is_the_exact_sum_and_counts_its_calls(n):
    """1000 calls with values that are multiples of 2^-10 in [-8, 8]: every partial sum is exact in fp64, so the accumulator equals the exact
    sum, its last entry the number of calls, and the accumulator next to it in memory keeps its contents."""
    from geometry_rl_amd import hip
    calls = 1000
    g = torch.Generator().manual_seed(n)
    src = (torch.randint(-8 * 1024, 8 * 1024 + 1, (calls, n), generator=g).float() / 1024).to(DEV)
    both = torch.zeros(2 * (n + 1), device=DEV, dtype=torch.float64)
    both[n + 1:] = 7.0
    acc, other = both[:n + 1], both[n + 1:]
    for i in range(calls):
        hip.call("grl_stats_accumulate", src[i], n, acc)
    ref = np.zeros(n + 1)
    for row in src.cpu().numpy():
        stats_ref.accumulate(ref, row)
    assert acc.cpu().numpy().tolist() == ref.tolist()
    assert float(acc[n]) == calls
    assert torch.equal(other.cpu(), torch.full((n + 1,), 7.0, dtype=torch.float64))


def test_accumulate_rejects_more_than_32_values():
    from geometry_rl_amd import hip
    with pytest.raises(RuntimeError, match="status -2"):
        hip.call("grl_stats_accumulate", torch.zeros(33, device=DEV), 33, torch.zeros(34, device=DEV, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------- grl_explained_variance
def _standardised(N, T, g):
    """[N, T] with sample mean 0 and (biased) sample variance 1 in every column (N >= 2)."""
    z = torch.randn(N, T, generator=g, dtype=torch.float64)
    z = z - z.mean(0, keepdim=True)
    return z / z.pow(2).mean(0, keepdim=True).sqrt()


def _ev_case(N, T):
    """(value, target) float32 [N, T] with mean^2 / var <= 100 in every column of target and of target - value (|mean| <= 8 std), except
    the special columns: (5, 3) has a CONSTANT target column whose value differs (zero denominator, non-zero numerator), (300, 7) has
    value == target (every numerator 0), N = 1 makes every column's two variances 0."""
    g = torch.Generator().manual_seed(1000 * N + T)
    if N == 1:
        target = torch.randn(1, T, generator=g, dtype=torch.float64)
        value = target + torch.randn(1, T, generator=g, dtype=torch.float64)
        return value.float(), target.float()
    std_t = torch.rand(T, generator=g, dtype=torch.float64) * 3 + 0.1
    mean_t = (torch.rand(T, generator=g, dtype=torch.float64) * 16 - 8) * std_t
    target = (mean_t + std_t * _standardised(N, T, g)).float()
    std_d = torch.rand(T, generator=g, dtype=torch.float64) * 2 + 0.1
    mean_d = (torch.rand(T, generator=g, dtype=torch.float64) * 16 - 8) * std_d
    value = (target.double() - (mean_d + std_d * _standardised(N, T, g))).float()
    if (N, T) == (5, 3):
        target[:, 1] = 2.75
    if (N, T) == (300, 7):
        value = target.clone()
    return value, target


@pytest.mark.parametrize("N,T", [(2, 1), (5, 3), (64, 64), (65, 130), (300, 7), (1, 4)])
def test_explained_variance_against_float64(N, T):
    """Allowance 4 * 2^-23 * max(1, |ref|): the fp64 one-pass sums of float32 inputs with N*T <= 2^20 and mean^2 / var <= 100 are good
    to below 1e-8 relative; what remains is the float32 rounding of the result.  A second run gives the same bits."""
    from geometry_rl_amd.rollout import explained_variance
    value, target = _ev_case(N, T)
    ref = stats_ref.explained_variance(value.numpy(), target.numpy())
    got = explained_variance(value.to(DEV), target.to(DEV))
    again = explained_variance(value.to(DEV).unsqueeze(-1), target.to(DEV).unsqueeze(-1))   # ([N, T, 1], as the rollout buffer holds them)
    assert torch.equal(got, again)
    got = got.cpu().double().tolist()
    for name, a, b in zip(("per column", "flat"), got, ref):
        print(f"explained variance ({N}, {T}) {name}: kernel {a!r}, float64 {b!r}, |diff| {abs(a - b):.3e}")
    for a, b in zip(got, ref):
        assert abs(a - b) <= 4 * 2.0 ** -23 * max(1.0, abs(b)), (a, b)
    if (N, T) == (5, 3):     # (the zero-denominator column scores 0: the mean of three scores, two of them below 1)
        per_col = [stats_ref.explained_variance(value[:, c:c + 1].numpy(), target[:, c:c + 1].numpy())[0] for c in range(3)]
        assert per_col[1] == 0.0 and ref[0] == pytest.approx(sum(per_col) / 3, abs=1e-15)
    if (N, T) == (300, 7):
        assert got == [1.0, 1.0]
    if N == 1:
        assert got[0] == 1.0


# ------------------------------------------------------------------------------------------------------------- grl_episode_scan
def _episode_case(N, T, pattern):
    g = torch.Generator().manual_seed(100 * N + T)
    reward = torch.randint(-4 * 256, 4 * 256 + 1, (N, T), generator=g).float() / 256   # multiples of 2^-8: every float32 sum is exact
    if pattern == "none":
        done = torch.zeros(N, T, dtype=torch.bool)
    elif pattern == "all":
        done = torch.ones(N, T, dtype=torch.bool)
    elif pattern == "random":
        done = torch.rand(N, T, generator=g) < 0.05
    else:
        done = torch.zeros(N, T, dtype=torch.bool)
        done[:, -1] = True
    return reward, done


@pytest.mark.parametrize("pattern", ["none", "all", "random", "last"])
@pytest.mark.parametrize("N,T", [(1, 1), (3, 5), (64, 64), (70, 130), (130, 65)])
def test_episode_scan_equals_the_restatement(N, T, pattern):
    """episode_reward, step_count, the end states and the sums equal the restatement EXACTLY (carried-in states included), and two calls on
    the halves of the rollout, the state carried, equal one call on the whole."""
    from geometry_rl_amd.rollout import EpisodeStats
    reward, done = _episode_case(N, T, pattern)
    g = torch.Generator().manual_seed(7)
    ret0 = torch.randint(-512, 513, (N,), generator=g).float() / 256    # an episode already running when the rollout starts
    len0 = torch.randint(0, 50, (N,), generator=g).int()
    er, sc, ret, length, sums = stats_ref.episode_scan(reward.numpy(), done.numpy(), ret0.numpy(), len0.numpy())

    def fresh():
        es = EpisodeStats(N, DEV)
        es.ret_state.copy_(ret0)
        es.len_state.copy_(len0)
        return es
    es = fresh()
    got_er, got_sc = es.scan(reward.to(DEV).unsqueeze(-1), done.to(DEV).unsqueeze(-1))
    assert got_er.shape == (N, T, 1) and got_er.dtype == torch.float32 and got_sc.dtype == torch.int32
    assert np.array_equal(got_er.reshape(N, T).cpu().numpy(), er) and np.array_equal(got_sc.reshape(N, T).cpu().numpy(), sc)
    assert np.array_equal(es.ret_state.cpu().numpy(), ret) and np.array_equal(es.len_state.cpu().numpy(), length)
    assert es.sums.cpu().numpy().tolist() == sums.tolist()
    if T >= 2:
        h = T // 2
        es2 = fresh()
        a_er, a_sc = es2.scan(reward[:, :h].contiguous().to(DEV), done[:, :h].contiguous().to(DEV))
        a_sums = es2.sums.clone()
        b_er, b_sc = es2.scan(reward[:, h:].contiguous().to(DEV), done[:, h:].contiguous().to(DEV))
        assert torch.equal(torch.cat([a_er, b_er], 1), got_er.reshape(N, T)) and torch.equal(torch.cat([a_sc, b_sc], 1), got_sc.reshape(N, T))
        assert torch.equal(es2.ret_state, es.ret_state) and torch.equal(es2.len_state, es.len_state)
        assert torch.equal(a_sums + es2.sums, es.sums)
