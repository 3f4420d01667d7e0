"""tests/stats_ref.py (the float64 restatements the kernels of csrc/stats_ops.hip are tested against) on cases computed by hand."""
import numpy as np
import pytest

import stats_ref


def test_accumulate_adds_values_and_counts_calls():
    acc = np.zeros(4)
    stats_ref.accumulate(acc, [1.0, -2.0, 0.5])
    stats_ref.accumulate(acc, [3.0, 2.0, 0.25])
    assert acc.tolist() == [4.0, 0.0, 0.75, 2.0]


def test_explained_variance_by_hand():
    # column 0: target (0, 2), value (0, 1): d = (0, 1), Var d = 1/4, Var t = 1 -> 3/4
    # column 1: target (1, 3), value (1, 3): d = 0 -> 1
    value = np.array([[0.0, 1.0], [1.0, 3.0]], np.float32)
    target = np.array([[0.0, 1.0], [2.0, 3.0]], np.float32)
    per_column, flat = stats_ref.explained_variance(value, target)
    assert per_column == pytest.approx((0.75 + 1.0) / 2, abs=1e-15)
    # all four frames: d = (0, 0, 1, 0): Var = 3/16; t = (0, 1, 2, 3): Var = 5/4 -> 1 - 3/20
    assert flat == pytest.approx(0.85, abs=1e-15)


def test_explained_variance_zero_denominator_branches():
    # column 0: constant target, value differs -> numerator 1/4, denominator 0 -> 0
    # column 1: constant target, value = target -> both 0 -> 1
    # column 2: an ordinary column, target (0, 4), value (1, 3): d = (-1, 1): Var d = 1, Var t = 4 -> 3/4
    value = np.array([[1.0, 5.0, 1.0], [2.0, 5.0, 3.0]], np.float32)
    target = np.array([[2.0, 5.0, 0.0], [2.0, 5.0, 4.0]], np.float32)
    per_column, _ = stats_ref.explained_variance(value, target)
    assert per_column == pytest.approx((0.0 + 1.0 + 0.75) / 3, abs=1e-15)
    # one environment: every column's variances are 0 -> every score is 1
    assert stats_ref.explained_variance(value[:1], target[:1])[0] == 1.0
    # ... and the flat score of one frame is 1 as well
    assert stats_ref.explained_variance(value[:1, :1], target[:1, :1]) == (1.0, 1.0)


def test_episode_scan_by_hand():
    reward = np.array([[1.0, 2.0, 0.5, 1.0], [0.25, 0.25, 0.25, 0.25]], np.float32)
    done = np.array([[0, 1, 0, 0], [0, 0, 0, 1]], bool)
    er, sc, ret, length, sums = stats_ref.episode_scan(reward, done, np.zeros(2), np.zeros(2))
    assert er.tolist() == [[1.0, 3.0, 0.5, 1.5], [0.25, 0.5, 0.75, 1.0]]
    assert sc.tolist() == [[1, 2, 1, 2], [1, 2, 3, 4]]
    assert ret.tolist() == [1.5, 0.0] and length.tolist() == [2, 0]
    assert sums.tolist() == [3.0 + 1.0, 2.0 + 4.0, 2.0]
    assert er.dtype == np.float32 and sc.dtype == np.int32


def test_episode_spans_two_calls():
    """An episode that starts in one rollout and ends in the next: the carried state makes two calls on the halves equal one on the whole."""
    reward = np.array([[1.0, 1.0, 2.0, 4.0, 8.0, 1.0]], np.float32)
    done = np.array([[0, 0, 0, 0, 1, 0]], bool)
    whole = stats_ref.episode_scan(reward, done, np.zeros(1), np.zeros(1))
    a = stats_ref.episode_scan(reward[:, :3], done[:, :3], np.zeros(1), np.zeros(1))
    assert a[2].tolist() == [4.0] and a[3].tolist() == [3] and a[4].tolist() == [0.0, 0.0, 0.0]
    b = stats_ref.episode_scan(reward[:, 3:], done[:, 3:], a[2], a[3])
    assert b[0].tolist() == [[8.0, 16.0, 1.0]] and b[1].tolist() == [[4, 5, 1]]
    assert b[4].tolist() == [16.0, 5.0, 1.0]
    assert np.array_equal(np.concatenate([a[0], b[0]], 1), whole[0]) and np.array_equal(np.concatenate([a[1], b[1]], 1), whole[1])
    assert np.array_equal(b[2], whole[2]) and np.array_equal(b[3], whole[3]) and np.array_equal(a[4] + b[4], whole[4])


def test_running_return_is_a_float32_sum():
    """2^24 + 1 is not a float32: the running return stays at 2^24 (as the transform's float32 tensor does), a float64 sum would not."""
    reward = np.array([[2.0 ** 24, 1.0, 1.0]], np.float32)
    er = stats_ref.episode_scan(reward, np.zeros((1, 3), bool), np.zeros(1), np.zeros(1))[0]
    assert er.tolist() == [[2.0 ** 24, 2.0 ** 24, 2.0 ** 24]]
