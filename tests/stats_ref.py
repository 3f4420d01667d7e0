"""numpy float64 restatements of the three kernels of csrc/stats_ops.hip.  TEST INFRASTRUCTURE ONLY, a plain module like
tests/train_ops_ref.py.  The semantics of torchmetrics' ``ExplainedVariance`` and of torchrl's ``RewardSum`` / ``StepCounter`` are restated
from their documentation (neither library is installed, no fixture from the reference pins them: UNPINNED)."""
import numpy as np


def accumulate(acc, src):
    """grl_stats_accumulate: acc[:n] += src, acc[n] += 1 (in place, float64)."""
    n = len(src)
    acc[:n] += np.asarray(src, dtype=np.float64)
    acc[n] += 1.0
    return acc


def _score(num, den):
    """1 - num / den; a zero denominator scores 1 where the numerator is 0 as well, else 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.ones_like(num)
    ok = den != 0
    out[ok] = 1.0 - num[ok] / den[ok]
    out[~ok & (num != 0)] = 0.0
    return out


def explained_variance(value, target):
    """[N, T] -> (mean over the T columns of the per-column score, the score over all N*T frames): two-pass, centred, biased variances."""
    v, t = np.asarray(value, dtype=np.float64), np.asarray(target, dtype=np.float64)
    d = t - v

    def var0(x):
        return ((x - x.mean(axis=0, keepdims=True)) ** 2).mean(axis=0)
    per_column = _score(var0(d), var0(t))
    flat = _score(var0(d.reshape(-1, 1)), var0(t.reshape(-1, 1)))
    return float(per_column.mean()), float(flat[0])


def episode_scan(reward, done, ret_state, len_state):
    """reward float32 [N, T], done bool [N, T], states [N] -> (episode_reward float32 [N, T], step_count int32 [N, T], new ret_state,
    new len_state, sums float64[3] over the done frames).  The running return is a float32 sum, one add per step."""
    reward, done = np.asarray(reward, dtype=np.float32), np.asarray(done, dtype=bool)
    N, T = reward.shape
    er, sc = np.zeros((N, T), np.float32), np.zeros((N, T), np.int32)
    ret, length = np.array(ret_state, dtype=np.float32), np.array(len_state, dtype=np.int32)
    sums = np.zeros(3, np.float64)
    for n in range(N):
        run, cnt = np.float32(ret[n]), int(length[n])
        for t in range(T):
            run = np.float32(run + reward[n, t])
            cnt += 1
            er[n, t], sc[n, t] = run, cnt
            if done[n, t]:
                sums += (float(run), float(cnt), 1.0)
                run, cnt = np.float32(0.0), 0
        ret[n], length[n] = run, cnt
    return er, sc, ret, length, sums
