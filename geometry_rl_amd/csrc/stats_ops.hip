// The read-out of a training run (examples/torchrl/train.py:237-246, 318-333), on the device: running sums of the values every update
// reports (the mean over ppo_epochs x minibatches of train.py:294,320), the explained variance of the value function (train.py:142,325) and
// the collector-side RewardSum / StepCounter transforms (configs/rigid_insertion_multi_hepi_trpl_cfg.yaml:74-76).  None of it feeds an
// update.  All kernels are deterministic -- fixed summation order, no floating-point atomics -- and capturable: no host read, no allocation.
#include "grl_common.h"

namespace {

// acc[i] += src[i] (i < n <= 32), acc[n] += 1: the launch that rides at the end of a lane.  Launches of one stream are ordered, so the
// fp64 sums are those of the updates in their order.
__global__ __launch_bounds__(64) void stats_accumulate_kernel(const float* __restrict__ src, int n, double* __restrict__ acc) {
  const int i = threadIdx.x;
  if (i < n) acc[i] += (double)src[i];
  else if (i == n) acc[n] += 1.0;
}

// The sum of ``v`` over the workgroup's NT threads, in the fixed order of a binary tree; every thread gets it.
template <int NT>
GRL_DEVINL double block_sum(double v, double* sh) {
  const int i = threadIdx.x;
  sh[i] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (i < s) sh[i] += sh[i + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// torchmetrics ExplainedVariance: 1 - Var(target - value) / Var(target); where the denominator is 0 the score is 1 if the numerator is 0
// as well and 0 otherwise.
GRL_DEVINL double ev_score(double num, double den) { return den != 0.0 ? 1.0 - num / den : (num != 0.0 ? 0.0 : 1.0); }

// Explained variance, first launch.  value / target are [N, T] row-major: a thread owns one column (time step), so the 64 threads of a
// workgroup read 64 consecutive floats of a row; workgroup (x, y) sums rows [64 y, 64 y + 64) of columns [64 x, 64 x + 64) in row order.
// The sums are taken of (d - d0) and (t - t0), d = target - value, (d0, t0) = the column's row 0: a constant column gives exact zeros,
// and the one-pass variance loses nothing to a large mean.  scratch [R][4][T] fp64 = (sum d, sum d^2, sum t, sum t^2) per row group.
constexpr int EV_ROWS = 64;
__global__ __launch_bounds__(64) void ev_partial_kernel(const float* __restrict__ value, const float* __restrict__ target, int N, int T,
                                                       double* __restrict__ scratch) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  const int r0 = blockIdx.y * EV_ROWS, r1 = min(r0 + EV_ROWS, N);
  const double t0 = (double)target[t], d0 = t0 - (double)value[t];
  double sd = 0, sdd = 0, st = 0, stt = 0;
  for (int r = r0; r < r1; ++r) {
    const size_t i = (size_t)r * T + t;
    const double tv = (double)target[i], d = (tv - (double)value[i]) - d0, tt = tv - t0;
    sd += d;
    sdd += d * d;
    st += tt;
    stt += tt * tt;
  }
  double* o = scratch + (size_t)blockIdx.y * 4 * T + t;
  o[0] = sd;
  o[(size_t)T] = sdd;
  o[(size_t)2 * T] = st;
  o[(size_t)3 * T] = stt;
}

// Second launch, ONE workgroup: the row groups of a column are added in their order, the columns' scores and moments through the tree.
// out[0] = mean over the columns of the per-column score; out[1] = the score of all N*T frames, from the columns' centred sums of squares
// and the spread of their means (sum (x - m)^2 = sum_c [ sum_r (x - m_c)^2 + N (m_c - m)^2 ]).
__global__ __launch_bounds__(256) void ev_final_kernel(const float* __restrict__ value, const float* __restrict__ target, int N, int T, int R,
                                                      const double* __restrict__ scratch, float* __restrict__ out) {
  __shared__ double sh[256];
  const double inv_n = 1.0 / (double)N;
  double ev = 0, m2d = 0, m2t = 0, md = 0, mt = 0;
  for (int t = threadIdx.x; t < T; t += 256) {
    double s[4] = {0, 0, 0, 0};
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += scratch[((size_t)r * 4 + q) * T + t];
    const double cd = s[1] - s[0] * s[0] * inv_n, ct = s[3] - s[2] * s[2] * inv_n;   // centred sums of squares of the column
    ev += ev_score(cd * inv_n, ct * inv_n);
    m2d += cd;
    m2t += ct;
    const double t0 = (double)target[t], d0 = t0 - (double)value[t];
    md += d0 + s[0] * inv_n;
    mt += t0 + s[2] * inv_n;
  }
  ev = block_sum<256>(ev, sh);
  m2d = block_sum<256>(m2d, sh);
  m2t = block_sum<256>(m2t, sh);
  const double gd = block_sum<256>(md, sh) / (double)T, gt = block_sum<256>(mt, sh) / (double)T;
  double bd = 0, bt = 0;
  for (int t = threadIdx.x; t < T; t += 256) {
    double s0 = 0, s2 = 0;
    for (int r = 0; r < R; ++r) {
      s0 += scratch[((size_t)r * 4) * T + t];
      s2 += scratch[((size_t)r * 4 + 2) * T + t];
    }
    const double t0 = (double)target[t], d0 = t0 - (double)value[t];
    const double ed = (d0 + s0 * inv_n) - gd, et = (t0 + s2 * inv_n) - gt;
    bd += ed * ed;
    bt += et * et;
  }
  bd = block_sum<256>(bd, sh);
  bt = block_sum<256>(bt, sh);
  if (threadIdx.x == 0) {
    const double frames = (double)N * (double)T;
    out[0] = (float)(ev / (double)T);
    out[1] = (float)ev_score((m2d + (double)N * bd) / frames, (m2t + (double)N * bt) / frames);
  }
}

// RewardSum / StepCounter over a rollout: one thread per environment, sequential in t, forwards; a 64 x 64 tile is transposed through LDS
// so that the global accesses run along t (gae_kernel of train_ops.hip, the other way round).  The running return is a float32 sum, one
// add per step; a done frame carries the finished episode's return and length, the frame behind it starts from 0.
constexpr int EP_TT = 64;
__global__ __launch_bounds__(64) void episode_scan_kernel(const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                                         float* __restrict__ ret_state, int* __restrict__ len_state,
                                                         float* __restrict__ episode_reward, int* __restrict__ step_count, int N, int T) {
  __shared__ float s_r[64][EP_TT + 1];
  __shared__ int s_n[64][EP_TT + 1];
  __shared__ unsigned char s_d[64][EP_TT + 4];
  const int env0 = blockIdx.x * 64, lane = threadIdx.x;
  const bool live = env0 + lane < N;
  float run = live ? ret_state[env0 + lane] : 0.f;
  int cnt = live ? len_state[env0 + lane] : 0;
  for (int t0 = 0; t0 < T; t0 += EP_TT) {
    const int len = min(EP_TT, T - t0);
    for (int e = 0; e < 64; ++e) {
      const int env = env0 + e;
      if (env >= N) break;
      if (lane < len) {
        s_r[e][lane] = reward[(size_t)env * T + t0 + lane];
        s_d[e][lane] = done[(size_t)env * T + t0 + lane];
      }
    }
    __syncthreads();
    if (live) {
      for (int k = 0; k < len; ++k) {
        run += s_r[lane][k];
        cnt += 1;
        s_r[lane][k] = run;
        s_n[lane][k] = cnt;
        if (s_d[lane][k]) {
          run = 0.f;
          cnt = 0;
        }
      }
    }
    __syncthreads();
    for (int e = 0; e < 64; ++e) {
      const int env = env0 + e;
      if (env >= N) break;
      if (lane < len) {
        episode_reward[(size_t)env * T + t0 + lane] = s_r[e][lane];
        step_count[(size_t)env * T + t0 + lane] = s_n[e][lane];
      }
    }
    __syncthreads();
  }
  if (live) {
    ret_state[env0 + lane] = run;
    len_state[env0 + lane] = cnt;
  }
}

// sums = (sum of episode_reward, sum of step_count, count) over the done frames: ONE workgroup, thread-strided partial sums, then the tree.
__global__ __launch_bounds__(1024) void episode_sums_kernel(const unsigned char* __restrict__ done, const float* __restrict__ episode_reward,
                                                          const int* __restrict__ step_count, long long n, double* __restrict__ sums) {
  __shared__ double sh[1024];
  double a = 0, b = 0, c = 0;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    if (done[i]) {
      a += (double)episode_reward[i];
      b += (double)step_count[i];
      c += 1.0;
    }
  }
  a = block_sum<1024>(a, sh);
  b = block_sum<1024>(b, sh);
  c = block_sum<1024>(c, sh);
  if (threadIdx.x == 0) {
    sums[0] = a;
    sums[1] = b;
    sums[2] = c;
  }
}

}  // namespace

extern "C" {

int grl_stats_accumulate(const float* src, int n, double* acc, hipStream_t stream) {
  if (!src || !acc || n < 1 || n > 32) return -2;
  hipLaunchKernelGGL(stats_accumulate_kernel, dim3(1), dim3(64), 0, stream, src, n, acc);
  GRL_CHECK_LAUNCH();
  return 0;
}

int grl_explained_variance_scratch_bytes(int n_env, int n_steps) {
  if (n_env <= 0 || n_steps <= 0) return -2;
  const long long bytes = (long long)((n_env + EV_ROWS - 1) / EV_ROWS) * 4 * n_steps * (long long)sizeof(double);
  return bytes > 0x7fffffffLL ? -2 : (int)bytes;
}

int grl_explained_variance(const float* value, const float* target, int n_env, int n_steps, void* scratch, float* out, hipStream_t stream) {
  const int R = (n_env + EV_ROWS - 1) / EV_ROWS;
  if (!value || !target || !scratch || !out || grl_explained_variance_scratch_bytes(n_env, n_steps) < 0 || R > 65535) return -2;
  hipLaunchKernelGGL(ev_partial_kernel, dim3((n_steps + 63) / 64, R), dim3(64), 0, stream, value, target, n_env, n_steps,
                     static_cast<double*>(scratch));
  GRL_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_final_kernel, dim3(1), dim3(256), 0, stream, value, target, n_env, n_steps, R, static_cast<const double*>(scratch),
                     out);
  GRL_CHECK_LAUNCH();
  return 0;
}

int grl_episode_scan(const float* reward, const unsigned char* done, float* ret_state, int* len_state, float* episode_reward,
                     int* step_count, double* sums, int n_env, int n_steps, hipStream_t stream) {
  if (!reward || !done || !ret_state || !len_state || !episode_reward || !step_count || !sums || n_env <= 0 || n_steps <= 0) return -2;
  hipLaunchKernelGGL(episode_scan_kernel, dim3((n_env + 63) / 64), dim3(64), 0, stream, reward, done, ret_state, len_state, episode_reward,
                     step_count, n_env, n_steps);
  GRL_CHECK_LAUNCH();
  hipLaunchKernelGGL(episode_sums_kernel, dim3(1), dim3(1024), 0, stream, done, episode_reward, step_count, (long long)n_env * n_steps, sums);
  GRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
