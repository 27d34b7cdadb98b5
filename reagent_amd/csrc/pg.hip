// pg.hip — the policy-gradient step's own kernels: the ragged reward-to-go over packed trajectories (clamp, reverse
// discounted scan, whitening / mean subtraction per trajectory) and the categorical policy head (temperature log-softmax,
// the logged action's log-probability, importance ratio, REINFORCE's clamp or PPO's clip, entropy bonus, baseline MSE and
// the gradients with respect to scores and values).  Per-row VALU work on [N] and [N, A] arrays; no atomics: loss sums
// leave as per-workgroup partials in a fixed order (rg_reduce_sum finishes them).
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"  // shfl_xor_f64, wave_sum_f64

// The scan is held to the reference's bits: a multiply and an add, each rounded.  hipcc contracts a * b + c into a fused
// multiply-add by default, and the runtime's __fmul_rn / __fadd_rn are plain operators compiled under that default: inlined,
// they fuse (v_fmac_f32 in the scan's chain).  No contraction in this unit, and its individually rounded operations are
// the operators below, compiled under this pragma.
#pragma clang fp contract(off)

namespace rg {

__device__ __forceinline__ float pg_add(float a, float b) { return a + b; }
__device__ __forceinline__ float pg_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float pg_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float pg_div(float a, float b) { return a / b; }

constexpr int PG_THREADS = 256;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr float PG_INVALID_ACTION = -1e10f;  // INVALID_ACTION_CONSTANT (models/dqn.py:13)

// discounted_returns (training/utils.py:42-54) on clamp(reward, max = clip) (reinforce_trainer.py:106-108), then whiten
// (utils.py:32-39) or REINFORCE's mean subtraction (:113-114), then clamp(min = 0) (:115-116).  One wave per trajectory
// [offsets[t], offsets[t + 1]).  The scan walks 64-element chunks from the trajectory's END: lane k of a chunk owns the
// k-th element from the chunk's end, every lane runs the same 64-step chain run = r[k] + gamma * run on lane-broadcast
// values (multiply and add rounded separately, as the reference's two tensor operations are) and lane k keeps step k.
// The mean and the centred sum of squares are two wave reductions (per-lane and across lanes in double) over the stored
// values, each lane reading back only what it wrote itself.
__global__ void pg_returns_kernel(const float* __restrict__ reward, const int32_t* __restrict__ offsets, int T, long N,
                                  float gamma, float clip, int normalize, int subtract_mean, int clamp_min,
                                  float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave_t = blockIdx.x * PG_WAVES + (threadIdx.x >> 6);
  const int t = wave_t < T ? wave_t : T - 1;  // a wave past the last trajectory repeats it and writes nothing
  long s = offsets[t], e = offsets[t + 1];
  s = s < 0 ? 0 : (s > N ? N : s);  // offsets are the caller's; no address outside [0, N) is formed whatever they hold
  e = e < s ? s : (e > N ? N : e);
  if (wave_t >= T) e = s;
  const long len = e - s;
  const int chunks = (int)((len + 63) >> 6);
  float run = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const long i = e - 1 - ((long)c << 6) - lane;
    const bool valid = i >= s;
    float r = valid ? reward[i] : 0.f;
    r = r > clip ? clip : r;  // torch.clamp(max=): a NaN stays a NaN
    float mine = r;           // gamma == 0: the copy the reference makes
    if (gamma != 0.f) {
#pragma unroll 1
      for (int k0 = 0; k0 < 64; k0 += 16) {  // (16 broadcast values in flight: 64 would not fit the scalar registers)
#pragma unroll
        for (int k = k0; k < k0 + 16; ++k) {
          run = pg_add(shfl_idx(r, k), pg_mul(gamma, run));
          if (lane == k) mine = run;
        }
      }
    }
    if (valid && !normalize && !subtract_mean) mine = clamp_min ? (mine < 0.f ? 0.f : mine) : mine;
    if (valid) out[i] = mine;
  }
  if (!normalize && !subtract_mean) return;  // (wave-uniform)
  double sum = 0.0;
  for (int c = 0; c < chunks; ++c) {
    const long i = e - 1 - ((long)c << 6) - lane;
    if (i >= s) sum += (double)out[i];
  }
  const double mean = len > 0 ? wave_sum_f64(sum) / (double)len : 0.0;
  float denom = 1.f;
  if (normalize) {  // x.std(unbiased=False) + EPS, EPS = float64's epsilon added in fp32
    double ss = 0.0;
    for (int c = 0; c < chunks; ++c) {
      const long i = e - 1 - ((long)c << 6) - lane;
      if (i >= s) {
        const double d = (double)out[i] - mean;
        ss += d * d;
      }
    }
    const double var = len > 0 ? wave_sum_f64(ss) / (double)len : 0.0;
    denom = pg_add((float)sqrt(var), 2.220446049250313e-16f);
  }
  const float mean_f = subtract_mean ? (float)mean : 0.f;
  for (int c = 0; c < chunks; ++c) {
    const long i = e - 1 - ((long)c << 6) - lane;
    if (i >= s) {
      float v = out[i];
      if (subtract_mean) v = pg_sub(v, mean_f);
      if (normalize) v = pg_div(v, denom);
      if (clamp_min) v = v < 0.f ? 0.f : v;
      out[i] = v;
    }
  }
}

template <int G>
__device__ __forceinline__ double pg_group_max(double v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v = fmax(v, shfl_xor_f64(v, off));
  return v;
}
template <int G>
__device__ __forceinline__ double pg_group_sum(double v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) v += shfl_xor_f64(v, off);
  return v;
}

__device__ __forceinline__ double pg_block_sum(double v, double* scratch) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
  __syncthreads();
  return s;
}

struct PgHeadArgs {
  const float* scores;
  long ld_scores;
  const float* mask;  // possible_actions_mask [N, A] contiguous, or NULL: the scores already carry the penalty
  const void* action;
  int action_i64;
  long ld_action;
  const float* returns;
  const float* values;
  const float* old_log_prob;
  double temperature, log_clip, lo, hi, entropy_weight, value_scale;
  int mode, N, A, vec_in, vec_out;
  float* dscores;
  long ld_dscores;
  float *dvalues, *log_prob, *ratio, *advantage, *policy_partials, *value_partials;
};

// SoftmaxActionSampler.log_prob / entropy (gym/policies/samplers/discrete_sampler.py:45-79) on scores / temperature and
// the losses of reinforce_trainer.py:105-132 and ppo_trainer.py:127-152 with their gradients.  A group of G lanes per
// row, lane g of the group holding actions 4g .. 4g + 3 in registers (an absent action scores -inf: probability 0).
// The row's arithmetic runs in double on the fp32 inputs and is rounded once where it is stored: a summed loss over
// thousands of rows then carries the rounding of its sum, not a random walk of the rows' log-probability roundings
// (A double exponentials per row are nothing next to the scorer's forward).
template <int G>
__global__ void pg_head_kernel(const PgHeadArgs a) {
  __shared__ double scratch[PG_WAVES];
  constexpr int ROWS = PG_THREADS / G;
  const int g = threadIdx.x & (G - 1);
  const int wave_row = blockIdx.x * ROWS + threadIdx.x / G;
  const bool live = wave_row < a.N;  // a group past the last row repeats it and writes nothing
  const long row = live ? wave_row : a.N - 1;
  const int A = a.A, j0 = 4 * g;
  double z[4];
  float act[4];
  {
    const float* sp = a.scores + row * a.ld_scores;
    float sc[4];
    if (a.vec_in && j0 + 4 <= A) {
      const f32x4 v = *(const f32x4*)(sp + j0);
      sc[0] = v[0], sc[1] = v[1], sc[2] = v[2], sc[3] = v[3];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) sc[k] = j0 + k < A ? sp[j0 + k] : -INFINITY;
    }
    if (a.mask) {  // FullyConnectedDQN.forward (models/dqn.py:60-62): x + (1 - mask) * INVALID_ACTION_CONSTANT in fp32
      const float* mp = a.mask + row * A;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < A) sc[k] = pg_add(sc[k], pg_mul(pg_sub(1.f, mp[j0 + k]), PG_INVALID_ACTION));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = j0 + k < A ? (double)sc[k] / a.temperature : -(double)INFINITY;
    if (a.action_i64) {
      const int64_t* ap = (const int64_t*)a.action + row * a.ld_action;
#pragma unroll
      for (int k = 0; k < 4; ++k) act[k] = j0 + k < A ? (float)ap[j0 + k] : -INFINITY;
    } else {
      const float* ap = (const float*)a.action + row * a.ld_action;
#pragma unroll
      for (int k = 0; k < 4; ++k) act[k] = j0 + k < A ? ap[j0 + k] : -INFINITY;
    }
  }
  // action.argmax(dim=1): the first maximum (discrete_sampler.py:71)
  float best = act[0];
  int best_j = j0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (act[k] > best) best = act[k], best_j = j0 + k;
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    const float other = shfl_xor(best, off);
    const int other_j = shfl_xor(best_j, off);
    if (other > best || (other == best && other_j < best_j)) best = other, best_j = other_j;
  }
  // Categorical(logits = z): logits - logsumexp(logits), probs = softmax
  const double m = pg_group_max<G>(fmax(fmax(z[0], z[1]), fmax(z[2], z[3])));
  double p[4], sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p[k] = exp(z[k] - m);
    sum += p[k];
  }
  sum = pg_group_sum<G>(sum);
  const double lse = m + log(sum);
  double logp[4], ent = 0.0, lsel = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    logp[k] = z[k] - lse;
    p[k] = p[k] / sum;
    ent -= p[k] == 0.0 ? 0.0 : p[k] * logp[k];
    if (j0 + k == best_j) lsel = logp[k];
  }
  const double H = pg_group_sum<G>(ent);
  const double l = pg_group_sum<G>(lsel);  // one lane of the group holds it, the others add 0
  const double ret = a.returns[row];
  const double v = a.values ? (double)a.values[row] : 0.0;
  const double adv = ret - v;
  const double w = a.entropy_weight;
  double rho = 1.0, gl, loss;
  if (a.mode == RG_PG_REINFORCE) {
    loss = -(adv * l);
    gl = -adv;
  } else if (a.mode == RG_PG_REINFORCE_OFF_POLICY) {
    const double d = l - (double)a.old_log_prob[row];
    rho = exp(fmin(d, a.log_clip));
    loss = -(adv * rho);
    gl = d <= a.log_clip ? loss : 0.0;
  } else {
    rho = exp(l - (double)a.old_log_prob[row]);
    const double s1 = adv * rho, s2 = adv * fmin(fmax(rho, a.lo), a.hi);
    loss = -fmin(s1, s2);
    gl = (s1 < s2 || (rho >= a.lo && rho <= a.hi)) ? -s1 : 0.0;
  }
  if (w != 0.0) loss -= w * H;
  float dz[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double d = gl * ((j0 + k == best_j ? 1.0 : 0.0) - p[k]);
    if (w != 0.0 && p[k] != 0.0) d += w * p[k] * (logp[k] + H);
    dz[k] = (float)(d / a.temperature);
  }
  double vloss = 0.0;
  if (live) {
    float* dp = a.dscores + row * a.ld_dscores;
    if (a.vec_out && j0 + 4 <= A) {
      const f32x4 o = {dz[0], dz[1], dz[2], dz[3]};
      *(f32x4*)(dp + j0) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < A) dp[j0 + k] = dz[k];
    }
    if (g == 0) {
      if (a.log_prob) a.log_prob[row] = (float)l;
      if (a.ratio) a.ratio[row] = (float)rho;
      if (a.advantage) a.advantage[row] = (float)adv;
      if (a.values) {
        const double d = v - ret;
        a.dvalues[row] = (float)(2.0 * a.value_scale * d);
        vloss = a.value_scale * (d * d);
      }
    }
  }
  const double ps = pg_block_sum(live && g == 0 ? loss : 0.0, scratch);
  if (threadIdx.x == 0) a.policy_partials[blockIdx.x] = (float)ps;
  if (a.values) {  // (uniform over the launch)
    const double vs = pg_block_sum(vloss, scratch);
    if (threadIdx.x == 0) a.value_partials[blockIdx.x] = (float)vs;
  }
}

static int pg_group(int A) { return A <= 4 ? 1 : (A <= 16 ? 4 : (A <= 64 ? 16 : 64)); }

}  // namespace rg

using namespace rg;

extern "C" {

int rg_pg_returns(const float* reward, const int32_t* offsets, int num_trajectories, int64_t n, double gamma,
                  double reward_clip, int normalize, int subtract_mean, int clamp_min, float* out, rg_stream_t stream) {
  if (num_trajectories < 1 || n < 0 || !offsets) return RG_EINVAL;
  if (n > 0 && (!reward || !out)) return RG_EINVAL;
  if (n == 0) return RG_OK;
  RG_LAUNCH(pg_returns_kernel, dim3((num_trajectories + PG_WAVES - 1) / PG_WAVES), dim3(PG_THREADS), (hipStream_t)stream,
            reward, offsets, num_trajectories, (long)n, (float)gamma, (float)reward_clip, normalize != 0, subtract_mean != 0,
            clamp_min != 0, out);
  return (int)hipGetLastError();
}

int rg_pg_head_partials(int n, int num_actions) {
  if (n < 1 || num_actions < 1 || num_actions > RG_PG_MAX_ACTIONS) return 0;
  const int rows = PG_THREADS / pg_group(num_actions);
  return (n + rows - 1) / rows;
}

int rg_pg_head(const float* scores, int64_t ld_scores, const float* possible_actions_mask, const void* action,
               int action_is_int64, int64_t ld_action, const float* returns, const float* values, const float* old_log_prob,
               double temperature, int mode, double clip, double entropy_weight, double value_scale, int n, int num_actions,
               float* dscores, int64_t ld_dscores, float* dvalues, float* log_prob, float* ratio, float* advantage,
               float* policy_partials, float* value_partials, rg_stream_t stream) {
  if (!scores || !action || !returns || !dscores || !policy_partials) return RG_EINVAL;
  if (n < 1 || num_actions < 1 || num_actions > RG_PG_MAX_ACTIONS) return RG_EINVAL;
  if (ld_scores < num_actions || ld_action < num_actions || ld_dscores < num_actions) return RG_EINVAL;
  if (mode != RG_PG_REINFORCE && mode != RG_PG_REINFORCE_OFF_POLICY && mode != RG_PG_PPO) return RG_EINVAL;
  if (mode != RG_PG_REINFORCE && !old_log_prob) return RG_EINVAL;
  if (!(temperature > 0.0)) return RG_EINVAL;
  if (mode == RG_PG_REINFORCE_OFF_POLICY && !(clip > 0.0)) return RG_EINVAL;
  if (mode == RG_PG_PPO && !(clip >= 0.0 && clip <= 1.0)) return RG_EINVAL;
  if (values && (!dvalues || !value_partials)) return RG_EINVAL;
  PgHeadArgs a;
  a.scores = scores, a.ld_scores = (long)ld_scores, a.mask = possible_actions_mask;
  a.action = action, a.action_i64 = action_is_int64 != 0, a.ld_action = (long)ld_action;
  a.returns = returns, a.values = values, a.old_log_prob = old_log_prob;
  a.temperature = temperature;
  // torch.clamp(x, max = math.log(float(clip_param))) / torch.clamp(x, 1 - eps, 1 + eps): the python doubles as they are
  a.log_clip = mode == RG_PG_REINFORCE_OFF_POLICY ? log(clip) : 0.0;
  a.lo = 1.0 - clip, a.hi = 1.0 + clip;
  a.entropy_weight = entropy_weight, a.value_scale = value_scale;
  a.mode = mode, a.N = n, a.A = num_actions;
  a.vec_in = (ld_scores & 3) == 0 && (((uintptr_t)scores) & 15) == 0;
  a.vec_out = (ld_dscores & 3) == 0 && (((uintptr_t)dscores) & 15) == 0;
  a.dscores = dscores, a.ld_dscores = (long)ld_dscores;
  a.dvalues = dvalues, a.log_prob = log_prob, a.ratio = ratio, a.advantage = advantage;
  a.policy_partials = policy_partials, a.value_partials = value_partials;
  const dim3 grid(rg_pg_head_partials(n, num_actions)), block(PG_THREADS);
  switch (pg_group(num_actions)) {
    case 1: RG_LAUNCH(pg_head_kernel<1>, grid, block, (hipStream_t)stream, a); break;
    case 4: RG_LAUNCH(pg_head_kernel<4>, grid, block, (hipStream_t)stream, a); break;
    case 16: RG_LAUNCH(pg_head_kernel<16>, grid, block, (hipStream_t)stream, a); break;
    default: RG_LAUNCH(pg_head_kernel<64>, grid, block, (hipStream_t)stream, a); break;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
