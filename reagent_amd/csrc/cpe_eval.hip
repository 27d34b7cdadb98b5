// cpe_eval.hip — counterfactual policy evaluation of the discrete DQN trainers on a device-resident EvaluationDataPage
// (reagent/evaluation/evaluation_data_page.py, doubly_robust_estimator.py, sequential_doubly_robust_estimator.py, cpe.py):
//   rg_cpe_page_rows       the row arithmetic of create_from_tensors_dqn (:334-378, 408-433), one launch per validation batch
//   rg_cpe_episode_values  compute_values_for_mdps (:523-540), one lane per episode
//   rg_cpe_dr_rows         the row quantities of the one-step DM / IPS / DR estimates and of sequential DR, and their totals
//   rg_cpe_sdr             the sequential-DR recurrence (:70-95), one lane per episode
//   rg_cpe_bootstrap       bootstrapped_std_error_of_mean (cpe.py:176-191), one workgroup per resample
// These are row-wise, gather-bound and latency-bound launches: no matrix cores, no LDS tiles.  No atomics; sums are double
// and added in a fixed order (wave butterflies, waves in order, workgroups in order), so two runs give the same bits.  Row and
// episode indices read from device memory (episode offsets) are clamped to the page before use.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"        // wave_sum_f64, lds_tree_sum
#include "rg_dqn_head_row.h"  // masked_max_row, masked_softmax_stats / _p: the rules rg_dqn_head and rg_cpe_head run
#include "rg_philox.h"

// every row value is held to the reference's fp32 operation order: each multiply, add and divide is rounded on its own
// (the shared row rules above were compiled before this line, so they are the bits rg_cpe_head gives)
#pragma clang fp contract(off)

namespace rg {

constexpr int CPE_THREADS = 256;  // one row (or one episode) a thread
constexpr int CPE_WAVES = CPE_THREADS / 64;
constexpr int CPE_SUMS = 5;       // logged_rewards, dm, model_rewards_for_logged_action, ips, dr
constexpr int CPE_FINISH_LANES = 32;  // slices one finishing pass reads at once, per sum (8 segments, 5 used)

struct CpePageArgs {
  const float *q, *q_cpe, *reward_est, *action, *mask, *reward, *boosts;
  float temperature;
  int B, A, M;
  float *logged_rewards, *propensities, *mr_logged, *mm_logged, *mmv_logged;
  int64_t* eval_idx;
};

// Thread t of workgroup g has row r = 256 g + t and walks its A (and M A) entries left to right.
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1) cpe_page_rows_kernel(const CpePageArgs a) {
  const long r = (long)blockIdx.x * CPE_THREADS + threadIdx.x;
  if (r >= a.B) return;
  const int A = a.A, M = a.M;
  const long o = r * A, om = r * M * A;
  const float* act = a.action + o;
  const float* mask = a.mask ? a.mask + o : nullptr;
  // boost_rewards (dqn_trainer_base.py:216-241): reward + sum_a action * boost
  float rb = 0.f;
  if (a.boosts)
    for (int j = 0; j < A; ++j) rb += act[j] * a.boosts[j];
  a.logged_rewards[r] = a.reward[r] + rb;
  // eval_action_idxs = get_max_q_values(q, possible_actions_mask)[1]
  float best_t;
  int best_i;
  masked_max_row(a.q + o, a.q + o, mask, A, best_t, best_i);
  a.eval_idx[r] = best_i;
  // model_propensities = masked_softmax(q, possible_actions_mask, temperature)
  float mx, den;
  masked_softmax_stats(a.q + o, mask, A, a.temperature, mx, den);
  for (int j = 0; j < A; ++j)
    a.propensities[o + j] = masked_softmax_p(a.q[o + j], mask ? mask[j] : 1.f, a.temperature, mx, den);
  // sum_a model[:, i A + a] * action_mask, metric by metric (metric 0 of the reward network is the reward itself)
  for (int i = 0; i < M; ++i) {
    float sr = 0.f, sv = 0.f;
    for (int j = 0; j < A; ++j) {
      sr += a.reward_est[om + (long)i * A + j] * act[j];
      if (i > 0) sv += a.q_cpe[om + (long)i * A + j] * act[j];
    }
    if (i == 0) {
      a.mr_logged[r] = sr;
    } else {
      a.mm_logged[r * (M - 1) + (i - 1)] = sr;
      a.mmv_logged[r * (M - 1) + (i - 1)] = sv;
    }
  }
}

// episode e is rows [begin, end) of the sorted page; the offsets come from device memory and are clamped to it
__device__ __forceinline__ void episode_span(const int32_t* __restrict__ offsets, int e, int rows, int& begin, int& end) {
  int b = offsets[e], n = offsets[e + 1];
  b = b < 0 ? 0 : (b > rows ? rows : b);
  n = n < b ? b : (n > rows ? rows : n);
  begin = b;
  end = n;
}

// v[x] = c[x] + v[x + 1] * fp32(pow(gamma, double(seq[x + 1] - seq[x]))) backwards through the episode; v of its last row is c
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1)
    cpe_episode_values_kernel(const float* __restrict__ c, long ld, const int64_t* __restrict__ seq,
                              const int32_t* __restrict__ offsets, int episodes, int rows, double gamma, float* v, long ldv) {
  const int e = blockIdx.x * CPE_THREADS + threadIdx.x;
  if (e >= episodes) return;
  int begin, end;
  episode_span(offsets, e, rows, begin, end);
  if (end <= begin) return;
  float val = c[(long)(end - 1) * ld];
  v[(long)(end - 1) * ldv] = val;
  for (int x = end - 2; x >= begin; --x) {
    const float g = (float)pow(gamma, (double)(seq[x + 1] - seq[x]));
    const float t = val * g;
    val = c[(long)x * ld] + t;
    v[(long)x * ldv] = val;
  }
}

struct CpeDrArgs {
  const float *prop, *mask, *mr, *mv, *logged_p, *logged_r, *mr_logged;
  long ld_mr, ld_mv, ld_r, ld_mrl;
  int N, A;
  float *tp, *iw, *est, *sv, *ql;  // est [3, N]: dm, ips, dr
  double* partials;                // [CPE_SUMS][P]
  int P;
};

// Thread t of workgroup g has row r = 256 g + t.  The four sums over actions accumulate left to right in fp32; the row's five
// terms of the totals are added in double: across the wave by butterflies, across the four waves through LDS in wave order.
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1) cpe_dr_rows_kernel(const CpeDrArgs a) {
  __shared__ double wave_sums[CPE_WAVES][CPE_SUMS];
  const long r = (long)blockIdx.x * CPE_THREADS + threadIdx.x;
  double t[CPE_SUMS];
#pragma unroll
  for (int k = 0; k < CPE_SUMS; ++k) t[k] = 0.0;
  if (r < a.N) {
    const float* p = a.prop + r * a.A;
    const float* m = a.mask + r * a.A;
    const float* mr = a.mr + r * a.ld_mr;
    const float* mv = a.mv + r * a.ld_mv;
    float tp = 0.f, dm = 0.f, sv = 0.f, ql = 0.f;
    for (int j = 0; j < a.A; ++j) {
      tp += p[j] * m[j];
      dm += p[j] * mr[j];
      sv += p[j] * mv[j];
      ql += mv[j] * m[j];
    }
    const float iw = tp / a.logged_p[r];
    const float rew = a.logged_r[r * a.ld_r], mrl = a.mr_logged[r * a.ld_mrl];
    const float ips = iw * rew;
    const float dr = iw * (rew - mrl) + dm;
    a.tp[r] = tp;
    a.iw[r] = iw;
    a.est[r] = dm;
    a.est[(long)a.N + r] = ips;
    a.est[2L * a.N + r] = dr;
    a.sv[r] = sv;
    a.ql[r] = ql;
    t[0] = (double)rew, t[1] = (double)dm, t[2] = (double)mrl, t[3] = (double)ips, t[4] = (double)dr;
  }
#pragma unroll
  for (int k = 0; k < CPE_SUMS; ++k) t[k] = wave_sum_f64(t[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < CPE_SUMS; ++k) wave_sums[threadIdx.x >> 6][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < CPE_SUMS) {
    const int k = threadIdx.x;
    a.partials[(long)k * a.P + blockIdx.x] = ((wave_sums[0][k] + wave_sums[1][k]) + wave_sums[2][k]) + wave_sums[3][k];
  }
}

// The finishing launch, one workgroup: thread 32 k + j adds the slices j, j + 32, ... of sum k in slice order, the 32 lane sums
// meet in LDS by a fixed tree, and lane 0 of the segment writes the total.
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1)
    cpe_dr_finish_kernel(const double* __restrict__ partials, int P, double* __restrict__ totals) {
  __shared__ double sums[CPE_THREADS];
  const int k = threadIdx.x / CPE_FINISH_LANES, j = threadIdx.x % CPE_FINISH_LANES;
  double v = 0.0;
  if (k < CPE_SUMS)
    for (int p = j; p < P; p += CPE_FINISH_LANES) v += partials[(long)k * P + p];
  sums[threadIdx.x] = v;
  lds_tree_sum<CPE_FINISH_LANES>(sums);
  if (j == 0 && k < CPE_SUMS) totals[k] = sums[threadIdx.x];
}

// d = sv[j] + iw[j] * ((r[j] + g * d) - q[j]);  e = e * g + r[j], backwards through the episode, g = fp32(gamma)
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1)
    cpe_sdr_kernel(const float* __restrict__ sv, const float* __restrict__ iw, const float* __restrict__ rew, long ld_r,
                   const float* __restrict__ ql, const int32_t* __restrict__ offsets, int episodes, int rows, float g,
                   float* __restrict__ doubly_robust, float* __restrict__ episode_value) {
  const int ep = blockIdx.x * CPE_THREADS + threadIdx.x;
  if (ep >= episodes) return;
  int begin, end;
  episode_span(offsets, ep, rows, begin, end);
  float d = 0.f, e = 0.f;
  for (int j = end - 1; j >= begin; --j) {
    const float r = rew[(long)j * ld_r];
    const float gd = g * d;
    const float inner = (r + gd) - ql[j];
    const float w = iw[j] * inner;
    d = sv[j] + w;
    const float eg = e * g;
    e = eg + r;
  }
  doubly_robust[ep] = d;
  episode_value[ep] = e;
}

constexpr int CPE_MAX_COLUMNS = RG_CPE_BOOTSTRAP_MAX_COLUMNS;

// Workgroup k is resample k.  Lane t of its THREADS lanes takes the Philox groups t, t + THREADS, ... (draws 4 g .. 4 g + 3 of
// the resample, those below sample_size), adds what it gathers per column in double, and the lane sums meet by wave
// butterflies and the wave sums in wave order.  One index stream serves every column.  THREADS is 64 where one wave holds
// every group (sample_size <= 256), else 256: the launch shape, and with it the order of the adds, depends on the arguments alone.
template <int THREADS>
__global__ void RG_LAUNCH_BOUNDS(THREADS, 1)
    cpe_bootstrap_kernel(const float* __restrict__ values, long ld, int C, int n, int sample_size, int K, uint64_t seed,
                         double* __restrict__ means) {
  constexpr int WAVES = THREADS / 64;
  __shared__ double wave_sums[WAVES][CPE_MAX_COLUMNS];
  const int k = blockIdx.x;
  const int groups = (int)(((long)sample_size + 3) / 4);
  double s[CPE_MAX_COLUMNS];
#pragma unroll
  for (int c = 0; c < CPE_MAX_COLUMNS; ++c) s[c] = 0.0;
  for (int g = threadIdx.x; g < groups; g += THREADS) {
    uint32_t u[4];
    philox4x32_10(seed, (uint64_t)g, (uint64_t)k, u);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if ((long)g * 4 + w < sample_size) {
        const long idx = (long)(((uint64_t)u[w] * (uint64_t)(uint32_t)n) >> 32);  // < n by construction
#pragma unroll
        for (int c = 0; c < CPE_MAX_COLUMNS; ++c)
          if (c < C) s[c] += (double)values[(long)c * ld + idx];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CPE_MAX_COLUMNS; ++c)
    if (c < C) s[c] = wave_sum_f64(s[c]);  // (C is the same in every lane)
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < CPE_MAX_COLUMNS; ++c) wave_sums[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    double total = wave_sums[0][c];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) total += wave_sums[w][c];
    means[(long)c * K + k] = total / (double)sample_size;  // sample_size == 0: 0 / 0 = NaN, np.mean of nothing
  }
}

// Workgroup c: the population standard deviation (ddof 0) of column c's K means in two passes, each a strided lane sum in
// resample order and a fixed LDS tree.
__global__ void RG_LAUNCH_BOUNDS(CPE_THREADS, 1)
    cpe_bootstrap_finish_kernel(const double* __restrict__ means, int K, double* __restrict__ std_out) {
  __shared__ double sums[CPE_THREADS];
  const double* m = means + (long)blockIdx.x * K;
  double v = 0.0;
  for (int i = threadIdx.x; i < K; i += CPE_THREADS) v += m[i];
  sums[threadIdx.x] = v;
  lds_tree_sum<CPE_THREADS>(sums);
  const double mean = sums[0] / (double)K;
  __syncthreads();
  v = 0.0;
  for (int i = threadIdx.x; i < K; i += CPE_THREADS) {
    const double d = m[i] - mean;
    v += d * d;
  }
  sums[threadIdx.x] = v;
  lds_tree_sum<CPE_THREADS>(sums);
  if (threadIdx.x == 0) std_out[blockIdx.x] = sqrt(sums[0] / (double)K);
}

static inline int cpe_blocks(int n) { return (n + CPE_THREADS - 1) / CPE_THREADS; }

}  // namespace rg

using namespace rg;

extern "C" {

int rg_cpe_page_rows(const float* q, const float* q_cpe, const float* reward_est, const float* action,
                     const float* possible_actions_mask, const float* reward, const float* reward_boosts, double temperature,
                     int batch, int num_actions, int num_metrics, float* logged_rewards, float* model_propensities,
                     int64_t* eval_action_idxs, float* model_rewards_for_logged_action,
                     float* model_metrics_for_logged_action, float* model_metrics_values_for_logged_action,
                     rg_stream_t stream) {
  if (batch < 1 || num_actions < 1 || num_metrics < 1) return RG_EINVAL;
  if (!q || !reward_est || !action || !reward || !logged_rewards || !model_propensities || !eval_action_idxs ||
      !model_rewards_for_logged_action)
    return RG_EINVAL;
  if (num_metrics > 1 && (!q_cpe || !model_metrics_for_logged_action || !model_metrics_values_for_logged_action))
    return RG_EINVAL;
  CpePageArgs a;
  a.q = q, a.q_cpe = q_cpe, a.reward_est = reward_est, a.action = action, a.mask = possible_actions_mask;
  a.reward = reward, a.boosts = reward_boosts, a.temperature = (float)temperature;
  a.B = batch, a.A = num_actions, a.M = num_metrics;
  a.logged_rewards = logged_rewards, a.propensities = model_propensities, a.eval_idx = eval_action_idxs;
  a.mr_logged = model_rewards_for_logged_action, a.mm_logged = model_metrics_for_logged_action;
  a.mmv_logged = model_metrics_values_for_logged_action;
  RG_LAUNCH(cpe_page_rows_kernel, dim3(cpe_blocks(batch)), dim3(CPE_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_cpe_episode_values(const float* column, int64_t ld, const int64_t* sequence_number, const int32_t* episode_offsets,
                          int episodes, int rows, double gamma, float* values, int64_t ld_values, rg_stream_t stream) {
  if (episodes < 1 || rows < 1 || episodes > rows || ld < 1 || ld_values < 1) return RG_EINVAL;
  if (!column || !sequence_number || !episode_offsets || !values) return RG_EINVAL;
  RG_LAUNCH(cpe_episode_values_kernel, dim3(cpe_blocks(episodes)), dim3(CPE_THREADS), (hipStream_t)stream, column, (long)ld,
            sequence_number, episode_offsets, episodes, rows, gamma, values, (long)ld_values);
  return (int)hipGetLastError();
}

int rg_cpe_dr_partials(int rows) { return rows < 1 ? 0 : cpe_blocks(rows); }

int rg_cpe_dr_rows(const float* model_propensities, const float* action_mask, const float* model_rewards,
                   int64_t ld_model_rewards, const float* model_values, int64_t ld_model_values,
                   const float* logged_propensities, const float* logged_rewards, int64_t ld_logged_rewards,
                   const float* model_rewards_for_logged_action, int64_t ld_model_rewards_for_logged_action, int rows,
                   int num_actions, float* target_propensity, float* importance_weight, float* dm_ips_dr,
                   float* state_value, float* q_logged, double* partials, double* totals, rg_stream_t stream) {
  if (rows < 1 || num_actions < 1) return RG_EINVAL;
  if (ld_model_rewards < num_actions || ld_model_values < num_actions || ld_logged_rewards < 1 ||
      ld_model_rewards_for_logged_action < 1)
    return RG_EINVAL;
  if (!model_propensities || !action_mask || !model_rewards || !model_values || !logged_propensities || !logged_rewards ||
      !model_rewards_for_logged_action || !target_propensity || !importance_weight || !dm_ips_dr || !state_value ||
      !q_logged || !partials || !totals)
    return RG_EINVAL;
  CpeDrArgs a;
  a.prop = model_propensities, a.mask = action_mask, a.mr = model_rewards, a.mv = model_values;
  a.logged_p = logged_propensities, a.logged_r = logged_rewards, a.mr_logged = model_rewards_for_logged_action;
  a.ld_mr = (long)ld_model_rewards, a.ld_mv = (long)ld_model_values, a.ld_r = (long)ld_logged_rewards;
  a.ld_mrl = (long)ld_model_rewards_for_logged_action;
  a.N = rows, a.A = num_actions;
  a.tp = target_propensity, a.iw = importance_weight, a.est = dm_ips_dr, a.sv = state_value, a.ql = q_logged;
  a.partials = partials, a.P = rg_cpe_dr_partials(rows);
  RG_LAUNCH(cpe_dr_rows_kernel, dim3(a.P), dim3(CPE_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(cpe_dr_finish_kernel, dim3(1), dim3(CPE_THREADS), (hipStream_t)stream, (const double*)partials, a.P, totals);
  return (int)hipGetLastError();
}

int rg_cpe_sdr(const float* state_value, const float* importance_weight, const float* logged_rewards,
               int64_t ld_logged_rewards, const float* q_logged, const int32_t* episode_offsets, int episodes, int rows,
               double gamma, float* doubly_robust, float* episode_value, rg_stream_t stream) {
  if (episodes < 1 || rows < 1 || episodes > rows || ld_logged_rewards < 1) return RG_EINVAL;
  if (!state_value || !importance_weight || !logged_rewards || !q_logged || !episode_offsets || !doubly_robust ||
      !episode_value)
    return RG_EINVAL;
  RG_LAUNCH(cpe_sdr_kernel, dim3(cpe_blocks(episodes)), dim3(CPE_THREADS), (hipStream_t)stream, state_value,
            importance_weight, logged_rewards, (long)ld_logged_rewards, q_logged, episode_offsets, episodes, rows,
            (float)gamma, doubly_robust, episode_value);
  return (int)hipGetLastError();
}

int rg_cpe_bootstrap(const float* values, int64_t ld, int columns, int n, int sample_size, int num_samples, uint64_t seed,
                     double* means, double* std, rg_stream_t stream) {
  if (columns < 1 || columns > RG_CPE_BOOTSTRAP_MAX_COLUMNS || n < 1 || sample_size < 0 || num_samples < 1 || ld < n)
    return RG_EINVAL;
  if (!values || !means || !std) return RG_EINVAL;
  if (sample_size <= 4 * 64)
    RG_LAUNCH(cpe_bootstrap_kernel<64>, dim3(num_samples), dim3(64), (hipStream_t)stream, values, (long)ld, columns, n,
              sample_size, num_samples, seed, means);
  else
    RG_LAUNCH(cpe_bootstrap_kernel<CPE_THREADS>, dim3(num_samples), dim3(CPE_THREADS), (hipStream_t)stream, values, (long)ld,
              columns, n, sample_size, num_samples, seed, means);
  RG_LAUNCH(cpe_bootstrap_finish_kernel, dim3(columns), dim3(CPE_THREADS), (hipStream_t)stream, (const double*)means,
            num_samples, std);
  return (int)hipGetLastError();
}

}  // extern "C"
