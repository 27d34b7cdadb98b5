// cb_eval.hip — offline policy evaluation inside the contextual-bandit training loop: the replay estimator of Li et al.
// (arXiv 1003.0146, Algorithm 3) as the reference's PolicyEvaluator runs it.  rg_cb_eval_ingest is BaseOfflineEval.
// ingest_batch (reagent/evaluation/cb/base_evaluator.py:147-169) — _process_all_data (policy_evaluator.py:22-35),
// add_importance_weights (evaluation/cb/utils.py:9-47), _process_used_data (policy_evaluator.py:38-68) — and the
// trainer's sum_weight_since_update_local += ... (reagent/training/cb/base_trainer.py:127-129) in one main and one
// finishing launch on device-resident state.  No atomics, no host synchronisation: per-workgroup partials (double) leave
// the main launch and the finishing launch adds them in a fixed order, so two runs give the same bits.  The fp64 wave sum
// and the LDS tree of the finishing launch are rg_reduce.h's, shared with the other bandit files (see rg_cb.h).
//
// A QUIRK OF THE REFERENCE THAT IS KEPT.  Without arm_presence the reference's `sizes` is [B, 1] while `weights.squeeze()`
// is [B]: their product broadcasts to [B, B], and the two size sums come out `batch` times too large (B * A * sum w;
// avg_size_accepted is B * A, not A).  Users compare these logged metrics between the two implementations, so the
// finishing launch multiplies the two size sums by `batch` where arm_presence is NULL.  With arm_presence they are plain.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"  // wave_sum_f64, lds_tree_sum

// every row value is held to the reference's fp32 operation order: each multiply and divide is rounded on its own
#pragma clang fp contract(off)

namespace rg {

constexpr int CBE_THREADS = 256;  // one row a thread: a workgroup is a slice of 256 rows
constexpr int CBE_WAVES = CBE_THREADS / 64;
constexpr int CBE_SUMS = 8;       // the ninth running sum is the first one again
constexpr int CBE_FINISH_LANES = CBE_THREADS / CBE_SUMS;  // slices one finishing pass reads at once, per sum

struct CbEvalArgs {
  const int64_t *action, *model_action;
  const float *reward, *weight, *logp;
  const uint8_t* presence;
  int B, arms, clip;
  float max_iw;
  float *iw, *eff;
  double* partials;  // [CBE_SUMS][P]
  int P;
};

// Thread t of workgroup g has row r = 256 g + t.  Adjacent lanes read adjacent rows, so every load of a wave covers one
// contiguous span (512 bytes of action, 256 of reward, 64 * arms of arm_presence) and every fetched line is used whole.
// The row's eight terms are fp32 products as the reference forms them; they are added in double: across the wave by
// butterflies, across the four waves through LDS in wave order.
__global__ void RG_LAUNCH_BOUNDS(CBE_THREADS, 1) cb_eval_ingest_kernel(const CbEvalArgs a) {
  __shared__ double wave_sums[CBE_WAVES][CBE_SUMS];
  const long r = (long)blockIdx.x * CBE_THREADS + threadIdx.x;
  double t[CBE_SUMS];
#pragma unroll
  for (int k = 0; k < CBE_SUMS; ++k) t[k] = 0.0;
  if (r < a.B) {
    const float w = a.weight ? a.weight[r] : 1.f, rew = a.reward[r];
    int size = a.arms;
    if (a.presence) {
      const uint8_t* p = a.presence + r * a.arms;
      size = 0;
      for (int j = 0; j < a.arms; ++j) size += p[j] != 0;
    }
    const float fsize = (float)size;
    const float prob = a.logp ? expf(a.logp[r]) : 1.0f / fsize;
    float iw = 1.0f / prob;
    if (a.clip && iw > a.max_iw) iw = a.max_iw;  // (torch.clamp(max=): a NaN is not above the clip and passes)
    const float match = a.action[r] == a.model_action[r] ? 1.f : 0.f;
    iw = match * iw;  // a multiplication: 0 * inf = NaN, as in the reference
    const float eff = w * iw;
    const float acc = iw > 0.f ? 1.f : 0.f;
    const float wacc = w * acc;
    a.iw[r] = iw;
    a.eff[r] = eff;
    t[0] = (double)w;
    t[1] = (double)(w * rew);
    t[2] = (double)(w * fsize);
    t[3] = (double)(eff * rew);
    t[4] = (double)(wacc * rew);
    t[5] = (double)wacc;
    t[6] = (double)eff;
    t[7] = (double)(wacc * fsize);
  }
#pragma unroll
  for (int k = 0; k < CBE_SUMS; ++k) t[k] = wave_sum_f64(t[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < CBE_SUMS; ++k) wave_sums[threadIdx.x >> 6][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < CBE_SUMS) {
    const int k = threadIdx.x;
    a.partials[(long)k * a.P + blockIdx.x] = ((wave_sums[0][k] + wave_sums[1][k]) + wave_sums[2][k]) + wave_sums[3][k];
  }
}

struct CbEvalState {
  float* sum[CBE_SUMS];
  float* since_update;
};

// The finishing launch, one workgroup: thread 32 k + j adds the slices j, j + 32, ... of sum k in slice order (32 slices a
// pass), the 32 lane sums meet in LDS by a fixed tree, and lane 0 adds the total to the sum's one-element buffer: one
// rounding to fp32.  size_scale is `batch` for the two size sums where arm_presence is NULL (the quirk above), else 1.
__global__ void RG_LAUNCH_BOUNDS(CBE_THREADS, 1) cb_eval_finish_kernel(const double* __restrict__ partials, int P,
                                                                        double size_scale, const CbEvalState s) {
  __shared__ double sums[CBE_THREADS];
  const int k = threadIdx.x / CBE_FINISH_LANES, j = threadIdx.x % CBE_FINISH_LANES;
  double v = 0.0;
  for (int p = j; p < P; p += CBE_FINISH_LANES) v += partials[(long)k * P + p];
  sums[threadIdx.x] = v;
  lds_tree_sum<CBE_FINISH_LANES>(sums);
  if (j == 0) {
    double total = sums[threadIdx.x];
    if (k == 2 || k == 7) total *= size_scale;
    *s.sum[k] = (float)((double)*s.sum[k] + total);
    if (k == 0) *s.since_update = (float)((double)*s.since_update + total);
  }
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_cb_eval_ingest_partials(int batch) { return batch < 1 ? 0 : (batch + CBE_THREADS - 1) / CBE_THREADS; }

int rg_cb_eval_ingest(const int64_t* action, const int64_t* model_action, const float* reward, const float* weight,
                      const float* action_log_probability, const uint8_t* arm_presence, int batch, int arms,
                      int clip, double max_importance_weight, float* importance_weight, float* effective_weight,
                      double* partials, float* sum_weight_all_data, float* sum_reward_weighted_all_data,
                      float* sum_size_weighted_all_data, float* sum_reward_importance_weighted_accepted,
                      float* sum_reward_weighted_accepted, float* sum_weight_accepted,
                      float* sum_importance_weight_accepted, float* sum_size_weighted_accepted,
                      float* sum_weight_since_update, rg_stream_t stream) {
  if (batch < 1 || arms < 1) return RG_EINVAL;
  if (!action || !model_action || !reward || !importance_weight || !effective_weight || !partials) return RG_EINVAL;
  CbEvalState s;
  s.sum[0] = sum_weight_all_data, s.sum[1] = sum_reward_weighted_all_data, s.sum[2] = sum_size_weighted_all_data;
  s.sum[3] = sum_reward_importance_weighted_accepted, s.sum[4] = sum_reward_weighted_accepted;
  s.sum[5] = sum_weight_accepted, s.sum[6] = sum_importance_weight_accepted, s.sum[7] = sum_size_weighted_accepted;
  s.since_update = sum_weight_since_update;
  for (int k = 0; k < CBE_SUMS; ++k)
    if (!s.sum[k]) return RG_EINVAL;
  if (!s.since_update) return RG_EINVAL;
  CbEvalArgs a;
  a.action = action, a.model_action = model_action, a.reward = reward, a.weight = weight;
  a.logp = action_log_probability, a.presence = arm_presence;
  a.B = batch, a.arms = arms, a.clip = clip != 0, a.max_iw = (float)max_importance_weight;
  a.iw = importance_weight, a.eff = effective_weight, a.partials = partials;
  a.P = rg_cb_eval_ingest_partials(batch);
  RG_LAUNCH(cb_eval_ingest_kernel, dim3(a.P), dim3(CBE_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(cb_eval_finish_kernel, dim3(1), dim3(CBE_THREADS), (hipStream_t)stream, (const double*)partials, a.P,
            arm_presence ? 1.0 : (double)batch, s);
  return (int)hipGetLastError();
}

}  // extern "C"
