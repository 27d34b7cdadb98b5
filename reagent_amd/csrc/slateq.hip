// slateq.hip — the SlateQ step's own kernels: the gather of a slate's K documents out of a state's C candidates (with
// the documents' value * mask), the top-K slate choice of maxq learning, and the TD head over [B, K] slate items.
// Per-row VALU work on [B, C], [B, K] and [B * K, D] arrays: HBM- and latency-bound, small next to the critic's forwards.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"

namespace rg {

constexpr int SLATE_THREADS = 256;
constexpr int SLATE_WAVES = SLATE_THREADS / 64;
constexpr int SLATE_TOPK_PER_LANE = RG_SLATE_MAX_CANDIDATES / 64;

__device__ __forceinline__ float slate_block_sum(float v, float* scratch) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
  __syncthreads();
  return s;
}

// DocList.select_slate (core/types.py:277-284) and _get_docs_value's value * mask (slate_q_trainer.py:164).  One work item
// = one 16-byte piece or one scalar tail element of an output row's D features, or the row's weight: per row vD pieces +
// tD scalars + 1 (copy_dim = D, or 0 where only the weights are wanted).  Row r = b * K + k reads document clamp(index[r]) of state b, document 0 where not_terminal[b] == 0
// (_action_docs :112-117).  With count_mask, the block after the last copying block counts its true bytes into count_out[0]
// (one block, in index order: the count is the same in every run).
template <typename I>
__global__ void slate_gather_kernel(const float* __restrict__ features, const uint8_t* __restrict__ mask,
                                    const float* __restrict__ value, const int64_t* __restrict__ index,
                                    const float* __restrict__ not_terminal, int B, int C, int K, int D, int copy_dim, int vD,
                                    float* __restrict__ out, long ldo, float* __restrict__ out_weight,
                                    const uint8_t* __restrict__ count_mask, long count_n, int* __restrict__ count_out,
                                    int copy_blocks) {
  __shared__ int counts[SLATE_WAVES];
  if ((int)blockIdx.x >= copy_blocks) {
    int c = 0;
    for (long i = threadIdx.x; i < count_n; i += SLATE_THREADS) c += count_mask[i] != 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) counts[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) count_out[0] = (counts[0] + counts[1]) + (counts[2] + counts[3]);
    return;
  }
  const int tD = copy_dim - 4 * vD, W = vD + tD + 1;
  const I total = (I)B * K * W;
  for (I idx = (I)blockIdx.x * SLATE_THREADS + threadIdx.x; idx < total; idx += (I)copy_blocks * SLATE_THREADS) {
    const I r = idx / W;
    const int i = (int)(idx - r * W);
    const int b = (int)(r / K);
    long c = (not_terminal && not_terminal[b] == 0.f) ? 0 : (long)index[r];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    const long doc = (long)b * C + c;
    if (i == W - 1) {
      out_weight[r] = __fmul_rn(value[doc], mask[doc] ? 1.f : 0.f);
    } else {
      const float* s = features + doc * D;
      float* o = out + (long)r * ldo;
      if (i < vD) {
        *(f32x4*)(o + 4 * i) = *(const f32x4*)(s + 4 * i);
      } else {
        const int col = 4 * vD + (i - vD);
        o[col] = s[col];
      }
    }
  }
}

// _get_maxq_topk (slate_q_trainer.py:145-160).  One wave per state; lane l holds the scores of candidates l, l + 64, ...
// (PER of them, in registers).  K rounds of an arg-max over the wave: the larger score wins, of equal scores the lower
// index — torch.sort(descending=True, stable=True).  A chosen or absent slot holds -inf, below every score (finite by
// contract); K <= C leaves a live candidate in every round.
template <int PER>
__global__ void slate_topk_kernel(const float* __restrict__ q_all, const float* __restrict__ value,
                                  const uint8_t* __restrict__ mask, int B, int C, int K, int single,
                                  int64_t* __restrict__ next_index, float* __restrict__ q_sel) {
  const int lane = threadIdx.x & 63;
  const int wave_b = blockIdx.x * SLATE_WAVES + (threadIdx.x >> 6);
  const bool live = wave_b < B;  // a wave past the batch repeats the last state and writes nothing
  const int b = live ? wave_b : B - 1;
  const long o = (long)b * C;
  float s[PER], w[PER];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int c = j * 64 + lane;
    w[j] = c < C ? __fmul_rn(value[o + c], mask[o + c] ? 1.f : 0.f) : -INFINITY;
    m = fmaxf(m, w[j]);
  }
  if (single) {  // F.softmax(value * mask, dim=1) in its max-subtracted form, divided by the row sum
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, shfl_xor(m, off));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      w[j] = j * 64 + lane < C ? expf(__fsub_rn(w[j], m)) : 0.f;
      sum += w[j];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += shfl_xor(sum, off);
#pragma unroll
    for (int j = 0; j < PER; ++j) w[j] = __fdiv_rn(w[j], sum);
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int c = j * 64 + lane;
    s[j] = c < C ? __fmul_rn(q_all[o + c], w[j]) : -INFINITY;
  }
  for (int r = 0; r < K; ++r) {
    float best = s[0];
    int best_i = lane;
#pragma unroll
    for (int j = 1; j < PER; ++j)
      if (s[j] > best) {
        best = s[j];
        best_i = j * 64 + lane;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float other = shfl_xor(best, off);
      const int other_i = shfl_xor(best_i, off);
      if (other > best || (other == best && other_i < best_i)) {
        best = other;
        best_i = other_i;
      }
    }
    if (lane == 0 && live) {
      next_index[(long)b * K + r] = best_i;
      q_sel[(long)b * K + r] = q_all[o + best_i];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (best_i == j * 64 + lane) s[j] = -INFINITY;
  }
}

// train_step_gen (slate_q_trainer.py:204-259) after the forwards, one thread per state, in the reference's order with
// individually rounded operations: next_q = sum_k qn * (softmax_K(wn) | wn) (:228-237), / min(sum mask, slate_size)
// (:169-175, :240-241), * not_terminal (:243), y = reward + discount * next_q (:244), F.mse_loss over the n selected
// elements (single selection, :246-259) or over all B * K.  The block's partial is already divided by the element count.
__global__ void slateq_head_kernel(const float* __restrict__ q, const float* __restrict__ qn, const float* __restrict__ wn,
                                   const float* __restrict__ reward, const uint8_t* __restrict__ reward_mask,
                                   const float* __restrict__ not_terminal, float gamma, const float* __restrict__ time_diff,
                                   float time_scale, int single, const uint8_t* __restrict__ norm_mask, int C,
                                   int slate_size, const int* __restrict__ n_selected, int B, int K,
                                   float* __restrict__ target, float* __restrict__ dq, float* __restrict__ loss_part,
                                   float* __restrict__ next_q_out) {
  __shared__ float scratch[SLATE_WAVES];
  const int b = blockIdx.x * SLATE_THREADS + threadIdx.x;
  const double count = single ? (double)n_selected[0] : (double)B * (double)K;
  float row_loss = 0.f;
  if (b < B) {
    const long o = (long)b * K;
    float nq = 0.f;
    if (single) {
      float m = wn[o];
      for (int k = 1; k < K; ++k) m = fmaxf(m, wn[o + k]);
      float sum = 0.f;
      for (int k = 0; k < K; ++k) sum = __fadd_rn(sum, expf(__fsub_rn(wn[o + k], m)));
      for (int k = 0; k < K; ++k)
        nq = __fadd_rn(nq, __fmul_rn(qn[o + k], __fdiv_rn(expf(__fsub_rn(wn[o + k], m)), sum)));
    } else {
      for (int k = 0; k < K; ++k) nq = __fadd_rn(nq, __fmul_rn(qn[o + k], wn[o + k]));
      int present = 0;
      for (int c = 0; c < C; ++c) present += norm_mask[(long)b * C + c] != 0;
      nq = __fdiv_rn(nq, (float)(present < slate_size ? present : slate_size));
    }
    nq = __fmul_rn(nq, not_terminal[b]);
    // gamma ** (time_diff / scale) on fp32 operands (:211-214), evaluated in double and rounded once: the correctly
    // rounded fp32 power, whatever the device's powf does in its last bit
    const float disc = time_diff ? (float)pow((double)gamma, (double)__fdiv_rn(time_diff[b], time_scale)) : gamma;
    const float boot = __fmul_rn(disc, nq);
    const float norm = (float)(2.0 / count);  // mse_loss_backward: 2 / numel, rounded to fp32, times (q - y)
    for (int k = 0; k < K; ++k) {
      const float y = __fadd_rn(reward[o + k], boot);
      const bool on = !single || reward_mask[o + k];
      const float d = on ? __fsub_rn(q[o + k], y) : 0.f;
      row_loss = __fadd_rn(row_loss, __fmul_rn(d, d));
      target[o + k] = y;
      dq[o + k] = on ? __fmul_rn(norm, d) : 0.f;
    }
    next_q_out[b] = nq;
  }
  const float s = slate_block_sum(row_loss, scratch);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = (float)((double)s / count);
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_slate_gather(const float* features, const uint8_t* mask, const float* value, const int64_t* index,
                    const float* not_terminal, int batch, int num_candidates, int slate_size, int feature_dim,
                    float* out_features, int64_t ldo, float* out_weight, const uint8_t* count_mask, int64_t count_n,
                    int32_t* count_out, rg_stream_t stream) {
  if (!features || !mask || !value || !index || !out_weight) return RG_EINVAL;
  if (batch <= 0 || num_candidates < 1 || slate_size < 1 || feature_dim < 1) return RG_EINVAL;
  if (out_features && ldo < feature_dim) return RG_EINVAL;
  if ((count_mask != nullptr) != (count_out != nullptr) || (count_mask && count_n <= 0)) return RG_EINVAL;
  const int copy_dim = out_features ? feature_dim : 0;  // no output panel: the weights alone
  const bool vec = (feature_dim & 3) == 0 && (((uintptr_t)features) & 15) == 0 && (((uintptr_t)out_features) & 15) == 0 &&
                   (ldo & 3) == 0;
  const int vD = vec ? copy_dim / 4 : 0;
  const long W = (long)vD + (copy_dim - 4 * vD) + 1;
  const long total = (long)batch * slate_size * W;
  long blocks = (total + SLATE_THREADS - 1) / SLATE_THREADS;
  if (blocks > 16384) blocks = 16384;
  const unsigned grid = (unsigned)blocks + (count_mask ? 1u : 0u);
  if (total + (blocks + 1) * SLATE_THREADS < 0x7fffffffL)
    RG_LAUNCH(slate_gather_kernel<int>, dim3(grid), dim3(SLATE_THREADS), (hipStream_t)stream, features, mask, value, index,
              not_terminal, batch, num_candidates, slate_size, feature_dim, copy_dim, vD, out_features, (long)ldo, out_weight,
              count_mask, (long)count_n, count_out, (int)blocks);
  else
    RG_LAUNCH(slate_gather_kernel<long>, dim3(grid), dim3(SLATE_THREADS), (hipStream_t)stream, features, mask, value, index,
              not_terminal, batch, num_candidates, slate_size, feature_dim, copy_dim, vD, out_features, (long)ldo, out_weight,
              count_mask, (long)count_n, count_out, (int)blocks);
  return (int)hipGetLastError();
}

int rg_slate_topk(const float* q_all, const float* value, const uint8_t* mask, int batch, int num_candidates, int slate_size,
                  int single_selection, int64_t* next_index, float* q_sel, rg_stream_t stream) {
  if (!q_all || !value || !mask || !next_index || !q_sel || batch <= 0) return RG_EINVAL;
  if (slate_size < 1 || slate_size > num_candidates || num_candidates > RG_SLATE_MAX_CANDIDATES) return RG_EINVAL;
  const dim3 grid((batch + SLATE_WAVES - 1) / SLATE_WAVES), block(SLATE_THREADS);
  const int per = (num_candidates + 63) / 64;
#define RG_TOPK(P)                                                                                                      \
  RG_LAUNCH(slate_topk_kernel<P>, grid, block, (hipStream_t)stream, q_all, value, mask, batch, num_candidates, slate_size, \
            single_selection, next_index, q_sel)
  if (per <= 1) RG_TOPK(1);
  else if (per <= 2) RG_TOPK(2);
  else if (per <= 4) RG_TOPK(4);
  else if (per <= 8) RG_TOPK(8);
  else RG_TOPK(SLATE_TOPK_PER_LANE);
#undef RG_TOPK
  return (int)hipGetLastError();
}

int rg_slateq_head_partials(int batch) { return (batch + SLATE_THREADS - 1) / SLATE_THREADS; }

int rg_slateq_head(const float* q, const float* qn, const float* wn, const float* reward, const uint8_t* reward_mask,
                   const float* not_terminal, double gamma, const float* time_diff, double discount_time_scale,
                   int single_selection, const uint8_t* norm_mask, int num_candidates, int slate_size,
                   const int32_t* n_selected, int batch, int num_items, float* target, float* dq, float* loss_partials,
                   float* next_q, rg_stream_t stream) {
  if (!q || !qn || !wn || !reward || !not_terminal || !target || !dq || !loss_partials || !next_q) return RG_EINVAL;
  if (batch <= 0 || num_items < 1 || (time_diff && !(discount_time_scale != 0.0))) return RG_EINVAL;
  if (single_selection ? (!reward_mask || !n_selected) : (!norm_mask || num_candidates < 1 || slate_size < 1))
    return RG_EINVAL;
  RG_LAUNCH(slateq_head_kernel, dim3(rg_slateq_head_partials(batch)), dim3(SLATE_THREADS), (hipStream_t)stream, q, qn, wn,
            reward, reward_mask, not_terminal, (float)gamma, time_diff, (float)discount_time_scale, single_selection,
            norm_mask, num_candidates, slate_size, n_selected, batch, num_items, target, dq, loss_partials, next_q);
  return (int)hipGetLastError();
}

}  // extern "C"
