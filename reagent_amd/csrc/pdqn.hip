// pdqn.hip — the parametric DQN step's own kernels: the tiled concatenation cat(state[r / M], candidate[r]) for the
// engines that do not read two panels in place, and the TD head over a per-state list of M candidate actions (masked
// arg-max of a scalar-output critic, TD target, loss and d(mean loss)/dq).  Per-row VALU work on [B], [B, M] and
// [B * M, S + A] arrays: HBM-bound, small next to the critic's forwards.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"

namespace rg {

constexpr int PDQN_THREADS = 256;

// One work item = one 16-byte piece or one scalar tail element of an output row: per row vS pieces + tS scalars of the
// state panel, then vA pieces + tA scalars of the candidate panel (a panel whose pitch or base is not 16-byte aligned
// has no pieces: all of it is tail).
template <typename I>
__global__ void tile_concat_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ x2, long ldx2, int rows,
                                   int M, int S, int vS, int vA, int A, float* __restrict__ out, long ldo) {
  const int tS = S - 4 * vS, tA = A - 4 * vA, W = vS + tS + vA + tA;
  const I total = (I)rows * W;
  for (I idx = (I)blockIdx.x * PDQN_THREADS + threadIdx.x; idx < total; idx += (I)gridDim.x * PDQN_THREADS) {
    const int r = (int)(idx / W);
    int i = (int)(idx - (I)r * W);
    float* o = out + (long)r * ldo;
    if (i < vS + tS) {
      const float* s = x + (long)(r / M) * ldx;
      if (i < vS) {
        *(f32x4*)(o + 4 * i) = *(const f32x4*)(s + 4 * i);
      } else {
        const int c = 4 * vS + (i - vS);
        o[c] = s[c];
      }
    } else {
      i -= vS + tS;
      const float* s = x2 + (long)r * ldx2;
      if (i < vA) {
        *(f32x4*)(o + S + 4 * i) = *(const f32x4*)(s + 4 * i);
      } else {
        const int c = 4 * vA + (i - vA);
        o[S + c] = s[c];
      }
    }
  }
}

__device__ __forceinline__ float pdqn_block_sum(float v, float* scratch) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
  __syncthreads();
  return s;
}

// One thread per state.  get_max_q_values_with_target (dqn_trainer_base.py:33-77) in its own fp32 arithmetic: the penalty
// -1e9 * (1 - mask) is ADDED to both value rows (individually rounded operations: a fused multiply-add would round once
// where torch rounds twice), the first maximal index wins, and a fully masked row selects index 0 and yields the
// penalised value.  Then target = reward + (not_terminal * discount) * next_q in the reference's order
// (parametric_dqn_trainer.py:160), the loss term and d(mean loss)/dq (:170).
__global__ void pdqn_head_kernel(const float* __restrict__ q, const float* __restrict__ qn_online_all,
                                 const float* __restrict__ qn_target_all, const float* __restrict__ next_mask,
                                 const float* __restrict__ reward, const float* __restrict__ not_terminal, float gamma,
                                 const float* __restrict__ gamma_exponent, int batch, int M, int maxq, int double_q,
                                 int loss_type, float* __restrict__ target, float* __restrict__ dq,
                                 float* __restrict__ loss_part, float* __restrict__ next_q_out,
                                 int64_t* __restrict__ next_idx_out) {
  __shared__ float scratch[4];
  const int b = blockIdx.x * PDQN_THREADS + threadIdx.x;
  float row_loss = 0.f;
  if (b < batch) {
    float nq;
    int best_i = 0;
    if (maxq) {
      const long o = (long)b * M;
      float best = 0.f, best_t = 0.f;
      for (int j = 0; j < M; ++j) {
        const float pen = __fmul_rn(-1e9f, __fsub_rn(1.f, next_mask[o + j]));  // ACTION_NOT_POSSIBLE_VAL * (1 - mask)
        const float qt = __fadd_rn(qn_target_all[o + j], pen);
        const float key = double_q ? __fadd_rn(qn_online_all[o + j], pen) : qt;
        if (j == 0 || key > best) {
          best = key;
          best_t = qt;
          best_i = j;
        }
      }
      nq = best_t;
    } else {
      nq = qn_target_all[b];  // SARSA: the target network's value of (next_state, next_action)
    }
    const float disc = gamma_exponent ? powf(gamma, gamma_exponent[b]) : gamma;
    const float y = __fadd_rn(reward[b], __fmul_rn(__fmul_rn(not_terminal[b], disc), nq));
    const float x = q[b];
    // d(mean loss)/dq as autograd evaluates it: mse 2/B (rounded to fp32) times d, smooth-l1 1/B times d or +-1/B, bce
    // (sigmoid(x) - y) divided by B
    float g;
    if (loss_type == RG_LOSS_BCE_LOGITS) {
      // F.binary_cross_entropy_with_logits in the stable form: max(x, 0) - x y + log(1 + exp(-|x|))
      const float e = expf(-fabsf(x));
      row_loss = fmaxf(x, 0.f) - x * y + log1pf(e);
      const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      g = (sig - y) / (float)batch;
    } else {
      const float d = __fsub_rn(x, y);
      if (loss_type == RG_LOSS_HUBER) {
        const float ad = fabsf(d), norm = (float)(1.0 / (double)batch);
        row_loss = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
        g = ad < 1.f ? __fmul_rn(norm, d) : (d > 0.f ? norm : -norm);
      } else {
        row_loss = __fmul_rn(d, d);
        g = __fmul_rn((float)(2.0 / (double)batch), d);
      }
    }
    target[b] = y;
    dq[b] = g;
    next_q_out[b] = nq;
    if (next_idx_out) next_idx_out[b] = best_i;
  }
  const float s = pdqn_block_sum(row_loss, scratch);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_tile_concat(const float* x, int64_t ldx, const float* x2, int64_t ldx2, int rows, int x_tile, int x_cols, int x2_cols,
                   float* out, int64_t ldo, rg_stream_t stream) {
  if (!x || !x2 || !out || rows <= 0 || x_tile < 1 || x_cols <= 0 || x2_cols <= 0) return RG_EINVAL;
  if (ldx < x_cols || ldx2 < x2_cols || ldo < (int64_t)x_cols + x2_cols) return RG_EINVAL;
  const bool out16 = (((uintptr_t)out) & 15) == 0 && (ldo & 3) == 0;
  const bool vec_s = out16 && (((uintptr_t)x) & 15) == 0 && (ldx & 3) == 0;
  const bool vec_a = out16 && (x_cols & 3) == 0 && (((uintptr_t)x2) & 15) == 0 && (ldx2 & 3) == 0;
  const int vS = vec_s ? x_cols / 4 : 0, vA = vec_a ? x2_cols / 4 : 0;
  const long W = (long)vS + (x_cols - 4 * vS) + vA + (x2_cols - 4 * vA);
  const long total = (long)rows * W;
  long blocks = (total + PDQN_THREADS - 1) / PDQN_THREADS;
  if (blocks > 16384) blocks = 16384;
  if (total + (long)blocks * PDQN_THREADS < 0x7fffffffL)
    RG_LAUNCH(tile_concat_kernel<int>, dim3((unsigned)blocks), dim3(PDQN_THREADS), (hipStream_t)stream, x, (long)ldx, x2,
              (long)ldx2, rows, x_tile, x_cols, vS, vA, x2_cols, out, (long)ldo);
  else
    RG_LAUNCH(tile_concat_kernel<long>, dim3((unsigned)blocks), dim3(PDQN_THREADS), (hipStream_t)stream, x, (long)ldx, x2,
              (long)ldx2, rows, x_tile, x_cols, vS, vA, x2_cols, out, (long)ldo);
  return (int)hipGetLastError();
}

int rg_pdqn_head_partials(int batch) { return (batch + PDQN_THREADS - 1) / PDQN_THREADS; }

int rg_pdqn_head(const float* q, const float* qn_online_all, const float* qn_target_all, const float* next_mask,
                 const float* reward, const float* not_terminal, double gamma, const float* gamma_exponent, int batch,
                 int max_num_actions, int maxq, int double_q, int loss_type, float* target, float* dq,
                 float* loss_partials, float* next_q, int64_t* next_idx, rg_stream_t stream) {
  if (!q || !qn_target_all || !reward || !not_terminal || !target || !dq || !loss_partials || !next_q || batch <= 0)
    return RG_EINVAL;
  if (maxq && (!next_mask || max_num_actions < 1 || (double_q && !qn_online_all))) return RG_EINVAL;
  if (loss_type != RG_LOSS_MSE && loss_type != RG_LOSS_HUBER && loss_type != RG_LOSS_BCE_LOGITS) return RG_EINVAL;
  RG_LAUNCH(pdqn_head_kernel, dim3(rg_pdqn_head_partials(batch)), dim3(PDQN_THREADS), (hipStream_t)stream, q, qn_online_all,
            qn_target_all, next_mask, reward, not_terminal, (float)gamma, gamma_exponent, batch, max_num_actions, maxq,
            double_q, loss_type, target, dq, loss_partials, next_q, next_idx);
  return (int)hipGetLastError();
}

}  // extern "C"
