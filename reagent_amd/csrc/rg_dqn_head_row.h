// rg_dqn_head_row.h — the row arithmetic of the DQN TD head with G = A / 4 lanes per transition, shared by
// dqn_head_lanes_kernel (heads.hip) and the paired online forward (mlp_fused.hip: the head runs in the row-store pass
// of the second output layer).  One definition, so that both launches give the same bits.
#pragma once
#include <rg_platform.h>
#include "../../include/reagent_hip.h"

namespace rg {

// Lane `sub` of row b holds float4 number `sub` of each [B, 4G] operand (qo4 = the values the arg-max keys on: the online
// network's with double-Q, else qt4 itself); reward_b / not_terminal_b / gamma_exp_b are the row's scalars.  The row
// reductions run over the G lanes of a row with xor shuffles, so every lane of the wave must call this (rows past the
// batch: live = false, operands of any valid row, nothing stored).  Stores dq (and next_q / next_idx / q_sel from lane
// sub == 0) and returns the row's loss term in lane sub == 0 of a live row, 0 elsewhere.
template <int G>
__device__ __forceinline__ float dqn_head_lanes_row(const f32x4 m4, const f32x4 qt4, const f32x4 qo4, const f32x4 ac4,
                                                    const f32x4 q4, int sub, int b, bool live, float reward_b,
                                                    const float* __restrict__ reward_boosts, float not_terminal_b,
                                                    float gamma, bool has_gamma_exp, float gamma_exp_b, int batch,
                                                    int double_q, int loss_type, float* __restrict__ dq,
                                                    float* __restrict__ next_q_out, int64_t* __restrict__ next_idx_out,
                                                    float* __restrict__ q_sel_out) {
  constexpr int A = 4 * G;
  const long o = (long)b * A + sub * 4;
  float best = 0.f, best_t = 0.f, rb = 0.f, qs = 0.f;
  int best_i = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float pen = -1e9f * (1.f - m4[e]);  // ACTION_NOT_POSSIBLE_VAL * (1 - mask)
    const float qo = qo4[e] + pen, qt = qt4[e] + pen;
    const float key = double_q ? qo : qt;
    if (e == 0 || key > best) {
      best = key;
      best_t = qt;
      best_i = sub * 4 + e;
    }
    if (reward_boosts) rb += ac4[e] * reward_boosts[sub * 4 + e];
    qs += q4[e] * ac4[e];
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const float ok = shfl_xor(best, off), ot = shfl_xor(best_t, off);
    const int oi = shfl_xor(best_i, off);
    if (ok > best || (ok == best && oi < best_i)) {
      best = ok;
      best_t = ot;
      best_i = oi;
    }
    rb += shfl_xor(rb, off);
    qs += shfl_xor(qs, off);
  }
  const float rew = reward_b + rb;
  const float disc = has_gamma_exp ? powf(gamma, gamma_exp_b) : gamma;
  const float target = rew + disc * (best_t * not_terminal_b);
  const float d = qs - target;
  float g, row_loss;
  if (loss_type == RG_LOSS_HUBER) {
    const float ad = fabsf(d);
    row_loss = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
    g = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
  } else {
    row_loss = d * d;
    g = 2.f * d;
  }
  g /= (float)batch;
  if (live) *(f32x4*)(dq + o) = f32x4{g * ac4[0], g * ac4[1], g * ac4[2], g * ac4[3]};
  float loss = 0.f;
  if (live && sub == 0) {
    loss = row_loss;
    if (next_q_out) next_q_out[b] = best_t;
    if (next_idx_out) next_idx_out[b] = best_i;
    if (q_sel_out) q_sel_out[b] = qs;
  }
  return loss;
}

// a wave's loss terms (64 / G rows) summed in a fixed order
__device__ __forceinline__ float dqn_head_wave_sum(float loss) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) loss += shfl_xor(loss, off);
  return loss;
}

// ---- row rules shared with the evaluation page (cpe_eval.hip: rg_cpe_page_rows) ----------------------------------------------
// get_max_q_values_with_target (dqn_trainer_base.py:33-77) over one row of A entries: the first maximal key[a] +
// ACTION_NOT_POSSIBLE_VAL * (1 - mask[a]) (torch.max's first-index rule), its index and the target value at it (penalty
// included).  mask == nullptr: every action possible (the penalty is then -1e9f * 0).
__device__ __forceinline__ void masked_max_row(const float* __restrict__ key, const float* __restrict__ target,
                                               const float* __restrict__ mask, int A, float& best_t, int& best_i) {
  float best = 0.f;
  best_t = 0.f;
  best_i = 0;
  for (int a = 0; a < A; ++a) {
    const float pen = -1e9f * (1.f - (mask ? mask[a] : 1.f));  // ACTION_NOT_POSSIBLE_VAL * (1 - mask)
    const float k = key[a] + pen, t = target[a] + pen;
    if (a == 0 || k > best) {
      best = k;
      best_t = t;
      best_i = a;
    }
  }
}

// masked_softmax (core/torch_utils.py:62-73) over one row: v = x / T - (1 - mask) * 1e20; p = exp(v - max v) * mask / sum,
// a NaN (a fully masked row: 0 / 0) replaced by 0.  masked_softmax_stats is passes 1 and 2 (row max, denominator),
// masked_softmax_p one entry from them.  mask == nullptr: every action possible.
__device__ __forceinline__ float masked_softmax_logit(float x, float m, float temperature) {
  return x / temperature - ((1.0f - m) * 1e20f);
}
__device__ __forceinline__ void masked_softmax_stats(const float* __restrict__ x, const float* __restrict__ mask, int A,
                                                     float temperature, float& mx, float& den) {
  mx = 0.f;
  for (int a = 0; a < A; ++a) {
    const float v = masked_softmax_logit(x[a], mask ? mask[a] : 1.f, temperature);
    if (a == 0 || v > mx) mx = v;
  }
  den = 0.f;
  for (int a = 0; a < A; ++a) {
    const float m = mask ? mask[a] : 1.f;
    den += expf(masked_softmax_logit(x[a], m, temperature) - mx) * m;
  }
}
__device__ __forceinline__ float masked_softmax_p(float x, float m, float temperature, float mx, float den) {
  const float p = expf(masked_softmax_logit(x, m, temperature) - mx) * m / den;
  return p != p ? 0.f : p;
}

}  // namespace rg
