// rg_mdn_row.h — a row of the mixture-density head, written once: gmm_loss's row (the sum over S of the normal log-densities,
// the log-sum-exp over G, the responsibilities) on one wave, in double.  mdn_head_kernel, mdn_nll_kernel (mdn.hip) and
// wm_mdn_losses_kernel (wm_eval.hip: the losses of every variant of an ablation sweep) call the same function, so a row has
// the same bits in each because it is the same code.  What stays in each kernel is its row addressing and its stores.
#pragma once
#include <rg_platform.h>
#include "rg_reduce.h"  // shfl_xor_f64, wave_sum_f64

namespace rg {

constexpr int MDN_THREADS = 256;
constexpr int MDN_WAVES = MDN_THREADS / 64;  // rows per workgroup
constexpr double MDN_HALF_LOG_2PI = 0.91893853320467274178;  // math.log(math.sqrt(2 * math.pi)) of Normal.log_prob

__device__ __forceinline__ double mdn_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, shfl_xor_f64(v, off));
  return v;
}

struct MdnRow {
  double logp;   // log sum_g pi_g N(x | mu_g, sigma_g): the same in every lane
  double resp;   // lane g < G: component g's responsibility (0 in the other lanes)
  double logpi;  // lane g < G: log pi_g
};

// gmm_loss's row (mdn_rnn.py:215-230).  FROM_Z: sg holds log sigma and pl the mixture logits (log_softmax here, :85-90);
// otherwise sg holds sigma and pl log pi as they are.  Lane g keeps component g's sum over S (G <= 32).
template <bool FROM_Z>
__device__ __forceinline__ MdnRow mdn_row(const float* __restrict__ x, const float* __restrict__ mu,
                                          const float* __restrict__ sg, const float* __restrict__ pl, int G, int S, int lane) {
  double lp = 0.0;
  for (int g = 0; g < G; ++g) {
    double s = 0.0;
    for (int j = lane; j < S; j += 64) {
      const double v = sg[g * S + j];
      const double sigma = FROM_Z ? exp(v) : v, ls = FROM_Z ? v : log(v);
      const double d = ((double)x[j] - (double)mu[g * S + j]) / sigma;
      s += -0.5 * d * d - ls - MDN_HALF_LOG_2PI;
    }
    s = wave_sum_f64(s);
    if (lane == g) lp = s;
  }
  const bool mine = lane < G;
  MdnRow r;
  r.logpi = mine ? (double)pl[lane] : -(double)INFINITY;
  if (FROM_Z) {
    const double m = mdn_wave_max(r.logpi);
    const double se = wave_sum_f64(mine ? exp(r.logpi - m) : 0.0);
    r.logpi = mine ? r.logpi - m - log(se) : r.logpi;
  }
  const double a = mine ? r.logpi + lp : -(double)INFINITY;
  const double m = mdn_wave_max(a);
  const double se = wave_sum_f64(mine ? exp(a - m) : 0.0);
  r.logp = m + log(se);
  r.resp = mine ? exp(a - r.logp) : 0.0;
  return r;
}

}  // namespace rg
