// mdn.hip — the mixture-density head of the world model: the split of gmm_linear's output into mus / sigmas / logpi / reward /
// not_terminal (reagent/models/mdn_rnn.py:75-92), gmm_loss (:188-233) and the three weighted losses of MDNRNNTrainer.get_loss
// (reagent/training/world_model/mdnrnn_trainer.py:164-177) with d loss / d gmm_outs.  One wave per row; a row's arithmetic (the
// sum over S of the normal log-densities, the log-sum-exp over G, the responsibilities) runs in double on the fp32 inputs and
// is rounded once where it is stored.  No atomics: the losses leave as per-workgroup partials in double, a finishing launch
// adds them in a fixed order and rounds once.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"  // shfl_xor_f64, wave_sum_f64, lds_tree_sum

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

struct MdnHeadArgs {
  const float* z;
  long ldz;
  const float *next_state, *reward, *not_terminal;
  double scale_gmm, scale_bce, scale_mse;  // weight / rows that count (the gmm term's also / (S + 2) where the loss divides)
  int N, G, S, first_row;
  float* dz;
  long lddz;
  float *sigmas, *logpi;
  double* partials;  // [workgroups][3]: the sums of the rows' -log p, BCE and squared error
};

__global__ void mdn_head_kernel(const MdnHeadArgs a) {
  __shared__ double resp_s[MDN_WAVES][32];
  __shared__ double part[MDN_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long wave_row = (long)blockIdx.x * MDN_WAVES + wave;
  const bool live = wave_row < a.N;  // a wave past the last row repeats it and writes nothing
  const long row = live ? wave_row : a.N - 1;
  const bool counts = live && row >= a.first_row;
  const int G = a.G, S = a.S, stride = G * S;
  const float* zp = a.z + row * a.ldz;
  const float* x = a.next_state + row * S;
  const MdnRow r = mdn_row<true>(x, zp, zp + stride, zp + 2 * stride, G, S, lane);
  if (lane < 32) resp_s[wave][lane] = r.resp;
  wave_lds_sync();
  float* dp = a.dz + row * a.lddz;
  for (int g = 0; g < G; ++g) {
    const double rg = counts ? resp_s[wave][g] * a.scale_gmm : 0.0;
    for (int j = lane; j < S; j += 64) {
      const double v = zp[stride + g * S + j];
      const double sigma = exp(v);
      const double d = ((double)x[j] - (double)zp[g * S + j]) / sigma;
      if (live) {
        dp[g * S + j] = (float)(-rg * d / sigma);
        dp[stride + g * S + j] = (float)(-rg * (d * d - 1.0));
        if (a.sigmas) a.sigmas[row * stride + g * S + j] = (float)sigma;
      }
    }
  }
  if (live && lane < G) {
    dp[2 * stride + lane] = counts ? (float)(-(r.resp - exp(r.logpi)) * a.scale_gmm) : 0.f;
    if (a.logpi) a.logpi[row * G + lane] = (float)r.logpi;
  }
  // F.mse_loss on column -2, F.binary_cross_entropy_with_logits on column -1
  const double rz = zp[2 * stride + G], nz = zp[2 * stride + G + 1];
  const double dr = rz - (double)a.reward[row], y = a.not_terminal[row];
  const double bce = fmax(nz, 0.0) - nz * y + log1p(exp(-fabs(nz)));
  if (live && lane == 0) {
    dp[2 * stride + G] = counts ? (float)(2.0 * dr * a.scale_mse) : 0.f;
    dp[2 * stride + G + 1] = counts ? (float)((1.0 / (1.0 + exp(-nz)) - y) * a.scale_bce) : 0.f;
  }
  if (lane == 0) {
    part[wave][0] = counts ? -r.logp : 0.0;
    part[wave][1] = counts ? bce : 0.0;
    part[wave][2] = counts ? dr * dr : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    a.partials[(long)blockIdx.x * 3 + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
  }
}

// One workgroup: the ordered sum of each of the three partials over the head's workgroups (thread i adds i, i + 256, ...,
// then a fixed LDS tree), times its weight / rows, rounded once; the loss (mdnrnn_trainer.py:173-176) from the three doubles
__global__ void mdn_finish_kernel(const double* __restrict__ partials, int blocks, double scale_gmm, double scale_bce,
                                  double scale_mse, double gmm_in_loss, float* __restrict__ losses) {
  __shared__ double vals[MDN_THREADS];
  double total[3];
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int p = threadIdx.x; p < blocks; p += MDN_THREADS) s += partials[(long)p * 3 + k];
    vals[threadIdx.x] = s;
    lds_tree_sum<MDN_THREADS>(vals);
    total[k] = vals[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double gmm = total[0] * scale_gmm, bce = total[1] * scale_bce, mse = total[2] * scale_mse;
    losses[0] = (float)gmm, losses[1] = (float)bce, losses[2] = (float)mse;
    losses[3] = (float)(gmm * gmm_in_loss + bce + mse);
  }
}

__global__ void mdn_nll_kernel(const float* __restrict__ batch, const float* __restrict__ mus, const float* __restrict__ sigmas,
                               const float* __restrict__ logpi, int N, int G, int S, float* __restrict__ nll) {
  const int lane = threadIdx.x & 63;
  const long wave_row = (long)blockIdx.x * MDN_WAVES + (threadIdx.x >> 6);
  const bool live = wave_row < N;
  const long row = live ? wave_row : N - 1;
  const MdnRow r = mdn_row<false>(batch + row * S, mus + row * G * S, sigmas + row * G * S, logpi + row * G, G, S, lane);
  if (live && lane == 0) nll[row] = (float)(-r.logp);
}

// the forward's split alone (mdn_rnn.py:80-90): sigmas = exp(log sigma), logpi = log_softmax(logits); one wave per row
__global__ void mdn_outputs_kernel(const float* __restrict__ z, long ldz, int N, int G, int S, float* __restrict__ sigmas,
                                   float* __restrict__ logpi) {
  const int lane = threadIdx.x & 63;
  const long wave_row = (long)blockIdx.x * MDN_WAVES + (threadIdx.x >> 6);
  const bool live = wave_row < N;
  const long row = live ? wave_row : N - 1;
  const int stride = G * S;
  const float* zp = z + row * ldz;
  if (live)
    for (int e = lane; e < stride; e += 64) sigmas[row * stride + e] = (float)exp((double)zp[stride + e]);
  const bool mine = lane < G;
  const double pl = mine ? (double)zp[2 * stride + lane] : -(double)INFINITY;
  const double m = mdn_wave_max(pl);
  const double se = wave_sum_f64(mine ? exp(pl - m) : 0.0);
  if (live && mine) logpi[row * G + lane] = (float)(pl - m - log(se));
}

static int mdn_check(int n, int G, int S) {
  if (n < 1 || G < 1 || S < 1) return RG_EINVAL;
  if (G > RG_MDN_MAX_GAUSSIANS || S > RG_MDN_MAX_STATE_DIM) return RG_EUNSUPPORTED;
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_mdn_head_partials(int n) { return n < 1 ? 0 : (n + MDN_WAVES - 1) / MDN_WAVES; }

int rg_mdn_head(const float* z, int64_t ldz, const float* next_state, const float* reward, const float* not_terminal,
                double next_state_loss_weight, double not_terminal_loss_weight, double reward_loss_weight,
                int divide_by_state_dim, int first_row, int n, int num_gaussians, int state_dim, float* dz, int64_t lddz,
                float* sigmas, float* logpi, double* partials, float* losses, rg_stream_t stream) {
  const int rc = mdn_check(n, num_gaussians, state_dim);
  if (rc != RG_OK) return rc;
  const int64_t width = (2 * (int64_t)state_dim + 1) * num_gaussians + 2;
  if (!z || !next_state || !reward || !not_terminal || !dz || !partials || !losses) return RG_EINVAL;
  if (ldz < width || lddz < width || first_row < 0 || first_row >= n) return RG_EINVAL;
  const double rows = (double)(n - first_row);
  const double in_loss = divide_by_state_dim ? 1.0 / (double)(state_dim + 2) : 1.0;
  MdnHeadArgs a;
  a.z = z, a.ldz = (long)ldz, a.next_state = next_state, a.reward = reward, a.not_terminal = not_terminal;
  a.scale_gmm = next_state_loss_weight / rows * in_loss;
  a.scale_bce = not_terminal_loss_weight / rows, a.scale_mse = reward_loss_weight / rows;
  a.N = n, a.G = num_gaussians, a.S = state_dim, a.first_row = first_row;
  a.dz = dz, a.lddz = (long)lddz, a.sigmas = sigmas, a.logpi = logpi, a.partials = partials;
  const int blocks = rg_mdn_head_partials(n);
  RG_LAUNCH(mdn_head_kernel, dim3(blocks), dim3(MDN_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(mdn_finish_kernel, dim3(1), dim3(MDN_THREADS), (hipStream_t)stream, (const double*)partials, blocks,
            next_state_loss_weight / rows, a.scale_bce, a.scale_mse, in_loss, losses);
  return (int)hipGetLastError();
}

int rg_mdn_outputs(const float* z, int64_t ldz, int n, int num_gaussians, int state_dim, float* sigmas, float* logpi,
                   rg_stream_t stream) {
  const int rc = mdn_check(n, num_gaussians, state_dim);
  if (rc != RG_OK) return rc;
  if (!z || !sigmas || !logpi || ldz < (2 * (int64_t)state_dim + 1) * num_gaussians + 2) return RG_EINVAL;
  RG_LAUNCH(mdn_outputs_kernel, dim3(rg_mdn_head_partials(n)), dim3(MDN_THREADS), (hipStream_t)stream, z, (long)ldz, n,
            num_gaussians, state_dim, sigmas, logpi);
  return (int)hipGetLastError();
}

int rg_mdn_gmm_nll(const float* batch, const float* mus, const float* sigmas, const float* logpi, int n, int num_gaussians,
                   int state_dim, float* nll, rg_stream_t stream) {
  const int rc = mdn_check(n, num_gaussians, state_dim);
  if (rc != RG_OK) return rc;
  if (!batch || !mus || !sigmas || !logpi || !nll) return RG_EINVAL;
  RG_LAUNCH(mdn_nll_kernel, dim3(rg_mdn_head_partials(n)), dim3(MDN_THREADS), (hipStream_t)stream, batch, mus, sigmas, logpi,
            n, num_gaussians, state_dim, nll);
  return (int)hipGetLastError();
}

}  // extern "C"
