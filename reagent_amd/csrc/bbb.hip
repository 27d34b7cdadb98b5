// bbb.hip — the reward models of reagent/training/cfeval/: Bayes by backprop on a FullyConnectedProbabilisticNetwork
// (reagent/models/probabilistic_fully_connected_network.py) and the per-action bandit reward head
// (cfeval/bandit_reward_network_trainer.py).
//
// rg_bbb_sample, rg_bbb_fill_noise and rg_bbb_grad walk a segment table passed by value (a layer's weights and its biases
// are a segment each): a workgroup takes RG_BBB_CHUNK consecutive elements of one segment, so the launches do not depend on
// the network's depth.  The reference spends about a dozen small torch operations per layer, twice, and autograd on top
// (:87-105); here the draw, softplus, both log-densities and later the chain rule into mu and rho are an element-wise pass in
// double each.  rg_bbb_elbo_head is sample_elbo's likelihood and loss (:190-213); rg_bandit_reward_head is everything behind
// the bandit trainer's [B, A] forward.  Sums are per-workgroup double partials added in a fixed order by a finishing launch:
// no atomics, no flag a workgroup waits on, two runs give the same bits.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_philox.h"
#include "rg_reduce.h"  // wave_sum_f64

namespace rg {

constexpr int BBB_THREADS = 256;
constexpr int BBB_WAVES = BBB_THREADS / 64;
constexpr int BBB_PER_THREAD = RG_BBB_CHUNK / BBB_THREADS;
constexpr double BBB_HALF_LOG_2PI = 0.91893853320467274178;

struct BbbArgs {
  rg_bbb_table t;
  int begin[RG_BBB_MAX_SEGMENTS + 1];  // the first workgroup of every segment; unused slots hold the end
  double prior_var, scale;
  uint64_t seed;
  int sample, draw, accumulate;
  double* partials;  // [workgroups][2]
};

// the workgroup's segment: the last s with begin[s] <= block
__device__ __forceinline__ int bbb_segment(const BbbArgs& a, int block) {
  int s = 0;
  for (int i = 1; i < RG_BBB_MAX_SEGMENTS; ++i)
    if (i < a.t.n_segments && block >= a.begin[i]) s = i;
  return s;
}

// cos(2 pi u) for u in [0, 1): 4 u = q + r with q an integer and |r| <= 1/2 (exact), x = r pi / 2, and cos(q pi / 2 + x) is
// cos x, -sin x, -cos x or sin x by their series to x^14 and x^15 (|x| <= pi / 4: the next terms are under 2e-15)
__device__ __forceinline__ double bbb_cos2pi(double u) {
  const double t = 4.0 * u, q = rint(t), x = (t - q) * 1.57079632679489661923, x2 = x * x;
  double c = -1.0 / 87178291200.0, s = -1.0 / 1307674368000.0;  // -1 / 14!, -1 / 15!
  c = fma(c, x2, 1.0 / 479001600.0), s = fma(s, x2, 1.0 / 6227020800.0);
  c = fma(c, x2, -1.0 / 3628800.0), s = fma(s, x2, -1.0 / 39916800.0);
  c = fma(c, x2, 1.0 / 40320.0), s = fma(s, x2, 1.0 / 362880.0);
  c = fma(c, x2, -1.0 / 720.0), s = fma(s, x2, -1.0 / 5040.0);
  c = fma(c, x2, 1.0 / 24.0), s = fma(s, x2, 1.0 / 120.0);
  c = fma(c, x2, -0.5), s = fma(s, x2, -1.0 / 6.0);
  c = fma(c, x2, 1.0), s = x * fma(s, x2, 1.0);
  const int qi = (int)q & 3;
  const double v = (qi & 1) ? s : c;
  return (qi == 1 || qi == 2) ? -v : v;
}

// the draw of element e of segment seg for one sample (include/reagent_hip.h states the counter's layout): Box-Muller in
// double on the first two words, rounded once
__device__ __forceinline__ float bbb_normal(uint64_t seed, int seg, long e, int sample) {
  uint32_t x[4];
  philox4x32_10(seed, (uint64_t)e, (uint64_t)(uint32_t)sample | ((uint64_t)(uint32_t)seg << 32), x);
  const double u1 = ((double)x[0] + 1.0) * 0x1p-32, u2 = (double)x[1] * 0x1p-32;
  return (float)(sqrt(-2.0 * log(u1)) * bbb_cos2pi(u2));
}

// log(1 + exp(rho)) without the overflow of exp above and the loss of the 1 below
__device__ __forceinline__ double bbb_softplus(double rho) { return rho > 0.0 ? rho + log1p(exp(-rho)) : log1p(exp(rho)); }

__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1) bbb_fill_noise_kernel(const BbbArgs a) {
  const int s = bbb_segment(a, blockIdx.x);
  const rg_bbb_segment& g = a.t.seg[s];
  const long base = (long)(blockIdx.x - a.begin[s]) * RG_BBB_CHUNK;
#pragma unroll
  for (int j = 0; j < BBB_PER_THREAD; ++j) {
    const long e = base + j * BBB_THREADS + threadIdx.x;
    if (e < g.n) g.eps[e] = bbb_normal(a.seed, s, e, a.sample);
  }
}

__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1) bbb_sample_kernel(const BbbArgs a) {
  __shared__ double red[BBB_WAVES][2];
  const int s = bbb_segment(a, blockIdx.x);
  const rg_bbb_segment& g = a.t.seg[s];
  const long base = (long)(blockIdx.x - a.begin[s]) * RG_BBB_CHUNK;
  const double pv = a.prior_var, log_pv = log(pv), inv_2pv2 = 0.5 / (pv * pv);
  double prior = 0.0, post = 0.0;
#pragma unroll
  for (int j = 0; j < BBB_PER_THREAD; ++j) {
    const long e = base + j * BBB_THREADS + threadIdx.x;
    if (e < g.n) {
      float epsf;
      if (a.draw) g.eps[e] = epsf = bbb_normal(a.seed, s, e, a.sample);
      else epsf = g.eps[e];
      const double mu = (double)g.mu[e], sigma = bbb_softplus((double)g.rho[e]);
      const float wf = (float)fma(sigma, (double)epsf, mu);
      g.w[e] = wf;
      const double w = (double)wf, d = w - mu;
      prior += -(w * w) * inv_2pv2 - log_pv - BBB_HALF_LOG_2PI;
      post += -(d * d) / (2.0 * sigma * sigma) - log(sigma) - BBB_HALF_LOG_2PI;
    }
  }
  prior = wave_sum_f64(prior), post = wave_sum_f64(post);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = prior, red[wave][1] = post;
  __syncthreads();
  if (threadIdx.x < 2)
    a.partials[(long)blockIdx.x * 2 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one workgroup of two waves: wave c adds column c of partials [blocks][2], lanes striding over the blocks
__global__ void bbb_sample_finish_kernel(const double* __restrict__ partials, int blocks, float* __restrict__ log_prior,
                                         float* __restrict__ log_post, double* __restrict__ terms) {
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
  double s = 0.0;
  for (int q = lane; q < blocks; q += 64) s += partials[(long)q * 2 + c];
  s = wave_sum_f64(s);
  if (lane != 0) return;
  terms[c] = s;
  (c == 0 ? log_prior : log_post)[0] = (float)s;
}

__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1) bbb_grad_kernel(const BbbArgs a) {
  const int s = bbb_segment(a, blockIdx.x);
  const rg_bbb_segment& g = a.t.seg[s];
  const long base = (long)(blockIdx.x - a.begin[s]) * RG_BBB_CHUNK;
  const double inv_pv2 = 1.0 / (a.prior_var * a.prior_var), scale = a.scale;
#pragma unroll
  for (int j = 0; j < BBB_PER_THREAD; ++j) {
    const long e = base + j * BBB_THREADS + threadIdx.x;
    if (e < g.n) {
      const double rho = (double)g.rho[e], mu = (double)g.mu[e], w = (double)g.w[e], eps = (double)g.eps[e];
      const double sigma = bbb_softplus(rho), d = w - mu, is = 1.0 / sigma;
      const double sig = rho >= 0.0 ? 1.0 / (1.0 + exp(-rho)) : exp(rho) / (1.0 + exp(rho));  // sigmoid(rho) = d sigma / d rho
      const double gw = (double)g.dw[e] + scale * (w * inv_pv2 - d * is * is);
      const double gr = sig * (gw * eps + scale * (d * d * is * is * is - is));
      g.dmu[e] = a.accumulate ? (float)((double)g.dmu[e] + gw) : (float)gw;
      g.drho[e] = a.accumulate ? (float)((double)g.drho[e] + gr) : (float)gr;
    }
  }
}

// ---- the ELBO head -------------------------------------------------------------------------------------------------------
__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1)
    bbb_elbo_rows_kernel(const float* __restrict__ out, long ld_out, const float* __restrict__ target, int B, double noise_tol,
                         double scale, float* __restrict__ dout, double* __restrict__ partials) {
  __shared__ double red[BBB_WAVES];
  const long r = (long)blockIdx.x * BBB_THREADS + threadIdx.x;
  double ll = 0.0;
  if (r < B) {
    const double d = (double)out[r * ld_out] - (double)target[r], it = 1.0 / noise_tol;
    ll = -(d * d) * (0.5 * it * it) - log(noise_tol) - BBB_HALF_LOG_2PI;
    if (dout) dout[r] = (float)(scale * d * it * it);
  }
  ll = wave_sum_f64(ll);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ll;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave: the partials in lane-strided order, then the loss and its terms
__global__ void bbb_elbo_finish_kernel(const double* __restrict__ partials, int blocks, const double* __restrict__ terms,
                                       double scale, int accumulate, double* __restrict__ acc, float* __restrict__ result) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int q = lane; q < blocks; q += 64) s += partials[q];
  const double like = wave_sum_f64(s);
  if (lane >= 4) return;
  const double prior = terms[0], post = terms[1];
  const double v = lane == 0 ? (post - prior) - like : (lane == 1 ? prior : (lane == 2 ? post : like));
  const double t = (accumulate ? acc[lane] : 0.0) + scale * v;
  acc[lane] = t;
  result[lane] = (float)t;
}

// ---- the bandit reward head ----------------------------------------------------------------------------------------------
struct BanditArgs {
  const float *q, *action, *reward, *action_prob;
  long ld_q, ld_action, ld_dq;
  int B, A, loss_type, filter, blocks;
  float threshold;
  float *pred, *loss, *unweighted, *dq;
  int32_t* n_kept;
  double* partials;  // [blocks][3]: the kept rows' weighted loss, their unweighted loss, their count
  double* g;         // [B]: weight * d l / d pred of a kept row, 0 of a dropped one
  int32_t* idx;      // [B]: the logged action
};

__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1) bandit_rows_kernel(const BanditArgs a) {
  __shared__ double red[BBB_WAVES][3];
  const long r = (long)blockIdx.x * BBB_THREADS + threadIdx.x;
  double wl = 0.0, ul = 0.0, kept = 0.0;
  if (r < a.B) {
    const float* act = a.action + r * a.ld_action;
    int idx = 0;
    float best = act[0];
    for (int c = 1; c < a.A; ++c) {  // the first maximum; the first NaN beats everything (torch.argmax)
      const float v = act[c];
      if (best == best && (v > best || v != v)) best = v, idx = c;
    }
    const float predf = a.q[r * a.ld_q + idx], target = a.reward[r];
    a.pred[r] = predf;
    a.idx[r] = idx;
    const double d = (double)predf - (double)target, ad = fabs(d);
    const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);  // 0 at 0, NaN at NaN
    double l, dl;
    if (a.loss_type == RG_SRW_LOSS_MSE) l = d * d, dl = 2.0 * d;
    else if (a.loss_type == RG_SRW_LOSS_L1) l = ad, dl = sign;
    else l = ad < 1.0 ? 0.5 * d * d : ad - 0.5, dl = ad < 1.0 ? d : sign;  // SmoothL1, beta 1
    const double weight = a.action_prob ? 1.0 / (double)a.action_prob[r] : 1.0;
    const bool keep = !a.filter || target <= a.threshold;
    if (keep) wl = weight * l, ul = l, kept = 1.0;
    a.g[r] = keep ? weight * dl : 0.0;
  }
  wl = wave_sum_f64(wl), ul = wave_sum_f64(ul), kept = wave_sum_f64(kept);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = wl, red[wave][1] = ul, red[wave][2] = kept;
  __syncthreads();
  if (threadIdx.x < 3)
    a.partials[(long)blockIdx.x * 3 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Every workgroup adds the whole partial table in the same order (wave c its column c, lanes striding over the blocks), so
// each has the same n_kept to the bit; workgroup 0 writes the scalars, and each writes dq of its 256 rows, whole.
__global__ void RG_LAUNCH_BOUNDS(BBB_THREADS, 1) bandit_finish_kernel(const BanditArgs a) {
  __shared__ double tot[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < 3) {
    double s = 0.0;
    for (int q = lane; q < a.blocks; q += 64) s += a.partials[(long)q * 3 + wave];
    s = wave_sum_f64(s);
    if (lane == 0) tot[wave] = s;
  }
  __syncthreads();
  const double n = tot[2], scale = n > 0.0 ? 1.0 / n : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.loss[0] = n > 0.0 ? (float)(tot[0] * scale) : NAN;
    if (a.unweighted) a.unweighted[0] = n > 0.0 ? (float)(tot[1] * scale) : NAN;
    a.n_kept[0] = (int32_t)n;
  }
  if (!a.dq) return;
  const long row0 = (long)blockIdx.x * BBB_THREADS;
  const long rows = a.B - row0 < BBB_THREADS ? a.B - row0 : BBB_THREADS;
  for (long e = threadIdx.x; e < rows * a.A; e += BBB_THREADS) {
    const long r = row0 + e / a.A;
    const int c = (int)(e % a.A);
    const double g = a.g[r];
    a.dq[r * a.ld_dq + c] = (c == a.idx[r] && g != 0.0) ? (float)(g * scale) : 0.0f;
  }
}

// the table's workgroups and every segment's first; -1 for a table the kernels do not take
static int bbb_plan(const rg_bbb_table* t, BbbArgs& a, int* rc) {
  *rc = RG_EINVAL;
  if (!t || t->n_segments < 1 || t->n_segments > RG_BBB_MAX_SEGMENTS) return -1;
  long blocks = 0;
  for (int s = 0; s < t->n_segments; ++s) {
    if (t->seg[s].n < 1) return -1;
    if (t->seg[s].n >= (1LL << 31)) {
      *rc = RG_EUNSUPPORTED;
      return -1;
    }
    a.begin[s] = (int)blocks;
    blocks += (t->seg[s].n + RG_BBB_CHUNK - 1) / RG_BBB_CHUNK;
  }
  if (blocks >= (1L << 31)) {
    *rc = RG_EUNSUPPORTED;
    return -1;
  }
  pad_begin_table(a.begin, t->n_segments, blocks);
  a.t = *t;
  for (int s = t->n_segments; s < RG_BBB_MAX_SEGMENTS; ++s) a.t.seg[s] = rg_bbb_segment{};
  a.prior_var = 1.0, a.scale = 1.0, a.seed = 0, a.sample = 0, a.draw = 0, a.accumulate = 0, a.partials = nullptr;
  *rc = RG_OK;
  return (int)blocks;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_bbb_chunks(const rg_bbb_table* table) {
  BbbArgs a;
  int rc;
  const int blocks = bbb_plan(table, a, &rc);
  return blocks < 0 ? 0 : blocks;
}

int rg_bbb_fill_noise(const rg_bbb_table* table, uint64_t seed, int sample, rg_stream_t stream) {
  BbbArgs a;
  int rc;
  const int blocks = bbb_plan(table, a, &rc);
  if (blocks < 0) return rc;
  if (sample < 0) return RG_EINVAL;
  for (int s = 0; s < table->n_segments; ++s)
    if (!table->seg[s].eps) return RG_EINVAL;
  a.seed = seed, a.sample = sample;
  RG_LAUNCH(bbb_fill_noise_kernel, dim3(blocks), dim3(BBB_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_bbb_sample(const rg_bbb_table* table, double prior_var, int draw, uint64_t seed, int sample, float* log_prior,
                  float* log_post, double* terms, double* workspace, rg_stream_t stream) {
  BbbArgs a;
  int rc;
  const int blocks = bbb_plan(table, a, &rc);
  if (blocks < 0) return rc;
  if (!(prior_var > 0.0) || sample < 0 || !log_prior || !log_post || !terms || !workspace) return RG_EINVAL;
  for (int s = 0; s < table->n_segments; ++s) {
    const rg_bbb_segment& g = table->seg[s];
    if (!g.mu || !g.rho || !g.w || !g.eps) return RG_EINVAL;
  }
  a.prior_var = prior_var, a.draw = draw ? 1 : 0, a.seed = seed, a.sample = sample, a.partials = workspace;
  RG_LAUNCH(bbb_sample_kernel, dim3(blocks), dim3(BBB_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(bbb_sample_finish_kernel, dim3(1), dim3(128), (hipStream_t)stream, (const double*)workspace, blocks, log_prior,
            log_post, terms);
  return (int)hipGetLastError();
}

int rg_bbb_grad(const rg_bbb_table* table, double prior_var, double scale, int accumulate, rg_stream_t stream) {
  BbbArgs a;
  int rc;
  const int blocks = bbb_plan(table, a, &rc);
  if (blocks < 0) return rc;
  if (!(prior_var > 0.0)) return RG_EINVAL;
  for (int s = 0; s < table->n_segments; ++s) {
    const rg_bbb_segment& g = table->seg[s];
    if (!g.mu || !g.rho || !g.w || !g.eps || !g.dw || !g.dmu || !g.drho) return RG_EINVAL;
  }
  a.prior_var = prior_var, a.scale = scale, a.accumulate = accumulate ? 1 : 0;
  RG_LAUNCH(bbb_grad_kernel, dim3(blocks), dim3(BBB_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_bbb_elbo_head_partials(int batch) { return batch < 1 ? 0 : (batch + BBB_THREADS - 1) / BBB_THREADS; }

int rg_bbb_elbo_head(const float* out, int64_t ld_out, const float* target, int batch, double noise_tol, double scale,
                     int accumulate, const double* terms, double* acc, float* result, float* dout, double* workspace,
                     rg_stream_t stream) {
  if (batch < 1 || ld_out < 1 || !(noise_tol > 0.0)) return RG_EINVAL;
  if (!out || !target || !terms || !acc || !result || !workspace) return RG_EINVAL;
  const int blocks = rg_bbb_elbo_head_partials(batch);
  RG_LAUNCH(bbb_elbo_rows_kernel, dim3(blocks), dim3(BBB_THREADS), (hipStream_t)stream, out, (long)ld_out, target, batch,
            noise_tol, scale, dout, workspace);
  RG_LAUNCH(bbb_elbo_finish_kernel, dim3(1), dim3(64), (hipStream_t)stream, (const double*)workspace, blocks, terms, scale,
            accumulate ? 1 : 0, acc, result);
  return (int)hipGetLastError();
}

// partials [blocks][3], g [B], then idx [B] as int32 (two to a double)
int rg_bandit_reward_head_workspace(int batch) {
  if (batch < 1) return 0;
  return 3 * ((batch + BBB_THREADS - 1) / BBB_THREADS) + batch + (batch + 1) / 2;
}

int rg_bandit_reward_head(const float* q, int64_t ld_q, const float* action, int64_t ld_action, const float* reward,
                          const float* action_prob, int loss_type, int has_threshold, double threshold, int apply_threshold,
                          int batch, int num_actions, float* predicted_reward, float* loss, float* unweighted_loss,
                          int32_t* n_kept, float* dq, int64_t ld_dq, double* workspace, rg_stream_t stream) {
  if (batch < 1 || num_actions < 1 || ld_q < num_actions || ld_action < num_actions) return RG_EINVAL;
  if (!q || !action || !reward || !predicted_reward || !loss || !n_kept || !workspace) return RG_EINVAL;
  if (loss_type != RG_SRW_LOSS_MSE && loss_type != RG_SRW_LOSS_SMOOTH_L1 && loss_type != RG_SRW_LOSS_L1) return RG_EINVAL;
  if (dq && ld_dq < num_actions) return RG_EINVAL;
  if ((int64_t)batch * num_actions >= (1LL << 31)) return RG_EUNSUPPORTED;
  BanditArgs a;
  a.q = q, a.action = action, a.reward = reward, a.action_prob = action_prob;
  a.ld_q = (long)ld_q, a.ld_action = (long)ld_action, a.ld_dq = (long)ld_dq;
  a.B = batch, a.A = num_actions, a.loss_type = loss_type, a.filter = has_threshold && apply_threshold;
  a.blocks = (batch + BBB_THREADS - 1) / BBB_THREADS;
  a.threshold = (float)threshold;
  a.pred = predicted_reward, a.loss = loss, a.unweighted = unweighted_loss, a.dq = dq, a.n_kept = n_kept;
  a.partials = workspace;
  a.g = workspace + 3L * a.blocks;
  a.idx = (int32_t*)(a.g + batch);
  RG_LAUNCH(bandit_rows_kernel, dim3(a.blocks), dim3(BBB_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(bandit_finish_kernel, dim3(a.blocks), dim3(BBB_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
