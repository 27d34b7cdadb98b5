// synthetic_reward.hip — the synthetic-reward nets' own kernels (reagent/models/synthetic_reward.py,
// reagent/training/reward_network_trainer.py).
//
// rg_ngram_concat is ngram() over cat(state, action) (synthetic_reward.py:177-205, :399-403) as one copy: no shifted
// copies, no tiles of the zero padding, no second concatenation.  A wave per output row, lanes along the feature axis.
//
// rg_step_reward_head is everything behind the nets' trunk: the last Linear(P, 1) and its activation, _gen_mask, the masked
// sum (:245-266), the loss wrapper of reward_network_trainer.py:27-66 (BCE's division by valid_step, the threshold filter,
// the mean over the kept rows) and the gradients into the trunk's output and the last layer.  A wave per batch row walks
// the row's T steps; lanes stride over P and a butterfly adds their doubles in a fixed order.  The count of kept rows is
// grid-wide and the gradient's scale needs it, so the entry point is three launches: the main one (outputs, the row's
// d loss / d pred, per-workgroup double partials of dw, dbias, the loss and the count, all unscaled), a finishing one (the
// partials added in a fixed order, times 1 / n_kept, rounded once) and the one that writes dh.  No atomics, no flag a
// workgroup waits on: two runs give the same bits.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"  // wave_sum_f64

namespace rg {

constexpr int SRW_THREADS = 256;
constexpr int SRW_WAVES = SRW_THREADS / 64;  // rows of a workgroup: a wave each
constexpr int SRW_DH_ROWS = 16;              // (t, b) rows of a workgroup of the dh launch: four per wave

struct NgramArgs {
  const float *state, *action;
  long ld_state, ld_action, ld_out;
  long N;  // T * B
  int T, B, S, A, n;
  float* out;
};

// out[t, b, i * F + f] = cat(state, action)[t + i - n / 2, b, f] inside the sequence, else 0
__global__ void srw_ngram_kernel(const NgramArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * SRW_WAVES + (threadIdx.x >> 6);
  if (row >= a.N) return;
  const int F = a.S + a.A, W = F * a.n, half = a.n / 2;
  const int t = (int)(row / a.B);
  const long b = row - (long)t * a.B;
  float* out = a.out + row * a.ld_out;
  for (int col = lane; col < W; col += 64) {
    const int i = col / F, f = col - i * F;
    const int ts = t + i - half;
    float v = 0.0f;
    if (ts >= 0 && ts < a.T) {
      const long src = (long)ts * a.B + b;
      v = f < a.S ? a.state[src * a.ld_state + f] : a.action[src * a.ld_action + (f - a.S)];
    }
    out[col] = v;
  }
}

// the six activations on a double and their derivatives at z (r = act(z)); a NaN stays a NaN
__device__ __forceinline__ double srw_act(double z, int act, double* dz) {
  switch (act) {
    case RG_ACT_RELU: *dz = z > 0.0 ? 1.0 : 0.0; return z < 0.0 ? 0.0 : z;
    case RG_ACT_LEAKY_RELU: *dz = z > 0.0 ? 1.0 : 0.01; return z < 0.0 ? 0.01 * z : z;
    case RG_ACT_TANH: { const double r = tanh(z); *dz = 1.0 - r * r; return r; }
    case RG_ACT_SIGMOID: { const double r = 1.0 / (1.0 + exp(-z)); *dz = r * (1.0 - r); return r; }
    case RG_ACT_SOFTPLUS: {  // nn.Softplus(beta 1, threshold 20)
      if (z > 20.0) { *dz = 1.0; return z; }
      *dz = 1.0 / (1.0 + exp(-z));
      return log1p(exp(z));
    }
    default: *dz = 1.0; return z;
  }
}

// the row's loss and d loss / d pred from its summed prediction and target (v: the clamped valid step)
__device__ __forceinline__ double srw_row_loss(double pred, double target, int v, int loss_type, double* dpred) {
  if (loss_type == RG_SRW_LOSS_BCE) {  // reward_network_trainer.py:44-48, nn.BCELoss: both logs clamped at -100
    const double p = pred / (double)v, y = target / (double)v;
    if (!(p >= 0.0 && p <= 1.0)) {  // (torch raises; a NaN for the row here)
      *dpred = NAN;
      return NAN;
    }
    const double lp = fmax(log(p), -100.0), l1p = fmax(log1p(-p), -100.0);
    *dpred = (p - y) / fmax((1.0 - p) * p, 1e-12) / (double)v;  // binary_cross_entropy_backward's epsilon
    return -(y * lp + (1.0 - y) * l1p);
  }
  const double d = pred - target, ad = fabs(d);
  const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);  // 0 at 0, NaN at NaN
  if (loss_type == RG_SRW_LOSS_MSE) {
    *dpred = 2.0 * d;
    return d * d;
  }
  if (loss_type == RG_SRW_LOSS_L1) {
    *dpred = sign;
    return ad;
  }
  *dpred = ad < 1.0 ? d : sign;  // SmoothL1, beta 1
  return ad < 1.0 ? 0.5 * d * d : ad - 0.5;
}

struct SrwHeadArgs {
  const float *h, *w, *bias;
  const int64_t* valid_step;
  const float* target;
  int act, loss_type, filter;  // filter: has_threshold && apply_threshold
  float threshold;
  int T, B, P;
  float *output, *mask, *pred;
  int grad;          // dh wanted: da, g and the dw / dbias partials are written
  double* partials;  // [workgroups][cols]: dw [P] and dbias (grad), the kept rows' loss, their count
  double* da;        // [T, B]: mask * act'(z)
  double* g;         // [B]: the kept row's d loss_b / d pred_b, unscaled; 0 for a dropped row
};

__device__ __forceinline__ int srw_cols(int P, int grad) { return (grad ? P + 1 : 0) + 2; }

__global__ void RG_LAUNCH_BOUNDS(SRW_THREADS, 1) srw_head_kernel(const SrwHeadArgs a) {
  __shared__ double red[SRW_WAVES][64];
  __shared__ double row_s[SRW_WAVES][3];  // the row's dbias term, loss and kept flag
  const int T = a.T, B = a.B, P = a.P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * SRW_WAVES + wave;
  const bool live = b < B;  // a wave past the last row computes nothing and adds zeros
  const double bias = (double)a.bias[0];
  double g = 0.0, loss = 0.0, kept = 0.0, sum_da = 0.0;
  if (live) {
    const int64_t vs = a.valid_step[b];
    const int v = (int)(vs < 1 ? 1 : (vs > T ? T : vs));
    double pred = 0.0;
    for (int t = 0; t < T; ++t) {
      const float* hr = a.h + ((long)t * B + b) * P;
      double s = 0.0;
      for (int k = lane; k < P; k += 64) s = fma((double)hr[k], (double)a.w[k], s);
      const double z = wave_sum_f64(s) + bias;
      double dz;
      const double r = srw_act(z, a.act, &dz);
      const bool in = t >= T - v;
      if (in) pred += r;
      if (lane == 0) {
        a.output[b * T + t] = (float)r;
        a.mask[b * T + t] = in ? 1.0f : 0.0f;
        if (a.grad) a.da[(long)t * B + b] = in ? dz : 0.0;
      }
      if (in) sum_da += dz;
    }
    if (lane == 0) a.pred[b] = (float)pred;
    if (a.target) {
      const float target = a.target[b];
      // the filter compares what the reference compares: the fp32 target, for BCE after its fp32 division by valid_step
      const float shown = a.loss_type == RG_SRW_LOSS_BCE ? __fdiv_rn(target, (float)v) : target;
      const bool keep = !a.filter || shown <= a.threshold;
      double dpred;
      const double l = srw_row_loss(pred, (double)target, v, a.loss_type, &dpred);
      if (keep) g = dpred, loss = l, kept = 1.0;
      if (a.grad && lane == 0) a.g[b] = g;
    }
  }
  if (!a.target) return;  // (the outputs alone; uniform over the launch)
  double* part = a.partials + (long)blockIdx.x * srw_cols(P, a.grad);
  if (lane == 0) row_s[wave][0] = g * sum_da, row_s[wave][1] = loss, row_s[wave][2] = kept;
  __syncthreads();  // row_s; and every da of the workgroup's rows, written by lane 0, is visible to all lanes
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int r = 0; r < SRW_WAVES; ++r) s += row_s[r][threadIdx.x];
    if (threadIdx.x > 0) part[(a.grad ? P + 1 : 0) + threadIdx.x - 1] = s;
    else if (a.grad) part[P] = s;
  }
  if (!a.grad) return;
  // dw: 64 columns at a time, each wave its row's sum over the steps, the four rows added in order
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    double acc = 0.0;
    if (live && p < P && g != 0.0) {
      for (int t = 0; t < T; ++t) {
        const long row = (long)t * B + b;
        acc = fma(g * a.da[row], (double)a.h[row * P + p], acc);
      }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && p < P) part[p] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    __syncthreads();
  }
}

// A wave per column of partials [blocks][cols]: lanes stride over the blocks, a butterfly adds them.  The count first (every
// wave needs the scale), then the column: dw and dbias and the loss times 1 / n_kept, rounded once.
__global__ void srw_finish_kernel(const double* __restrict__ partials, int blocks, int cols, int P, int grad,
                                  float* __restrict__ dw, float* __restrict__ dbias, float* __restrict__ loss,
                                  int32_t* __restrict__ n_kept) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * SRW_WAVES + (threadIdx.x >> 6);
  double n = 0.0, s = 0.0;
  for (int q = lane; q < blocks; q += 64) n += partials[(long)q * cols + cols - 1];
  n = wave_sum_f64(n);
  if (c >= cols) return;
  for (int q = lane; q < blocks; q += 64) s += partials[(long)q * cols + c];
  s = wave_sum_f64(s);
  if (lane != 0) return;
  const double scale = n > 0.0 ? 1.0 / n : 0.0;  // (no row kept: zero gradients and, below, a NaN loss)
  if (c == cols - 1) n_kept[0] = (int32_t)n;
  else if (c == cols - 2) loss[0] = n > 0.0 ? (float)(s * scale) : NAN;
  else if (c == P) dbias[0] = (float)(s * scale);
  else dw[c] = (float)(s * scale);
}

// dh[t, b, :] = da[t, b] * g[b] / n_kept * w, written entirely
__global__ void srw_dh_kernel(const double* __restrict__ da, const double* __restrict__ g, const int32_t* __restrict__ n_kept,
                              const float* __restrict__ w, long N, int B, int P, float* __restrict__ dh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = n_kept[0];
  const double scale = n > 0 ? 1.0 / (double)n : 0.0;
  for (int j = 0; j < SRW_DH_ROWS / SRW_WAVES; ++j) {
    const long row = (long)blockIdx.x * SRW_DH_ROWS + j * SRW_WAVES + wave;
    if (row >= N) return;
    const double gb = g[row % B], d = da[row];
    // (a row the mask or the filter drops is +0 whatever w holds)
    const double coef = (d == 0.0 || gb == 0.0) ? 0.0 : d * gb * scale;
    float* out = dh + row * P;
    for (int p = lane; p < P; p += 64) out[p] = coef == 0.0 ? 0.0f : (float)(coef * (double)w[p]);
  }
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_ngram_concat(const float* state, int64_t ld_state, const float* action, int64_t ld_action, int seq_len, int batch,
                    int state_dim, int action_dim, int context_size, float* out, int64_t ld_out, rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || state_dim < 1 || action_dim < 1) return RG_EINVAL;
  if (context_size < 1 || context_size % 2 == 0) return RG_EINVAL;
  if (!state || !action || !out) return RG_EINVAL;
  const int64_t width = ((int64_t)state_dim + action_dim) * context_size;
  if (ld_state < state_dim || ld_action < action_dim || ld_out < width) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29) || width >= (1LL << 31)) return RG_EUNSUPPORTED;
  NgramArgs a;
  a.state = state, a.action = action, a.ld_state = (long)ld_state, a.ld_action = (long)ld_action, a.ld_out = (long)ld_out;
  a.N = (long)seq_len * batch, a.T = seq_len, a.B = batch, a.S = state_dim, a.A = action_dim, a.n = context_size, a.out = out;
  RG_LAUNCH(srw_ngram_kernel, dim3((unsigned)((a.N + SRW_WAVES - 1) / SRW_WAVES)), dim3(SRW_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_step_reward_head_partials(int batch) { return batch < 1 ? 0 : (batch + SRW_WAVES - 1) / SRW_WAVES; }

int rg_step_reward_head(const float* h, const float* w, const float* bias, int act, const int64_t* valid_step,
                        const float* target, int loss_type, int has_threshold, double threshold, int apply_threshold,
                        int seq_len, int batch, int width, float* output, float* mask, float* predicted_reward, float* loss,
                        int32_t* n_kept, float* dh, float* dw, float* dbias, double* workspace, rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || width < 1) return RG_EINVAL;
  if (act < RG_ACT_LINEAR || act > RG_ACT_SOFTPLUS) return RG_EINVAL;
  if (!h || !w || !bias || !valid_step || !output || !mask || !predicted_reward) return RG_EINVAL;
  if (target && (loss_type < RG_SRW_LOSS_MSE || loss_type > RG_SRW_LOSS_BCE)) return RG_EINVAL;
  if (target && (!loss || !n_kept || !workspace)) return RG_EINVAL;
  if (dh && (!target || !dw || !dbias)) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29)) return RG_EUNSUPPORTED;
  const int blocks = rg_step_reward_head_partials(batch), grad = dh ? 1 : 0;
  const int cols = (grad ? width + 1 : 0) + 2;
  SrwHeadArgs a;
  a.h = h, a.w = w, a.bias = bias, a.valid_step = valid_step, a.target = target;
  a.act = act, a.loss_type = loss_type, a.filter = has_threshold && apply_threshold, a.threshold = (float)threshold;
  a.T = seq_len, a.B = batch, a.P = width, a.output = output, a.mask = mask, a.pred = predicted_reward, a.grad = grad;
  a.partials = workspace;
  a.da = workspace ? workspace + (int64_t)blocks * cols : nullptr;
  a.g = a.da ? a.da + (int64_t)seq_len * batch : nullptr;
  RG_LAUNCH(srw_head_kernel, dim3(blocks), dim3(SRW_THREADS), (hipStream_t)stream, a);
  if (!target) return (int)hipGetLastError();
  RG_LAUNCH(srw_finish_kernel, dim3((cols + SRW_WAVES - 1) / SRW_WAVES), dim3(SRW_THREADS), (hipStream_t)stream,
            (const double*)a.partials, blocks, cols, width, grad, dw, dbias, loss, n_kept);
  if (grad) {
    const long N = (long)seq_len * batch;
    RG_LAUNCH(srw_dh_kernel, dim3((unsigned)((N + SRW_DH_ROWS - 1) / SRW_DH_ROWS)), dim3(SRW_THREADS), (hipStream_t)stream,
              (const double*)a.da, (const double*)a.g, (const int32_t*)n_kept, w, N, batch, width, dh);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
