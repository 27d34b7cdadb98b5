// seq2reward.hip — the Seq2Reward world model's own kernels (reagent/models/seq2reward_model.py, reagent/training/
// world_model/seq2reward_trainer.py, compress_model_trainer.py).
//
// Planning (get_Q, seq2reward_trainer.py:31-64) enumerates all P = A^H action sequences in lexical order and runs the LSTM
// over B * P rows for H steps.  Sequences that share a prefix share every cell of that prefix, so the rollout is a tree:
// depth t has B * A^t distinct rows, and child r of a level continues parent r / A with action r % A.  rg_lstm_fanout_step
// is one layer's step over one level: lstm_forward_kernel's tile and arithmetic (rg_lstm_cell.h), with h_{t-1} and c_{t-1}
// read from the parent's row and layer 0's input projection read from the A rows of the projected identity.
// rg_seq2reward_plan_max is lstm_linear over the leaves and the max per first action.
//
// Training: rg_seq2reward_head (lstm_linear at each row's valid step, the discounted reward target, the mse loss and its
// gradients) and rg_step_ce_head (the step predictor's cross-entropy).  Sums leave as per-workgroup partials in double; a
// finishing launch adds them in a fixed order and rounds once.  No atomics.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"
#include "rg_reduce.h"  // shfl_xor_f64

namespace rg {

struct FanoutArgs {
  const float *h_prev, *c_prev, *proj, *w_hh, *b_hh;
  float *h, *c;
  long N;
  int fanout, table_rows, H, Hp;
};

// lstm_forward_kernel's step for t = 0, with the row's initial state read from its parent and nothing kept for a next step
__global__ void RG_LAUNCH_BOUNDS(LSTM_THREADS, 1) s2r_fanout_kernel(const FanoutArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  const int H = a.H, Hp = a.Hp, pitch = Hp + 1, tiles = Hp / LSTM_TILE;
  const long N = a.N;
  float* cur = (float*)smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * LSTM_ROWS;
  for (int e = threadIdx.x; e < LSTM_ROWS * Hp; e += LSTM_THREADS) {
    const int r = e / Hp, u = e % Hp;
    const long row = row0 + r;
    cur[r * pitch + u] = (row < N && u < H) ? a.h_prev[row / a.fanout * H + u] : 0.f;
  }
  __syncthreads();
  for (int tile = wave; tile < tiles; tile += LSTM_WAVES) {
    const int u = tile * LSTM_TILE + col;
    const bool u_ok = u < H;
    const int uc = u_ok ? u : H - 1;
    const LstmGates p = lstm_gate_products(cur, pitch, a.w_hh, H, H, Hp, uc, u_ok, col, half);
    double bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = a.b_hh ? (double)a.b_hh[g * H + uc] : 0.0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const f32x4 qi = lstm_acc_quad(p.i, q), qf = lstm_acc_quad(p.f, q), qg = lstm_acc_quad(p.g, q), qo = lstm_acc_quad(p.o, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long row = row0 + lstm_acc_row(4 * q + j, half);
        const bool ok = u_ok && row < N;
        const long rowc = row < N ? row : N - 1;  // (addresses stay inside the arrays; the values are dropped)
        const long prow = a.table_rows > 0 ? rowc % a.table_rows : rowc;
        const float* xp = a.proj + prow * 4 * H + uc;
        LstmCell e = lstm_gates(qi[j], qf[j], qg[j], qo[j], xp, H, bias, ec);
        const float cp = a.c_prev ? a.c_prev[rowc / a.fanout * H + uc] : 0.f;
        lstm_cell(e, cp, ec);
        if (ok) {
          a.h[rowc * H + uc] = e.h;
          a.c[rowc * H + uc] = e.c;
        }
      }
    }
  }
}

constexpr int S2R_THREADS = 256;
constexpr int S2R_WAVES = S2R_THREADS / 64;

// lstm_linear on one row: the sum in double in index order, the bias added last
__device__ __forceinline__ double s2r_dot(const float* __restrict__ h, const float* __restrict__ w, int H, double bias) {
  double s = 0.0;
  for (int k = 0; k < H; ++k) s = fma((double)h[k], (double)w[k], s);
  return s + bias;
}

// max that keeps a NaN (torch.max's): the order of the comparisons does not change the result
__device__ __forceinline__ float s2r_max(float a, float b) { return (a != a || b != b) ? (a != a ? a : b) : fmaxf(a, b); }

// a wave per group of `size` consecutive leaves: lane l takes leaves l, l + 64, ...
__global__ void s2r_plan_max_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                    long groups, int size, int H, float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const long wave_group = (long)blockIdx.x * S2R_WAVES + (threadIdx.x >> 6);
  const bool live = wave_group < groups;
  const long g = live ? wave_group : groups - 1;
  const double b = bias[0];
  float m = -INFINITY;
  for (int i = lane; i < size; i += 64) m = s2r_max(m, (float)s2r_dot(h + (g * size + i) * H, w, H, b));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = s2r_max(m, shfl_xor(m, off));
  if (live && lane == 0) q[g] = m;
}

struct S2rHeadArgs {
  const float* h_all;
  const int64_t* valid_step;
  const float *reward, *gamma_pow, *w, *bias;
  int T, B, H;
  float *acc_reward, *dh_all;
  double* partials;  // [workgroups][H + 2]: dw, dbias, the sum of the squared errors
};

// the step of row b as the kernels read it: valid_step clamped into [1, T], or T without one; zero-based
__device__ __forceinline__ int s2r_step(const int64_t* valid_step, long b, int T) {
  if (!valid_step) return T - 1;
  const int64_t v = valid_step[b];
  return (int)(v < 1 ? 1 : (v > T ? T : v)) - 1;
}

// A thread per row for the row's prediction and target; then the workgroup writes its rows of dh_all and its partial of dw
// together (consecutive threads, consecutive addresses).
__global__ void s2r_head_kernel(const S2rHeadArgs a) {
  __shared__ double d_s[S2R_THREADS];  // d loss / d pred of the workgroup's rows
  __shared__ int step_s[S2R_THREADS];
  const int T = a.T, B = a.B, H = a.H;
  const long row0 = (long)blockIdx.x * S2R_THREADS, b = row0 + threadIdx.x;
  const int rows = (int)(B - row0 < S2R_THREADS ? B - row0 : S2R_THREADS);
  double d = 0.0, sq = 0.0;
  int step = 0;
  if (b < B) {
    step = s2r_step(a.valid_step, b, T);
    const double pred = s2r_dot(a.h_all + ((long)step * B + b) * H, a.w, H, (double)a.bias[0]);
    a.acc_reward[b] = (float)pred;
    if (a.dh_all) {
      float target = 0.f;
      for (int i = 0; i <= step; ++i) target = __fadd_rn(target, __fmul_rn(a.reward[(long)i * B + b], a.gamma_pow[i]));
      const double diff = pred - (double)target;
      sq = diff * diff;
      d = 2.0 * diff / (double)B;
    }
  }
  if (!a.dh_all) return;  // (the forward alone; uniform over the launch)
  d_s[threadIdx.x] = d, step_s[threadIdx.x] = step;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    float* out = a.dh_all + ((long)t * B + row0) * H;
    for (int e = threadIdx.x; e < rows * H; e += S2R_THREADS) {
      const int r = e / H, u = e % H;
      out[e] = step_s[r] == t ? (float)(d_s[r] * (double)a.w[u]) : 0.f;
    }
  }
  double* part = a.partials + (long)blockIdx.x * (H + 2);
  for (int u = threadIdx.x; u < H; u += S2R_THREADS) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s = fma(d_s[r], (double)a.h_all[((long)step_s[r] * B + row0 + r) * H + u], s);
    part[u] = s;
  }
  // dbias and the squared errors: the workgroup's rows in order
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += d_s[r];
    part[H] = s;
  }
  __syncthreads();
  d_s[threadIdx.x] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += d_s[r];
    part[H + 1] = s;
  }
}

// One workgroup: column c of partials [blocks][cols] summed over the blocks in order and rounded once.  Columns below vec_n
// go to vec, the last one, times `scale`, to loss, one between them to scalar.
__global__ void s2r_finish_kernel(const double* __restrict__ partials, int blocks, int cols, float* __restrict__ vec, int vec_n,
                                  float* __restrict__ scalar, float* __restrict__ loss, double scale) {
  for (int c = threadIdx.x; c < cols; c += S2R_THREADS) {
    double s = 0.0;
    for (int p = 0; p < blocks; ++p) s += partials[(long)p * cols + c];
    if (c < vec_n) vec[c] = (float)s;
    else if (c == cols - 1) loss[0] = (float)(s * scale);
    else scalar[0] = (float)s;
  }
}

constexpr int CE_GROUP = 32;                      // lanes per row: lane k holds class k
constexpr int CE_ROWS = S2R_THREADS / CE_GROUP;  // rows per workgroup

__device__ __forceinline__ double ce_group_max(double v) {
#pragma unroll
  for (int off = CE_GROUP / 2; off >= 1; off >>= 1) v = fmax(v, shfl_xor_f64(v, off));
  return v;
}
__device__ __forceinline__ double ce_group_sum(double v) {
#pragma unroll
  for (int off = CE_GROUP / 2; off >= 1; off >>= 1) v += shfl_xor_f64(v, off);
  return v;
}

__global__ void s2r_step_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ valid_step, int B, int K,
                                   float* __restrict__ dlogits, float* __restrict__ softmax, double* __restrict__ partials) {
  __shared__ double part[CE_ROWS];
  const int k = threadIdx.x % CE_GROUP, g = threadIdx.x / CE_GROUP;
  const long group_row = (long)blockIdx.x * CE_ROWS + g;
  const bool live = group_row < B;  // a group past the last row repeats it and writes nothing
  const long row = live ? group_row : B - 1;
  const bool mine = k < K;
  const double z = mine ? (double)logits[row * K + k] : -(double)INFINITY;
  const double m = ce_group_max(z);
  const double e = mine ? exp(z - m) : 0.0;
  const double se = ce_group_sum(e);
  const double p = e / se;
  if (live && mine && softmax) softmax[row * K + k] = (float)p;
  if (!valid_step) return;  // (the prediction alone; uniform over the launch)
  const int target = s2r_step(valid_step, row, K);
  if (live && mine) dlogits[row * K + k] = (float)((p - (k == target ? 1.0 : 0.0)) / (double)B);
  const double zt = ce_group_sum(k == target ? z : 0.0);
  if (k == 0) part[g] = live ? m + log(se) - zt : 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int r = 0; r < CE_ROWS; ++r) s += part[r];
    partials[blockIdx.x] = s;
  }
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_lstm_fanout_step(const float* h_prev, const float* c_prev, const float* proj, int table_rows, const float* w_hh,
                        const float* b_hh, int parents, int fanout, int hidden, float* h, float* c, rg_stream_t stream) {
  if (parents < 1 || fanout < 1 || hidden < 1 || table_rows < 0) return RG_EINVAL;
  if (hidden > RG_LSTM_MAX_HIDDEN) return RG_EUNSUPPORTED;
  const int64_t n = (int64_t)parents * fanout;
  if (n >= (1LL << 29)) return RG_EUNSUPPORTED;
  if (!h_prev || !proj || !w_hh || !h || !c) return RG_EINVAL;
  FanoutArgs a;
  a.h_prev = h_prev, a.c_prev = c_prev, a.proj = proj, a.w_hh = w_hh, a.b_hh = b_hh;
  a.h = h, a.c = c, a.N = (long)n, a.fanout = fanout, a.table_rows = table_rows, a.H = hidden, a.Hp = lstm_padded(hidden);
  const size_t lds = lstm_tile_floats(hidden) * sizeof(float);
  RG_ALLOW_LDS(s2r_fanout_kernel, lds);
  RG_LAUNCH_DYN(s2r_fanout_kernel, dim3((unsigned)((n + LSTM_ROWS - 1) / LSTM_ROWS)), dim3(LSTM_THREADS), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_seq2reward_plan_max(const float* h, const float* w, const float* bias, int groups, int group_size, int hidden, float* q,
                           rg_stream_t stream) {
  if (groups < 1 || group_size < 1 || hidden < 1) return RG_EINVAL;
  if ((int64_t)groups * group_size >= (1LL << 29)) return RG_EUNSUPPORTED;
  if (!h || !w || !bias || !q) return RG_EINVAL;
  RG_LAUNCH(s2r_plan_max_kernel, dim3((groups + S2R_WAVES - 1) / S2R_WAVES), dim3(S2R_THREADS), (hipStream_t)stream, h, w,
            bias, (long)groups, group_size, hidden, q);
  return (int)hipGetLastError();
}

int rg_seq2reward_head_partials(int batch) { return batch < 1 ? 0 : (batch + S2R_THREADS - 1) / S2R_THREADS; }

int rg_seq2reward_head(const float* h_all, const int64_t* valid_step, const float* reward, const float* gamma_pow,
                       const float* w, const float* bias, int seq_len, int batch, int hidden, float* acc_reward, float* dh_all,
                       float* dw, float* dbias, double* partials, float* loss, rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || hidden < 1) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29)) return RG_EUNSUPPORTED;
  if (!h_all || !w || !bias || !acc_reward) return RG_EINVAL;
  if (dh_all && (!reward || !gamma_pow || !dw || !dbias || !partials || !loss)) return RG_EINVAL;
  S2rHeadArgs a;
  a.h_all = h_all, a.valid_step = valid_step, a.reward = reward, a.gamma_pow = gamma_pow, a.w = w, a.bias = bias;
  a.T = seq_len, a.B = batch, a.H = hidden, a.acc_reward = acc_reward, a.dh_all = dh_all, a.partials = partials;
  const int blocks = rg_seq2reward_head_partials(batch);
  RG_LAUNCH(s2r_head_kernel, dim3(blocks), dim3(S2R_THREADS), (hipStream_t)stream, a);
  if (dh_all)
    RG_LAUNCH(s2r_finish_kernel, dim3(1), dim3(S2R_THREADS), (hipStream_t)stream, (const double*)partials, blocks, hidden + 2,
              dw, hidden, dbias, loss, 1.0 / (double)batch);
  return (int)hipGetLastError();
}

int rg_step_ce_head_partials(int batch) { return batch < 1 ? 0 : (batch + CE_ROWS - 1) / CE_ROWS; }

int rg_step_ce_head(const float* logits, const int64_t* valid_step, int batch, int classes, float* dlogits, float* softmax,
                    double* partials, float* loss, rg_stream_t stream) {
  if (batch < 1 || classes < 1) return RG_EINVAL;
  if (classes > RG_STEP_CE_MAX_CLASSES) return RG_EUNSUPPORTED;
  if (!logits) return RG_EINVAL;
  if (valid_step ? (!dlogits || !partials || !loss) : !softmax) return RG_EINVAL;
  const int blocks = rg_step_ce_head_partials(batch);
  RG_LAUNCH(s2r_step_ce_kernel, dim3(blocks), dim3(S2R_THREADS), (hipStream_t)stream, logits, valid_step, batch, classes,
            dlogits, softmax, partials);
  if (valid_step)
    RG_LAUNCH(s2r_finish_kernel, dim3(1), dim3(S2R_THREADS), (hipStream_t)stream, (const double*)partials, blocks, 1,
              (float*)nullptr, 0, (float*)nullptr, loss, 1.0 / (double)batch);
  return (int)hipGetLastError();
}

}  // extern "C"
