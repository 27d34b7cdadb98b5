// seq2slate.hip — what sits behind the transformer encoder of the Seq2Slate ranking nets (reagent/models/seq2slate.py,
// reagent/model_utils/seq2slate_utils.py, reagent/training/ranking/seq2slate_trainer.py): the embedding join, the
// Plackett-Luce ("Frechet sort") sequence likelihood with the trainer's importance-sampling REINFORCE loss, and the ranking
// and sampling pass.
//
// Rows of the encoder's matrices are ordered (s, b): row s * B + b of an [N, E] view, N = S * B, as rg_attn_* reads them.
//
// rg_s2s_embed_join: src_embed[(s, b), :] = (sqrt(Es) * state_embed[b] | sqrt(Ec) * cand_embed[(s, b)]) in one launch (encode,
// seq2slate.py:776-796: two Embedders' scalings, repeat, reshape, cat); each element one fp32 multiply by the fp32-rounded root.
// rg_s2s_embed_join_backward: d state_embed[b] = sqrt(Es) * sum_s d src_embed[(s, b), :Es], fp32 adds in ascending s, and
// d cand_embed = sqrt(Ec) * the right-hand slice.
//
// rg_frechet_head: a wave per batch row, a lane per candidate (S <= 64).  score[c] = w . mem[(c, b)] + bias with lanes along the
// columns and a butterfly per candidate; T steps of a soft-max over the candidates not chosen before (maximum subtracted), the
// product of the chosen candidates' probabilities clamped at 1e-40, its log, the importance weight against the logged
// propensity, the clamp of helper.ips_clamp and the loss terms; d loss / d score by
//   g_b * p_b * sum_{t : c remaining at t} (1[c = a_t] - pi_t(c)),
// g_b = d loss / d p_b following autograd through each clamp, and from it d mem (written whole), and per-workgroup partials of
// d w, d bias and the three means, which a second launch adds in workgroup order.  Everything is double on the fp32 inputs and
// each output is rounded once.  No atomics, no scratch; every trip count depends on the shapes alone: two runs give the same
// bits.
//
// rg_frechet_rank: one launch, a wave per row: argsort of the scores (encoder rank) or of the first step's soft-max (Frechet
// greedy), descending, ties to the lower index, with one-hot "probabilities"; or T draws without replacement, each from its
// step's soft-max by inversion of the cumulative sum (double, ascending candidate order) at a Philox4x32-10 uniform keyed by
// the seed with counter (row, step).  The reference draws with torch.multinomial: its law is reproduced, not its stream.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"  // lstm_exp: the exponential with its constants in LDS
#include "rg_philox.h"
#include "rg_reduce.h"  // shfl_xor_f64, wave_sum_f64

namespace rg {

constexpr int S2S_MAX_S = RG_S2S_MAX_SEQ_LEN;
constexpr int S2S_MAX_E = RG_S2S_MAX_EMBED;
static_assert(S2S_MAX_E == 512, "the kernels' instances hold a lane's share of the scorer's weight in 1, 2, 4 or 8 registers");
constexpr int S2S_WAVES = 4;               // rows of a workgroup in flight: a wave each
constexpr int S2S_THREADS = 64 * S2S_WAVES;
constexpr int S2S_MAX_BLOCKS = 512;  // workgroups of the head: rows beyond 4 * 512 share waves (rows_per_wave)
constexpr int S2S_SUMS = 4;          // d bias, loss, unclamped IPS, clamped IPS: the partial columns after d w's E
constexpr int S2S_REDUCE_THREADS = 64;
constexpr int JOIN_THREADS = 256;
constexpr double S2S_MIN_P = 1e-40;  // per_symbol_to_per_seq_probs' clamp (seq2slate_utils.py:152-160)

struct EmbedJoinArgs {
  const float *state, *cand;
  long ld_state, ld_cand, ld_out;
  long n;  // N * E
  int B, Es, Ec;
  float scale_s, scale_c;  // (float)sqrt(Es), (float)sqrt(Ec): Embedder's python double as torch hands it to the fp32 multiply
  float* out;
};

__global__ void s2s_embed_join_kernel(const EmbedJoinArgs a) {
  const long idx = (long)blockIdx.x * JOIN_THREADS + threadIdx.x;
  if (idx >= a.n) return;
  const int E = a.Es + a.Ec;
  const long row = idx / E;
  const int col = (int)(idx - row * E);
  const long b = row % a.B;
  a.out[row * a.ld_out + col] = col < a.Es ? __fmul_rn(a.state[b * a.ld_state + col], a.scale_s)
                                           : __fmul_rn(a.cand[row * a.ld_cand + (col - a.Es)], a.scale_c);
}

struct EmbedJoinBackwardArgs {
  const float* d;
  long ld_d, ld_dstate, ld_dcand;
  long n_cand, n;  // N * Ec; N * Ec + B * Es
  int S, B, Es, Ec;
  float scale_s, scale_c;
  float *dstate, *dcand;
};

__global__ void s2s_embed_join_backward_kernel(const EmbedJoinBackwardArgs a) {
  const long idx = (long)blockIdx.x * JOIN_THREADS + threadIdx.x;
  if (idx >= a.n) return;
  if (idx < a.n_cand) {
    const long row = idx / a.Ec;
    const int col = (int)(idx - row * a.Ec);
    a.dcand[row * a.ld_dcand + col] = __fmul_rn(a.d[row * a.ld_d + a.Es + col], a.scale_c);
    return;
  }
  const long x = idx - a.n_cand;
  const long b = x / a.Es;
  const int col = (int)(x - b * a.Es);
  float s = a.d[b * a.ld_d + col];
  for (int t = 1; t < a.S; ++t) s = __fadd_rn(s, a.d[((long)t * a.B + b) * a.ld_d + col]);
  a.dstate[b * a.ld_dstate + col] = __fmul_rn(s, a.scale_s);
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, shfl_xor_f64(v, off));
  return v;
}

// this lane's share of the scorer's weight: K registers for E <= 64 * K (K = 1, 2, 4, 8: the kernels' instances)
template <int K> __device__ __forceinline__ void s2s_load_w(double (&wr)[K], const float* w, int E, int lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) wr[k] = lane + 64 * k < E ? (double)w[lane + 64 * k] : 0.0;
}

// score[c] = w . mem[(c, b)] + bias for every candidate of batch row b: lane c returns candidate c's (lanes >= S: 0)
template <int K>
__device__ __forceinline__ double s2s_scores(const float* mem, long ld, const double (&wr)[K], double bias, int S, int B, long b,
                                             int E, int lane) {
  double mine = 0.0;
  for (int c = 0; c < S; ++c) {
    const float* row = mem + ((long)c * B + b) * ld;
    const int col = opaque(lane);  // (the column tests are made here, not kept as K lane masks across the kernel)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (col + 64 * k < E) acc = fma(wr[k], (double)row[col + 64 * k], acc);
    acc = wave_sum_f64(acc);
    if (lane == c) mine = acc + bias;
  }
  return mine;
}

// a step's soft-max over the remaining candidates (maximum subtracted): this lane's probability, 0 where not remaining.
// lstm_exp holds its argument at -745, so a remaining candidate more than 745 below the maximum weighs 4.9e-324 where the
// library's exp gives 0: a relative 1e-323 of the sum, which no double sum, no fp32 output and no draw (u has 53 bits) sees.
__device__ __forceinline__ double s2s_step_softmax(double s, bool rem, const double* ec) {
  const double m = wave_max_f64(rem ? s : -(double)INFINITY);
  const double e = rem ? lstm_exp(s - m, ec) : 0.0;
  return e / wave_sum_f64(e);
}

struct FrechetHeadArgs {
  const float *mem, *w, *bias, *logged, *reward, *baseline;
  const int64_t* idx;
  long ld_mem, ld_idx, ld_dscore, ld_dmem;
  int S, T, B, E, rows_per_wave, clamp;
  double clamp_max, inv_b;
  float *log_prob, *p, *impt, *clamped, *dscore, *dmem;
  double* partials;  // [workgroups][E + S2S_SUMS]
};

template <int K> __global__ void RG_LAUNCH_BOUNDS(S2S_THREADS, 1) frechet_head_kernel(const FrechetHeadArgs a) {
  __shared__ double ds[S2S_WAVES][64];                      // a row's d loss / d score, handed from the lanes to the columns
  __shared__ double red[S2S_WAVES][S2S_MAX_E + S2S_SUMS];   // the waves' sums, added in wave order
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = a.S, T = a.T, B = a.B, E = a.E;
  const bool train = a.dscore != nullptr;
  double wr[K], dw[K];
  s2s_load_w<K>(wr, a.w, E, lane);
#pragma unroll
  for (int k = 0; k < K; ++k) dw[k] = 0.0;
  const double bias = (double)a.bias[0];
  double s_db = 0.0, s_loss = 0.0, s_ips = 0.0, s_cips = 0.0;
  for (int r = 0; r < a.rows_per_wave; ++r) {
    const long row = ((long)blockIdx.x * S2S_WAVES + wave) * a.rows_per_wave + r;
    const bool live = row < B;  // (the same in every lane) a wave past the last row repeats it and writes nothing
    const long b = live ? row : B - 1;
    const double s = s2s_scores<K>(a.mem, a.ld_mem, wr, bias, S, B, b, E, lane);
    bool rem = lane < S;
    double acc = 0.0, prod = 1.0;
    for (int t = 0; t < T; ++t) {
      const bool chosen = (int64_t)lane == a.idx[b * a.ld_idx + t] - 2;  // (in int64: a wild index matches no lane)
      const double pi = s2s_step_softmax(s, rem, ec);
      prod *= wave_sum_f64(chosen ? pi : 0.0);  // (one lane holds it, the others add 0)
      if (rem) acc += (chosen ? 1.0 : 0.0) - pi;
      rem = rem && !chosen;
    }
    const bool flows = prod >= S2S_MIN_P;  // clamp(min=1e-40) passes the gradient where the product is at or above it
    const double p = flows ? prod : S2S_MIN_P;
    if (live && lane == 0) {
      a.p[b] = (float)p;
      a.log_prob[b] = (float)log(p);
    }
    if (!a.logged) continue;  // (the same in every lane) log-probabilities alone
    const double lg = (double)a.logged[b], rw = (double)a.reward[b], bl = a.baseline ? (double)a.baseline[b] : 0.0;
    const double impt = p / lg;
    double cl = impt;
    bool pass = true;
    if (a.clamp == RG_IPS_CLAMP_UNIVERSAL) {  // torch.clamp(x, 0, max): gradient where 0 <= x <= max
      cl = fmin(fmax(impt, 0.0), a.clamp_max);
      pass = impt >= 0.0 && impt <= a.clamp_max;
    } else if (a.clamp == RG_IPS_CLAMP_AGGRESSIVE) {  // torch.where(x > max, 0, x): gradient where not x > max
      pass = !(impt > a.clamp_max);
      cl = pass ? impt : 0.0;
    }
    const double adv = rw - bl;
    if (live) {
      s_loss += -cl * adv;
      s_ips += -impt * rw;
      s_cips += -cl * rw;
      if (lane == 0) {
        a.impt[b] = (float)impt;
        a.clamped[b] = (float)cl;
      }
    }
    if (!train) continue;
    const double g = live && flows && pass ? -adv * a.inv_b / lg : 0.0;  // d loss / d p
    const double d = g * p * acc;                                       // (lanes at or beyond S: acc = 0)
    if (live && lane < S) a.dscore[b * a.ld_dscore + lane] = (float)d;
    s_db += wave_sum_f64(d);
    ds[wave][lane] = d;
    wave_lds_sync();
    for (int c = 0; c < S; ++c) {
      const double dc = ds[wave][c];
      const float* mrow = a.mem + ((long)c * B + b) * a.ld_mem;
      float* drow = a.dmem + ((long)c * B + b) * a.ld_dmem;
      const int col = opaque(lane);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = col + 64 * k;
        if (e < E) {
          if (live) drow[e] = (float)(dc * wr[k]);
          dw[k] = fma(dc, (double)mrow[e], dw[k]);
        }
      }
    }
    wave_lds_sync();  // the next row writes ds
  }
  const int col = opaque(lane);  // (tested again, not kept as K lane masks since the weights' load)
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (col + 64 * k < E) red[wave][col + 64 * k] = dw[k];
  if (lane == 0) {
    red[wave][S2S_MAX_E + 0] = s_db;
    red[wave][S2S_MAX_E + 1] = s_loss;
    red[wave][S2S_MAX_E + 2] = s_ips;
    red[wave][S2S_MAX_E + 3] = s_cips;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < E + S2S_SUMS; x += S2S_THREADS) {
    const int col = x < E ? x : S2S_MAX_E + (x - E);
    a.partials[(long)blockIdx.x * (E + S2S_SUMS) + x] = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
  }
}

// column x of the workgroups' partials added in workgroup order: d w [E], d bias, and the three sums divided by the batch
__global__ void frechet_reduce_kernel(const double* __restrict__ partials, int G, int E, double batch, float* dw, float* dbias,
                                      float* sums) {
  const int x = blockIdx.x * S2S_REDUCE_THREADS + threadIdx.x;
  const int cols = E + S2S_SUMS;
  if (x >= cols) return;
  double s = 0.0;
  int r = 0;
  for (; r + 8 <= G; r += 8) {  // eight loads in flight, added in order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[(long)(r + u) * cols + x];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; r < G; ++r) s += partials[(long)r * cols + x];
  if (x < E) {
    if (dw) dw[x] = (float)s;
  } else if (x == E) {
    if (dbias) dbias[0] = (float)s;
  } else if (sums) {
    sums[x - E - 1] = (float)(s / batch);
  }
}

struct FrechetRankArgs {
  const float *scores, *mem, *w, *bias;
  long ld_scores, ld_mem;
  int S, T, B, E, mode;
  uint64_t seed;
  int64_t* idx;
  float *probs, *per_seq;
};

template <int K> __global__ void RG_LAUNCH_BOUNDS(S2S_THREADS, 1) frechet_rank_kernel(const FrechetRankArgs a) {
  __shared__ double key[S2S_WAVES][64];
  __shared__ int order[S2S_WAVES][64];
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * S2S_WAVES + wave;
  const int S = a.S, T = a.T, C = a.S + 2;
  if (row >= a.B) return;  // (a whole wave; the kernel has no workgroup barrier after this)
  double s;
  if (a.scores) {
    s = lane < S ? (double)a.scores[row * a.ld_scores + lane] : 0.0;
  } else {
    double wr[K];
    s2s_load_w<K>(wr, a.w, a.E, lane);
    s = s2s_scores<K>(a.mem, a.ld_mem, wr, (double)a.bias[0], S, a.B, row, a.E, lane);
  }
  float* pr = a.probs + row * T * C;
  int64_t* out = a.idx + row * T;
  if (a.mode != RG_FRECHET_RANK_SAMPLED) {
    // the rank of a candidate = how many come before it: a larger key, or an equal one at a lower index
    const double k = a.mode == RG_FRECHET_RANK_GREEDY ? s2s_step_softmax(s, lane < S, ec) : s;
    key[wave][lane] = k;
    order[wave][lane] = 0;
    wave_lds_sync();
    int rank = 0;
    for (int j = 0; j < S; ++j) {
      const double kj = key[wave][j];
      rank += (kj > k || (kj == k && j < lane)) ? 1 : 0;
    }
    if (lane < S) order[wave][rank] = lane;
    wave_lds_sync();
    for (int t = 0; t < T; ++t) {
      const int o = order[wave][t] + 2;
      for (int col = lane; col < C; col += 64) pr[t * C + col] = col == o ? 1.0f : 0.0f;
      if (lane == 0) out[t] = (int64_t)o;
    }
    if (lane == 0) a.per_seq[row] = 1.0f;
    return;
  }
  bool rem = lane < S;
  double prod = 1.0;
  for (int t = 0; t < T; ++t) {
    const double pi = s2s_step_softmax(s, rem, ec);
    const double cum = wave_inclusive_sum_f64(pi);
    uint32_t rnd[4];
    philox4x32_10(a.seed, (uint64_t)row, (uint64_t)t, rnd);
    const double u = (double)((((uint64_t)rnd[0] << 32) | (uint64_t)rnd[1]) >> 11) * 0x1.0p-53;  // [0, 1)
    const unsigned long long hit = wave_ballot(rem && cum > u), left = wave_ballot(rem);
    // the first remaining candidate whose cumulative sum passes u; where rounding leaves the last sum at or below u, the last
    const int chosen = hit ? __builtin_ctzll(hit) : 63 - __builtin_clzll(left | 1ull);
    if (lane < 2) pr[t * C + lane] = 0.0f;
    if (lane < S) pr[t * C + 2 + lane] = (float)pi;
    prod *= wave_sum_f64(lane == chosen ? pi : 0.0);
    rem = rem && lane != chosen;
    if (lane == 0) out[t] = (int64_t)(chosen + 2);
  }
  if (lane == 0) a.per_seq[row] = (float)(prod >= S2S_MIN_P ? prod : S2S_MIN_P);
}

static int s2s_check(int S, int T, int B, int E) {
  if (S < 1 || T < 1 || B < 1 || E < 1 || T > S) return RG_EINVAL;
  if (S > S2S_MAX_S || E > S2S_MAX_E) return RG_EUNSUPPORTED;
  if ((int64_t)S * B >= (1LL << 29)) return RG_EUNSUPPORTED;
  return RG_OK;
}

// the instance whose K registers per lane cover E columns
#define S2S_LAUNCH_BY_WIDTH(kernel, E, grid, block, stream, args)          \
  do {                                                                      \
    if ((E) <= 64) RG_LAUNCH(kernel<1>, grid, block, stream, args);         \
    else if ((E) <= 128) RG_LAUNCH(kernel<2>, grid, block, stream, args);   \
    else if ((E) <= 256) RG_LAUNCH(kernel<4>, grid, block, stream, args);   \
    else RG_LAUNCH(kernel<8>, grid, block, stream, args);                   \
  } while (0)

static int frechet_head_blocks(int B) {
  const int g = (B + S2S_WAVES - 1) / S2S_WAVES;
  return g > S2S_MAX_BLOCKS ? S2S_MAX_BLOCKS : g;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_s2s_embed_join(const float* state_embed, int64_t ld_state, const float* cand_embed, int64_t ld_cand, int seq_len, int batch,
                      int state_cols, int cand_cols, float* src_embed, int64_t ld_out, rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || state_cols < 1 || cand_cols < 1 || !state_embed || !cand_embed || !src_embed) return RG_EINVAL;
  if (ld_state < state_cols || ld_cand < cand_cols || ld_out < (int64_t)state_cols + cand_cols) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29) || (int64_t)state_cols + cand_cols > S2S_MAX_E) return RG_EUNSUPPORTED;
  EmbedJoinArgs a;
  a.state = state_embed, a.cand = cand_embed, a.ld_state = (long)ld_state, a.ld_cand = (long)ld_cand, a.ld_out = (long)ld_out;
  a.B = batch, a.Es = state_cols, a.Ec = cand_cols, a.n = (long)seq_len * batch * (state_cols + cand_cols);
  a.scale_s = (float)sqrt((double)state_cols), a.scale_c = (float)sqrt((double)cand_cols), a.out = src_embed;
  RG_LAUNCH(s2s_embed_join_kernel, dim3((unsigned)((a.n + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS),
            (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_s2s_embed_join_backward(const float* d_src_embed, int64_t ld_d, int seq_len, int batch, int state_cols, int cand_cols,
                               float* d_state_embed, int64_t ld_dstate, float* d_cand_embed, int64_t ld_dcand,
                               rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || state_cols < 1 || cand_cols < 1 || !d_src_embed || !d_state_embed || !d_cand_embed)
    return RG_EINVAL;
  if (ld_d < (int64_t)state_cols + cand_cols || ld_dstate < state_cols || ld_dcand < cand_cols) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29) || (int64_t)state_cols + cand_cols > S2S_MAX_E) return RG_EUNSUPPORTED;
  EmbedJoinBackwardArgs a;
  a.d = d_src_embed, a.ld_d = (long)ld_d, a.ld_dstate = (long)ld_dstate, a.ld_dcand = (long)ld_dcand;
  a.S = seq_len, a.B = batch, a.Es = state_cols, a.Ec = cand_cols;
  a.n_cand = (long)seq_len * batch * cand_cols, a.n = a.n_cand + (long)batch * state_cols;
  a.scale_s = (float)sqrt((double)state_cols), a.scale_c = (float)sqrt((double)cand_cols);
  a.dstate = d_state_embed, a.dcand = d_cand_embed;
  RG_LAUNCH(s2s_embed_join_backward_kernel, dim3((unsigned)((a.n + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS),
            (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

size_t rg_frechet_head_workspace(int batch, int embed) {
  if (batch < 1 || embed < 1 || embed > S2S_MAX_E) return 0;
  return (size_t)frechet_head_blocks(batch) * (embed + S2S_SUMS);
}

int rg_frechet_head(const float* mem, int64_t ld_mem, const float* w, const float* bias, const int64_t* tgt_out_idx,
                    int64_t ld_idx, const float* logged, const float* reward, const float* baseline, int clamp_method,
                    double clamp_max, int seq_len, int tgt_len, int batch, int embed, float* log_prob, float* p, float* impt,
                    float* clamped, float* sums, float* dscore, int64_t ld_dscore, float* dmem, int64_t ld_dmem, float* dw,
                    float* dbias, double* workspace, rg_stream_t stream) {
  const int rc = s2s_check(seq_len, tgt_len, batch, embed);
  if (rc != RG_OK) return rc;
  if (!mem || !w || !bias || !tgt_out_idx || !log_prob || !p || !workspace) return RG_EINVAL;
  if (ld_mem < embed || ld_idx < tgt_len) return RG_EINVAL;
  if (clamp_method != RG_IPS_CLAMP_NONE && clamp_method != RG_IPS_CLAMP_UNIVERSAL && clamp_method != RG_IPS_CLAMP_AGGRESSIVE)
    return RG_EINVAL;
  const bool train = dscore || dmem || dw || dbias;
  if (train && (!dscore || !dmem || !dw || !dbias || ld_dscore < seq_len || ld_dmem < embed)) return RG_EINVAL;
  if (logged ? (!reward || !impt || !clamped || !sums) : (reward || baseline || impt || clamped || sums || train)) return RG_EINVAL;
  FrechetHeadArgs a;
  a.mem = mem, a.w = w, a.bias = bias, a.logged = logged, a.reward = reward, a.baseline = baseline, a.idx = tgt_out_idx;
  a.ld_mem = (long)ld_mem, a.ld_idx = (long)ld_idx, a.ld_dscore = (long)ld_dscore, a.ld_dmem = (long)ld_dmem;
  a.S = seq_len, a.T = tgt_len, a.B = batch, a.E = embed, a.clamp = clamp_method, a.clamp_max = clamp_max;
  a.inv_b = 1.0 / (double)batch;
  const int blocks = frechet_head_blocks(batch);
  a.rows_per_wave = (batch + blocks * S2S_WAVES - 1) / (blocks * S2S_WAVES);
  a.log_prob = log_prob, a.p = p, a.impt = impt, a.clamped = clamped, a.dscore = dscore, a.dmem = dmem, a.partials = workspace;
  S2S_LAUNCH_BY_WIDTH(frechet_head_kernel, embed, dim3(blocks), dim3(S2S_THREADS), (hipStream_t)stream, a);
  if (logged) {
    const int cols = embed + S2S_SUMS;
    RG_LAUNCH(frechet_reduce_kernel, dim3((cols + S2S_REDUCE_THREADS - 1) / S2S_REDUCE_THREADS), dim3(S2S_REDUCE_THREADS),
              (hipStream_t)stream, (const double*)workspace, blocks, embed, (double)batch, dw, dbias, sums);
  }
  return (int)hipGetLastError();
}

int rg_frechet_rank(const float* scores, int64_t ld_scores, const float* mem, int64_t ld_mem, const float* w, const float* bias,
                    int mode, uint64_t seed, int seq_len, int tgt_len, int batch, int embed, int64_t* ranked_tgt_out_idx,
                    float* ranked_per_symbol_probs, float* ranked_per_seq_probs, rg_stream_t stream) {
  const int rc = s2s_check(seq_len, tgt_len, batch, scores ? 1 : embed);
  if (rc != RG_OK) return rc;
  if (!ranked_tgt_out_idx || !ranked_per_symbol_probs || !ranked_per_seq_probs) return RG_EINVAL;
  if (scores ? ld_scores < seq_len : (!mem || !w || !bias || ld_mem < embed)) return RG_EINVAL;
  if (mode != RG_FRECHET_RANK_ENCODER && mode != RG_FRECHET_RANK_GREEDY && mode != RG_FRECHET_RANK_SAMPLED) return RG_EINVAL;
  FrechetRankArgs a;
  a.scores = scores, a.mem = mem, a.w = w, a.bias = bias, a.ld_scores = (long)ld_scores, a.ld_mem = (long)ld_mem;
  a.S = seq_len, a.T = tgt_len, a.B = batch, a.E = embed, a.mode = mode, a.seed = seed;
  a.idx = ranked_tgt_out_idx, a.probs = ranked_per_symbol_probs, a.per_seq = ranked_per_seq_probs;
  S2S_LAUNCH_BY_WIDTH(frechet_rank_kernel, scores ? 1 : embed, dim3((unsigned)((batch + S2S_WAVES - 1) / S2S_WAVES)),
                      dim3(S2S_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
