// attention.hip — multi-head self-attention over short sequences, forward and backward, and the residual joins of the
// transformer reward net (reagent/models/synthetic_reward.py:46-174: PETransformerEncoderLayer around nn.MultiheadAttention).
//
// Rows are ordered (t, b): row t * B + b of an [N, E] view, N = T * B; head h owns columns h * hd .. (h + 1) * hd.
//
// rg_attn_forward: ctx = softmax(q k^T / sqrt(hd)) v per (b, head) pair, no mask.  A wave owns a pair entirely: it reads the
// pair's T rows of q, k and v once, in contiguous chunks of hd floats, into its own slice of LDS (k with an odd pitch, so that a
// lane per key reads its row without bank conflicts) and nothing is added across waves.  T <= 64, so a score row fits a wave with
// a lane per key; with kpad = the power of two at or above T, 64 / kpad queries share a wave instruction (at T = 10 four
// queries: 40 of 64 lanes busy where a query per instruction keeps 10), and the row maximum and the row sum are butterflies
// inside the kpad lanes of a query.  The dot products, the soft-max (maximum subtracted, lstm_exp) and p v are double on the
// fp32 inputs; p and ctx are rounded once.  The p v products run with lanes along the head's columns and p broadcast from LDS.
//
// rg_attn_backward: dv = p^T dctx, dp = dctx v^T, ds = p * (dp - rowsum(dp * p)), dq = ds k / sqrt(hd), dk = ds^T q / sqrt(hd),
// again a wave per pair: dctx, v and p in LDS for dv and ds (ds kept whole, in double), then k and q over the same two
// buffers for dq and dk.  The problems are T x T with T <= 64 and the work is bound by the rows read: no MFMA.
//
// No atomics, no scratch; every trip count depends on the shapes alone; two runs give the same bits.
//
// rg_residual_join: out = act((a + b) + pe[row / B]) on strided [N, E] views in one launch (b, pe nullable; act linear or
// relu): x + pe, relu(x + block(x)) and the pre-norm sums.  rg_residual_join_backward: dx = (((g0 + g1) + g2) + g3) where the
// saved output is positive (out nullable: no mask; g1 .. g3 nullable).  Every element is fp32 adds in that order.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"  // lstm_exp
#include "rg_reduce.h"     // shfl_xor_f64

namespace rg {

constexpr int ATTN_MAX_T = RG_ATTN_MAX_SEQ_LEN;
constexpr int ATTN_MAX_HD = RG_ATTN_MAX_HEAD_DIM;
constexpr int ATTN_MAX_E = RG_ATTN_MAX_EMBED;
constexpr int ATTN_MAX_WAVES = 4;       // pairs of a workgroup: a wave each
constexpr int ATTN_LDS_SHARED = 65536;  // bytes of LDS the waves of a workgroup share before the workgroup shrinks
constexpr int JOIN_THREADS = 256;

struct AttnArgs {
  const float *q, *k, *v, *p_in, *dctx;
  long ldq, ldk, ldv, ld_ctx, ld_dq, ld_dk, ld_dv;
  int T, B, hd, nhead, kpad, pk;  // kpad: the power of two at or above T; pk: k's (and, backward, v's) odd LDS pitch
  int pairs, wave_floats;         // B * nhead; floats of LDS per wave (even)
  double scale;                   // 1 / sqrt(hd)
  float *ctx, *p, *dq, *dk, *dv;
};

static inline int attn_kpad(int T) {
  int k = 1;
  while (k < T) k <<= 1;
  return k;
}
static inline int attn_forward_wave_floats(int T, int hd) { return (128 + 2 * T * hd + T * (hd | 1) + 1) & ~1; }
static inline int attn_backward_wave_floats(int T, int hd) {
  return (2 * T * attn_kpad(T) + T * hd + T * (hd | 1) + T * T + 1) & ~1;
}
static inline int attn_waves(int wave_floats) {
  const int w = ATTN_LDS_SHARED / (wave_floats * 4);
  return w < 1 ? 1 : (w > ATTN_MAX_WAVES ? ATTN_MAX_WAVES : w);
}

// the pair's T rows of one operand, columns h * hd .. + hd, into LDS with the given pitch: lanes along the columns
__device__ __forceinline__ void attn_load_rows(float* dst, int pitch, const float* src, long ld, int T, int B, long b, int col0,
                                               int hd, int lane) {
  for (int t = 0; t < T; ++t) {
    const float* row = src + ((long)t * B + b) * ld + col0;
    for (int d = lane; d < hd; d += 64) dst[t * pitch + d] = row[d];
  }
}

// out[r, d] = scale * sum_c coef[r * cr + c * cc] * rows[c * hd + d] for r, c < T, rounded once: lanes along d
__device__ __forceinline__ void attn_mix_rows(const double* coef, int cr, int cc, const float* rows, double scale, float* out,
                                              long ld, int T, int B, long b, int col0, int hd, int lane) {
  for (int r = 0; r < T; ++r) {
    float* dst = out + ((long)r * B + b) * ld + col0;
    for (int d = lane; d < hd; d += 64) {
      double acc = 0.0;
      for (int c = 0; c < T; ++c) acc = fma(coef[r * cr + c * cc], (double)rows[c * hd + d], acc);
      dst[d] = (float)(acc * scale);
    }
  }
}

__global__ void attn_forward_kernel(const AttnArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  const int T = a.T, B = a.B, hd = a.hd, kpad = a.kpad, pk = a.pk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long pair = (long)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = pair < a.pairs;
  const long b = pair / a.nhead;
  const int col0 = (int)(pair - b * a.nhead) * hd;
  double* prow = (double*)((float*)smem + (long)wave * a.wave_floats);  // [64 / kpad queries][kpad keys] of a round
  float* Q = (float*)(prow + 64);
  float* V = Q + T * hd;
  float* K = V + T * hd;
  if (live) {
    attn_load_rows(Q, hd, a.q, a.ldq, T, B, b, col0, hd, lane);
    attn_load_rows(V, hd, a.v, a.ldv, T, B, b, col0, hd, lane);
    attn_load_rows(K, pk, a.k, a.ldk, T, B, b, col0, hd, lane);
  }
  __syncthreads();  // ec, and the wave's own rows
  if (!live) return;
  const int per_round = 64 / kpad, g = lane / kpad, j = lane - g * kpad;
  const bool key_ok = j < T;
  const float* kr = K + (key_ok ? j : 0) * pk;
  for (int r0 = 0; r0 < T; r0 += per_round) {
    const int i = r0 + g;
    const bool ok = key_ok && i < T;
    const float* qr = Q + (i < T ? i : 0) * hd;
    double s = 0.0;
    for (int d = 0; d < hd; ++d) s = fma((double)qr[d], (double)kr[d], s);
    s *= a.scale;
    double m = key_ok ? s : -INFINITY;
    for (int off = kpad >> 1; off >= 1; off >>= 1) m = fmax(m, shfl_xor_f64(m, off));
    const double e = key_ok ? lstm_exp(s - m, ec) : 0.0;
    double sum = e;
    for (int off = kpad >> 1; off >= 1; off >>= 1) sum += shfl_xor_f64(sum, off);
    const double pj = e / sum;
    prow[lane] = pj;
    if (a.p && ok) a.p[(pair * T + i) * T + j] = (float)pj;
    wave_lds_sync();
    const int rows = T - r0 < per_round ? T - r0 : per_round;
    for (int gg = 0; gg < rows; ++gg) {
      float* dst = a.ctx + ((long)(r0 + gg) * B + b) * a.ld_ctx + col0;
      const double* pr = prow + gg * kpad;
      for (int d = lane; d < hd; d += 64) {
        double acc = 0.0;
        for (int c = 0; c < T; ++c) acc = fma(pr[c], (double)V[c * hd + d], acc);
        dst[d] = (float)acc;
      }
    }
    wave_lds_sync();  // the next round writes prow
  }
}

__global__ void attn_backward_kernel(const AttnArgs a) {
  RG_DYN_LDS(smem);
  const int T = a.T, B = a.B, hd = a.hd, kpad = a.kpad, pk = a.pk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long pair = (long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (pair >= a.pairs) return;  // (a whole wave; the kernel has no workgroup barrier)
  const long b = pair / a.nhead;
  const int col0 = (int)(pair - b * a.nhead) * hd;
  double* dS = (double*)((float*)smem + (long)wave * a.wave_floats);  // [T][kpad]
  float* A = (float*)(dS + T * kpad);                                  // dctx, then k: [T][hd]
  float* Bf = A + T * hd;                                              // v [T][pk], then q [T][hd]
  float* P = Bf + T * pk;                                              // [T][T]
  attn_load_rows(A, hd, a.dctx, a.ld_ctx, T, B, b, col0, hd, lane);
  attn_load_rows(Bf, pk, a.v, a.ldv, T, B, b, col0, hd, lane);
  for (int x = lane; x < T * T; x += 64) P[x] = a.p_in[pair * T * T + x];
  wave_lds_sync();
  // dv[j] = sum_i p[i, j] dctx[i]
  for (int c = 0; c < T; ++c) {
    float* dst = a.dv + ((long)c * B + b) * a.ld_dv + col0;
    for (int d = lane; d < hd; d += 64) {
      double acc = 0.0;
      for (int i = 0; i < T; ++i) acc = fma((double)P[i * T + c], (double)A[i * hd + d], acc);
      dst[d] = (float)acc;
    }
  }
  // ds, 64 / kpad queries a round, a lane per key
  const int per_round = 64 / kpad, g = lane / kpad, j = lane - g * kpad;
  const bool key_ok = j < T;
  const float* vr = Bf + (key_ok ? j : 0) * pk;
  for (int r0 = 0; r0 < T; r0 += per_round) {
    const int i = r0 + g;
    const bool ok = key_ok && i < T;
    const float* gr = A + (i < T ? i : 0) * hd;
    double dp = 0.0;
    for (int d = 0; d < hd; ++d) dp = fma((double)gr[d], (double)vr[d], dp);
    const double pij = ok ? (double)P[i * T + j] : 0.0;
    double rs = ok ? dp * pij : 0.0;
    for (int off = kpad >> 1; off >= 1; off >>= 1) rs += shfl_xor_f64(rs, off);
    if (i < T) dS[i * kpad + j] = ok ? pij * (dp - rs) : 0.0;
  }
  wave_lds_sync();  // dS written; dctx and v read for the last time
  attn_load_rows(A, hd, a.k, a.ldk, T, B, b, col0, hd, lane);
  attn_load_rows(Bf, hd, a.q, a.ldq, T, B, b, col0, hd, lane);
  wave_lds_sync();
  attn_mix_rows(dS, kpad, 1, A, a.scale, a.dq, a.ld_dq, T, B, b, col0, hd, lane);   // dq[i] = sum_j ds[i, j] k[j]
  attn_mix_rows(dS, 1, kpad, Bf, a.scale, a.dk, a.ld_dk, T, B, b, col0, hd, lane);  // dk[j] = sum_i ds[i, j] q[i]
}

struct JoinArgs {
  const float *a, *b, *pe;
  long lda, ldb, ld_pe, ldo;
  long n;  // N * E
  int E, B, act;
  float* out;
};

__global__ void residual_join_kernel(const JoinArgs j) {
  const long idx = (long)blockIdx.x * JOIN_THREADS + threadIdx.x;
  if (idx >= j.n) return;
  const long row = idx / j.E;
  const int col = (int)(idx - row * j.E);
  float s = j.a[row * j.lda + col];
  if (j.b) s = __fadd_rn(s, j.b[row * j.ldb + col]);
  if (j.pe) s = __fadd_rn(s, j.pe[(row / j.B) * j.ld_pe + col]);
  if (j.act == RG_ACT_RELU) s = s < 0.0f ? 0.0f : s;  // (a NaN stays a NaN)
  j.out[row * j.ldo + col] = s;
}

struct JoinBackwardArgs {
  const float* out;
  const float* g[4];
  long ldo, ldg[4], ld_dx;
  long n;
  int E;
  float* dx;
};

__global__ void residual_join_backward_kernel(const JoinBackwardArgs j) {
  const long idx = (long)blockIdx.x * JOIN_THREADS + threadIdx.x;
  if (idx >= j.n) return;
  const long row = idx / j.E;
  const int col = (int)(idx - row * j.E);
  float s = j.g[0][row * j.ldg[0] + col];
  if (j.g[1]) s = __fadd_rn(s, j.g[1][row * j.ldg[1] + col]);
  if (j.g[2]) s = __fadd_rn(s, j.g[2][row * j.ldg[2] + col]);
  if (j.g[3]) s = __fadd_rn(s, j.g[3][row * j.ldg[3] + col]);
  if (j.out && j.out[row * j.ldo + col] <= 0.0f) s = 0.0f;  // relu through its output (threshold_backward)
  j.dx[row * j.ld_dx + col] = s;
}

static int attn_check(int T, int B, int E, int nhead) {
  if (T < 1 || B < 1 || E < 1 || nhead < 1) return RG_EINVAL;
  if (E % nhead != 0) return RG_EINVAL;
  if (T > ATTN_MAX_T || E > ATTN_MAX_E || E / nhead > ATTN_MAX_HD) return RG_EUNSUPPORTED;
  if ((int64_t)T * B >= (1LL << 29) || (int64_t)B * nhead >= (1LL << 29)) return RG_EUNSUPPORTED;
  return RG_OK;
}

static void attn_shape(AttnArgs& a, int T, int B, int E, int nhead, int wave_floats) {
  a.T = T, a.B = B, a.nhead = nhead, a.hd = E / nhead, a.kpad = attn_kpad(T), a.pk = a.hd | 1;
  a.pairs = B * nhead, a.wave_floats = wave_floats, a.scale = 1.0 / sqrt((double)a.hd);
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_attn_forward(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int seq_len, int batch,
                    int embed, int nhead, float* ctx, int64_t ld_ctx, float* p, rg_stream_t stream) {
  const int rc = attn_check(seq_len, batch, embed, nhead);
  if (rc != RG_OK) return rc;
  if (!q || !k || !v || !ctx) return RG_EINVAL;
  if (ldq < embed || ldk < embed || ldv < embed || ld_ctx < embed) return RG_EINVAL;
  AttnArgs a = {};
  attn_shape(a, seq_len, batch, embed, nhead, attn_forward_wave_floats(seq_len, embed / nhead));
  a.q = q, a.k = k, a.v = v, a.ldq = (long)ldq, a.ldk = (long)ldk, a.ldv = (long)ldv;
  a.ctx = ctx, a.ld_ctx = (long)ld_ctx, a.p = p;
  const int waves = attn_waves(a.wave_floats);
  const size_t lds = (size_t)waves * a.wave_floats * 4;
  if (lds > ATTN_LDS_SHARED) RG_ALLOW_LDS(attn_forward_kernel, lds);
  RG_LAUNCH_DYN(attn_forward_kernel, dim3((unsigned)((a.pairs + waves - 1) / waves)), dim3(64 * waves), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_attn_backward(const float* dctx, int64_t ld_dctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                     int64_t ldv, const float* p, int seq_len, int batch, int embed, int nhead, float* dq, int64_t ld_dq,
                     float* dk, int64_t ld_dk, float* dv, int64_t ld_dv, rg_stream_t stream) {
  const int rc = attn_check(seq_len, batch, embed, nhead);
  if (rc != RG_OK) return rc;
  if (!dctx || !q || !k || !v || !p || !dq || !dk || !dv) return RG_EINVAL;
  if (ld_dctx < embed || ldq < embed || ldk < embed || ldv < embed) return RG_EINVAL;
  if (ld_dq < embed || ld_dk < embed || ld_dv < embed) return RG_EINVAL;
  AttnArgs a = {};
  attn_shape(a, seq_len, batch, embed, nhead, attn_backward_wave_floats(seq_len, embed / nhead));
  a.dctx = dctx, a.ld_ctx = (long)ld_dctx, a.q = q, a.k = k, a.v = v, a.ldq = (long)ldq, a.ldk = (long)ldk, a.ldv = (long)ldv;
  a.p_in = p, a.dq = dq, a.dk = dk, a.dv = dv, a.ld_dq = (long)ld_dq, a.ld_dk = (long)ld_dk, a.ld_dv = (long)ld_dv;
  const int waves = attn_waves(a.wave_floats);
  const size_t lds = (size_t)waves * a.wave_floats * 4;
  if (lds > ATTN_LDS_SHARED) RG_ALLOW_LDS(attn_backward_kernel, lds);
  RG_LAUNCH_DYN(attn_backward_kernel, dim3((unsigned)((a.pairs + waves - 1) / waves)), dim3(64 * waves), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_residual_join(const float* a, int64_t lda, const float* b, int64_t ldb, const float* pe, int64_t ld_pe, int seq_len,
                     int batch, int cols, int act, float* out, int64_t ldo, rg_stream_t stream) {
  if (seq_len < 1 || batch < 1 || cols < 1 || !a || !out) return RG_EINVAL;
  if (act != RG_ACT_LINEAR && act != RG_ACT_RELU) return RG_EINVAL;
  if (lda < cols || ldo < cols || (b && ldb < cols) || (pe && ld_pe < cols)) return RG_EINVAL;
  if ((int64_t)seq_len * batch >= (1LL << 29)) return RG_EUNSUPPORTED;
  JoinArgs j;
  j.a = a, j.b = b, j.pe = pe, j.lda = (long)lda, j.ldb = (long)ldb, j.ld_pe = (long)ld_pe, j.ldo = (long)ldo;
  j.n = (long)seq_len * batch * cols, j.E = cols, j.B = batch, j.act = act, j.out = out;
  RG_LAUNCH(residual_join_kernel, dim3((unsigned)((j.n + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS),
            (hipStream_t)stream, j);
  return (int)hipGetLastError();
}

int rg_residual_join_backward(const float* out, int64_t ldo, const float* g0, int64_t ld0, const float* g1, int64_t ld1,
                              const float* g2, int64_t ld2, const float* g3, int64_t ld3, int64_t rows, int cols, float* dx,
                              int64_t ld_dx, rg_stream_t stream) {
  if (rows < 1 || cols < 1 || !g0 || !dx) return RG_EINVAL;
  if (ld0 < cols || ld_dx < cols || (out && ldo < cols) || (g1 && ld1 < cols) || (g2 && ld2 < cols) || (g3 && ld3 < cols))
    return RG_EINVAL;
  if (rows >= (1LL << 29)) return RG_EUNSUPPORTED;
  JoinBackwardArgs j;
  j.out = out, j.ldo = (long)ldo, j.g[0] = g0, j.g[1] = g1, j.g[2] = g2, j.g[3] = g3;
  j.ldg[0] = (long)ld0, j.ldg[1] = (long)ld1, j.ldg[2] = (long)ld2, j.ldg[3] = (long)ld3;
  j.ld_dx = (long)ld_dx, j.n = (long)rows * cols, j.E = cols, j.dx = dx;
  RG_LAUNCH(residual_join_backward_kernel, dim3((unsigned)((j.n + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS),
            (hipStream_t)stream, j);
  return (int)hipGetLastError();
}

}  // extern "C"
