// rg_lstm_cell.h — the LSTM cell of the recurrent kernels, written once: the tile shape, the accumulator layout of
// v_mfma_f32_32x32x2_f32, the gate products (lstm_gate_products), the gate arithmetic's exp / sigmoid / tanh in double with
// their constants in LDS, the gates and the cell update (lstm_gates, lstm_cell).  lstm_forward_kernel (lstm.hip: a layer
// over a whole sequence), s2r_fanout_kernel (seq2reward.hip: a layer's single step over the children of a prefix tree) and
// cem_rollout_kernel (cem.hip: the planner's layers from a zero state) call the same product function; the first two call
// the same gate and cell functions, so a step has the same bits in either because it is the same code.  The rollout's cell
// is the zero-state special case and stays in cem.hip: with h = c = 0 it never forms the forget gate
// (lstm_gate_products<false> skips its row), adds both biases to the products of W_ih, ((acc + b_ih) + b_hh), and takes
// c = i * g.  lstm_cell with c_{t-1} = 0 is not that: f * 0 + i * g is +0 where i * g is -0, and NaN where the forget
// pre-activation is NaN, which the rollout never computes.  What stays in each kernel is its row addressing and its stores.
#pragma once
#include <rg_platform.h>

namespace rg {

constexpr int LSTM_THREADS = 256;
constexpr int LSTM_WAVES = LSTM_THREADS / 64;
constexpr int LSTM_ROWS = 32;  // batch rows per workgroup: one MFMA tile of rows
constexpr int LSTM_TILE = 32;  // hidden units per accumulator tile

// exp in double with its constants read from LDS.  The library's exp keeps sixteen 64-bit constants, which the compiler hoists
// out of the step loop into scalar registers for the whole kernel: with the kernel's own scalars that is more than a wave has,
// and it spills them.  Read from LDS inside the loop they are vector registers for the length of a tile's epilogue only.
// exp(x) = 2^k * exp(r), k = rint(x / ln 2), r = x - k * ln2_hi - k * ln2_lo (|r| <= 0.347), exp(r) by its series to r^13
// (the next term is under 4e-18).  The argument is clamped to where the result is a finite double.
constexpr int LSTM_EXP_COEFS = 15;
__device__ __forceinline__ void lstm_exp_table(double* c) {  // by one thread, before the workgroup's first barrier
  c[0] = 1.44269504088896338700e+00;  // 1 / ln 2
  c[1] = 6.93147180369123816490e-01;  // ln2_hi: the low 32 bits of the fraction are zero, so k * ln2_hi is exact
  c[2] = 1.90821492927058770002e-10;  // ln2_lo
  double f = 1.0;
  for (int n = 2; n <= 13; ++n) {
    f *= (double)n;
    c[16 - n] = 1.0 / f;  // c[3] = 1 / 13!, ..., c[14] = 1 / 2!
  }
}
__device__ __forceinline__ double lstm_exp(double x, const double* c) {
  x = fmin(fmax(x, -745.0), 709.0);
  const double k = rint(x * c[0]);
  const double r = fma(-k, c[2], fma(-k, c[1], x));
  double p = c[3];
#pragma unroll
  for (int i = 4; i < LSTM_EXP_COEFS; ++i) p = fma(p, r, c[i]);
  return ldexp(fma(p, r * r, r) + 1.0, (int)k);
}
__device__ __forceinline__ double lstm_sigmoid(double x, const double* c) { return 1.0 / (1.0 + lstm_exp(-x, c)); }
// tanh through the same exponential: (1 - e) / (1 + e) with e = exp(-2 |x|), relative error below 2e-14 from |x| = 2^-8 up;
// below it the odd series to x^7, whose next term is under 1e-21 x
__device__ __forceinline__ double lstm_tanh(double x, const double* c) {
  const double ax = fabs(x), x2 = x * x;
  const double e = lstm_exp(-2.0 * ax, c);
  const double big = copysign((1.0 - e) / (1.0 + e), x);
  const double small = x * (1.0 - x2 * (1.0 / 3.0 - x2 * (2.0 / 15.0 - x2 * (17.0 / 315.0))));
  return ax < 0x1p-8 ? small : big;
}
// row of accumulator register r in the 32x32 result tile (column = lane & 31)
__device__ __forceinline__ int lstm_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// registers 4q .. 4q + 3 of an accumulator (rows 8q + 4 * half + 0 .. 3) for a wave-uniform q: selects, not an indexed
// register file
__device__ __forceinline__ f32x4 lstm_acc_quad(const f32x16& v, int q) {
  f32x4 o;
  switch (q) {
    case 0: o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3]; break;
    case 1: o[0] = v[4], o[1] = v[5], o[2] = v[6], o[3] = v[7]; break;
    case 2: o[0] = v[8], o[1] = v[9], o[2] = v[10], o[3] = v[11]; break;
    default: o[0] = v[12], o[1] = v[13], o[2] = v[14], o[3] = v[15]; break;
  }
  return o;
}

// The i, f, g, o products of one 32 x 32 tile: src [32 rows, K] (LDS, pitch) times rows uc, H + uc, 2H + uc, 3H + uc of
// w [4H, K] (global; one row per lane's column), exact fp32 products accumulated in k order.  A masked column (u_ok false, uc
// clamped) and the k past K multiply zeros; Kp is K rounded up to even.  WITH_F = false leaves the forget gate's row unread.
struct LstmGates {
  f32x16 i, f, g, o;
};
template <bool WITH_F = true>
__device__ __forceinline__ LstmGates lstm_gate_products(const float* src, int pitch, const float* w, int H, int K, int Kp,
                                                        int uc, bool u_ok, int col, int half) {
  const float* wi = w + (long)uc * K;
  const float* wf = wi + (long)H * K;
  const float* wg = wf + (long)H * K;
  const float* wo = wg + (long)H * K;
  f32x16 zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero[r] = 0.f;
  LstmGates a = {zero, zero, zero, zero};
#pragma unroll 4
  for (int k = 0; k < Kp; k += 2) {
    const int kk = k + half;  // (< Kp: Kp is even)
    const bool ok = u_ok && kk < K;
    const int kc = kk < K ? kk : 0;
    const float av = src[col * pitch + kk];
    const float bi = wi[kc], bf = WITH_F ? wf[kc] : 0.f, bg = wg[kc], bo = wo[kc];
    a.i = mfma_32x32x2_f32(av, ok ? bi : 0.f, a.i);
    if (WITH_F) a.f = mfma_32x32x2_f32(av, ok ? bf : 0.f, a.f);
    a.g = mfma_32x32x2_f32(av, ok ? bg : 0.f, a.g);
    a.o = mfma_32x32x2_f32(av, ok ? bo : 0.f, a.o);
  }
  return a;
}

// One element's cell in two calls, between which the kernel reads c_{t-1}.  lstm_gates: from the four products p*, the input
// projection xp[g * H] and bias[g], (i, f, o) = sigmoid, g = tanh.  lstm_cell: c = f * c_{t-1} + i * g, h = o * tanh(c) of the
// stored c (the backward takes tanh of the same value).  Two calls because of where the c_{t-1} load lands: read before the
// gates, it is issued and waited for ahead of the four xp loads (one more exposed memory latency per row quad, 1.4 % of
// rg_lstm_forward at 32 workgroups); read between the calls it is in flight with them, as in the kernels before the sharing.
struct LstmCell {
  double gi, gf, gg, go;
  float c, h;
};
__device__ __forceinline__ LstmCell lstm_gates(float pi, float pf, float pg, float po, const float* xp, int H,
                                               const double* bias, const double* ec) {
  LstmCell r;
  r.gi = lstm_sigmoid((double)pi + (double)xp[0] + bias[0], ec);
  r.gf = lstm_sigmoid((double)pf + (double)xp[H] + bias[1], ec);
  r.gg = lstm_tanh((double)pg + (double)xp[2 * H] + bias[2], ec);
  r.go = lstm_sigmoid((double)po + (double)xp[3 * H] + bias[3], ec);
  return r;
}
__device__ __forceinline__ void lstm_cell(LstmCell& r, float cp, const double* ec) {
  r.c = (float)(r.gf * (double)cp + r.gi * r.gg);
  r.h = (float)(r.go * lstm_tanh((double)r.c, ec));
}

static inline int lstm_padded(int H) { return (H + LSTM_TILE - 1) / LSTM_TILE * LSTM_TILE; }
static inline size_t lstm_tile_floats(int H) { return (size_t)LSTM_ROWS * (lstm_padded(H) + 1); }

}  // namespace rg
