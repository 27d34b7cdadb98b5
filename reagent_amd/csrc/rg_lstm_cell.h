// rg_lstm_cell.h — what the LSTM kernels of lstm.hip (a layer over a whole sequence) and seq2reward.hip (a layer's single
// step over the children of a prefix tree) share: the tile shape, the gate arithmetic's exp / sigmoid / tanh in double with
// their constants in LDS, and the accumulator layout of v_mfma_f32_32x32x2_f32.  Both files compute a cell from the same
// functions on the same operands in the same order, so a step gives the same bits in either.
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

static inline int lstm_padded(int H) { return (H + LSTM_TILE - 1) / LSTM_TILE * LSTM_TILE; }
static inline size_t lstm_tile_floats(int H) { return (size_t)LSTM_ROWS * (lstm_padded(H) + 1); }

}  // namespace rg
