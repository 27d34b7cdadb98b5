// seqconv.hip — the conv tower of NGramConvolutionalNetwork (reagent/models/synthetic_reward.py:311-370 over
// reagent/models/convolutional_network.py:34-97) as a one-dimensional valid convolution along time, computed once per absolute
// position instead of once per window, and the window gather behind it.
//
// The reference copies every step into context_size windows ([T * B, 1, n, S + A]) and runs Conv2d -> relu -> MaxPool2d(1) per
// window.  The first conv kernel spans the whole width and the later ones have width 1, so a layer's output at one absolute
// position is the same in every window that holds the position.  Here an activation is fp32 [P, B, C] with rows ordered
// (position, b): tap dh of row m is row m + dh * B, and a layer is an implicit GEMM with M = P_out * B, N = C_out and
// K = kh * C_in over row-shifted reads of ONE activation matrix.  Layer 0 reads state | action in place and predicates the
// reference's zero ngram_padding (`pad` positions on either side); nothing is copied, nothing is materialised per window.
//
// rg_seqconv_forward / rg_seqconv_dgrad: a workgroup (4 waves, 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles) owns a 128-row x
//   128-channel tile.  The K loop runs over (tap, 16-channel slab): the A slab of tap dh is staged from rows m + dh * B (dgrad:
//   m - dh * B, zero outside), the B slab from the weights in torch's Conv2d layout through a (channel stride, tap stride) pair,
//   both k-major in LDS ([16][128 + 4] floats each, 16.5 KB in all, rg_gemm.h's fp32 image); the next slab's global loads are
//   issued before the MFMA block and stored after it (two barriers per slab).  v_mfma_f32_32x32x2_f32: exact fp32 products, every
//   accumulator sees its (tap, channel) pairs in ascending order.  Epilogue: bias + relu (forward); the relu mask of the layer
//   below (dgrad), whose operand takes the relu mask of its own layer on load.
// rg_seqconv_wgrad: dW[co, ci, dh] = sum_m dz[m, co] g[m + dh * B, ci] reduces over rows, and for the fp32 32x32x2 MFMA both
//   operands are then read ALONG CHANNELS — lane l supplies dz[m + l / 32][co0 + l % 32] and g[m + dh * B + l / 32][ci0 + l % 32]
//   — which are coalesced loads of the layout the forward wrote: the operands go from global memory straight into the MFMA's
//   registers, with no LDS, no barrier and no transposed copy of anything.  A workgroup owns (row split, tap, 128 x 128 tile of
//   (co, ci)), a wave 64 x 64 of it; the loads of the next eight rows are in flight during the MFMAs of these.  dbias rides
//   along as dz x 1.  Split partials go to the workspace and a finishing launch adds them in split order: no atomics.
// rg_ngram_window / rg_ngram_window_backward: feat[(t, b), c * H + h] = g[(t + h, b), c] and its reverse (+ relu mask), the
//   (h, c) -> c * H + h transpose made in LDS so that global reads and writes both run along contiguous floats.
//
// No atomics, no scratch; every trip count depends on the shapes alone; two runs give the same bits; every output element is
// written whole; every operand takes a row pitch.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_gemm.h"

namespace rg {

constexpr int SC_MAX_C = RG_SEQCONV_MAX_CHANNELS;
constexpr int SC_MAX_KH = RG_SEQCONV_MAX_CONTEXT;
constexpr int SC_THREADS = 256;
constexpr int SC_WIN_FLOATS = 8192;  // the window kernels' LDS image (32 KB)
constexpr int SC_WIN_PCHUNK = 8;     // positions a window-backward workgroup owns

// An activation matrix that may be virtual: logical row r, column c.  Columns [0, ka) come from a, [ka, cols) from a2 (layer
// 0: state | action); physical row = r - row_off, zero outside [0, n_rows) (the padding positions; dgrad's shifted rows).
// mask (nullable): the relu output of the operand's own layer — the element passes where it is positive.
struct RowSrc {
  const float *a, *a2, *mask;
  long lda, lda2, ldm;
  long row_off, n_rows;
  int ka, cols;
};

__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// four consecutive columns gk .. gk + 3 of physical row prow (the row is known to exist)
__device__ __forceinline__ f32x4 rowsrc_load4(const RowSrc& s, long prow, int gk) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const bool in_a = gk + 4 <= s.ka, in_a2 = gk >= s.ka && gk + 4 <= s.cols;
  const float* p = in_a ? s.a + prow * s.lda + gk : s.a2 + prow * s.lda2 + (gk - s.ka);
  if ((in_a || in_a2) && aligned16(p)) {
    v = *(const f32x4*)p;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = gk + e;
      if (c < s.cols) v[e] = c < s.ka ? s.a[prow * s.lda + c] : s.a2[prow * s.lda2 + (c - s.ka)];
    }
  }
  if (s.mask) {
    const float* m = s.mask + prow * s.ldm + gk;
    if (gk + 4 <= s.cols && aligned16(m)) {
      const f32x4 y = *(const f32x4*)m;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = y[e] > 0.f ? v[e] : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gk + e < s.cols) v[e] = m[e] > 0.f ? v[e] : 0.f;
    }
  }
  return v;
}

typedef TileWide SCTile;
typedef PrecF32::Stage<SCTile::BM, SC_THREADS> SCStageA;
typedef PrecF32::Stage<SCTile::BN, SC_THREADS> SCStageB;

struct ConvArgs {
  RowSrc A;
  const float* w;        // element (n, tap, k) at w[n * w_sn + tap * w_st + k * w_sk]
  long w_sn, w_sk, w_st;
  long tap_step;         // logical A row of output row m and tap dh: m + dh * tap_step  (+B forward, -B dgrad)
  int M, N, Kc, kh;      // rows, output channels, channels reduced per tap, taps
  const float* bias;     // forward: y = relu(acc + bias)
  const float* below;    // dgrad (nullable): relu output of the layer below — dx = acc where it is positive
  long ld_below;
  int relu;
  float* out;
  long ldo;
};

// the A slab of one (tap, channel slab): rows m0 .. m0 + 127 shifted by the tap, 16 channels from c0
__device__ __forceinline__ void sc_load_a(SCStageA& st, const ConvArgs& g, int m0, long shift, int c0, int tid) {
#pragma unroll
  for (int i = 0; i < SCStageA::PER; ++i) {
    const int c = tid + i * SC_THREADS, row = c >> 2, gk = c0 + (c & 3) * 4;
    const long prow = (long)m0 + row + shift - g.A.row_off;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m0 + row < g.M && prow >= 0 && prow < g.A.n_rows && gk < g.Kc) v = rowsrc_load4(g.A, prow, gk);
    st.r[i] = v;
  }
}
// the weight slab: output channels n0 .. n0 + 127 of one tap, 16 reduced channels from c0
__device__ __forceinline__ void sc_load_b(SCStageB& st, const ConvArgs& g, int n0, int tap, int c0, int tid) {
#pragma unroll
  for (int i = 0; i < SCStageB::PER; ++i) {
    const int c = tid + i * SC_THREADS, n = n0 + (c >> 2), gk = c0 + (c & 3) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < g.N && gk < g.Kc) {
      const float* p = g.w + (long)n * g.w_sn + (long)tap * g.w_st + (long)gk * g.w_sk;
      if (g.w_sk == 1 && gk + 4 <= g.Kc && aligned16(p)) {
        v = *(const f32x4*)p;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gk + e < g.Kc) v[e] = p[(long)e * g.w_sk];
      }
    }
    st.r[i] = v;
  }
}

__device__ __forceinline__ void seqconv_gemm(const ConvArgs& g) {
  typedef SCTile C;
  __shared__ __attribute__((aligned(16))) float As[PrecF32::lds_elems<C::BM>()];
  __shared__ __attribute__((aligned(16))) float Bs[PrecF32::lds_elems<C::BN>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / C::WN, wn = wave % C::WN;
  const int tiles_m = (g.M + C::BM - 1) / C::BM, tiles_n = (g.N + C::BN - 1) / C::BN;
  int tile_m, tile_n;
  decode_wg((int)blockIdx.x, tiles_m, tiles_n, tile_m, tile_n);
  const int m0 = tile_m * C::BM, n0 = tile_n * C::BN;

  f32x16 acc[C::TM][C::TN];
  // PrecF32::compute's signature carries the bias row sums; with BIAS_MODE 0 nothing reads them and the compiler drops the array
  f32x16 accb[C::TM];
#pragma unroll
  for (int i = 0; i < C::TM; ++i) {
#pragma unroll
    for (int j = 0; j < C::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[i][r] = 0.f;
  }

  const int slabs = (g.Kc + PrecF32::BK - 1) / PrecF32::BK, iters = g.kh * slabs;
  SCStageA sa;
  SCStageB sb;
  sc_load_a(sa, g, m0, 0, 0, tid);
  sc_load_b(sb, g, n0, 0, 0, tid);
  PrecF32::store_lds<C::BM, SC_THREADS>(sa, As, tid);
  PrecF32::store_lds<C::BN, SC_THREADS>(sb, Bs, tid);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const bool more = it + 1 < iters;
    if (more) {
      const int tap = (it + 1) / slabs, c0 = ((it + 1) - tap * slabs) * PrecF32::BK;
      sc_load_a(sa, g, m0, (long)tap * g.tap_step, c0, tid);
      sc_load_b(sb, g, n0, tap, c0, tid);
    }
    PrecF32::compute<C, 0>(As, Bs, wm * (C::TM * 32), wn * (C::TN * 32), lane, acc, accb, false);
    __syncthreads();
    if (more) {
      PrecF32::store_lds<C::BM, SC_THREADS>(sa, As, tid);
      PrecF32::store_lds<C::BN, SC_THREADS>(sb, Bs, tid);
      __syncthreads();
    }
  }

  const int lr = lane & 31, lh = lane >> 5;
  static_for<0, C::TM>([&](auto tm_c) __attribute__((always_inline)) {
    static_for<0, C::TN>([&](auto tn_c) __attribute__((always_inline)) {
      constexpr int tm = decltype(tm_c)::value, tn = decltype(tn_c)::value;
      const int col = n0 + wn * (C::TN * 32) + tn * 32 + lr;
      if (col < g.N) {
        const float b = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * (C::TM * 32) + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (row < g.M) {
            float o = acc[tm][tn][r] + b;
            if (g.relu) o = o > 0.f ? o : 0.f;
            if (g.below) o = g.below[(long)row * g.ld_below + col] > 0.f ? o : 0.f;
            g.out[(long)row * g.ldo + col] = o;
          }
        }
      }
    });
  });
}

__global__ void RG_LAUNCH_BOUNDS(SC_THREADS, 1) seqconv_forward_kernel(const ConvArgs g) { seqconv_gemm(g); }
__global__ void RG_LAUNCH_BOUNDS(SC_THREADS, 1) seqconv_dgrad_kernel(const ConvArgs g) { seqconv_gemm(g); }

// ---------------------------------------------------------------------------------------------------------------------------------
struct WgradArgs {
  RowSrc G;              // the layer's input; logical row of output row m and tap dh: m + dh * B
  const float* dz;       // [M, Cout]
  long ld_dz;
  int M, Cout, Cin, kh, B;
  int rows_per_split, splits;  // rows_per_split a multiple of SC_WG_ROWS
  float* ws;             // [splits][Cout][kh][Cin]
  float* wsb;            // [splits][Cout]
};
constexpr int SC_WG_STEPS = 4;               // MFMA k steps (two rows each) per register stage
constexpr int SC_WG_ROWS = 2 * SC_WG_STEPS;  // rows per register stage

struct WgradStage {
  float a[SC_WG_STEPS][2], b[SC_WG_STEPS][2];
};

__global__ void RG_LAUNCH_BOUNDS(SC_THREADS, 1) seqconv_wgrad_kernel(const WgradArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wa = wave >> 1, wb = wave & 1, lr = lane & 31, lk = lane >> 5;
  const int tiles_co = (g.Cout + 127) / 128, tiles_ci = (g.Cin + 127) / 128;
  int id = (int)blockIdx.x;
  const int tile_ci = id % tiles_ci;
  id /= tiles_ci;
  const int tile_co = id % tiles_co;
  id /= tiles_co;
  const int dh = id % g.kh, split = id / g.kh;
  const int m_begin = split * g.rows_per_split;
  const int m_end = m_begin + g.rows_per_split < g.M ? m_begin + g.rows_per_split : g.M;

  // this lane's columns: pointers at row 0 and pitches (a column past the end reads nothing)
  const float* pa[2];
  const float* pb[2];
  long ldb[2];
  int co[2], ci[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    co[t] = tile_co * 128 + wa * 64 + t * 32 + lr;
    ci[t] = tile_ci * 128 + wb * 64 + t * 32 + lr;
    pa[t] = co[t] < g.Cout ? g.dz + co[t] : nullptr;
    const bool first = ci[t] < g.G.ka;
    pb[t] = ci[t] < g.Cin ? (first ? g.G.a + ci[t] : g.G.a2 + (ci[t] - g.G.ka)) : nullptr;
    ldb[t] = first ? g.G.lda : g.G.lda2;
  }
  const long shift = (long)dh * g.B - g.G.row_off;
  auto load = [&](WgradStage& s, int m) {
#pragma unroll
    for (int k = 0; k < SC_WG_STEPS; ++k) {
      const int row = m + 2 * k + lk;
      const long prow = (long)row + shift;
      const bool row_ok = row < m_end, g_ok = row_ok && prow >= 0 && prow < g.G.n_rows;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s.a[k][t] = (row_ok && pa[t]) ? pa[t][(long)row * g.ld_dz] : 0.f;
        s.b[k][t] = (g_ok && pb[t]) ? pb[t][prow * ldb[t]] : 0.f;
      }
    }
  };

  f32x16 acc[2][2], accb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[i][r] = 0.f;
  }
  const bool do_bias = tile_ci == 0 && dh == 0 && wb == 0;  // (wave-uniform)

  WgradStage cur, nxt;
  load(cur, m_begin);
  for (int m = m_begin; m < m_end; m += SC_WG_ROWS) {
    load(nxt, m + SC_WG_ROWS);  // (past m_end: zeros, no memory touched)
#pragma unroll
    for (int k = 0; k < SC_WG_STEPS; ++k) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_32x32x2_f32(cur.a[k][i], cur.b[k][j], acc[i][j]);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 2; ++i) accb[i] = mfma_32x32x2_f32(cur.a[k][i], 1.0f, accb[i]);
      }
    }
    cur = nxt;
  }

  float* ws = g.ws + (long)split * g.Cout * g.kh * g.Cin;
  static_for<0, 2>([&](auto i_c) __attribute__((always_inline)) {
    constexpr int i = decltype(i_c)::value;
    static_for<0, 2>([&](auto j_c) __attribute__((always_inline)) {
      constexpr int j = decltype(j_c)::value;
      if (ci[j] < g.Cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = tile_co * 128 + wa * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (o < g.Cout) ws[((long)o * g.kh + dh) * g.Cin + ci[j]] = acc[i][j][r];
        }
      }
    });
    if (do_bias && lr == 0) {  // D[o][0] = sum over rows of dz[., o]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = tile_co * 128 + wa * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (o < g.Cout) g.wsb[(long)split * g.Cout + o] = accb[i][r];
      }
    }
  });
}

struct WgradFinishArgs {
  const float *ws, *wsb;
  int Cout, Cin, kh, splits;
  long w_sn, w_sk, w_st;
  float *dw, *dbias;
};

__global__ void seqconv_wgrad_finish_kernel(const WgradFinishArgs g) {
  const long per = (long)g.Cout * g.kh * g.Cin;
  const long idx = (long)blockIdx.x * SC_THREADS + threadIdx.x;
  if (idx < per) {
    float s = 0.f;
    for (int k = 0; k < g.splits; ++k) s = __fadd_rn(s, g.ws[(long)k * per + idx]);
    const int c = (int)(idx % g.Cin), dh = (int)((idx / g.Cin) % g.kh), o = (int)(idx / ((long)g.Cin * g.kh));
    g.dw[o * g.w_sn + c * g.w_sk + dh * g.w_st] = s;
  } else if (idx < per + g.Cout) {
    const int o = (int)(idx - per);
    float s = 0.f;
    for (int k = 0; k < g.splits; ++k) s = __fadd_rn(s, g.wsb[(long)k * g.Cout + o]);
    g.dbias[o] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct WindowArgs {
  const float* src;   // forward: g [(T + H - 1) * B, C]; backward: dfeat [T * B, C * H]
  const float* mask;  // backward (nullable): g, the relu output whose positive entries pass
  long ld_src, ld_mask, ld_dst;
  int T, B, C, H;
  int rows_per_wg;    // forward: batch rows a workgroup owns
  int chan_per_wg;    // backward: channels a workgroup owns
  float* dst;         // forward: feat [T * B, C * H]; backward: dg [(T + H - 1) * B, C]
};

// a workgroup owns step t and rows_per_wg consecutive batch rows: reads along c, writes along c * H + h
__global__ void RG_LAUNCH_BOUNDS(SC_THREADS, 1) ngram_window_kernel(const WindowArgs a) {
  __shared__ float tile[SC_WIN_FLOATS];
  const int blocks_b = (a.B + a.rows_per_wg - 1) / a.rows_per_wg;
  const int t = (int)blockIdx.x / blocks_b, b0 = ((int)blockIdx.x % blocks_b) * a.rows_per_wg;
  const int R = a.B - b0 < a.rows_per_wg ? a.B - b0 : a.rows_per_wg, W = a.C * a.H;
  for (int x = threadIdx.x; x < R * W; x += SC_THREADS) {
    const int c = x % a.C, h = (x / a.C) % a.H, r = x / W;
    tile[r * W + c * a.H + h] = a.src[((long)(t + h) * a.B + b0 + r) * a.ld_src + c];
  }
  __syncthreads();
  for (int x = threadIdx.x; x < R * W; x += SC_THREADS) {
    const int r = x / W, j = x - r * W;
    a.dst[((long)t * a.B + b0 + r) * a.ld_dst + j] = tile[x];
  }
}

// a workgroup owns batch row b, SC_WIN_PCHUNK positions from p0 and chan_per_wg channels from c0: the dfeat rows of the steps
// p0 - H + 1 .. p0 + 7 (their columns c0 * H .. contiguous) go to LDS, then dg[(p, b), c] = sum_h dfeat[(p - h, b), c * H + h]
// in ascending h over the steps that exist, masked
__global__ void RG_LAUNCH_BOUNDS(SC_THREADS, 1) ngram_window_backward_kernel(const WindowArgs a) {
  __shared__ float tile[SC_WIN_FLOATS];
  const int P = a.T + a.H - 1;
  const int chunks_p = (P + SC_WIN_PCHUNK - 1) / SC_WIN_PCHUNK, chunks_c = (a.C + a.chan_per_wg - 1) / a.chan_per_wg;
  int id = (int)blockIdx.x;
  const int c0 = (id % chunks_c) * a.chan_per_wg;
  id /= chunks_c;
  const int p0 = (id % chunks_p) * SC_WIN_PCHUNK, b = id / chunks_p;
  const int CC = a.C - c0 < a.chan_per_wg ? a.C - c0 : a.chan_per_wg, W = CC * a.H;
  const int t_lo = p0 - (a.H - 1), rows = SC_WIN_PCHUNK + a.H - 1;
  for (int x = threadIdx.x; x < rows * W; x += SC_THREADS) {
    const int r = x / W, j = x - r * W, t = t_lo + r;
    tile[x] = (t >= 0 && t < a.T) ? a.src[((long)t * a.B + b) * a.ld_src + (long)c0 * a.H + j] : 0.f;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < SC_WIN_PCHUNK * CC; x += SC_THREADS) {
    const int q = x / CC, c = x - q * CC, p = p0 + q;
    if (p >= P) continue;
    float s = 0.f;
    for (int h = 0; h < a.H; ++h) {
      const int t = p - h;
      if (t >= 0 && t < a.T) s = __fadd_rn(s, tile[(t - t_lo) * W + c * a.H + h]);
    }
    const long row = (long)p * a.B + b;
    if (a.mask && !(a.mask[row * a.ld_mask + c0 + c] > 0.f)) s = 0.f;
    a.dst[row * a.ld_dst + c0 + c] = s;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int sc_check(int64_t positions, int batch, int kh, int cin, int cout) {
  if (positions < 1 || batch < 1 || kh < 1 || cin < 1 || cout < 1) return RG_EINVAL;
  if (kh > SC_MAX_KH || cin > SC_MAX_C || cout > SC_MAX_C) return RG_EINVAL;
  if (positions * batch >= (1LL << 29)) return RG_EINVAL;
  return RG_OK;
}

static int sc_input(RowSrc& s, const float* x, int64_t ldx, const float* x2, int64_t ldx2, int cols, int cols2, int positions, int pad,
                    int batch) {
  if (!x || cols < 1 || cols2 < 0 || ldx < cols || (cols2 > 0 && (!x2 || ldx2 < cols2))) return RG_EINVAL;
  if (pad < 0 || pad > SC_MAX_KH / 2) return RG_EINVAL;
  s.a = x, s.lda = (long)ldx, s.ka = cols, s.a2 = cols2 > 0 ? x2 : x, s.lda2 = cols2 > 0 ? (long)ldx2 : (long)ldx;
  s.cols = cols + cols2, s.mask = nullptr, s.ldm = 0;
  s.row_off = (long)pad * batch, s.n_rows = (long)positions * batch;
  return RG_OK;
}

static void sc_wgrad_plan(int M, int cout, int cin, int kh, int& rows_per_split, int& splits) {
  const int tiles = ((cout + 127) / 128) * ((cin + 127) / 128) * kh;
  const int want = tiles >= 1024 ? 1 : 1024 / tiles;
  int rows = (M + want - 1) / want;
  rows = rows < 64 ? 64 : rows;
  rows_per_split = (rows + SC_WG_ROWS - 1) / SC_WG_ROWS * SC_WG_ROWS;
  splits = (M + rows_per_split - 1) / rows_per_split;
}

static int win_check(int T, int B, int C, int H) {
  if (T < 1 || B < 1 || C < 1 || H < 1) return RG_EINVAL;
  if (C > SC_MAX_C || H > SC_MAX_KH) return RG_EINVAL;
  if (((int64_t)T + H - 1) * B >= (1LL << 29)) return RG_EINVAL;
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_seqconv_forward(const float* x, int64_t ldx, const float* x2, int64_t ldx2, int cols, int cols2, int positions, int pad,
                       int batch, int kh, const float* w, int64_t w_chan_stride, int64_t w_tap_stride, const float* bias,
                       int out_channels, float* y, int64_t ldy, rg_stream_t stream) {
  ConvArgs g = {};
  int rc = sc_input(g.A, x, ldx, x2, ldx2, cols, cols2, positions, pad, batch);
  if (rc != RG_OK) return rc;
  const int64_t p_out = (int64_t)positions + 2 * pad - kh + 1;
  rc = sc_check(p_out, batch, kh, cols + cols2, out_channels);
  if (rc != RG_OK) return rc;
  if (!w || !bias || !y || ldy < out_channels || w_chan_stride < 1 || w_tap_stride < 1) return RG_EINVAL;
  g.w = w, g.w_sn = (long)kh * (cols + cols2), g.w_sk = (long)w_chan_stride, g.w_st = (long)w_tap_stride;
  g.tap_step = batch, g.M = (int)(p_out * batch), g.N = out_channels, g.Kc = cols + cols2, g.kh = kh;
  g.bias = bias, g.below = nullptr, g.relu = 1, g.out = y, g.ldo = (long)ldy;
  const unsigned grid = (unsigned)(((g.M + SCTile::BM - 1) / SCTile::BM) * ((g.N + SCTile::BN - 1) / SCTile::BN));
  RG_LAUNCH(seqconv_forward_kernel, dim3(grid), dim3(SC_THREADS), (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int rg_seqconv_dgrad(const float* dy, int64_t ld_dy, const float* y, int64_t ldy, int out_positions, int batch, int kh,
                     const float* w, int64_t w_chan_stride, int64_t w_tap_stride, int in_channels, int out_channels,
                     const float* below, int64_t ld_below, float* dx, int64_t ld_dx, rg_stream_t stream) {
  const int rc = sc_check((int64_t)out_positions + kh - 1, batch, kh, in_channels, out_channels);
  if (rc != RG_OK) return rc;
  if (out_positions < 1 || !dy || !w || !dx || ld_dy < out_channels || ld_dx < in_channels) return RG_EINVAL;
  if ((y && ldy < out_channels) || (below && ld_below < in_channels) || w_chan_stride < 1 || w_tap_stride < 1) return RG_EINVAL;
  ConvArgs g = {};
  g.A.a = dy, g.A.a2 = dy, g.A.lda = g.A.lda2 = (long)ld_dy, g.A.ka = g.A.cols = out_channels;
  g.A.mask = y, g.A.ldm = (long)ldy, g.A.row_off = 0, g.A.n_rows = (long)out_positions * batch;
  g.w = w, g.w_sn = (long)w_chan_stride, g.w_sk = (long)kh * in_channels, g.w_st = (long)w_tap_stride;
  g.tap_step = -(long)batch, g.M = (out_positions + kh - 1) * batch, g.N = in_channels, g.Kc = out_channels, g.kh = kh;
  g.bias = nullptr, g.below = below, g.ld_below = (long)ld_below, g.relu = 0, g.out = dx, g.ldo = (long)ld_dx;
  const unsigned grid = (unsigned)(((g.M + SCTile::BM - 1) / SCTile::BM) * ((g.N + SCTile::BN - 1) / SCTile::BN));
  RG_LAUNCH(seqconv_dgrad_kernel, dim3(grid), dim3(SC_THREADS), (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

size_t rg_seqconv_wgrad_workspace_bytes(int out_positions, int batch, int kh, int in_channels, int out_channels) {
  if (sc_check(out_positions, batch, kh, in_channels, out_channels) != RG_OK) return 0;
  int rows, splits;
  sc_wgrad_plan(out_positions * batch, out_channels, in_channels, kh, rows, splits);
  return (size_t)splits * ((size_t)out_channels * kh * in_channels + out_channels) * sizeof(float);
}

int rg_seqconv_wgrad(const float* dz, int64_t ld_dz, const float* x, int64_t ldx, const float* x2, int64_t ldx2, int cols, int cols2,
                     int positions, int pad, int batch, int kh, int out_channels, int64_t w_chan_stride, int64_t w_tap_stride,
                     float* dw, float* dbias, void* workspace, size_t workspace_bytes, rg_stream_t stream) {
  WgradArgs g = {};
  int rc = sc_input(g.G, x, ldx, x2, ldx2, cols, cols2, positions, pad, batch);
  if (rc != RG_OK) return rc;
  const int64_t p_out = (int64_t)positions + 2 * pad - kh + 1;
  const int cin = cols + cols2;
  rc = sc_check(p_out, batch, kh, cin, out_channels);
  if (rc != RG_OK) return rc;
  if (!dz || !dw || !dbias || !workspace || ld_dz < out_channels || w_chan_stride < 1 || w_tap_stride < 1) return RG_EINVAL;
  if (workspace_bytes < rg_seqconv_wgrad_workspace_bytes((int)p_out, batch, kh, cin, out_channels)) return RG_EWORKSPACE;
  g.dz = dz, g.ld_dz = (long)ld_dz, g.M = (int)(p_out * batch), g.Cout = out_channels, g.Cin = cin, g.kh = kh, g.B = batch;
  sc_wgrad_plan(g.M, out_channels, cin, kh, g.rows_per_split, g.splits);
  g.ws = (float*)workspace, g.wsb = g.ws + (size_t)g.splits * out_channels * kh * cin;
  const unsigned grid = (unsigned)(g.splits * kh * ((out_channels + 127) / 128) * ((cin + 127) / 128));
  RG_LAUNCH(seqconv_wgrad_kernel, dim3(grid), dim3(SC_THREADS), (hipStream_t)stream, g);
  WgradFinishArgs f;
  f.ws = g.ws, f.wsb = g.wsb, f.Cout = out_channels, f.Cin = cin, f.kh = kh, f.splits = g.splits;
  f.w_sn = (long)kh * cin, f.w_sk = (long)w_chan_stride, f.w_st = (long)w_tap_stride, f.dw = dw, f.dbias = dbias;
  const long n = (long)out_channels * kh * cin + out_channels;
  RG_LAUNCH(seqconv_wgrad_finish_kernel, dim3((unsigned)((n + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), (hipStream_t)stream,
            f);
  return (int)hipGetLastError();
}

int rg_ngram_window(const float* g, int64_t ldg, int seq_len, int batch, int channels, int height, float* feat, int64_t ld_feat,
                    rg_stream_t stream) {
  const int rc = win_check(seq_len, batch, channels, height);
  if (rc != RG_OK) return rc;
  if (!g || !feat || ldg < channels || ld_feat < (int64_t)channels * height) return RG_EINVAL;
  WindowArgs a = {};
  a.src = g, a.ld_src = (long)ldg, a.dst = feat, a.ld_dst = (long)ld_feat, a.T = seq_len, a.B = batch, a.C = channels, a.H = height;
  int rows = SC_WIN_FLOATS / (channels * height);
  a.rows_per_wg = rows > 16 ? 16 : rows;
  const unsigned grid = (unsigned)seq_len * (unsigned)((batch + a.rows_per_wg - 1) / a.rows_per_wg);
  RG_LAUNCH(ngram_window_kernel, dim3(grid), dim3(SC_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_ngram_window_backward(const float* dfeat, int64_t ld_dfeat, const float* g, int64_t ldg, int seq_len, int batch, int channels,
                             int height, float* dg, int64_t ld_dg, rg_stream_t stream) {
  const int rc = win_check(seq_len, batch, channels, height);
  if (rc != RG_OK) return rc;
  if (!dfeat || !dg || ld_dfeat < (int64_t)channels * height || ld_dg < channels || (g && ldg < channels)) return RG_EINVAL;
  WindowArgs a = {};
  a.src = dfeat, a.ld_src = (long)ld_dfeat, a.mask = g, a.ld_mask = (long)ldg, a.dst = dg, a.ld_dst = (long)ld_dg;
  a.T = seq_len, a.B = batch, a.C = channels, a.H = height;
  const int cc = SC_WIN_FLOATS / ((SC_WIN_PCHUNK + height - 1) * height);
  a.chan_per_wg = cc > channels ? channels : cc;
  const int P = seq_len + height - 1;
  const int64_t grid = (int64_t)batch * ((P + SC_WIN_PCHUNK - 1) / SC_WIN_PCHUNK) * ((channels + a.chan_per_wg - 1) / a.chan_per_wg);
  if (grid >= (1LL << 31)) return RG_EINVAL;
  RG_LAUNCH(ngram_window_backward_kernel, dim3((unsigned)grid), dim3(SC_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
