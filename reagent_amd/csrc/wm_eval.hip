// wm_eval.hip — the world-model evaluators' kernels (reagent/evaluation/world_model_evaluator.py): the feature-importance
// sweep as ONE widened batch of virtual rows, and the feature-sensitivity reduction.  The reference ablates one feature at a
// time: it clones the [T, B, .] input, overwrites a column block with its replacement value and runs a whole get_loss, F + 1
// times.  Here a variant v is (start, end, fill) and row (v, b) is derived from row b: layer 0 reads the SHARED base
// projection xproj[t, b] = x W_ih^T + b_ih and adds the block's correction sum_c (fill_c - x[t, b, c]) W_ih[., c], a product
// end - start wide, so neither an ablated input nor an ablated projection is ever written; the layers above and gmm_linear
// are the existing launches over T * V * B rows; the losses read the unreplicated targets.
//
//   wm_feature_fill_kernel   the replacement value of every block: a column's mean, or the reference's one-hot rule
//   lstm_ablate_kernel       layer 0 over V x B virtual rows, all T steps: rg_lstm_forward's tile and arithmetic
//   wm_mdn_losses_kernel     the three loss sums of every variant (rg_mdn_head's row, no dz), wm_losses_finish_kernel
//   wm_sensitivity_kernel    sum |mus_shuffled - mus| per state-feature block, wm_sensitivity_finish_kernel
//
// No atomics anywhere: sums leave as per-workgroup partials in double and a finishing launch adds them in a fixed order and
// rounds once, so two runs give the same bits.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"  // the tile shape, lstm_gate_products / lstm_gates / lstm_cell, lstm_acc_row / lstm_acc_quad
#include "rg_mdn_row.h"    // MdnRow, mdn_row
#include "rg_reduce.h"     // lds_tree_sum

namespace rg {

constexpr int WM_THREADS = 256;

__device__ __forceinline__ int wm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the replacement values ----------------------------------------------------------------------------------------
// One workgroup per block.  Column c's sum over the N rows: thread i adds rows i, i + 256, ... in double, then a fixed LDS
// tree.  A block one column wide gets fp32(sum / N).  A wider block is a one-hot enum (compute_median_feature_value,
// world_model_evaluator.py:159-173): the sums rounded to fp32 (exact for counts below 2^24), their lower median (what
// torch.median returns: the element of rank (w - 1) / 2), 1 at the first column whose sum equals it and 0 at the others; with
// a NaN among the sums torch.median is NaN, nothing equals it and the reference's loop ends on the last column: so here.
__global__ void wm_feature_fill_kernel(const float* __restrict__ x, long ldx, int N, int W, const int* __restrict__ blocks,
                                       float* __restrict__ fill) {
  __shared__ double vals[WM_THREADS];
  __shared__ float sums[RG_WM_MAX_BLOCK];
  int s = blocks[2 * blockIdx.x], e = blocks[2 * blockIdx.x + 1];
  s = wm_clamp(s, 0, W), e = wm_clamp(e, s, wm_clamp(s + RG_WM_MAX_BLOCK, s, W));  // (the host has refused what this would change)
  const int w = e - s;
  for (int j = 0; j < w; ++j) {
    double a = 0.0;
    for (long r = threadIdx.x; r < N; r += WM_THREADS) a += (double)x[r * ldx + s + j];
    vals[threadIdx.x] = a;
    lds_tree_sum<WM_THREADS>(vals);
    if (threadIdx.x == 0) {
      if (w == 1) fill[s] = (float)(vals[0] / (double)N);
      sums[j] = (float)vals[0];
    }
    __syncthreads();
  }
  if (w < 2) return;
  for (int j = threadIdx.x; j < w; j += WM_THREADS) {
    const float v = sums[j];
    int below = 0, upto = 0, nan = 0;
    for (int i = 0; i < w; ++i) below += sums[i] < v, upto += sums[i] <= v, nan += sums[i] != sums[i];
    const int k = (w - 1) / 2;
    bool first = below <= k && k < upto && nan == 0;  // v is the lower median
    for (int i = 0; i < j && first; ++i) first = sums[i] != v;
    if (nan) first = j == w - 1;
    fill[s + j] = first ? 1.f : 0.f;
  }
}

// ---- layer 0 over the virtual rows -----------------------------------------------------------------------------------
struct LstmAblateArgs {
  const float *xproj, *x, *w_ih, *w_hh, *b_hh, *fill;
  const int* blocks;  // [V][2]: start, end
  long ldx, fill_stride;
  float *h_all, *c_all;
  int T, B, H, Hp, In, V, Wp;  // Wp: the launch's widest block rounded up to even (the pitch of the delta image, less one)
};

// rg_lstm_forward's step for the tile's 32 batch rows of variant blockIdx.y, with one more product in front of the gates: per
// step the tile's deltas fill_c - x[t, row, c] (32 x width, zeros past the width and past the batch) are staged in LDS (pitch
// Wp + 1: the A fragment's 32 rows on 32 banks) and multiplied with columns start .. end of rows g H + u of W_ih, read as
// lstm_gate_products reads w_hh (a row per lane's column, k along the row), on the same exact-product fp32 MFMA chain in k
// order: ONE path for every width (a block one column wide costs one MFMA per gate and step next to the recurrence's Hp / 2,
// so a second path of plain FMAs would buy nothing and could differ).  The correction enters the pre-activation in double
// next to b_hh: pre = (h W_hh^T + xproj) + (b_hh + delta W_ih^T).  A zero delta gives an accumulator of +0 (it starts at +0
// and adds +-0 products), b_hh + 0 is b_hh or +0 for -0, and the product accumulator (which also starts at +0) plus xproj is
// never -0: the sum is then rg_lstm_forward's, bit for bit.  Trip counts depend on H and the block's width alone, a row's bits
// on that row and its variant alone.
__global__ void RG_LAUNCH_BOUNDS(LSTM_THREADS, 1) lstm_ablate_kernel(const LstmAblateArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  const int H = a.H, Hp = a.Hp, B = a.B, In = a.In, pitch = Hp + 1, tiles = Hp / LSTM_TILE, dpitch = a.Wp + 1;
  float* cur = (float*)smem;
  float* nxt = cur + LSTM_ROWS * pitch;
  float* dl = nxt + LSTM_ROWS * pitch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * LSTM_ROWS;
  const int v = blockIdx.y;
  int s = a.blocks[2 * v], e = a.blocks[2 * v + 1];
  s = wm_clamp(s, 0, In), e = wm_clamp(e, s, wm_clamp(s + a.Wp, s, In));  // (the host has refused what this would change)
  const int w = e - s, wp = (w + 1) & ~1;
  // (bases of the per-step staging and of the bias reads held per lane: as scalars they, with the kernel's other scalars, are
  // more than a wave has; the vector file has room)
  const float* fill = a.fill + (long)v * a.fill_stride + opaque(s);
  const float* xs = a.x + opaque(s);
  const float* b_hh = a.b_hh ? a.b_hh + opaque(0) : nullptr;
  const long vstep = (long)a.V * B * H;  // elements of one step of h_all / c_all
  for (int i = threadIdx.x; i < LSTM_ROWS * Hp; i += LSTM_THREADS) {
    const int r = i / Hp, u = i % Hp;
    cur[r * pitch + u] = 0.f;  // (the sweep starts every variant from the zero state)
  }
  for (int t = 0; t < a.T; ++t) {
    for (int i = threadIdx.x; i < LSTM_ROWS * wp; i += LSTM_THREADS) {
      const int r = i / wp, j = i % wp;
      const long row = row0 + r;
      dl[r * dpitch + j] = (row < B && j < w) ? fill[j] - xs[((long)t * B + row) * a.ldx + j] : 0.f;
    }
    __syncthreads();  // (the first turn's also publishes the zero image; the turn's last barrier guards dl against the next turn)
    for (int tile = wave; tile < tiles; tile += LSTM_WAVES) {
      const int u = tile * LSTM_TILE + col;
      const bool u_ok = u < H;
      const int uc = u_ok ? u : H - 1;
      f32x16 zero;
#pragma unroll
      for (int r = 0; r < 16; ++r) zero[r] = 0.f;
      LstmGates d = {zero, zero, zero, zero};
      {
        const float* wi = a.w_ih + (long)uc * In + s;
        const float* wf = wi + (long)H * In;
        const float* wg = wf + (long)H * In;
        const float* wo = wg + (long)H * In;
        for (int k = 0; k < wp; k += 2) {
          const int kk = k + half;  // (< wp: wp is even)
          const bool ok = u_ok && kk < w;
          const int kc = kk < w ? kk : 0;
          const float av = dl[col * dpitch + kk];
          const float bi = wi[kc], bf = wf[kc], bg = wg[kc], bo = wo[kc];
          d.i = mfma_32x32x2_f32(av, ok ? bi : 0.f, d.i);
          d.f = mfma_32x32x2_f32(av, ok ? bf : 0.f, d.f);
          d.g = mfma_32x32x2_f32(av, ok ? bg : 0.f, d.g);
          d.o = mfma_32x32x2_f32(av, ok ? bo : 0.f, d.o);
        }
      }
      const LstmGates p = lstm_gate_products(cur, pitch, a.w_hh, H, H, Hp, uc, u_ok, col, half);
      double bias[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) bias[g] = b_hh ? (double)b_hh[g * H + uc] : 0.0;
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        const f32x4 qi = lstm_acc_quad(p.i, q), qf = lstm_acc_quad(p.f, q), qg = lstm_acc_quad(p.g, q), qo = lstm_acc_quad(p.o, q);
        const f32x4 di = lstm_acc_quad(d.i, q), df = lstm_acc_quad(d.f, q), dg = lstm_acc_quad(d.g, q), dq = lstm_acc_quad(d.o, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rl = lstm_acc_row(4 * q + j, half);
          const long row = row0 + rl;
          const bool ok = u_ok && row < B;
          const long rowc = row < B ? row : B - 1;  // (addresses stay inside the arrays; the values are dropped)
          const long at = (((long)t * a.V + v) * B + rowc) * H + uc;
          const float* xp = a.xproj + ((long)t * B + rowc) * 4 * H + uc;
          const double bd[4] = {bias[0] + (double)di[j], bias[1] + (double)df[j], bias[2] + (double)dg[j],
                                bias[3] + (double)dq[j]};
          LstmCell c = lstm_gates(qi[j], qf[j], qg[j], qo[j], xp, H, bd, ec);
          const float cp = t == 0 ? 0.f : a.c_all[at - vstep];
          lstm_cell(c, cp, ec);
          if (ok) {
            a.h_all[at] = c.h;
            a.c_all[at] = c.c;
          }
          nxt[rl * pitch + u] = ok ? c.h : 0.f;
        }
      }
    }
    __syncthreads();
    float* sw = cur;
    cur = nxt, nxt = sw;
  }
}

// ---- the losses of every variant -------------------------------------------------------------------------------------
struct WmLossArgs {
  const float* z;
  long ldz;
  const float *next_state, *reward, *not_terminal;
  int T, B, V, G, S, first_row;
  double* partials;  // [V][workgroups][3]: the sums of the rows' -log p, BCE and squared error
};

// mdn_head_kernel's row and sums without dz: a wave per row n = t B + b of variant blockIdx.y, whose z row is (t V + v) B + b
// and whose targets are row n of the unreplicated arrays.  The rows of a workgroup and the order of its sum are the head's.
__global__ void wm_mdn_losses_kernel(const WmLossArgs a) {
  __shared__ double part[MDN_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long N = (long)a.T * a.B;
  const long wave_row = (long)blockIdx.x * MDN_WAVES + wave;
  const bool live = wave_row < N;  // a wave past the last row repeats it and counts nothing
  const long row = live ? wave_row : N - 1;
  const bool counts = live && row >= a.first_row;
  const int G = a.G, S = a.S, stride = G * S, v = blockIdx.y;
  const float* zp = a.z + (((row / a.B) * a.V + v) * a.B + row % a.B) * a.ldz;
  const MdnRow r = mdn_row<true>(a.next_state + row * S, zp, zp + stride, zp + 2 * stride, G, S, lane);
  const double rz = zp[2 * stride + G], nz = zp[2 * stride + G + 1];
  const double dr = rz - (double)a.reward[row], y = a.not_terminal[row];
  const double bce = fmax(nz, 0.0) - nz * y + log1p(exp(-fabs(nz)));
  if (lane == 0) {
    part[wave][0] = counts ? -r.logp : 0.0;
    part[wave][1] = counts ? bce : 0.0;
    part[wave][2] = counts ? dr * dr : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    a.partials[((long)v * gridDim.x + blockIdx.x) * 3 + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
  }
}

// mdn_finish_kernel per variant: a workgroup adds its variant's partials (thread i adds i, i + 256, ..., then the LDS tree)
__global__ void wm_losses_finish_kernel(const double* __restrict__ partials, int blocks, double scale_gmm, double scale_bce,
                                        double scale_mse, double gmm_in_loss, float* __restrict__ losses) {
  __shared__ double vals[MDN_THREADS];
  const double* mine = partials + (long)blockIdx.x * blocks * 3;
  double total[3];
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int p = threadIdx.x; p < blocks; p += MDN_THREADS) s += mine[(long)p * 3 + k];
    vals[threadIdx.x] = s;
    lds_tree_sum<MDN_THREADS>(vals);
    total[k] = vals[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double gmm = total[0] * scale_gmm, bce = total[1] * scale_bce, mse = total[2] * scale_mse;
    float* out = losses + 4 * (long)blockIdx.x;
    out[0] = (float)gmm, out[1] = (float)bce, out[2] = (float)mse;
    out[3] = (float)(gmm * gmm_in_loss + bce + mse);
  }
}

// ---- the sensitivity reduction -----------------------------------------------------------------------------------------
// Workgroup (p, f): thread i owns row p * 256 + i and adds |z1 - z0| over the G components' columns start .. end of block f (g,
// then c) in double; the LDS tree gives the workgroup's partial.  The rows' cache lines are shared by the neighbouring blocks'
// workgroups, so each z is fetched from memory once.
__global__ void wm_sensitivity_kernel(const float* __restrict__ z0, const float* __restrict__ z1, long ldz, int N, int G, int S,
                                      const int* __restrict__ blocks, double* __restrict__ partials) {
  __shared__ double vals[WM_THREADS];
  const int f = blockIdx.y;
  int s = blocks[2 * f], e = blocks[2 * f + 1];
  s = wm_clamp(s, 0, S), e = wm_clamp(e, s, S);
  const long row = (long)blockIdx.x * WM_THREADS + threadIdx.x;
  double acc = 0.0;
  if (row < N)
    for (int g = 0; g < G; ++g)
      for (int c = s; c < e; ++c) acc += fabs((double)z1[row * ldz + g * S + c] - (double)z0[row * ldz + g * S + c]);
  vals[threadIdx.x] = acc;
  lds_tree_sum<WM_THREADS>(vals);
  if (threadIdx.x == 0) partials[(long)f * gridDim.x + blockIdx.x] = vals[0];
}

__global__ void wm_sensitivity_finish_kernel(const double* __restrict__ partials, int blocks, double scale,
                                             float* __restrict__ out) {
  __shared__ double vals[WM_THREADS];
  double s = 0.0;
  for (int p = threadIdx.x; p < blocks; p += WM_THREADS) s += partials[(long)blockIdx.x * blocks + p];
  vals[threadIdx.x] = s;
  lds_tree_sum<WM_THREADS>(vals);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(vals[0] * scale);
}

static int wm_rows_check(int seq_len, int batch, int variants) {
  if (seq_len < 1 || batch < 1 || variants < 1) return RG_EINVAL;
  if (variants > 65535) return RG_EUNSUPPORTED;  // (a grid's second dimension)
  if ((int64_t)seq_len * batch * variants > 0x7fffffffLL / 4) return RG_EUNSUPPORTED;  // the rows go through rg_fc_* as an int
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_wm_feature_fill(const float* x, int64_t ldx, int n, int width, const int32_t* blocks, int num_blocks, float* fill,
                       rg_stream_t stream) {
  if (n < 1 || width < 1 || num_blocks < 1 || !x || !blocks || !fill || ldx < width) return RG_EINVAL;
  if (num_blocks > 0x7fffffff / 2) return RG_EUNSUPPORTED;
  RG_LAUNCH(wm_feature_fill_kernel, dim3(num_blocks), dim3(WM_THREADS), (hipStream_t)stream, x, (long)ldx, n, width,
            (const int*)blocks, fill);
  return (int)hipGetLastError();
}

int rg_lstm_forward_ablate(const float* xproj, const float* x, int64_t ldx, const float* w_ih, const float* w_hh,
                           const float* b_hh, const int32_t* blocks, const float* fill,
                           int64_t fill_stride, int max_width, int seq_len, int batch, int hidden, int input_width, int variants,
                           float* h_all, float* c_all, rg_stream_t stream) {
  const int rc = wm_rows_check(seq_len, batch, variants);
  if (rc != RG_OK) return rc;
  if (hidden < 1 || input_width < 1 || max_width < 0 || fill_stride < 0 || ldx < input_width) return RG_EINVAL;
  if (!xproj || !x || !w_ih || !w_hh || !blocks || !fill || !h_all || !c_all) return RG_EINVAL;
  if (hidden > RG_LSTM_MAX_HIDDEN || max_width > RG_WM_MAX_BLOCK) return RG_EUNSUPPORTED;
  LstmAblateArgs a;
  a.xproj = xproj, a.x = x, a.w_ih = w_ih, a.w_hh = w_hh, a.b_hh = b_hh, a.fill = fill;
  a.blocks = (const int*)blocks, a.ldx = (long)ldx, a.fill_stride = (long)fill_stride;
  a.h_all = h_all, a.c_all = c_all;
  a.T = seq_len, a.B = batch, a.H = hidden, a.Hp = lstm_padded(hidden), a.In = input_width, a.V = variants;
  a.Wp = (max_width + 1) & ~1;
  const size_t lds = (2 * lstm_tile_floats(hidden) + (size_t)LSTM_ROWS * (a.Wp + 1)) * sizeof(float);
  RG_ALLOW_LDS(lstm_ablate_kernel, lds);
  RG_LAUNCH_DYN(lstm_ablate_kernel, dim3((batch + LSTM_ROWS - 1) / LSTM_ROWS, variants), dim3(LSTM_THREADS), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_wm_mdn_losses_partials(int seq_len, int batch, int variants) {
  if (seq_len < 1 || batch < 1 || variants < 1) return 0;
  const int64_t per = ((int64_t)seq_len * batch + MDN_WAVES - 1) / MDN_WAVES;
  return per * variants > 0x7fffffffLL / 3 ? 0 : (int)(per * variants);
}

int rg_wm_mdn_losses(const float* z, int64_t ldz, const float* next_state, const float* reward, const float* not_terminal,
                     double next_state_loss_weight, double not_terminal_loss_weight, double reward_loss_weight,
                     int divide_by_state_dim, int first_row, int seq_len, int batch, int variants, int num_gaussians,
                     int state_dim, double* partials, float* losses, rg_stream_t stream) {
  const int rc = wm_rows_check(seq_len, batch, variants);
  if (rc != RG_OK) return rc;
  if (num_gaussians < 1 || state_dim < 1) return RG_EINVAL;
  if (num_gaussians > RG_MDN_MAX_GAUSSIANS || state_dim > RG_MDN_MAX_STATE_DIM) return RG_EUNSUPPORTED;
  const int n = seq_len * batch;
  if (!z || !next_state || !reward || !not_terminal || !partials || !losses) return RG_EINVAL;
  if (ldz < (2 * (int64_t)state_dim + 1) * num_gaussians + 2 || first_row < 0 || first_row >= n) return RG_EINVAL;
  const double rows = (double)(n - first_row);
  const double in_loss = divide_by_state_dim ? 1.0 / (double)(state_dim + 2) : 1.0;
  WmLossArgs a;
  a.z = z, a.ldz = (long)ldz, a.next_state = next_state, a.reward = reward, a.not_terminal = not_terminal;
  a.T = seq_len, a.B = batch, a.V = variants, a.G = num_gaussians, a.S = state_dim, a.first_row = first_row;
  a.partials = partials;
  const int blocks = (n + MDN_WAVES - 1) / MDN_WAVES;
  RG_LAUNCH(wm_mdn_losses_kernel, dim3(blocks, variants), dim3(MDN_THREADS), (hipStream_t)stream, a);
  RG_LAUNCH(wm_losses_finish_kernel, dim3(variants), dim3(MDN_THREADS), (hipStream_t)stream, (const double*)partials, blocks,
            next_state_loss_weight / rows, not_terminal_loss_weight / rows, reward_loss_weight / rows, in_loss, losses);
  return (int)hipGetLastError();
}

int rg_wm_mus_sensitivity_partials(int n, int num_blocks) {
  if (n < 1 || num_blocks < 1) return 0;
  const int64_t per = ((int64_t)n + WM_THREADS - 1) / WM_THREADS;
  return per * num_blocks > 0x7fffffffLL ? 0 : (int)(per * num_blocks);
}

int rg_wm_mus_sensitivity(const float* z, const float* z_shuffled, int64_t ldz, int n, int num_gaussians, int state_dim,
                          const int32_t* blocks, int num_blocks, double* partials, float* sensitivity, rg_stream_t stream) {
  if (n < 1 || num_gaussians < 1 || state_dim < 1 || num_blocks < 1) return RG_EINVAL;
  if (!z || !z_shuffled || !blocks || !partials || !sensitivity || ldz < (int64_t)num_gaussians * state_dim) return RG_EINVAL;
  if (num_blocks > 65535 || rg_wm_mus_sensitivity_partials(n, num_blocks) == 0) return RG_EUNSUPPORTED;
  const int per = (n + WM_THREADS - 1) / WM_THREADS;
  RG_LAUNCH(wm_sensitivity_kernel, dim3(per, num_blocks), dim3(WM_THREADS), (hipStream_t)stream, z, z_shuffled, (long)ldz, n,
            num_gaussians, state_dim, (const int*)blocks, partials);
  RG_LAUNCH(wm_sensitivity_finish_kernel, dim3(num_blocks), dim3(WM_THREADS), (hipStream_t)stream, (const double*)partials,
            per, 1.0 / ((double)n * num_gaussians), sensitivity);
  return (int)hipGetLastError();
}

}  // extern "C"
