// cb_deep.hip — what the deep-represent LinUCB model adds to the step path: the ridge solve of LinearRegressionUCB on
// device-resident state (fold the epoch's averages, regularise, invert, coefficients: one launch of one workgroup, the
// matrix in registers) and the loss head behind the MLP (ones column, mean through linear_layer or the coefficients, output
// activation, weighted mse / mae / binary cross-entropy, the gradients into the MLP's output and linear_layer.weight).
// No atomics: partials leave per workgroup and a finishing launch adds them in a fixed order, so two runs give the same
// bits.  The launch constants are rg_cb.h's, the fp64 wave sum and the LDS tree rg_reduce.h's.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_cb.h"      // CB_THREADS, CB_WAVES: the bandit kernels' launch shape
#include "rg_gemm.h"    // act_apply / act_grad_from_output: the FC epilogues' activation functions
#include "rg_reduce.h"  // wave_sum_f64, lds_tree_sum

// The fold is held to the reference's fp32 operation order: every multiply, divide and add is rounded on its own.  Where a
// fused multiply-add is wanted (the elimination, the dots) it is written out as fmaf.
#pragma clang fp contract(off)

namespace rg {

// ---- rg_linucb_solve ----------------------------------------------------------------------------------------------------
constexpr int SOLVE_SIDE = 16;                                     // the workgroup is a 16 x 16 grid of threads
constexpr int SOLVE_PER = RG_LINUCB_SOLVE_MAX_DIM / SOLVE_SIDE;    // each holds 8 x 8 entries: (ty + 16 a, tx + 16 b)
static_assert(SOLVE_SIDE * SOLVE_SIDE == CB_THREADS && SOLVE_PER * SOLVE_SIDE == RG_LINUCB_SOLVE_MAX_DIM, "solve layout");

struct SolveArgs {
  int d;
  float lambda;
  float *avg_A, *avg_b, *sum_weight;
  int64_t* num_obs;
  float *cur_avg_A, *cur_avg_b, *cur_sum_weight;
  int64_t* cur_num_obs;
  float *inv_avg_A, *coefs, *valid;
  int32_t* status;
};

// One workgroup.  Thread (ty, tx) = (t >> 4, t & 15) owns the entries (ty + 16 a, tx + 16 b), a, b < NB, of the matrix in
// registers m[a][b]; NB = 1, 2, 4 or 8 is the least of them with 16 NB >= d, and entries outside d x d are those of the
// identity, which the d steps never touch.  Step k = 16 ka + kr of the in-place Gauss-Jordan inversion: the threads with
// ty == kr publish row k (their m[ka][.]), those with tx == kr column k (their m[.][ka]) — ka is a compile-time index of
// the unrolled outer loop, so no register array is indexed at run time — into one of two LDS buffers, ONE barrier, then
// every thread updates its NB x NB entries from NB row and NB column values:
//     m[i][j] -= m[i][k] * (m[k][j] / p)   (i, j != k);   row k: m[k][j] / p;   column k: -m[i][k] / p;   m[k][k] = 1 / p.
// The buffers alternate: a thread writes buffer k & 1 again at step k + 2, which it reaches only through the barrier of
// step k + 1, behind which every thread has finished reading step k's values.  The trip counts depend on d alone: a
// non-positive or non-finite pivot p raises the flag and the arithmetic goes on (infinities and NaNs, no loop on data).
template <int NB>
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_solve_kernel(const SolveArgs a) {
  __shared__ float rowk[2][RG_LINUCB_SOLVE_MAX_DIM], colk[2][RG_LINUCB_SOLVE_MAX_DIM];
  __shared__ float bvec[RG_LINUCB_SOLVE_MAX_DIM];
  const int t = threadIdx.x, tx = t & (SOLVE_SIDE - 1), ty = t >> 4;
  const int d = a.d;
  // reduce_avg (:54-89), one process: total = cur_sum_weight + sum_weight, the new sum_weight the same sum
  const float sw = *a.sum_weight, cw = *a.cur_sum_weight;
  const float total = cw + sw;
  const float reg = (a.lambda * 1.f) / total;  // l2_reg_lambda * eye / sum_weight on the diagonal
  float m[NB][NB];
#pragma unroll
  for (int ia = 0; ia < NB; ++ia) {
    sched_fence();  // a row of the share at a time: all NB x NB bounds compares hoisted together would not fit the SGPRs
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) {
      const int i = ty + SOLVE_SIDE * ia, j = tx + SOLVE_SIDE * jb;
      float v = i == j ? 1.f : 0.f;
      if (i < d && j < d) {
        const long e = (long)i * d + j;
        const float avg = (a.avg_A[e] * sw + a.cur_avg_A[e] * cw) / total;
        a.avg_A[e] = avg;
        a.valid[e] = avg;
        a.cur_avg_A[e] = 0.f;
        v = i == j ? avg + reg : avg;
      }
      m[ia][jb] = v;
    }
  }
  if (t < d) {
    const float b = (a.avg_b[t] * sw + a.cur_avg_b[t] * cw) / total;
    a.avg_b[t] = b;
    a.cur_avg_b[t] = 0.f;
    bvec[t] = b;
  }
  int bad = 0;
#pragma unroll
  for (int ka = 0; ka < NB; ++ka) {
    const int steps = d - SOLVE_SIDE * ka < SOLVE_SIDE ? d - SOLVE_SIDE * ka : SOLVE_SIDE;
    for (int kr = 0; kr < steps; ++kr) {  // (steps <= 0 past the last block of d: uniform)
      const int k = SOLVE_SIDE * ka + kr, buf = k & 1;
      if (ty == kr) {
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
          rowk[buf][tx + SOLVE_SIDE * jb] = m[ka][jb];
      }
      if (tx == kr) {
#pragma unroll
        for (int ia = 0; ia < NB; ++ia)
          colk[buf][ty + SOLVE_SIDE * ia] = m[ia][ka];
      }
      __syncthreads();
      const float p = rowk[buf][k];
      if (!(p > 0.f && p <= 3.4028234663852886e38f)) bad = 1;
      const float ip = 1.f / p;
      float r[NB], c[NB];
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        r[q] = rowk[buf][tx + SOLVE_SIDE * q] * ip;
        c[q] = colk[buf][ty + SOLVE_SIDE * q];
      }
      const bool row_mine = ty == kr, col_mine = tx == kr;
#pragma unroll
      for (int ia = 0; ia < NB; ++ia) {
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          float v = fmaf(-c[ia], r[jb], m[ia][jb]);
          const bool in_row = ia == ka && row_mine, in_col = jb == ka && col_mine;
          if (in_col) v = -c[ia] * ip;
          if (in_row) v = in_col ? ip : r[jb];
          m[ia][jb] = v;
        }
      }
    }
  }
  __syncthreads();  // bvec, and every read of sum_weight / cur_sum_weight lies before thread 0 rewrites them
  // (the bounds are compared afresh on a value the optimiser cannot equate with d: kept from the prologue, their 2 NB masks
  // would stay in SGPRs across the whole elimination and spill)
  const int de = opaque(d);
  // inv_avg_A, and coefs = inv_avg_A * avg_b: a thread's share of row i over its NB columns, then the 16 threads of the row
  // (consecutive lanes) by butterflies
#pragma unroll
  for (int ia = 0; ia < NB; ++ia) {
    sched_fence();
    const int i = ty + SOLVE_SIDE * ia;
    float part = 0.f;
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) {
      const int j = tx + SOLVE_SIDE * jb;
      if (i < de && j < de) {
        a.inv_avg_A[(long)i * d + j] = m[ia][jb];
        part = fmaf(m[ia][jb], bvec[j], part);
      }
    }
    part += shfl_xor(part, 1);
    part += shfl_xor(part, 2);
    part += shfl_xor(part, 4);
    part += shfl_xor(part, 8);
    if (tx == 0 && i < de) a.coefs[i] = part;
  }
  if (t == 0) {
    *a.sum_weight = total;
    *a.cur_sum_weight = 0.f;
    *a.num_obs += *a.cur_num_obs;
    *a.cur_num_obs = 0;
    if (bad) *a.status = 1;
  }
}

// ---- rg_drlinucb_head ---------------------------------------------------------------------------------------------------
constexpr int DRH_MIN_BLOCK_ROWS = 64;  // a workgroup takes at least this many rows (fewer, larger dv partials)

struct DrHeadArgs {
  const float* mlp;
  long ld;
  const float *v, *label, *weight;
  int act, loss, B, h, block_rows;
  float inv_B;
  float *z, *lin, *pred, *row_loss, *dmlp;
  long ld_dmlp;
  float *loss_partials, *dv_partials;
};

// A group of G lanes per row, 256 / G rows a pass, block_rows rows a workgroup.  Lane g of the group walks the columns
// g, g + G, ... of mlp_out (coalesced), copies them behind the ones column of z and adds up its share of z . v; the
// group's sum by butterflies is the same bits in each of its lanes.  Every lane then forms the row's prediction, loss and
// d loss / d lin and writes its columns of d loss / d mlp_out = dlin * v[1:].  dlin of the workgroup's rows meets in LDS:
// thread c owns column c of the dv partial and adds dlin_r * z_r[c] over the rows in order (z_r[c] read from mlp_out).
template <int G>
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) drlinucb_head_kernel(const DrHeadArgs a) {
  __shared__ float sdlin[CB_THREADS];
  __shared__ double scratch[CB_WAVES];
  constexpr int ROWS = CB_THREADS / G;
  const int g = threadIdx.x & (G - 1), rl = threadIdx.x / G;
  const int h = a.h, d = h + 1;
  const long row0 = (long)blockIdx.x * a.block_rows;
  const bool train = a.label != nullptr;
  double loss_acc = 0.0;
  for (int r0 = 0; r0 < a.block_rows; r0 += ROWS) {  // (block_rows is a multiple of ROWS: a uniform trip count)
    const long r = row0 + r0 + rl;
    const bool live = r < a.B;  // a group past the last row repeats it and writes nothing
    const long row = live ? r : a.B - 1;
    const float* xp = a.mlp + row * a.ld;
    float* zp = a.z + row * d;
    float acc = 0.f;
    if (g == 0) {
      acc = a.v[0];
      if (live) zp[0] = 1.f;
    }
    for (int j = g; j < h; j += G) {
      const float x = xp[j];
      if (live) zp[j + 1] = x;
      acc = fmaf(x, a.v[j + 1], acc);
    }
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) acc += shfl_xor(acc, off);
    const float lin = acc, p = act_apply(lin, a.act);
    if (live && g == 0) {
      a.lin[row] = lin;
      a.pred[row] = p;
    }
    if (!train) continue;  // (uniform over the launch)
    const float y = a.label[row], w = a.weight ? a.weight[row] : 1.f;
    const float diff = p - y;
    float lr, gr;
    if (a.loss == RG_CB_LOSS_MSE) {
      lr = diff * diff;
      gr = 2.f * diff;
    } else if (a.loss == RG_CB_LOSS_MAE) {
      lr = fabsf(diff);
      gr = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    } else {  // F.binary_cross_entropy: both logs clamped at -100 (log1p(-p), as torch takes it: 1 - p is 1 below
              // p = 2^-24 and the row's loss would vanish); its backward's denominator at 1e-12
      const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(log1pf(-p), -100.f);
      lr = (y - 1.f) * l1p - y * lp;
      gr = diff / fmaxf((1.f - p) * p, 1e-12f);
    }
    lr *= w;
    const float dlin = (gr * (w * a.inv_B)) * act_grad_from_output(p, a.act);
    if (live) {
      float* dp = a.dmlp + row * a.ld_dmlp;
      for (int j = g; j < h; j += G) dp[j] = dlin * a.v[j + 1];
      if (g == 0) {
        a.row_loss[row] = lr;
        loss_acc += (double)lr;
      }
    }
    if (g == 0) sdlin[r0 + rl] = live ? dlin : 0.f;
  }
  if (!train) return;
  loss_acc = wave_sum_f64(loss_acc);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = loss_acc;
  __syncthreads();  // (also: sdlin is complete)
  if (threadIdx.x == 0) a.loss_partials[blockIdx.x] = (float)((scratch[0] + scratch[1]) + (scratch[2] + scratch[3]));
  if (!a.dv_partials) return;
  const long left = a.B - row0;
  const int nrows = left < a.block_rows ? (int)left : a.block_rows;
  for (int c = threadIdx.x; c < d; c += CB_THREADS) {
    float s = 0.f;
    for (int r = 0; r < nrows; ++r) {
      const float zc = c == 0 ? 1.f : a.mlp[(row0 + r) * a.ld + (c - 1)];
      s = fmaf(sdlin[r], zc, s);
    }
    a.dv_partials[(long)blockIdx.x * d + c] = s;
  }
}

// The finishing launch: workgroup 0 the loss, workgroup 1 + c column c of dv.  Thread t adds the partials t, t + 256, ...
// in double, the 256 sums meet in LDS by a fixed tree.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) drlinucb_finish_kernel(const float* __restrict__ loss_partials,
                                                                         const float* __restrict__ dv_partials, int P, int d,
                                                                         int B, float* __restrict__ loss,
                                                                         float* __restrict__ dv) {
  __shared__ double sums[CB_THREADS];
  const int c = (int)blockIdx.x - 1;
  double s = 0.0;
  for (int p = threadIdx.x; p < P; p += CB_THREADS) s += (double)(c < 0 ? loss_partials[p] : dv_partials[(long)p * d + c]);
  sums[threadIdx.x] = s;
  lds_tree_sum<CB_THREADS>(sums);
  if (threadIdx.x == 0) {
    if (c < 0) *loss = (float)(sums[0] / (double)B);
    else dv[c] = (float)sums[0];
  }
}

__global__ void drlinucb_activate_kernel(float* __restrict__ x, float* __restrict__ y, int n, int act) {
  const long i = (long)blockIdx.x * CB_THREADS + threadIdx.x;
  if (i >= n) return;
  x[i] = act_apply(x[i], act);
  if (y) y[i] = act_apply(y[i], act);
}

static int drh_group(int h) { return h <= 4 ? 1 : (h <= 16 ? 4 : (h <= 64 ? 16 : 64)); }
static int drh_block_rows(int h) {
  const int rows = CB_THREADS / drh_group(h);
  return rows > DRH_MIN_BLOCK_ROWS ? rows : DRH_MIN_BLOCK_ROWS;
}
static bool drh_act_ok(int act) { return act >= RG_ACT_LINEAR && act <= RG_ACT_SOFTPLUS; }

}  // namespace rg

using namespace rg;

extern "C" {

int rg_linucb_solve(int dim, double l2_reg_lambda, float* avg_A, float* avg_b, float* sum_weight, int64_t* num_obs,
                    float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs, float* inv_avg_A,
                    float* coefs, float* coefs_valid_for_avg_A, int32_t* status, rg_stream_t stream) {
  if (dim < 1 || dim > RG_LINUCB_SOLVE_MAX_DIM) return RG_EINVAL;
  if (!avg_A || !avg_b || !sum_weight || !num_obs || !cur_avg_A || !cur_avg_b || !cur_sum_weight || !cur_num_obs ||
      !inv_avg_A || !coefs || !coefs_valid_for_avg_A || !status)
    return RG_EINVAL;
  SolveArgs a;
  a.d = dim, a.lambda = (float)l2_reg_lambda;
  a.avg_A = avg_A, a.avg_b = avg_b, a.sum_weight = sum_weight, a.num_obs = num_obs;
  a.cur_avg_A = cur_avg_A, a.cur_avg_b = cur_avg_b, a.cur_sum_weight = cur_sum_weight, a.cur_num_obs = cur_num_obs;
  a.inv_avg_A = inv_avg_A, a.coefs = coefs, a.valid = coefs_valid_for_avg_A, a.status = status;
  const dim3 grid(1), block(CB_THREADS);
  if (dim <= 16) RG_LAUNCH(linucb_solve_kernel<1>, grid, block, (hipStream_t)stream, a);
  else if (dim <= 32) RG_LAUNCH(linucb_solve_kernel<2>, grid, block, (hipStream_t)stream, a);
  else if (dim <= 64) RG_LAUNCH(linucb_solve_kernel<4>, grid, block, (hipStream_t)stream, a);
  else RG_LAUNCH(linucb_solve_kernel<8>, grid, block, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_drlinucb_head_partials(int batch, int h) {
  if (batch < 1 || h < 1 || h + 1 > RG_LINUCB_MAX_DIM) return 0;
  const int rows = drh_block_rows(h);
  return (batch + rows - 1) / rows;
}

int rg_drlinucb_head(const float* mlp_out, int64_t ld_mlp_out, const float* v, const float* label, const float* weight,
                     int act, int loss_type, int batch, int h, float* z, float* lin, float* pred_label, float* row_loss,
                     float* dmlp_out, int64_t ld_dmlp_out, float* loss_partials, float* dv_partials, float* loss, float* dv,
                     rg_stream_t stream) {
  if (batch < 1 || h < 1 || h + 1 > RG_LINUCB_MAX_DIM || ld_mlp_out < h) return RG_EINVAL;
  if (!mlp_out || !v || !z || !lin || !pred_label || !drh_act_ok(act)) return RG_EINVAL;
  if (label) {
    if (loss_type != RG_CB_LOSS_MSE && loss_type != RG_CB_LOSS_MAE && loss_type != RG_CB_LOSS_BCE) return RG_EINVAL;
    if (!row_loss || !dmlp_out || !loss_partials || !loss || ld_dmlp_out < h) return RG_EINVAL;
    if (dv && !dv_partials) return RG_EINVAL;
  }
  DrHeadArgs a;
  a.mlp = mlp_out, a.ld = (long)ld_mlp_out, a.v = v, a.label = label, a.weight = label ? weight : nullptr;
  a.act = act, a.loss = loss_type, a.B = batch, a.h = h, a.block_rows = drh_block_rows(h);
  a.inv_B = 1.f / (float)batch;
  a.z = z, a.lin = lin, a.pred = pred_label, a.row_loss = row_loss, a.dmlp = dmlp_out, a.ld_dmlp = (long)ld_dmlp_out;
  a.loss_partials = loss_partials, a.dv_partials = (label && dv) ? dv_partials : nullptr;
  const int P = rg_drlinucb_head_partials(batch, h);
  const dim3 grid(P), block(CB_THREADS);
  switch (drh_group(h)) {
    case 1: RG_LAUNCH(drlinucb_head_kernel<1>, grid, block, (hipStream_t)stream, a); break;
    case 4: RG_LAUNCH(drlinucb_head_kernel<4>, grid, block, (hipStream_t)stream, a); break;
    case 16: RG_LAUNCH(drlinucb_head_kernel<16>, grid, block, (hipStream_t)stream, a); break;
    default: RG_LAUNCH(drlinucb_head_kernel<64>, grid, block, (hipStream_t)stream, a); break;
  }
  if (label)
    RG_LAUNCH(drlinucb_finish_kernel, dim3(1 + (a.dv_partials ? h + 1 : 0)), block, (hipStream_t)stream,
              (const float*)loss_partials, (const float*)a.dv_partials, P, h + 1, batch, loss, dv);
  return (int)hipGetLastError();
}

int rg_drlinucb_activate(float* a, float* b, int n, int act, rg_stream_t stream) {
  if (n < 1 || !a || !drh_act_ok(act)) return RG_EINVAL;
  RG_LAUNCH(drlinucb_activate_kernel, dim3((n + CB_THREADS - 1) / CB_THREADS), dim3(CB_THREADS), (hipStream_t)stream, a, b,
            n, act);
  return (int)hipGetLastError();
}

}  // extern "C"
