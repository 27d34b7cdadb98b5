// cb.hip — the contextual-bandit (LinUCB) kernels.  Training is a weighted Gram matrix over the batch, S_A = X^T diag(w) X
// with S_b = X^T (w o y) and s_w = sum w, folded into running averages that live on the device (no host synchronisation);
// acting is the GEMM x * inv_avg_A fused with the row dot that turns it into x^T inv_avg_A x, the mean x * coefs, the
// upper confidence bound and a masked arg-max over each row's arms.  Both products run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation).  No atomics: partials leave per workgroup and a
// finishing launch adds them in a fixed order, so two runs give the same bits.  The accumulate path's body is rg_cb.h's,
// shared with cb_disjoint.hip; this file keeps the plan (how the batch is cut into slices) and the running average.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_cb.h"      // the Gram tile body, the finishing sum, the tile numbering, the arg-max rule
#include "rg_reduce.h"  // lds_tree_sum

// The running-average update is held to the reference's fp32 operation order: every multiply, divide, subtract and add is
// rounded on its own (hipcc would otherwise contract a * b + c into one fused multiply-add).
#pragma clang fp contract(off)

namespace rg {

constexpr int CB_SLICE_MIN_ROWS = 256;  // a workgroup's slice of the batch is at least this long (64 rows a wave) ...
constexpr int CB_MAX_BLOCKS = 1024;     // ... and the launch has about this many workgroups at the most
constexpr int CB_UNROLL = 4;            // MFMA steps whose operands are loaded together (cb_gram_tile)

struct CbPlan {
  int tiles_1d, tiles, slices, slice_rows;
};

// the same plan for rg_linucb_workspace_bytes and rg_linucb_accumulate: a function of (B, d) alone
static CbPlan cb_plan(int B, int d) {
  CbPlan p;
  p.tiles_1d = cb_tiles_1d(d);
  p.tiles = cb_tiles(p.tiles_1d);
  int slices = (B + CB_SLICE_MIN_ROWS - 1) / CB_SLICE_MIN_ROWS;
  const int cap = CB_MAX_BLOCKS / p.tiles > 1 ? CB_MAX_BLOCKS / p.tiles : 1;
  slices = slices < cap ? slices : cap;
  int rows = (B + slices - 1) / slices;
  rows = (rows + 2 * CB_WAVES - 1) / (2 * CB_WAVES) * (2 * CB_WAVES);  // whole MFMA steps (2 rows) for each wave
  p.slice_rows = rows;
  p.slices = (B + rows - 1) / rows;
  return p;
}

// workspace layout (floats): [slices][tiles][32 * 32] Gram partials, [slices][tiles_1d * 32] S_b partials,
// [slices] s_w partials, [1] the cur_sum_weight the main launch saw (the finishing launch rewrites the buffer itself)
struct CbWorkspace {
  float *gram, *sb, *sw, *old_sw;
};
static size_t cb_workspace_floats(const CbPlan& p) {
  return (size_t)p.slices * p.tiles * CB_TILE_ELEMS + (size_t)p.slices * p.tiles_1d * CB_TILE + p.slices + 1;
}
static CbWorkspace cb_carve(const CbPlan& p, void* workspace) {
  CbWorkspace w;
  w.gram = (float*)workspace;
  w.sb = w.gram + (size_t)p.slices * p.tiles * CB_TILE_ELEMS;
  w.sw = w.sb + (size_t)p.slices * p.tiles_1d * CB_TILE;
  w.old_sw = w.sw + p.slices;
  return w;
}

struct CbAccArgs {
  CbRows rows;  // x [B, d], or [B, A, d] with action
  const float* cur_sum_weight;
  int B, d, tiles_1d, slice_rows;
  CbWorkspace ws;
};

// Workgroup (t, s): tile t of the Gram matrix over the rows of slice s of the batch (cb_gram_tile).  Workgroup (0, s) also
// leaves the slice's sum of weights.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_gram_kernel(const CbAccArgs a) {
  const int t = blockIdx.x, s = blockIdx.y;
  int ti, tj;
  cb_tile_of(t, a.tiles_1d, ti, tj);
  const long row_begin = (long)s * a.slice_rows;
  const long row_end = row_begin + a.slice_rows < a.B ? row_begin + a.slice_rows : a.B;
  cb_gram_tile<CB_UNROLL, true>(a.rows, row_begin, row_end, a.d, ti, tj,
                                a.ws.gram + ((size_t)s * gridDim.x + t) * CB_TILE_ELEMS,
                                a.ws.sb + ((size_t)s * a.tiles_1d + ti) * CB_TILE, t == 0 ? a.ws.sw + s : nullptr);
  if (t == 0 && s == 0 && threadIdx.x == 0) *a.ws.old_sw = *a.cur_sum_weight;
}

struct CbFinishArgs {
  CbWorkspace ws;
  float *cur_avg_A, *cur_avg_b, *cur_sum_weight;
  int64_t* cur_num_obs;
  int B, d, tiles_1d, tiles, slices;
};

// linucb_trainer.py:64-75 in its fp32 operation order, on the ordered sums of the partials: one thread per entry
// (cb_finish_entry).  Every thread reads the sum of weights the MAIN launch saw from the workspace; thread 0 alone
// rewrites cur_sum_weight and cur_num_obs.
__global__ void linucb_finish_kernel(const CbFinishArgs a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)a.d * a.d + a.d) return;
  float batch_sw = 0.f;
  for (int s = 0; s < a.slices; ++s) batch_sw += a.ws.sw[s];
  const float sum_w = *a.ws.old_sw + batch_sw;                    // cur_sum_weight += batch_sum_weight
  const float keep = 1.f - batch_sw / sum_w;                      // (1 - batch_sum_weight / cur_sum_weight)
  if (e == 0) {
    *a.cur_sum_weight = sum_w;
    *a.cur_num_obs += (int64_t)a.B;                               // cur_num_obs += y.shape[0]
  }
  const CbEntry en = cb_finish_entry(e, a.d, a.tiles_1d, a.tiles, a.slices, a.ws.gram, a.ws.sb);
  if (en.below) return;
  float* out = en.in_A ? a.cur_avg_A : a.cur_avg_b;
  const float v = out[en.at] * keep + en.S / sum_w;
  out[en.at] = v;
  out[en.mirror] = v;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
constexpr int CB_SCORE_ROWS = 32;  // rows of x per workgroup (one MFMA tile of rows)
constexpr int CB_SCORE_KC = 128;   // columns of x staged in LDS at a time
constexpr int CB_SCORE_TILES = 4;  // output-column tiles per wave: 4 waves x 4 x 32 = 512 = RG_LINUCB_MAX_DIM

constexpr int CB_SCORE_KU = 8;     // MFMA steps whose inv_avg_A operands are loaded ahead, together

// One staged chunk of K for a wave that owns NQ output-column tiles: CB_SCORE_KU steps at a time, all their inv_avg_A
// operands loaded first (from addresses clamped into the matrix, zeroed where the step or the column is past the end:
// no branch in the block, so the loads run ahead of the MFMAs), then NQ MFMAs a step.
template <int NQ>
__device__ __forceinline__ void score_chunk(const float* __restrict__ M, const float (*xs)[CB_SCORE_KC + 1],
                                            f32x16 (&acc)[CB_SCORE_TILES], int k0, int kc, int d, int wave, int col,
                                            int half) {
  int jc[NQ];
  bool j_ok[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = (wave + q * CB_WAVES) * CB_TILE + col;
    j_ok[q] = j < d;
    jc[q] = j_ok[q] ? j : d - 1;
  }
  for (int k = 0; k < kc; k += 2 * CB_SCORE_KU) {
    float av[CB_SCORE_KU], bv[CB_SCORE_KU][NQ];
#pragma unroll
    for (int u = 0; u < CB_SCORE_KU; ++u) {
      const int kk = k + 2 * u + half;
      const bool k_ok = kk < kc;
      const long row = k_ok ? k0 + kk : d - 1;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float v = M[row * d + jc[q]];
        bv[u][q] = (k_ok && j_ok[q]) ? v : 0.f;
      }
      av[u] = k_ok ? xs[col][kk] : 0.f;  // (kk < kc <= CB_SCORE_KC: inside the staged columns)
    }
#pragma unroll
    for (int u = 0; u < CB_SCORE_KU; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = mfma_32x32x2_f32(av[u], bv[u][q], acc[q]);
  }
}

struct CbScoreArgs {
  const float *x, *coefs, *inv_avg_A, *sum_weight;
  float alpha;
  int N, d;
  float *pred_label, *pred_sigma, *ucb;
  int32_t* nan_partials;
};

// Workgroup = 32 rows of x.  The rows pass through LDS 128 columns at a time (pitch 129: the A fragment's 32 rows fall on
// 32 banks).  Wave w owns the output-column tiles w, w + 4, ... of Y = X * inv_avg_A and keeps them in registers over the
// whole K loop: Y never exists in memory.  The mean x * coefs is taken from the same staged columns by 8 lanes per row.
// At the end lane (j, half) multiplies its Y[i][j] by x[i][j] (global, coalesced), the 32 lanes of a half add up by
// butterflies, the waves' per-row sums meet in LDS in wave order: q = x^T inv_avg_A x, sigma = sqrt(q / sum_weight).
// ucb_alpha == 0: no product at all, sigma exactly 0 (linear_regression.py:222-227).
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_score_kernel(const CbScoreArgs a) {
  __shared__ float xs[CB_SCORE_ROWS][CB_SCORE_KC + 1];
  __shared__ float qpart[CB_WAVES][CB_SCORE_ROWS];
  __shared__ int nan_rows[CB_SCORE_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * CB_SCORE_ROWS;
  const int d = a.d;
  const int tiles_1d = cb_tiles_1d(d);
  const bool with_sigma = a.alpha != 0.f;
  f32x16 acc[CB_SCORE_TILES];
#pragma unroll
  for (int q = 0; q < CB_SCORE_TILES; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  const int lrow = threadIdx.x >> 3, lsub = threadIdx.x & 7;  // the mean: 8 lanes per row
  float label = 0.f;
  for (int k0 = 0; k0 < d; k0 += CB_SCORE_KC) {
    const int kc = d - k0 < CB_SCORE_KC ? d - k0 : CB_SCORE_KC;
    for (int e = threadIdx.x; e < CB_SCORE_ROWS * CB_SCORE_KC; e += CB_THREADS) {
      const int r = e / CB_SCORE_KC, c = e % CB_SCORE_KC;
      const long row = row0 + r;
      xs[r][c] = (row < a.N && c < kc) ? a.x[row * d + k0 + c] : 0.f;
    }
    __syncthreads();
    for (int c = lsub; c < kc; c += 8) label += xs[lrow][c] * a.coefs[k0 + c];
    if (with_sigma) {  // (uniform over the workgroup; the number of tiles a wave owns is wave-uniform)
      const int nq = tiles_1d > wave ? (tiles_1d - wave + CB_WAVES - 1) / CB_WAVES : 0;
      switch (nq) {
        case 1: score_chunk<1>(a.inv_avg_A, xs, acc, k0, kc, d, wave, col, half); break;
        case 2: score_chunk<2>(a.inv_avg_A, xs, acc, k0, kc, d, wave, col, half); break;
        case 3: score_chunk<3>(a.inv_avg_A, xs, acc, k0, kc, d, wave, col, half); break;
        case 4: score_chunk<4>(a.inv_avg_A, xs, acc, k0, kc, d, wave, col, half); break;
        default: break;
      }
    }
    __syncthreads();
  }
  label += shfl_xor(label, 1);
  label += shfl_xor(label, 2);
  label += shfl_xor(label, 4);
  if (with_sigma) {
    float part[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll
    for (int q = 0; q < CB_SCORE_TILES; ++q) {
      const int tj = wave + q * CB_WAVES;
      if (tj < tiles_1d) {
        const int j = tj * CB_TILE + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long row = row0 + cb_acc_row(r, half);
          const float xv = (row < a.N && j < d) ? a.x[row * d + j] : 0.f;
          part[r] += acc[q][r] * xv;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = cb_half_wave_sum(part[r]);
      if (col == 0) qpart[wave][cb_acc_row(r, half)] = v;
    }
  }
  __syncthreads();
  int is_nan = 0;
  if (lsub == 0) {
    const long row = row0 + lrow;
    float sigma = 0.f;
    if (with_sigma) {
      const float q = ((qpart[0][lrow] + qpart[1][lrow]) + qpart[2][lrow]) + qpart[3][lrow];
      sigma = sqrtf(q / *a.sum_weight);
    }
    if (row < a.N) {
      is_nan = sigma != sigma;
      a.pred_label[row] = label;
      a.pred_sigma[row] = sigma;
      a.ucb[row] = label + a.alpha * sigma;
    }
    nan_rows[lrow] = is_nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int r = 0; r < CB_SCORE_ROWS; ++r) n += nan_rows[r];
    a.nan_partials[blockIdx.x] = n;
  }
}

// The finishing launch of rg_linucb_score: workgroup 0 adds the per-workgroup NaN counts in order into nan_count[0]; every
// thread takes one batch row and walks its arms for the arg-max of ucb under arm_presence by CbBest's rule.
__global__ void linucb_select_kernel(const float* __restrict__ ucb, const uint8_t* __restrict__ arm_presence, int B,
                                     int arms, const int32_t* __restrict__ nan_partials, int partials,
                                     int32_t* __restrict__ nan_count, int64_t* __restrict__ best_arm) {
  __shared__ int counts[CB_THREADS];
  if (blockIdx.x == 0) {
    int n = 0;
    for (int p = threadIdx.x; p < partials; p += CB_THREADS) n += nan_partials[p];
    counts[threadIdx.x] = n;
    lds_tree_sum<CB_THREADS>(counts);
    if (threadIdx.x == 0) *nan_count = counts[0];
  }
  const long b = (long)blockIdx.x * CB_THREADS + threadIdx.x;
  if (arms < 1 || b >= B) return;
  CbBest best;
  for (int k = 0; k < arms && !best.closed; ++k)
    best.take(ucb[b * arms + k], k, !arm_presence || arm_presence[b * arms + k]);
  best_arm[b] = best.arm;
}

}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_linucb_workspace_bytes(int batch, int dim) {
  if (batch < 1 || dim < 1 || dim > RG_LINUCB_MAX_DIM) return 0;
  return cb_workspace_floats(cb_plan(batch, dim)) * sizeof(float);
}

int rg_linucb_accumulate(const float* x, const int64_t* action, int arms, const float* y, const float* weight, int batch,
                         int dim, float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs,
                         void* workspace, size_t workspace_bytes, rg_stream_t stream) {
  if (!x || !y || !cur_avg_A || !cur_avg_b || !cur_sum_weight || !cur_num_obs || !workspace) return RG_EINVAL;
  if (batch < 1 || dim < 1 || dim > RG_LINUCB_MAX_DIM) return RG_EINVAL;
  if (action && arms < 1) return RG_EINVAL;
  const CbPlan p = cb_plan(batch, dim);
  if (workspace_bytes < cb_workspace_floats(p) * sizeof(float)) return RG_EINVAL;
  CbAccArgs a;
  a.rows.x = x, a.rows.y = y, a.rows.weight = weight, a.rows.action = action, a.rows.arms = action ? arms : 1;
  a.cur_sum_weight = cur_sum_weight, a.B = batch, a.d = dim, a.tiles_1d = p.tiles_1d, a.slice_rows = p.slice_rows;
  a.ws = cb_carve(p, workspace);
  RG_LAUNCH(linucb_gram_kernel, dim3(p.tiles, p.slices), dim3(CB_THREADS), (hipStream_t)stream, a);
  CbFinishArgs f;
  f.ws = a.ws, f.cur_avg_A = cur_avg_A, f.cur_avg_b = cur_avg_b, f.cur_sum_weight = cur_sum_weight;
  f.cur_num_obs = cur_num_obs, f.B = batch, f.d = dim, f.tiles_1d = p.tiles_1d, f.tiles = p.tiles, f.slices = p.slices;
  const long entries = (long)dim * dim + dim;
  RG_LAUNCH(linucb_finish_kernel, dim3((unsigned)((entries + CB_THREADS - 1) / CB_THREADS)), dim3(CB_THREADS),
            (hipStream_t)stream, f);
  return (int)hipGetLastError();
}

int rg_linucb_score_partials(int n) { return n < 1 ? 0 : (n + CB_SCORE_ROWS - 1) / CB_SCORE_ROWS; }

int rg_linucb_score(const float* x, const float* coefs, const float* inv_avg_A, const float* sum_weight, double ucb_alpha,
                    int n, int dim, int arms, const uint8_t* arm_presence, float* pred_label, float* pred_sigma, float* ucb,
                    int32_t* nan_partials, int32_t* nan_count, int64_t* best_arm, rg_stream_t stream) {
  if (!x || !coefs || !inv_avg_A || !sum_weight || !pred_label || !pred_sigma || !ucb || !nan_partials || !nan_count)
    return RG_EINVAL;
  if (n < 1 || dim < 1 || dim > RG_LINUCB_MAX_DIM || arms < 0) return RG_EINVAL;
  if (arms > 0 && (!best_arm || n % arms != 0)) return RG_EINVAL;
  CbScoreArgs a;
  a.x = x, a.coefs = coefs, a.inv_avg_A = inv_avg_A, a.sum_weight = sum_weight, a.alpha = (float)ucb_alpha;
  a.N = n, a.d = dim, a.pred_label = pred_label, a.pred_sigma = pred_sigma, a.ucb = ucb, a.nan_partials = nan_partials;
  const int partials = rg_linucb_score_partials(n);
  RG_LAUNCH(linucb_score_kernel, dim3(partials), dim3(CB_THREADS), (hipStream_t)stream, a);
  const int B = arms > 0 ? n / arms : 0;
  const int blocks = B > 0 ? (B + CB_THREADS - 1) / CB_THREADS : 1;
  RG_LAUNCH(linucb_select_kernel, dim3(blocks), dim3(CB_THREADS), (hipStream_t)stream, (const float*)ucb, arm_presence, B,
            arms, (const int32_t*)nan_partials, partials, nan_count, best_arm);
  return (int)hipGetLastError();
}

}  // extern "C"
