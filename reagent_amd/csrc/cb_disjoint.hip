// cb_disjoint.hip — the disjoint LinUCB bandit: one ridge regression per arm.  Training is `arms` independent weighted Gram
// updates over the arms' sub-batches, which lie back to back in one packed batch (row_offsets, in device memory, says where
// each begins); acting scores every row against every arm's own inverse.  Both products run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation).  No atomics: partials leave per workgroup and are added
// in a fixed order, so two runs give the same bits.  The accumulate path's body is rg_cb.h's, shared with cb.hip; this file
// keeps the plan (how an arm's rows are cut into slices) and the plain add.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_cb.h"  // the Gram tile body, the finishing sum, the tile numbering, the arg-max rule (shared with cb.hip)

// every multiply and add is rounded on its own (ucb = mean + alpha * sigma is one multiply and one add; cur_A += S one add)
#pragma clang fp contract(off)

namespace rg {

constexpr int DCB_SLICE_UNIT = 256;        // a slice is 1 .. 8 units of rows, by the number of tiles (a function of d alone)
constexpr int DCB_MAX_BLOCKS = 1 << 20;    // workgroups of the main launch at the most
constexpr int DCB_MAX_ARMS = 65535;        // (a grid dimension)
constexpr int DCB_UNROLL = 4;              // MFMA steps whose operands are loaded together, ahead of the MFMAs

struct DcbPlan {
  int tiles_1d, tiles, slices, slice_rows;
};

// The same plan for rg_dlinucb_workspace_bytes and rg_dlinucb_accumulate.  slice_rows depends on d ALONE: where an arm's
// rows are cut into slices does not depend on the other arms or on the hint, so an arm's sums have the same bits in a packed
// call and in a call of its own.  The hint only says how many slices the grid has; the last one runs to the arm's end.
static DcbPlan dcb_plan(int max_arm_rows, int arms, int d) {
  DcbPlan p;
  p.tiles_1d = cb_tiles_1d(d);
  p.tiles = cb_tiles(p.tiles_1d);
  int units = p.tiles / 4;
  units = units < 1 ? 1 : (units > 8 ? 8 : units);
  p.slice_rows = DCB_SLICE_UNIT * units;
  long slices = ((long)max_arm_rows + p.slice_rows - 1) / p.slice_rows;
  const long cap = DCB_MAX_BLOCKS / ((long)p.tiles * arms);
  slices = slices < cap ? slices : cap;
  p.slices = slices < 1 ? 1 : (int)slices;
  return p;
}

// workspace layout (floats): [arms][slices][tiles][32 * 32] Gram partials, then [arms][slices][tiles_1d * 32] S_b partials
static size_t dcb_gram_floats(const DcbPlan& p, int arms) { return (size_t)arms * p.slices * p.tiles * CB_TILE_ELEMS; }
static size_t dcb_workspace_floats(const DcbPlan& p, int arms) {
  return dcb_gram_floats(p, arms) + (size_t)arms * p.slices * p.tiles_1d * CB_TILE;
}

struct DcbAccArgs {
  const float *x, *y, *weight;  // packed [N, d], [N], [N] or NULL
  const int64_t* row_offsets;   // [arms + 1], device memory
  int N, d, arms, tiles_1d, tiles, slices, slice_rows;
  float *gram, *sb;             // the workspace
  float *cur_A, *cur_b;
  int64_t* cur_num_obs;
};

// arm a's rows [begin, end) of the packed batch, forced into 0 <= begin <= end <= N whatever the offsets say
__device__ __forceinline__ void dcb_arm_rows(const DcbAccArgs& a, int arm, long& begin, long& end) {
  long b = a.row_offsets[arm], e = a.row_offsets[arm + 1];
  b = b < 0 ? 0 : (b > a.N ? a.N : b);
  e = e < b ? b : (e > a.N ? a.N : e);
  begin = b, end = e;
}

// Workgroup (s, t, arm): tile t of arm's Gram matrix over slice s of ITS rows, counted from the arm's first row: nothing
// depends on where the arm lies in the packed batch (cb_gram_tile).  An empty slice writes zero partials.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) dlinucb_gram_kernel(const DcbAccArgs a) {
  const int s = blockIdx.x, t = blockIdx.y, arm = blockIdx.z;
  int ti, tj;
  cb_tile_of(t, a.tiles_1d, ti, tj);
  long begin, end;
  dcb_arm_rows(a, arm, begin, end);
  long row_begin = begin + (long)s * a.slice_rows;
  row_begin = row_begin < end ? row_begin : end;
  long row_end = row_begin + a.slice_rows < end ? row_begin + a.slice_rows : end;
  if (s == a.slices - 1) row_end = end;  // the hint sizes the grid; it never decides which rows count
  const CbRows rows = {a.x, a.y, a.weight, nullptr, 1};
  const size_t slot = (size_t)arm * a.slices + s;
  cb_gram_tile<DCB_UNROLL, false>(rows, row_begin, row_end, a.d, ti, tj, a.gram + (slot * a.tiles + t) * CB_TILE_ELEMS,
                                  a.sb + (slot * a.tiles_1d + ti) * CB_TILE, nullptr);
}

// disjoint_linucb_trainer.py:66-76 on the ordered sums of the partials, per arm (blockIdx.y): one thread per entry
// (cb_finish_entry); thread 0 counts the arm's rows.  cur_A += S and cur_b += S_b are one fp32 add each.
__global__ void dlinucb_finish_kernel(const DcbAccArgs a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int arm = blockIdx.y;
  const long dd = (long)a.d * a.d;
  if (e >= dd + a.d) return;
  if (e == 0) {
    long begin, end;
    dcb_arm_rows(a, arm, begin, end);
    a.cur_num_obs[arm] += (int64_t)(end - begin);
  }
  const size_t slot0 = (size_t)arm * a.slices;
  const CbEntry en = cb_finish_entry(e, a.d, a.tiles_1d, a.tiles, a.slices, a.gram + slot0 * a.tiles * CB_TILE_ELEMS,
                                     a.sb + slot0 * a.tiles_1d * CB_TILE);
  if (en.below) return;
  float* out = en.in_A ? a.cur_A + (size_t)arm * dd : a.cur_b + (size_t)arm * a.d;
  const float v = out[en.at] + en.S;
  out[en.at] = v;
  out[en.mirror] = v;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// Structure, and why it is not rg_linucb_score's.  That kernel gives a workgroup 32 rows, so every inv_A operand it loads
// from global memory feeds ONE MFMA, and it waits for each group of loads before the MFMAs that use them.  Here a workgroup
// takes R row tiles (R = 4: 128 rows, or 2 where x would not fit in LDS), stages ALL d columns of them in LDS once, and
// reuses that image for every arm and every column tile.
//   - A wave owns output-column tiles jt = wave, wave + 4, ... of Y = X * inv_A[arm] and holds R accumulator tiles: one
//     inv_A operand loaded from global memory feeds R MFMAs.
//   - The loads of the NEXT 16 values of k are issued before the MFMAs of the current ones (registers b_next, a scheduling
//     fence on either side of the MFMA block, the zeroing select after it), so the matrix streams behind the MFMA pipe
//     instead of in front of it.
//   - The X operand comes from LDS as ds_read_b128: within a group of 8 values of k, half h of the wave takes
//     k = 8 g + 4 h + {0..3}, four consecutive floats of its row.  The row pitch is d_pad + 4 floats (d_pad a multiple of
//     16), which puts 16 consecutive rows on 16 different 16-byte bank slots.  Which k a half takes in which step is free
//     as long as A and B agree: it only permutes the fp32 summation order, identically in every run.
// The two scorers share their epilogue's helpers (rg_cb.h: accumulator row, half-wave sum, arg-max rule), not their K loops.
constexpr int DCB_KG = 2;  // groups of 8 values of k per batch of loads

struct DcbScoreArgs {
  const float *x, *coefs, *inv_A;
  const uint8_t* arm_presence;
  float alpha;
  int B, d, arms;
  float *mean, *sigma, *ucb;
  int64_t* best_arm;
};

// The inv_A operands of DCB_KG groups of k from k0 on, as loaded (addresses clamped into the matrix whatever k0 is) ...
__device__ __forceinline__ void dcb_load_b(const float* __restrict__ M, int d, int k0, int half, int jc,
                                           float (&b)[DCB_KG][4]) {
#pragma unroll
  for (int g = 0; g < DCB_KG; ++g)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kk = k0 + 8 * g + 4 * half + t;
      b[g][t] = M[(long)(kk < d ? kk : d - 1) * d + jc];
    }
}
// ... and zeroed where k or the column is past the end.  Apart, because the select is the first USE of a loaded value: next
// to the load it would make the wave wait for the load at once; here it runs after the MFMAs the load was issued ahead of.
__device__ __forceinline__ void dcb_mask_b(int d, int k0, int half, bool j_ok, float (&b)[DCB_KG][4]) {
#pragma unroll
  for (int g = 0; g < DCB_KG; ++g)
#pragma unroll
    for (int t = 0; t < 4; ++t) b[g][t] = (j_ok && k0 + 8 * g + 4 * half + t < d) ? b[g][t] : 0.f;
}

template <int R>
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) dlinucb_score_kernel(const DcbScoreArgs a) {
  constexpr int ROWS = R * CB_TILE;
  RG_DYN_LDS(smem);
  const int d = a.d, arms = a.arms;
  const int dp = (d + 15) & ~15, pitch = dp + 4;
  float* xs = (float*)smem;          // [ROWS][pitch], columns d .. dp - 1 and rows past B zero
  float* qpart = xs + ROWS * pitch;  // [2][CB_WAVES][ROWS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * ROWS;
  const int tiles_1d = cb_tiles_1d(d);
  for (int r = wave; r < ROWS; r += CB_WAVES) {
    const long row = row0 + r;
    for (int c = lane; c < dp; c += 64) xs[r * pitch + c] = (row < a.B && c < d) ? a.x[row * d + c] : 0.f;
  }
  __syncthreads();
  // the means x . coefs[arm], one (row, arm) pair a thread at a time; they wait in `ucb` for the deviations
  const bool with_sigma = a.alpha != 0.f;
  for (int p = threadIdx.x; p < ROWS * arms; p += CB_THREADS) {
    const int r = p % ROWS, arm = p / ROWS;
    const long row = row0 + r;
    const float* c = a.coefs + (long)arm * d;
    float m = 0.f;
    for (int k = 0; k < dp; k += 4) {
      const f32x4 v = *(const f32x4*)(xs + r * pitch + k);
#pragma unroll
      for (int t = 0; t < 4; ++t) m = fmaf(v[t], (k + t < d) ? c[k + t] : 0.f, m);
    }
    if (row < a.B) {
      const long o = row * arms + arm;
      a.ucb[o] = m;
      if (a.mean) a.mean[o] = m;
      if (a.sigma && !with_sigma) a.sigma[o] = 0.f;
    }
  }
  __syncthreads();  // (the workgroup's own global stores are visible to it past the barrier)
  CbBest best;
  const long my_row = row0 + threadIdx.x;
  const bool finisher = threadIdx.x < ROWS && my_row < a.B;
  if (!with_sigma) {  // the mean alone: inv_A is never read, sigma is exactly 0, ucb has the bits of the mean
    if (finisher && a.best_arm) {
      for (int k = 0; k < arms; ++k)
        best.take(a.ucb[my_row * arms + k], k, !a.arm_presence || a.arm_presence[my_row * arms + k]);
      a.best_arm[my_row] = best.arm;
    }
    return;
  }
  f32x16 acc[R];
  for (int arm = 0; arm < arms; ++arm) {
    const float* __restrict__ M = a.inv_A + (long)arm * d * d;
    float part[R][16];
#pragma unroll
    for (int rt = 0; rt < R; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) part[rt][r] = 0.f;
    for (int jt = wave; jt < tiles_1d; jt += CB_WAVES) {  // (wave-uniform)
      const int j = jt * CB_TILE + col;
      const bool j_ok = j < d;
      const int jc = j_ok ? j : d - 1;
#pragma unroll
      for (int rt = 0; rt < R; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
      float b_cur[DCB_KG][4], b_next[DCB_KG][4];
      dcb_load_b(M, d, 0, half, jc, b_cur);
      dcb_mask_b(d, 0, half, j_ok, b_cur);
      for (int k0 = 0; k0 < dp; k0 += 8 * DCB_KG) {
        dcb_load_b(M, d, k0 + 8 * DCB_KG, half, jc, b_next);  // (past the end: clamped addresses, zeroed below)
        sched_fence();  // the next operands' loads are issued BEFORE this batch's MFMAs, not sunk below them
#pragma unroll
        for (int g = 0; g < DCB_KG; ++g) {
          f32x4 av[R];
#pragma unroll
          for (int rt = 0; rt < R; ++rt)
            av[rt] = *(const f32x4*)(xs + (rt * CB_TILE + col) * pitch + k0 + 8 * g + 4 * half);
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rt = 0; rt < R; ++rt) acc[rt] = mfma_32x32x2_f32(av[rt][t], b_cur[g][t], acc[rt]);
        }
        sched_fence();
        dcb_mask_b(d, k0 + 8 * DCB_KG, half, j_ok, b_next);
#pragma unroll
        for (int g = 0; g < DCB_KG; ++g)
#pragma unroll
          for (int t = 0; t < 4; ++t) b_cur[g][t] = b_next[g][t];
      }
      // this tile's share of x^T inv_A x: lane (j, half) multiplies its Y[i][j] by x[i][j], from the staged image
#pragma unroll
      for (int rt = 0; rt < R; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = rt * CB_TILE + cb_acc_row(r, half);
          const float xv = j_ok ? xs[i * pitch + jc] : 0.f;
          part[rt][r] += acc[rt][r] * xv;
        }
    }
    float* qp = qpart + (arm & 1) * (CB_WAVES * ROWS) + wave * ROWS;
#pragma unroll
    for (int rt = 0; rt < R; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = cb_half_wave_sum(part[rt][r]);
        if (col == 0) qp[rt * CB_TILE + cb_acc_row(r, half)] = v;
      }
    __syncthreads();  // (one barrier an arm: the next arm writes the other half of qpart)
    if (finisher) {
      const float* q4 = qpart + (arm & 1) * (CB_WAVES * ROWS) + threadIdx.x;
      const float q = ((q4[0] + q4[ROWS]) + q4[2 * ROWS]) + q4[3 * ROWS];
      const float sigma = sqrtf(q);  // (a negative form gives NaN, silently: disjoint_linucb_predictor.py:171-173)
      const long o = my_row * arms + arm;
      const float u = a.ucb[o] + a.alpha * sigma;
      a.ucb[o] = u;
      if (a.sigma) a.sigma[o] = sigma;
      best.take(u, arm, !a.arm_presence || a.arm_presence[o]);
    }
  }
  if (finisher && a.best_arm) a.best_arm[my_row] = best.arm;
}

static size_t dcb_score_lds_bytes(int rows, int d) {
  const int dp = (d + 15) & ~15;
  return ((size_t)rows * (dp + 4) + 2 * CB_WAVES * rows) * sizeof(float);
}

}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_dlinucb_workspace_bytes(int max_arm_rows, int arms, int dim) {
  if (max_arm_rows < 0 || arms < 1 || arms > DCB_MAX_ARMS || dim < 1 || dim > RG_LINUCB_MAX_DIM) return 0;
  return dcb_workspace_floats(dcb_plan(max_arm_rows, arms, dim), arms) * sizeof(float);
}

int rg_dlinucb_accumulate(const float* x, const float* y, const float* weight, const int64_t* row_offsets, int n, int arms,
                          int max_arm_rows, int dim, float* cur_A, float* cur_b, int64_t* cur_num_obs, void* workspace,
                          size_t workspace_bytes, rg_stream_t stream) {
  if (!row_offsets || !cur_A || !cur_b || !cur_num_obs || !workspace) return RG_EINVAL;
  if (dim < 1 || dim > RG_LINUCB_MAX_DIM || arms < 1 || arms > DCB_MAX_ARMS || n < 0 || max_arm_rows < 0) return RG_EINVAL;
  if (n > 0 && (!x || !y)) return RG_EINVAL;
  const DcbPlan p = dcb_plan(max_arm_rows, arms, dim);
  if (workspace_bytes < dcb_workspace_floats(p, arms) * sizeof(float)) return RG_EINVAL;
  if (n == 0) return RG_OK;  // no row: nothing changes
  DcbAccArgs a;
  a.x = x, a.y = y, a.weight = weight, a.row_offsets = row_offsets;
  a.N = n, a.d = dim, a.arms = arms, a.tiles_1d = p.tiles_1d, a.tiles = p.tiles, a.slices = p.slices;
  a.slice_rows = p.slice_rows;
  a.gram = (float*)workspace, a.sb = a.gram + dcb_gram_floats(p, arms);
  a.cur_A = cur_A, a.cur_b = cur_b, a.cur_num_obs = cur_num_obs;
  RG_LAUNCH(dlinucb_gram_kernel, dim3(p.slices, p.tiles, arms), dim3(CB_THREADS), (hipStream_t)stream, a);
  const long entries = (long)dim * dim + dim;
  RG_LAUNCH(dlinucb_finish_kernel, dim3((unsigned)((entries + CB_THREADS - 1) / CB_THREADS), arms), dim3(CB_THREADS),
            (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_dlinucb_score(const float* x, const float* coefs, const float* inv_A, double ucb_alpha, int batch, int dim, int arms,
                     const uint8_t* arm_presence, float* mean, float* sigma, float* ucb, int64_t* best_arm,
                     rg_stream_t stream) {
  if (!x || !coefs || !inv_A || !ucb) return RG_EINVAL;
  if (batch < 1 || arms < 1 || dim < 1 || dim > RG_LINUCB_MAX_DIM) return RG_EINVAL;
  if (arm_presence && !best_arm) return RG_EINVAL;
  if ((long)batch * arms > 0x7fffffffL) return RG_EINVAL;
  DcbScoreArgs a;
  a.x = x, a.coefs = coefs, a.inv_A = inv_A, a.arm_presence = arm_presence, a.alpha = (float)ucb_alpha;
  a.B = batch, a.d = dim, a.arms = arms, a.mean = mean, a.sigma = sigma, a.ucb = ucb, a.best_arm = best_arm;
  // four row tiles a workgroup where their d columns fit in LDS and the batch has that many rows, two otherwise
  const bool four = ((dim + 15) & ~15) <= 256 && batch > 2 * CB_TILE;
  const int rows = (four ? 4 : 2) * CB_TILE;
  const size_t lds = dcb_score_lds_bytes(rows, dim);
  const dim3 grid((unsigned)((batch + rows - 1) / rows));
  if (four) {
    RG_ALLOW_LDS(dlinucb_score_kernel<4>, lds);
    RG_LAUNCH_DYN(dlinucb_score_kernel<4>, grid, dim3(CB_THREADS), lds, (hipStream_t)stream, a);
  } else {
    RG_ALLOW_LDS(dlinucb_score_kernel<2>, lds);
    RG_LAUNCH_DYN(dlinucb_score_kernel<2>, grid, dim3(CB_THREADS), lds, (hipStream_t)stream, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
