// cb_disjoint.hip — the disjoint LinUCB bandit: one ridge regression per arm.  Training is `arms` independent weighted Gram
// updates over the arms' sub-batches, which lie back to back in one packed batch (row_offsets, in device memory, says where
// each begins); acting scores every row against every arm's own inverse.  Both products run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation).  No atomics: partials leave per workgroup and are added
// in a fixed order, so two runs give the same bits.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"

// every multiply and add is rounded on its own (ucb = mean + alpha * sigma is one multiply and one add; cur_A += S one add)
#pragma clang fp contract(off)

namespace rg {

constexpr int DCB_THREADS = 256;
constexpr int DCB_WAVES = DCB_THREADS / 64;
constexpr int DCB_TILE = 32;               // the MFMA's 32 x 32 output tile
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
  p.tiles_1d = (d + DCB_TILE - 1) / DCB_TILE;
  p.tiles = p.tiles_1d * (p.tiles_1d + 1) / 2;  // tiles on or above the diagonal
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
static size_t dcb_gram_floats(const DcbPlan& p, int arms) {
  return (size_t)arms * p.slices * p.tiles * (DCB_TILE * DCB_TILE);
}
static size_t dcb_workspace_floats(const DcbPlan& p, int arms) {
  return dcb_gram_floats(p, arms) + (size_t)arms * p.slices * p.tiles_1d * DCB_TILE;
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

// Workgroup (s, t, arm): tile t = (ti, tj), ti <= tj, of arm's Gram matrix over slice s of ITS rows (counted from the arm's
// first row: nothing depends on where the arm lies in the packed batch).  Each wave walks its share of the slice two rows a
// step (rows 2 * wave + 8 * step + {0, 1}): lane l holds row k = l >> 5 of the step and column l & 31 of both tiles,
// A[i][k] = w_k * x[k][32 ti + i] and B[k][j] = x[k][32 tj + j], read straight from global memory (128 contiguous bytes per
// half wave), DCB_UNROLL steps' operands together from addresses clamped into the slice (no branch around a load).  The
// diagonal workgroups add S_b's partial from the registers they hold anyway.  The four waves' tiles meet in LDS and are
// added in wave order.  An empty slice writes zero partials.
__global__ void RG_LAUNCH_BOUNDS(DCB_THREADS, 1) dlinucb_gram_kernel(const DcbAccArgs a) {
  __shared__ float tile[DCB_WAVES][DCB_TILE * DCB_TILE];
  __shared__ float vec[DCB_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x, t = blockIdx.y, arm = blockIdx.z;
  int ti = 0, first = 0;  // tiles are numbered row by row over the upper triangle
  while (t >= first + (a.tiles_1d - ti)) first += a.tiles_1d - ti, ++ti;
  const int tj = ti + (t - first);
  const int col = lane & 31, half = lane >> 5;
  const int ca = ti * DCB_TILE + col, cb = tj * DCB_TILE + col;
  const bool ca_ok = ca < a.d, cb_ok = cb < a.d;
  const int cac = ca_ok ? ca : a.d - 1, cbc = cb_ok ? cb : a.d - 1;
  long begin, end;
  dcb_arm_rows(a, arm, begin, end);
  long row_begin = begin + (long)s * a.slice_rows;
  row_begin = row_begin < end ? row_begin : end;
  long row_end = row_begin + a.slice_rows < end ? row_begin + a.slice_rows : end;
  if (s == a.slices - 1) row_end = end;  // the hint sizes the grid; it never decides which rows count
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float sb = 0.f;
  for (long r0 = row_begin + 2 * wave; r0 < row_end; r0 += 2 * DCB_WAVES * DCB_UNROLL) {  // (wave-uniform trip count)
    float wv[DCB_UNROLL], yv[DCB_UNROLL], xa[DCB_UNROLL], xb[DCB_UNROLL];
    bool live[DCB_UNROLL];
#pragma unroll
    for (int u = 0; u < DCB_UNROLL; ++u) {
      const long row = r0 + 2 * DCB_WAVES * u + half;
      live[u] = row < row_end;
      const long rc = live[u] ? row : row_end - 1;  // (row_begin <= r0 <= row_end - 1: a row of this slice)
      wv[u] = a.weight ? a.weight[rc] : 1.f;
      yv[u] = a.y[rc];
      xa[u] = a.x[rc * a.d + cac];
      xb[u] = a.x[rc * a.d + cbc];
    }
#pragma unroll
    for (int u = 0; u < DCB_UNROLL; ++u) {
      // (uniform over the wave: the steps past the slice's end are skipped whole, a half step has its dead row zeroed)
      if (r0 + 2 * DCB_WAVES * u < row_end) {
        const float w = live[u] ? wv[u] : 0.f;
        const float va = (live[u] && ca_ok) ? xa[u] : 0.f;
        const float vb = (live[u] && cb_ok) ? xb[u] : 0.f;
        const float wy = w * (live[u] ? yv[u] : 0.f);
        acc = mfma_32x32x2_f32(w * va, vb, acc);
        sb += wy * va;
      }
    }
  }
  float* mine = tile[wave];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
    mine[i * DCB_TILE + col] = acc[r];
  }
  vec[wave][lane] = sb;
  __syncthreads();
  const size_t slot = (size_t)arm * a.slices + s;
  float* out = a.gram + (slot * a.tiles + t) * (DCB_TILE * DCB_TILE);
  for (int e = threadIdx.x; e < DCB_TILE * DCB_TILE; e += DCB_THREADS)
    out[e] = ((tile[0][e] + tile[1][e]) + tile[2][e]) + tile[3][e];
  if (ti == tj && threadIdx.x < DCB_TILE) {
    float v = 0.f;
#pragma unroll
    for (int wv = 0; wv < DCB_WAVES; ++wv) v = (v + vec[wv][threadIdx.x]) + vec[wv][threadIdx.x + 32];
    a.sb[(slot * a.tiles_1d + ti) * DCB_TILE + threadIdx.x] = v;
  }
}

// disjoint_linucb_trainer.py:66-76 on the ordered sums of the partials, per arm (blockIdx.y).  One thread per entry on or
// above the diagonal (it writes the mirrored entry too: an exactly symmetric matrix whatever was there) and, past those,
// one per entry of cur_b; thread 0 counts the arm's rows.  cur_A += S and cur_b += S_b are one fp32 add each.
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
  if (e < dd) {
    const int i = (int)(e / a.d), j = (int)(e % a.d);
    if (i > j) return;
    const int ti = i / DCB_TILE, tj = j / DCB_TILE;
    const int t = ti * a.tiles_1d - ti * (ti - 1) / 2 + (tj - ti);
    const size_t off = (size_t)t * (DCB_TILE * DCB_TILE) + (i % DCB_TILE) * DCB_TILE + (j % DCB_TILE);
    float S = 0.f;
    for (int s = 0; s < a.slices; ++s) S += a.gram[(slot0 + s) * a.tiles * (DCB_TILE * DCB_TILE) + off];
    float* A = a.cur_A + (size_t)arm * dd;
    const float v = A[e] + S;
    A[e] = v;
    A[(long)j * a.d + i] = v;
  } else {
    const int i = (int)(e - dd);
    float S = 0.f;
    for (int s = 0; s < a.slices; ++s) S += a.sb[(slot0 + s) * a.tiles_1d * DCB_TILE + i];
    a.cur_b[(size_t)arm * a.d + i] += S;
  }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// Structure, and why it is not rg_linucb_score's.  That kernel gives a workgroup 32 rows, so every inv_A operand it loads
// from global memory feeds ONE MFMA, and it waits for each group of loads before the MFMAs that use them.  Here a workgroup
// takes R row tiles (R = 4: 128 rows, or 2 where x would not fit in LDS), stages ALL d columns of them in LDS once, and
// reuses that image for every arm and every column tile.  A wave owns output-column tiles jt = wave, wave + 4, ... of
// Y = X * inv_A[arm] and holds R accumulator tiles: one inv_A operand loaded from global memory feeds R MFMAs, and the loads
// of the NEXT 16 values of k are issued before the MFMAs of the current ones (registers b_next, a scheduling fence on either
// side of the MFMA block, the zeroing select after it), so the matrix streams behind the MFMA pipe instead of in front of it.  The X operand comes from LDS as ds_read_b128: within a group of 8 values
// of k, half h of the wave takes k = 8 g + 4 h + {0..3}, four consecutive floats of its row, and the row pitch is
// d_pad + 4 floats (d_pad a multiple of 16), which puts 16 consecutive rows on 16 different 16-byte bank slots.  (Which k a
// half takes in which step is free as long as A and B agree; it only permutes the fp32 summation order, identically in
// every run.)
constexpr int DCB_KG = 2;  // groups of 8 values of k per batch of loads

struct DcbScoreArgs {
  const float *x, *coefs, *inv_A;
  const uint8_t* arm_presence;
  float alpha;
  int B, d, arms;
  float *mean, *sigma, *ucb;
  int64_t* best_arm;
};

// the masked arg-max's rule, that of rg_linucb_score: the lowest index among equals, a NaN before any number, arm 0 where
// no arm is present
struct DcbBest {
  float v;
  int arm;
  bool found, closed;
  __device__ __forceinline__ void take(float u, int k, bool present) {
    if (closed || !present) return;
    if (!found || u != u || u > v) v = u, arm = k, found = true;
    if (u != u) closed = true;
  }
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
__global__ void RG_LAUNCH_BOUNDS(DCB_THREADS, 1) dlinucb_score_kernel(const DcbScoreArgs a) {
  constexpr int ROWS = R * DCB_TILE;
  RG_DYN_LDS(smem);
  const int d = a.d, arms = a.arms;
  const int dp = (d + 15) & ~15, pitch = dp + 4;
  float* xs = (float*)smem;          // [ROWS][pitch], columns d .. dp - 1 and rows past B zero
  float* qpart = xs + ROWS * pitch;  // [2][DCB_WAVES][ROWS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * ROWS;
  const int tiles_1d = (d + DCB_TILE - 1) / DCB_TILE;
  for (int r = wave; r < ROWS; r += DCB_WAVES) {
    const long row = row0 + r;
    for (int c = lane; c < dp; c += 64) xs[r * pitch + c] = (row < a.B && c < d) ? a.x[row * d + c] : 0.f;
  }
  __syncthreads();
  // the means x . coefs[arm], one (row, arm) pair a thread at a time; they wait in `ucb` for the deviations
  const bool with_sigma = a.alpha != 0.f;
  for (int p = threadIdx.x; p < ROWS * arms; p += DCB_THREADS) {
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
  DcbBest best;
  best.v = 0.f, best.arm = 0, best.found = false, best.closed = false;
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
    for (int jt = wave; jt < tiles_1d; jt += DCB_WAVES) {  // (wave-uniform)
      const int j = jt * DCB_TILE + col;
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
            av[rt] = *(const f32x4*)(xs + (rt * DCB_TILE + col) * pitch + k0 + 8 * g + 4 * half);
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
          const int i = rt * DCB_TILE + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float xv = j_ok ? xs[i * pitch + jc] : 0.f;
          part[rt][r] += acc[rt][r] * xv;
        }
    }
    float* qp = qpart + (arm & 1) * (DCB_WAVES * ROWS) + wave * ROWS;
#pragma unroll
    for (int rt = 0; rt < R; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = part[rt][r];
        v += shfl_xor(v, 1);
        v += shfl_xor(v, 2);
        v += shfl_xor(v, 4);
        v += shfl_xor(v, 8);
        v += shfl_xor(v, 16);
        if (col == 0) qp[rt * DCB_TILE + (r & 3) + 8 * (r >> 2) + 4 * half] = v;
      }
    __syncthreads();  // (one barrier an arm: the next arm writes the other half of qpart)
    if (finisher) {
      const float* q4 = qpart + (arm & 1) * (DCB_WAVES * ROWS) + threadIdx.x;
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
  return ((size_t)rows * (dp + 4) + 2 * DCB_WAVES * rows) * sizeof(float);
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
  RG_LAUNCH(dlinucb_gram_kernel, dim3(p.slices, p.tiles, arms), dim3(DCB_THREADS), (hipStream_t)stream, a);
  const long entries = (long)dim * dim + dim;
  RG_LAUNCH(dlinucb_finish_kernel, dim3((unsigned)((entries + DCB_THREADS - 1) / DCB_THREADS), arms), dim3(DCB_THREADS),
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
  const bool four = ((dim + 15) & ~15) <= 256 && batch > 2 * DCB_TILE;
  const int rows = (four ? 4 : 2) * DCB_TILE;
  const size_t lds = dcb_score_lds_bytes(rows, dim);
  const dim3 grid((unsigned)((batch + rows - 1) / rows));
  if (four) {
    RG_ALLOW_LDS(dlinucb_score_kernel<4>, lds);
    RG_LAUNCH_DYN(dlinucb_score_kernel<4>, grid, dim3(DCB_THREADS), lds, (hipStream_t)stream, a);
  } else {
    RG_ALLOW_LDS(dlinucb_score_kernel<2>, lds);
    RG_LAUNCH_DYN(dlinucb_score_kernel<2>, grid, dim3(DCB_THREADS), lds, (hipStream_t)stream, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
