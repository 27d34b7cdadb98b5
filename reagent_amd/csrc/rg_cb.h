// rg_cb.h — what the contextual-bandit kernel files share.  cb.hip (one regression for all arms) and cb_disjoint.hip (one per
// arm) accumulate the same weighted Gram matrix, S_A = X^T diag(w) X with S_b = X^T (w o y), over different cuts of the
// batch: the walk over a slice's rows, the merge of the four waves and the ordered sum over the slices' partials are here
// once, and so are the upper-triangle tile numbering, the accumulator's row map, the half-wave sum and the masked arg-max
// rule of the two scorers.  cb_deep.hip takes the launch constants.  Which rows make a slice is each file's own plan: where
// the slices are cut decides the bits.
#pragma once
#include <rg_platform.h>

namespace rg {

constexpr int CB_THREADS = 256;
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_TILE = 32;  // the MFMA's 32 x 32 output tile
constexpr int CB_TILE_ELEMS = CB_TILE * CB_TILE;

constexpr int cb_tiles_1d(int d) { return (d + CB_TILE - 1) / CB_TILE; }
constexpr int cb_tiles(int tiles_1d) { return tiles_1d * (tiles_1d + 1) / 2; }  // tiles on or above the diagonal

// The tiles on or above the diagonal are numbered row by row: t -> (ti, tj), ti <= tj, and back.
__device__ __forceinline__ void cb_tile_of(int t, int tiles_1d, int& ti, int& tj) {
  int row = 0, first = 0;
  while (t >= first + (tiles_1d - row)) first += tiles_1d - row, ++row;
  ti = row, tj = row + (t - first);
}
__device__ __forceinline__ int cb_tile_index(int ti, int tj, int tiles_1d) {
  return ti * tiles_1d - ti * (ti - 1) / 2 + (tj - ti);
}

// row of the 32 x 32 tile that acc[r] holds in a lane of half `half` = lane >> 5 (its column is lane & 31: rg_platform.h)
__device__ __forceinline__ int cb_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// sum over the 32 lanes of a half wave, the same bits in each of them
__device__ __forceinline__ float cb_half_wave_sum(float v) {
  v += shfl_xor(v, 1);
  v += shfl_xor(v, 2);
  v += shfl_xor(v, 4);
  v += shfl_xor(v, 8);
  v += shfl_xor(v, 16);
  return v;
}

// The masked arg-max's rule: torch.argmax of the scores with every absent arm's score replaced by -inf, which is what the
// reference's masked argmax computes (tests/golden/cb/argmax_nonfinite.npz holds its answers).  The lowest index among
// equals, the first present NaN before any number, and arm 0 where nothing beats -inf (no arm present, or every present
// arm at -inf): a present -inf is worth what an absent arm is, and is passed over like one.  take() is called with the arms
// in rising order; past a NaN nothing changes (closed).  (Written as a skip, not as a start from v = -inf: that form, one
// register shorter, made hipcc spill two VGPRs in dlinucb_score_kernel<4>, which sits at 256.)
struct CbBest {
  float v = 0.f;
  int arm = 0;
  bool found = false, closed = false;
  __device__ __forceinline__ void take(float u, int k, bool present) {
    if (closed || !present || u == -INFINITY) return;
    if (!found || u != u || u > v) v = u, arm = k, found = true;
    if (u != u) closed = true;
  }
};

// Where the batch rows of a Gram launch lie: batch row r reads row r of x, or with `action` the chosen arm's row
// r * arms + clamp(action[r]) of x [B, arms, d]; y[r] and weight[r] (NULL: ones) are the batch row's own.
struct CbRows {
  const float *x, *y, *weight;
  const int64_t* action;
  int arms;
};

// One workgroup's tile (ti, tj), ti <= tj, of the Gram matrix over the batch rows [row_begin, row_end).  Each wave walks its
// share two rows a step (rows 2 * wave + 8 * step + {0, 1}): lane l holds row k = l >> 5 of the step and column l & 31 of
// both tiles, A[i][k] = w_k * x[k][32 ti + i] and B[k][j] = x[k][32 tj + j] in the fragment maps of rg_platform.h, read
// straight from global memory (128 contiguous bytes per half wave), UNROLL steps' operands together from addresses clamped
// into the range (no branch around a load) and zeroed at use.  A diagonal tile adds S_b's share from the registers it holds
// anyway, SUM_W the sum of weights.  The four waves' tiles meet in LDS and are added in wave order: gram_out [32 * 32], on a
// diagonal tile sb_out [32], and sw_out [1] unless NULL.  An empty range writes zeros.
template <int UNROLL, bool SUM_W>
__device__ __forceinline__ void cb_gram_tile(const CbRows& src, long row_begin, long row_end, int d, int ti, int tj,
                                             float* gram_out, float* sb_out, float* sw_out) {
#pragma clang fp contract(off)  // S_b's (w * y) * x is two multiplies and an add, whatever the including file has set
  __shared__ float tile[CB_WAVES][CB_TILE_ELEMS];
  __shared__ float vec[CB_WAVES][64];
  __shared__ float wsum[SUM_W ? CB_WAVES : 1][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int ca = ti * CB_TILE + col, cb = tj * CB_TILE + col;
  const bool ca_ok = ca < d, cb_ok = cb < d;
  const int cac = ca_ok ? ca : d - 1, cbc = cb_ok ? cb : d - 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float sb = 0.f, sw = 0.f;
  for (long r0 = row_begin + 2 * wave; r0 < row_end; r0 += 2 * CB_WAVES * UNROLL) {  // (wave-uniform trip count)
    float wv[UNROLL], yv[UNROLL], xa[UNROLL], xb[UNROLL];
    bool live[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long row = r0 + 2 * CB_WAVES * u + half;
      live[u] = row < row_end;
      const long rc = live[u] ? row : row_end - 1;  // (row_begin <= r0 <= row_end - 1: a row of this range)
      long xr = rc;
      if (src.action) {  // the index clamped into [0, arms)
        const long arm = src.action[rc];
        xr = rc * src.arms + (arm < 0 ? 0 : (arm >= src.arms ? src.arms - 1 : arm));
      }
      wv[u] = src.weight ? src.weight[rc] : 1.f;
      yv[u] = src.y[rc];
      xa[u] = src.x[xr * d + cac];
      xb[u] = src.x[xr * d + cbc];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      // (uniform over the wave: the steps past the range's end are skipped whole, a half step has its dead row zeroed)
      if (r0 + 2 * CB_WAVES * u < row_end) {
        const float w = live[u] ? wv[u] : 0.f;
        const float va = (live[u] && ca_ok) ? xa[u] : 0.f;
        const float vb = (live[u] && cb_ok) ? xb[u] : 0.f;
        const float wy = w * (live[u] ? yv[u] : 0.f);
        acc = mfma_32x32x2_f32(w * va, vb, acc);
        sb += wy * va;
        if (SUM_W) sw += w;
      }
    }
  }
  float* mine = tile[wave];
#pragma unroll
  for (int r = 0; r < 16; ++r) mine[cb_acc_row(r, half) * CB_TILE + col] = acc[r];
  vec[wave][lane] = sb;
  if (SUM_W && col == 0) wsum[wave][half] = sw;
  __syncthreads();
  for (int e = threadIdx.x; e < CB_TILE_ELEMS; e += CB_THREADS)
    gram_out[e] = ((tile[0][e] + tile[1][e]) + tile[2][e]) + tile[3][e];
  if (ti == tj && threadIdx.x < CB_TILE) {
    float v = 0.f;
#pragma unroll
    for (int wv = 0; wv < CB_WAVES; ++wv) v = (v + vec[wv][threadIdx.x]) + vec[wv][threadIdx.x + 32];
    sb_out[threadIdx.x] = v;
  }
  if (SUM_W && sw_out && threadIdx.x == 0) {
    float v = 0.f;
#pragma unroll
    for (int wv = 0; wv < CB_WAVES; ++wv) v = (v + wsum[wv][0]) + wsum[wv][1];
    *sw_out = v;
  }
}

// The finishing side.  Thread e of d * d + d owns entry (i, j) = (e / d, e % d) of the matrix A, or past those entry
// e - d * d of the vector b.  Below the diagonal there is nothing to do: the thread of (j, i) writes both entries (an
// exactly symmetric matrix whatever was there).  Else S is the sum of the entry's partials over the slices, in slice order
// (gram [slices][tiles][32 * 32], sb [slices][tiles_1d * 32]), `at` the entry's index in A or b and `mirror` that of its
// twin (the entry itself on the diagonal and in b): the caller stores its update of the entry to both.
struct CbEntry {
  bool below, in_A;
  float S;
  long at, mirror;
};
__device__ __forceinline__ CbEntry cb_finish_entry(long e, int d, int tiles_1d, int tiles, int slices, const float* gram,
                                                   const float* sb) {
  const long dd = (long)d * d;
  CbEntry en = {false, e < dd, 0.f, e, e};
  if (en.in_A) {
    const int i = (int)(e / d), j = (int)(e % d);
    en.below = i > j;
    if (en.below) return en;
    const int t = cb_tile_index(i / CB_TILE, j / CB_TILE, tiles_1d);
    const size_t off = (size_t)t * CB_TILE_ELEMS + (i % CB_TILE) * CB_TILE + (j % CB_TILE);
    for (int s = 0; s < slices; ++s) en.S += gram[(size_t)s * tiles * CB_TILE_ELEMS + off];
    en.mirror = (long)j * d + i;
  } else {
    en.at = en.mirror = e - dd;
    for (int s = 0; s < slices; ++s) en.S += sb[(size_t)s * tiles_1d * CB_TILE + en.at];
  }
  return en;
}

}  // namespace rg
