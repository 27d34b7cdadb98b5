// cb_solve.hip — rg_linucb_solve_blocked: the ridge solve of LinearRegressionUCB on device-resident state for every LinUCB
// width (1 <= d <= 512), where rg_linucb_solve (cb_deep.hip) keeps the matrix in one workgroup's registers and stops at 128.
// A blocked Cholesky route in 32 x 32 blocks, n = ceil(d / 32) block columns, on three P x P matrices (P = 32 n) of the
// workspace: A (A_ext padded with the identity), LT = L^T (A_ext = L L^T) and W = L^-1.  n + 3 ordinary launches on the
// stream, each depending on the one before through the stream's order alone — no cooperative launch, no flag a workgroup
// waits on, no atomics:
//   fold     elementwise: reduce_avg in the reference's fp32 order, A_ext into the workspace
//   column k (k = 0 .. n - 1), n workgroups.  EVERY workgroup forms S_kk = A_kk - sum_{j<k} L_kj L_kj^T, factors it
//            (L_kk, unblocked) and inverts the factor (W_kk, by substitution) for itself in LDS: the block is on every
//            workgroup's path anyway, and a launch of its own for it would cost more than the repeated arithmetic.  Then
//            workgroup g >  k: the panel block L_gk = (A_gk - sum_{j<k} L_gj L_kj^T) W_kk^T
//            workgroup g == k: stores L_kk and W_kk, raises the status flag
//            workgroup g <  k: row k of the block substitution, W_kg = -W_kk sum_{g<=j<k} L_kj W_jg
//            (left-looking: the trailing update of a block is the sum it is read with)
//   inverse  one workgroup per tile on or above the diagonal: inv_IJ = sum_{j>=J} W_jI^T W_jJ, stored and mirrored
//   finish   coefs = inv_avg_A * avg_b, a wave per row; the scalars of the fold
// Every block product runs on v_mfma_f32_32x32x2_f32 (mfma_32x32x2_f32 of rg_platform.h), its 2-row steps dealt to the four
// waves in turn and the four partial tiles added in wave order: the trip counts depend on d alone, two runs give the
// same bits.  LT and W are stored so that the summed index is the row: every operand read is 128 contiguous bytes a half wave.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_cb.h"  // CB_THREADS, CB_WAVES, CB_TILE, the upper-triangle tile numbering

// The fold is held to the reference's fp32 operation order: every multiply, divide and add is rounded on its own.  Where a
// fused multiply-add is wanted (the factorisation, the dots) it is written out as fmaf.
#pragma clang fp contract(off)

namespace rg {

constexpr int SB = CB_TILE;        // the block: one MFMA output tile
constexpr int SB_LD = SB + 1;      // a block's pitch in LDS: rows and columns are both read conflict-free
constexpr int SB_ROWS = CB_THREADS / SB;  // thread t owns column t & 31 of the rows (t >> 5) + 8 m, m < 4, of a block
constexpr int SB_PER = SB / SB_ROWS;
static_assert(SB_ROWS * SB_PER == SB && SB * SB == CB_TILE_ELEMS, "block layout");

struct BlockedArgs {
  int d, P, n, k;
  float lambda;
  float *avg_A, *avg_b, *sum_weight;
  int64_t* num_obs;
  float *cur_avg_A, *cur_avg_b, *cur_sum_weight;
  int64_t* cur_num_obs;
  float *inv_avg_A, *coefs, *valid;
  int32_t* status;
  float *A, *LT, *W;  // the workspace's three P x P matrices
};

// The four waves' share of X^T Y over the rows [row0, row1) (multiples of 32) of two row-major matrices of pitch ld, of
// which pa and pb point at the first column of a 32-column block: step s is the rows 2 s, 2 s + 1 (lane l: row l >> 5,
// column l & 31 of both operands), wave w takes the steps w, w + 4, ... — (row1 - row0) / 8 of them, whatever the wave.
// SB_AHEAD steps' operands are loaded together, from addresses clamped into the range (no branch around a load), and the
// steps past the range's end are skipped whole (uniform over the wave): the latency of a load is paid once per 16 steps.
constexpr int SB_AHEAD = 16;
__device__ __forceinline__ f32x16 rows_dot(const float* pa, const float* pb, int ld, int row0, int row1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int r0 = row0 + 2 * wave; r0 < row1; r0 += 2 * CB_WAVES * SB_AHEAD) {
    float xa[SB_AHEAD], xb[SB_AHEAD];
#pragma unroll
    for (int u = 0; u < SB_AHEAD; ++u) {
      const int r = r0 + 2 * CB_WAVES * u;
      const long at = (long)((r < row1 ? r : r0) + half) * ld + col;
      xa[u] = pa[at], xb[u] = pb[at];
    }
#pragma unroll
    for (int u = 0; u < SB_AHEAD; ++u)
      if (r0 + 2 * CB_WAVES * u < row1) acc = mfma_32x32x2_f32(xa[u], xb[u], acc);
  }
  return acc;
}

// The same share of X Y for two blocks in LDS: x(i, t) and y(t, j) are entry (i, t) of X and (t, j) of Y, t < 32.
template <typename FX, typename FY>
__device__ __forceinline__ f32x16 block_dot(FX x, FY y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < SB / (2 * CB_WAVES); ++s) {
    const int t = 2 * (wave + CB_WAVES * s) + half;
    acc = mfma_32x32x2_f32(x(col, t), y(t, col), acc);
  }
  return acc;
}

// The four waves' tiles meet in LDS and are added in wave order: out[m] is entry ((t >> 5) + 8 m, t & 31) of the sum.
// (The barrier in front: whoever still reads `parts`, or the LDS blocks the product was taken from, has finished.)
__device__ __forceinline__ void merge_tiles(float (*parts)[CB_TILE_ELEMS], const f32x16& acc, float (&out)[SB_PER]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) parts[wave][cb_acc_row(r, lane >> 5) * SB + (lane & 31)] = acc[r];
  __syncthreads();
#pragma unroll
  for (int m = 0; m < SB_PER; ++m) {
    const int e = threadIdx.x + CB_THREADS * m;
    out[m] = ((parts[0][e] + parts[1][e]) + parts[2][e]) + parts[3][e];
  }
}

// reduce_avg (:54-89), one process, and A_ext: thread e of P * P + d owns entry (e / P, e % P) of the padded matrix, or
// past those entry e - P * P of the vector.  The one-element buffers are read here and rewritten by the finishing launch.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_blocked_fold_kernel(const BlockedArgs a) {
  const int e = (int)blockIdx.x * CB_THREADS + threadIdx.x;
  const int d = a.d, P = a.P, PP = P * P;
  if (e >= PP + d) return;
  const float sw = *a.sum_weight, cw = *a.cur_sum_weight;
  const float total = cw + sw;
  if (e >= PP) {
    const int i = e - PP;
    a.avg_b[i] = (a.avg_b[i] * sw + a.cur_avg_b[i] * cw) / total;
    a.cur_avg_b[i] = 0.f;
    return;
  }
  const int i = e / P, j = e % P;
  float v = i == j ? 1.f : 0.f;
  if (i < d && j < d) {
    const float reg = (a.lambda * 1.f) / total;  // l2_reg_lambda * eye / sum_weight on the diagonal
    const long at = (long)i * d + j;
    const float avg = (a.avg_A[at] * sw + a.cur_avg_A[at] * cw) / total;
    a.avg_A[at] = avg;
    a.valid[at] = avg;
    a.cur_avg_A[at] = 0.f;
    v = i == j ? avg + reg : avg;
  }
  a.A[e] = v;
}

// Block column k (see the head of the file).  Only the lower triangle of A is read.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_blocked_column_kernel(const BlockedArgs a) {
  __shared__ float parts[CB_WAVES][CB_TILE_ELEMS];
  __shared__ float S[SB * SB_LD], Lk[SB * SB_LD], Wk[SB * SB_LD], T[SB * SB_LD];
  const int t = threadIdx.x, tx = t & (SB - 1), ty = t >> 5;
  const int P = a.P, k = a.k, g = (int)blockIdx.x;
  const int k0 = SB * k, g0 = SB * g;
  float v[SB_PER];
  // S_kk = A_kk - sum_{j<k} L_kj L_kj^T
  merge_tiles(parts, rows_dot(a.LT + k0, a.LT + k0, P, 0, k0), v);
#pragma unroll
  for (int m = 0; m < SB_PER; ++m) {
    const int i = ty + SB_ROWS * m;
    S[i * SB_LD + tx] = a.A[(long)(k0 + i) * P + k0 + tx] - v[m];
  }
  // L_kk, right-looking and unblocked: step p divides column p by the root of its pivot and takes its outer product off
  // the entries to the right of and below it.  Column p is not written in step p: one barrier a step.  A pivot that is not
  // positive or not finite raises the flag and the arithmetic goes on.
  int bad = 0;
  for (int p = 0; p < SB; ++p) {
    __syncthreads();
    const float piv = S[p * SB_LD + p];
    if (!(piv > 0.f && piv <= 3.4028234663852886e38f)) bad = 1;
    const float root = sqrtf(piv);
    const float lj = S[tx * SB_LD + p] / root;
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) {
      const int i = ty + SB_ROWS * m;
      const float li = S[i * SB_LD + p] / root;
      if (i > p && tx > p) S[i * SB_LD + tx] = fmaf(-li, lj, S[i * SB_LD + tx]);
      if (tx == p) Lk[i * SB_LD + p] = i > p ? li : (i == p ? root : 0.f);
    }
  }
  __syncthreads();
  // W_kk = L_kk^-1 by forward substitution, lane q < 32 of wave 0 column q (the column in registers under compile-time
  // indices): w_i = (delta_iq - sum_{t<i} L_it w_t) / L_ii, which is an exact 0 above the diagonal
  if (t < SB) {
    float w[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < i; ++u) s = fmaf(Lk[i * SB_LD + u], w[u], s);
      w[i] = ((i == t ? 1.f : 0.f) - s) / Lk[i * SB_LD + i];
      Wk[i * SB_LD + t] = w[i];
    }
  }
  __syncthreads();
  if (g == k) {  // (uniform over the workgroup, like the two branches below)
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) {
      const int i = ty + SB_ROWS * m;
      a.LT[(long)(k0 + i) * P + k0 + tx] = Lk[tx * SB_LD + i];
      a.W[(long)(k0 + i) * P + k0 + tx] = Wk[i * SB_LD + tx];
    }
    if (t == 0 && bad) *a.status = 1;
  } else if (g > k) {
    // S_gk = A_gk - sum_{j<k} L_gj L_kj^T, then L_gk^T = W_kk S_gk^T: row c, column i of it is entry (k0 + c, g0 + i) of LT
    merge_tiles(parts, rows_dot(a.LT + g0, a.LT + k0, P, 0, k0), v);
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) {
      const int i = ty + SB_ROWS * m;
      T[i * SB_LD + tx] = a.A[(long)(g0 + i) * P + k0 + tx] - v[m];
    }
    __syncthreads();
    merge_tiles(parts, block_dot([&](int c, int u) { return Wk[c * SB_LD + u]; }, [&](int u, int i) { return T[i * SB_LD + u]; }),
                v);
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) a.LT[(long)(k0 + ty + SB_ROWS * m) * P + g0 + tx] = v[m];
  } else {
    // W_kg = -W_kk sum_{g<=j<k} L_kj W_jg
    merge_tiles(parts, rows_dot(a.LT + k0, a.W + g0, P, g0, k0), v);
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) T[(ty + SB_ROWS * m) * SB_LD + tx] = v[m];
    __syncthreads();
    merge_tiles(parts, block_dot([&](int i, int u) { return Wk[i * SB_LD + u]; }, [&](int u, int q) { return T[u * SB_LD + q]; }),
                v);
#pragma unroll
    for (int m = 0; m < SB_PER; ++m) a.W[(long)(k0 + ty + SB_ROWS * m) * P + g0 + tx] = -v[m];
  }
}

// inv_avg_A = W^T W: workgroup t the tile (I, J), I <= J, of rg_cb.h's numbering, inv_IJ = sum_{j>=J} W_jI^T W_jJ.  The
// entries on or above the diagonal are stored to both sides of it: an exactly symmetric inverse.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_blocked_inverse_kernel(const BlockedArgs a) {
  __shared__ float parts[CB_WAVES][CB_TILE_ELEMS];
  const int tx = threadIdx.x & (SB - 1), ty = threadIdx.x >> 5;
  const int d = a.d, P = a.P;
  int I, J;
  cb_tile_of((int)blockIdx.x, a.n, I, J);
  float v[SB_PER];
  merge_tiles(parts, rows_dot(a.W + SB * I, a.W + SB * J, P, SB * J, P), v);
#pragma unroll
  for (int m = 0; m < SB_PER; ++m) {
    const int i = SB * I + ty + SB_ROWS * m, j = SB * J + tx;
    if (i <= j && j < d) {
      a.inv_avg_A[(long)i * d + j] = v[m];
      a.inv_avg_A[(long)j * d + i] = v[m];
    }
  }
}

// coefs = inv_avg_A * avg_b: a wave per row, lane l the columns l, l + 64, ..., the 64 sums by butterflies.  Thread 0 of
// workgroup 0 finishes the fold's one-element buffers.
__global__ void RG_LAUNCH_BOUNDS(CB_THREADS, 1) linucb_blocked_finish_kernel(const BlockedArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = a.d, i = (int)blockIdx.x * CB_WAVES + wave;
  const int row = i < d ? i : d - 1;  // a wave past the last row repeats it and writes nothing
  float s = 0.f;
  for (int j = lane; j < d; j += 64) s = fmaf(a.inv_avg_A[(long)row * d + j], a.avg_b[j], s);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += shfl_xor(s, off);
  if (lane == 0 && i < d) a.coefs[i] = s;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float total = *a.cur_sum_weight + *a.sum_weight;
    *a.sum_weight = total;
    *a.cur_sum_weight = 0.f;
    *a.num_obs += *a.cur_num_obs;
    *a.cur_num_obs = 0;
  }
}

static int blocked_blocks(int dim) { return (dim + SB - 1) / SB; }

}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_linucb_solve_blocked_workspace_bytes(int dim) {
  if (dim < 1 || dim > RG_LINUCB_MAX_DIM) return 0;
  const size_t P = (size_t)SB * blocked_blocks(dim);
  return 3 * P * P * sizeof(float);
}

int rg_linucb_solve_blocked(int dim, double l2_reg_lambda, float* avg_A, float* avg_b, float* sum_weight, int64_t* num_obs,
                            float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs,
                            float* inv_avg_A, float* coefs, float* coefs_valid_for_avg_A, int32_t* status, void* workspace,
                            size_t workspace_bytes, rg_stream_t stream) {
  if (dim < 1 || dim > RG_LINUCB_MAX_DIM) return RG_EINVAL;
  if (!avg_A || !avg_b || !sum_weight || !num_obs || !cur_avg_A || !cur_avg_b || !cur_sum_weight || !cur_num_obs ||
      !inv_avg_A || !coefs || !coefs_valid_for_avg_A || !status || !workspace)
    return RG_EINVAL;
  if (workspace_bytes < rg_linucb_solve_blocked_workspace_bytes(dim) || ((uintptr_t)workspace & 3)) return RG_EINVAL;
  BlockedArgs a;
  a.d = dim, a.n = blocked_blocks(dim), a.P = SB * a.n, a.k = 0, a.lambda = (float)l2_reg_lambda;
  a.avg_A = avg_A, a.avg_b = avg_b, a.sum_weight = sum_weight, a.num_obs = num_obs;
  a.cur_avg_A = cur_avg_A, a.cur_avg_b = cur_avg_b, a.cur_sum_weight = cur_sum_weight, a.cur_num_obs = cur_num_obs;
  a.inv_avg_A = inv_avg_A, a.coefs = coefs, a.valid = coefs_valid_for_avg_A, a.status = status;
  a.A = (float*)workspace, a.LT = a.A + (size_t)a.P * a.P, a.W = a.LT + (size_t)a.P * a.P;
  const dim3 block(CB_THREADS);
  const hipStream_t s = (hipStream_t)stream;
  RG_LAUNCH(linucb_blocked_fold_kernel, dim3((a.P * a.P + dim + CB_THREADS - 1) / CB_THREADS), block, s, a);
  for (a.k = 0; a.k < a.n; ++a.k) RG_LAUNCH(linucb_blocked_column_kernel, dim3(a.n), block, s, a);
  RG_LAUNCH(linucb_blocked_inverse_kernel, dim3(cb_tiles(a.n)), block, s, a);
  RG_LAUNCH(linucb_blocked_finish_kernel, dim3((dim + CB_WAVES - 1) / CB_WAVES), block, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
