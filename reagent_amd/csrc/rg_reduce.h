// rg_reduce.h — workgroup reductions shared by the loss heads (heads.hip, crr.hip) and by the fused stack's backward and
// weight-gradient launches (mlp_fused.hip, mlp_wgrad.hip: the bias gradients' column reduce and its argument table), and the
// fp64 wave sum and the 256-value LDS tree of the bandit, policy-gradient and SAC files.
#pragma once
#include <rg_platform.h>
#include "../../include/reagent_hip.h"

namespace rg {

// block-wide sum of a 256-thread workgroup in a fixed order (wave shuffles, then the 4 wave sums
// added in order): the same inputs give the same bits on every run
__device__ __forceinline__ float block_sum_256(float v, float* scratch /*[4]*/) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor(v, off);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) scratch[wave] = v;
  __syncthreads();
  const float s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
  __syncthreads();
  return s;
}

// lane ^ off's double, moved as its two words; the sum of a double over the 64 lanes of a wave by butterflies (offsets 32
// down to 1), the same bits in every lane
__device__ __forceinline__ double shfl_xor_f64(double v, int off) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = shfl_xor((int)b, off), hi = shfl_xor((int)(b >> 32), off);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_f64(v, off);
  return v;
}

// A 256-thread workgroup's values vals[threadIdx.x], already written, summed in place by a fixed tree inside every segment
// of SEG consecutive threads: the segment's sum ends in its first slot (visible to all threads on return).
template <int SEG, typename T>
__device__ __forceinline__ void lds_tree_sum(T* vals) {
  const int j = threadIdx.x % SEG;
  __syncthreads();
  for (int off = SEG / 2; off >= 1; off >>= 1) {
    if (j < off) vals[threadIdx.x] += vals[threadIdx.x + off];
    __syncthreads();
  }
}

// this thread's share in[tid], in[tid + 256], ... of a sum over n values, as 16 independent partial sums combined in a fixed
// order: 16 loads in flight per thread.  (One load per loop turn is a chain of n / 256 dependent round trips: ~0.4 us each
// when the chip is busy — 100 us for the 65536 row terms of a C3 step's loss, measured in round 4.)
__device__ __forceinline__ float strided_sum_256(const float* __restrict__ in, int n, int tid) {
  float a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = 0.f;
  int i = tid;
  for (; i + 15 * 256 < n; i += 16 * 256) {
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] += in[i + j * 256];
  }
  for (; i < n; i += 256) a[0] += in[i];
  return (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) +
         (((a[8] + a[9]) + (a[10] + a[11])) + ((a[12] + a[13]) + (a[14] + a[15])));
}

// The same sum over values that are themselves ordered sums of runs: value i = 0 + in[i * run] + in[i * run + 1] + ...
// (`run` terms, those past n_in counting as 0) — the per-wave loss sums of the paired online forward (mlp_fused.hip), whose
// runs of 16 are what dqn_head_lanes_kernel<4> adds, in this order, into one partial per 256 rows.
__device__ __forceinline__ float run_sum(const float* __restrict__ in, int n_in, int run, int i) {
  float s = 0.f;
  for (int w = 0; w < run; ++w) {
    const long j = (long)i * run + w;
    s += j < n_in ? in[j] : 0.f;
  }
  return s;
}
__device__ __forceinline__ float strided_sum_256_runs(const float* __restrict__ in, int n_in, int run, int tid) {
  const int n = (n_in + run - 1) / run;
  float a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = 0.f;
  int i = tid;
  for (; i + 15 * 256 < n; i += 16 * 256) {
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] += run_sum(in, n_in, run, i + j * 256);
  }
  for (; i < n; i += 256) a[0] += run_sum(in, n_in, run, i);
  return (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) +
         (((a[8] + a[9]) + (a[10] + a[11])) + ((a[12] + a[13]) + (a[14] + a[15])));
}

// out[c] = sum_s partials[s][c], S x N row-major: 32 columns x 8 row-groups per workgroup, each
// thread sums rows g, g+8, ... (independent loads in flight), groups combined in fixed order
__device__ __forceinline__ void reduce_cols_body(const float* __restrict__ partials, int S, int N,
                                                 float* __restrict__ out, int block) {
  __shared__ float red[8][33];
  const int c = block * 32 + (threadIdx.x & 31), g = threadIdx.x >> 5;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
  if (c < N) {
    // eight rows in flight per thread: the launch is a chain of dependent HBM round trips (S = 512 rows: 8 rounds)
    int r = g;
    for (; r + 248 < S; r += 256) {  // 32 in flight (round 5), added in the order of four passes of the 8-deep loop below
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = partials[(long)(r + 8 * u) * N + c];
#pragma unroll
      for (int u = 0; u < 32; u += 8) {
        s0 += v[u]; s1 += v[u + 1]; s2 += v[u + 2]; s3 += v[u + 3]; s4 += v[u + 4]; s5 += v[u + 5]; s6 += v[u + 6]; s7 += v[u + 7];
      }
    }
    for (; r + 56 < S; r += 64) {
      s0 += partials[(long)r * N + c];
      s1 += partials[(long)(r + 8) * N + c];
      s2 += partials[(long)(r + 16) * N + c];
      s3 += partials[(long)(r + 24) * N + c];
      s4 += partials[(long)(r + 32) * N + c];
      s5 += partials[(long)(r + 40) * N + c];
      s6 += partials[(long)(r + 48) * N + c];
      s7 += partials[(long)(r + 56) * N + c];
    }
    for (; r < S; r += 8) s0 += partials[(long)r * N + c];
  }
  red[g][threadIdx.x & 31] = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
  __syncthreads();
  if (g == 0 && c < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][threadIdx.x & 31];
    out[c] = t;
  }
}

// bias gradients of every layer in one launch (four ~7 us launches were 4 % of a C2 step)
struct ReduceColsGroupArgs {
  int n;
  int block_begin[RG_MLP_MAX_LAYERS + 1];
  const float* partials[RG_MLP_MAX_LAYERS];
  float* out[RG_MLP_MAX_LAYERS];
  int N[RG_MLP_MAX_LAYERS];
  int S;
};

// every unused slot of a begin-table (prefix sums, one slot per layer / entry and one for the end) gets the end value: the
// kernels' "last i with id >= begin[i]" scans then never pick a slot past the used ones
template <typename T, int N, typename V> static inline void pad_begin_table(T (&begin)[N], int used, V end) {
  for (int i = used; i < N; ++i) begin[i] = (T)end;
}

// the table of one launch: layer l (of n_layers) with partials[l] != null sums its S x N[l] partials into out[l]; returns the
// launch's workgroups (256 threads each)
static inline int fill_reduce_cols(ReduceColsGroupArgs& G, int S, int n_layers, const float* const* partials,
                                   float* const* out, const int* N) {
  G.n = 0; G.S = S;
  int blocks = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (!partials[l]) continue;
    const int i = G.n++;
    G.block_begin[i] = blocks; G.N[i] = N[l];
    G.partials[i] = partials[l]; G.out[i] = out[l];
    blocks += (N[l] + 31) / 32;
  }
  pad_begin_table(G.block_begin, G.n, blocks);
  for (int i = G.n; i < RG_MLP_MAX_LAYERS; ++i) { G.partials[i] = nullptr; G.out[i] = nullptr; G.N[i] = 0; }
  return blocks;
}

}  // namespace rg
