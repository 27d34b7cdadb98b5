// cpe_wsdr.hip — the row and episode arithmetic of the weighted sequential doubly-robust and MAGIC estimators on a sorted,
// device-resident EvaluationDataPage (reagent/evaluation/weighted_sequential_doubly_robust_estimator.py:27-155, 275-353):
//   wsdr_rows_kernel           ratio, state value and logged q of a row, a thread per row
//   wsdr_cumprod_kernel        the cumulative importance weight (:72-73), a lane per episode
//   wsdr_column_sums_kernel    the weight sums of a step over a subset of episodes, a thread per step
//   wsdr_column_totals_kernel  the whole set's sums from the subsets', and the discounts
//   wsdr_returns_kernel        calculate_step_return (:291-343) for every j-step at once, a lane per episode
//   wsdr_sums_kernel, wsdr_cov_kernel   j_step_returns, infinite_step_returns, the mean episode value; np.cov
// The reference pads every episode to the longest and holds [episodes, T, A] cubes; here padding is virtual and nothing of
// size episodes * T is stored.  Like cpe_eval.hip: gather-bound and latency-bound launches, no matrix cores, no atomics, double
// sums added in a fixed order (two runs give the same bits), offsets read from device memory clamped before use.  The
// 25-variable quadratic program over the j-step weights stays on the host.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_reduce.h"  // lds_tree_sum

// every double operation is rounded on its own: the interpreter's and the device's bits are the same statement
#pragma clang fp contract(off)

namespace rg {

constexpr int WSDR_THREADS = 256;
constexpr int WSDR_MAX_J = RG_CPE_WSDR_MAX_J_STEPS;
constexpr int WSDR_MAX_G = RG_CPE_WSDR_MAX_SUBSETS;

// what every launch after the row kernel shares; j_steps and subset_begin travel in the launch arguments
struct WsdrArgs {
  const float* rewards;
  long ld_r;
  const int32_t* offsets;
  int N, E, T, J, G;  // G: the subsets of the column sums (J == 1: even runs covering every episode)
  int self_normalize, want_inf;
  double gamma;
  int32_t j_steps[WSDR_MAX_J];
  int32_t subset_begin[WSDR_MAX_G + 1];
  double *w, *sv, *ql;           // [N]
  double *S_sub, *S_all, *disc;  // [G, T], [T], [T]
  double *inf_ret, *means;       // [E], [J + 1]
  double *ret, *out;             // [J + 1, E]; see rg_cpe_wsdr
};

// episode e is rows [begin, end) of the sorted page: offsets clamped to the page, and an episode to the T steps the column
// sums have
__device__ __forceinline__ void wsdr_span(const int32_t* __restrict__ offsets, int e, int rows, int T, int& begin, int& end) {
  int b = offsets[e], n = offsets[e + 1];
  b = b < 0 ? 0 : (b > rows ? rows : b);
  n = n < b ? b : (n > rows ? rows : n);
  if (n - b > T) n = b + T;
  begin = b;
  end = n;
}

// Thread t of workgroup g has row r = 256 g + t; the three sums over actions run left to right in double (a product of two
// floats is exact in double)
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1)
    wsdr_rows_kernel(const float* __restrict__ prop, const float* __restrict__ mask, const float* __restrict__ mv, long ld_mv,
                     const float* __restrict__ logged_p, int N, int A, double* __restrict__ ratio, double* __restrict__ sv,
                     double* __restrict__ ql) {
  const long r = (long)blockIdx.x * WSDR_THREADS + threadIdx.x;
  if (r >= N) return;
  const float* p = prop + r * A;
  const float* m = mask + r * A;
  const float* v = mv + r * ld_mv;
  double tp = 0.0, s = 0.0, q = 0.0;
  for (int j = 0; j < A; ++j) {
    const double pj = (double)p[j], mj = (double)m[j], vj = (double)v[j];
    tp += pj * mj;
    s += pj * vj;
    q += vj * mj;
  }
  ratio[r] = tp / (double)logged_p[r];
  sv[r] = s;
  ql[r] = q;
}

// w[x] = ratio[begin] * ... * ratio[x], in place
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1)
    wsdr_cumprod_kernel(const int32_t* __restrict__ offsets, int E, int N, int T, double* __restrict__ w) {
  const int e = blockIdx.x * WSDR_THREADS + threadIdx.x;
  if (e >= E) return;
  int begin, end;
  wsdr_span(offsets, e, N, T, begin, end);
  double c = 1.0;
  for (int x = begin; x < end; ++x) {
    c *= w[x];
    w[x] = c;
  }
}

// Workgroup (b, g), thread i: step t = 256 b + i of subset g.  The episode loop is the same in every lane (scalar offsets);
// lanes t, t + 1, ... read neighbouring rows of the episode.
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1) wsdr_column_sums_kernel(const WsdrArgs a) {
  const int t = blockIdx.x * WSDR_THREADS + threadIdx.x, g = blockIdx.y;
  const int e0 = a.subset_begin[g], e1 = a.subset_begin[g + 1];
  double s = 0.0;
  for (int e = e0; e < e1; ++e) {
    int begin, end;
    wsdr_span(a.offsets, e, a.N, a.T, begin, end);
    if (t < end - begin) s += a.w[(long)begin + t];
  }
  if (t < a.T) a.S_sub[(long)g * a.T + t] = s;
}

// Thread per step: S_all[t] = the subsets' sums in subset order, then the episodes before the first and after the last subset
// in episode order; disc[t] = pow(gamma, t)
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1) wsdr_column_totals_kernel(const WsdrArgs a) {
  const int t = blockIdx.x * WSDR_THREADS + threadIdx.x;
  double s = 0.0;
  for (int g = 0; g < a.G; ++g) s += t < a.T ? a.S_sub[(long)g * a.T + t] : 0.0;
  const int first = a.subset_begin[0], last = a.subset_begin[a.G];
  for (int e = 0; e < a.E; ++e) {
    if (e == first) e = last;  // (first <= last; the subsets are contiguous runs between them)
    if (e >= a.E) break;
    int begin, end;
    wsdr_span(a.offsets, e, a.N, a.T, begin, end);
    if (t < end - begin) s += a.w[(long)begin + t];
  }
  if (t < a.T) {
    a.S_all[t] = s;
    a.disc[t] = pow(a.gamma, (double)t);
  }
}

__device__ __forceinline__ double wsdr_weight(double w, double S, double n, int self_normalize) {
  if (!self_normalize) return w / n;
  return S == 0.0 ? 1.0 / n : w / S;
}

// A lane per episode, one walk over its rows carrying the whole-set prefix P, the subset prefix Pg and the episode value.
// ret[j, e] is written at the step its j-step names (or at the episode's last step for a j-step at or beyond it).
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1) wsdr_returns_kernel(const WsdrArgs a) {
  const int e = blockIdx.x * WSDR_THREADS + threadIdx.x;
  if (e >= a.E) return;
  int begin, end;
  wsdr_span(a.offsets, e, a.N, a.T, begin, end);
  const int len = end - begin;
  const double n = (double)a.E;
  int g = -1;
  if (a.want_inf)
    for (int i = 0; i < a.G; ++i)
      if (e >= a.subset_begin[i] && e < a.subset_begin[i + 1]) g = i;
  const double ng = g >= 0 ? (double)(a.subset_begin[g + 1] - a.subset_begin[g]) : 1.0;
  const double* Sg = a.S_sub + (long)(g >= 0 ? g : 0) * a.T;
  double* ret = a.ret + e;
  double P = 0.0, Pg = 0.0, ev = 0.0;
  double wprev = 1.0 / n, wprev_g = 1.0 / ng;
  // a j-step of -1, and every j-step of an episode without rows: the direct-method term of step 0 alone
  {
    const double dm0 = len > 0 ? (a.disc[0] * wprev) * a.sv[begin] : 0.0;
    for (int j = 0; j < a.J; ++j)
      if (a.j_steps[j] < 0 || len == 0) ret[(long)j * a.E] = a.j_steps[j] < 0 ? dm0 : 0.0;
  }
  for (int t = 0; t < len; ++t) {
    const long x = (long)begin + t;
    const double d = a.disc[t], w = a.w[x], r = (double)a.rewards[x * a.ld_r], q = a.ql[x], s = a.sv[x];
    const double wn = wsdr_weight(w, a.S_all[t], n, a.self_normalize);
    P += d * ((wn * r - wn * q) + wprev * s);
    ev += d * r;
    if (g >= 0) {
      const double wg = wsdr_weight(w, Sg[t], ng, a.self_normalize);
      Pg += d * ((wg * r - wg * q) + wprev_g * s);
      wprev_g = wg;
    }
    wprev = wn;
    const bool last = t + 1 == len;
    const double dm = last ? 0.0 : (a.disc[t + 1] * wn) * a.sv[x + 1];
    for (int j = 0; j < a.J; ++j) {
      const int js = a.j_steps[j];
      if (js == t || (last && js > t)) ret[(long)j * a.E] = P + dm;
    }
  }
  ret[(long)a.J * a.E] = ev;
  if (a.want_inf) a.inf_ret[e] = g >= 0 ? Pg : 0.0;
}

// lane i's share x[i], x[i + 256], ... of a sum over [e0, e1) in episode order, then the fixed tree; every lane returns it
__device__ __forceinline__ double wsdr_block_sum(const double* __restrict__ x, int e0, int e1, double* sums) {
  double v = 0.0;
  for (int i = e0 + (int)threadIdx.x; i < e1; i += WSDR_THREADS) v += x[i];
  __syncthreads();  // (the previous use of sums is read)
  sums[threadIdx.x] = v;
  lds_tree_sum<WSDR_THREADS>(sums);
  return sums[0];
}

// Workgroup b < J + 1: the sum of row b of ret (row J: the episode values) and its mean; workgroup J + 1 + g: the sum of
// subset g's inf_ret
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1) wsdr_sums_kernel(const WsdrArgs a) {
  __shared__ double sums[WSDR_THREADS];
  const int b = blockIdx.x;
  if (b <= a.J) {
    const double s = wsdr_block_sum(a.ret + (long)b * a.E, 0, a.E, sums);
    if (threadIdx.x == 0) {
      a.means[b] = s / (double)a.E;
      if (b < a.J) a.out[b] = s;
      else a.out[a.J == 1 ? 1 : a.J + a.G + a.J * a.J] = s / (double)a.E;
    }
  } else {
    const int g = b - (a.J + 1);
    const double s = wsdr_block_sum(a.inf_ret, a.subset_begin[g], a.subset_begin[g + 1], sums);
    if (threadIdx.x == 0) a.out[a.J + g] = s;
  }
}

// Workgroup p is the pair (j, k), k >= j, in row-major order of the upper triangle
__global__ void RG_LAUNCH_BOUNDS(WSDR_THREADS, 1) wsdr_cov_kernel(const WsdrArgs a) {
  __shared__ double sums[WSDR_THREADS];
  int j = 0, p = blockIdx.x;
  while (p >= a.J - j) {
    p -= a.J - j;
    ++j;
  }
  const int k = j + p;
  const double mj = a.means[j], mk = a.means[k];
  const double* rj = a.ret + (long)j * a.E;
  const double* rk = a.ret + (long)k * a.E;
  double v = 0.0;
  for (int i = threadIdx.x; i < a.E; i += WSDR_THREADS) v += (rj[i] - mj) * (rk[i] - mk);
  sums[threadIdx.x] = v;
  lds_tree_sum<WSDR_THREADS>(sums);
  if (threadIdx.x == 0) {
    const double c = sums[0] / (double)(a.E - 1);
    double* C = a.out + a.J + a.G;
    C[(long)j * a.J + k] = c;
    C[(long)k * a.J + j] = c;
  }
}

static inline int wsdr_blocks(int n) { return (n + WSDR_THREADS - 1) / WSDR_THREADS; }

// the subsets the column sums run over: the caller's where J > 1, else min(E, 32) even runs of episodes
static inline int wsdr_column_subsets(int episodes, int J, int G) {
  return J > 1 ? G : (episodes < WSDR_MAX_G ? episodes : WSDR_MAX_G);
}

static inline bool wsdr_sizes_ok(int rows, int episodes, int longest, int J, int G) {
  if (rows < 1 || episodes < 1 || episodes > rows || longest < 1 || longest > rows) return false;
  if (J < 1 || J > WSDR_MAX_J) return false;
  if (J > 1 && (G < 1 || G > WSDR_MAX_G)) return false;
  return true;
}

// the workspace in doubles: w, sv, ql [N]; S_sub [G, T]; S_all, disc [T]; inf_ret [E]; means [J + 1]
static inline size_t wsdr_workspace_doubles(int rows, int episodes, int longest, int J, int G) {
  const size_t Gc = (size_t)wsdr_column_subsets(episodes, J, G);
  return 3 * (size_t)rows + (Gc + 2) * (size_t)longest + (size_t)episodes + (size_t)(J + 1);
}

}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_cpe_wsdr_workspace_bytes(int rows, int episodes, int longest, int num_j_steps, int num_subsets) {
  if (!wsdr_sizes_ok(rows, episodes, longest, num_j_steps, num_subsets)) return 0;
  return sizeof(double) * wsdr_workspace_doubles(rows, episodes, longest, num_j_steps, num_subsets);
}

int rg_cpe_wsdr(const float* model_propensities, const float* action_mask, const float* model_values, int64_t ld_model_values,
                const float* logged_propensities, const float* logged_rewards, int64_t ld_logged_rewards,
                const int32_t* episode_offsets, int rows, int num_actions, int episodes, int longest, double gamma,
                int self_normalize, const int32_t* j_steps, int num_j_steps, const int32_t* subset_offsets, int num_subsets,
                void* workspace, size_t workspace_bytes, double* ret, double* out, rg_stream_t stream) {
  const int J = num_j_steps, G = num_subsets;
  if (!wsdr_sizes_ok(rows, episodes, longest, J, G) || num_actions < 1) return RG_EINVAL;
  if (ld_model_values < num_actions || ld_logged_rewards < 1) return RG_EINVAL;
  if (!model_propensities || !action_mask || !model_values || !logged_propensities || !logged_rewards || !episode_offsets ||
      !j_steps || !workspace || !ret || !out)
    return RG_EINVAL;
  if (J > 1 && !subset_offsets) return RG_EINVAL;
  if (workspace_bytes < sizeof(double) * wsdr_workspace_doubles(rows, episodes, longest, J, G)) return RG_EINVAL;
  WsdrArgs a;
  for (int j = 0; j < WSDR_MAX_J; ++j) {
    a.j_steps[j] = j < J ? j_steps[j] : -1;
    if (j < J && (j_steps[j] < -1 || j_steps[j] > longest - 1)) return RG_EINVAL;
  }
  a.G = wsdr_column_subsets(episodes, J, G);
  if (J > 1) {
    for (int g = 0; g <= G; ++g) {
      const int32_t b = subset_offsets[g];
      if (b < 0 || b > episodes || (g > 0 && b < subset_offsets[g - 1])) return RG_EINVAL;
      a.subset_begin[g] = b;
    }
  } else {
    for (int g = 0; g <= a.G; ++g) a.subset_begin[g] = (int32_t)((long)g * episodes / a.G);
  }
  for (int g = a.G + 1; g <= WSDR_MAX_G; ++g) a.subset_begin[g] = a.subset_begin[a.G];
  a.rewards = logged_rewards, a.ld_r = (long)ld_logged_rewards, a.offsets = episode_offsets;
  a.N = rows, a.E = episodes, a.T = longest, a.J = J;
  a.self_normalize = self_normalize ? 1 : 0, a.want_inf = J > 1 ? 1 : 0, a.gamma = gamma;
  double* ws = (double*)workspace;
  a.w = ws, a.sv = ws + rows, a.ql = ws + 2 * (size_t)rows;
  a.S_sub = ws + 3 * (size_t)rows;
  a.S_all = a.S_sub + (size_t)a.G * longest;
  a.disc = a.S_all + longest;
  a.inf_ret = a.disc + longest;
  a.means = a.inf_ret + episodes;
  a.ret = ret, a.out = out;
  const hipStream_t s = (hipStream_t)stream;
  RG_LAUNCH(wsdr_rows_kernel, dim3(wsdr_blocks(rows)), dim3(WSDR_THREADS), s, model_propensities, action_mask, model_values,
            (long)ld_model_values, logged_propensities, rows, num_actions, a.w, a.sv, a.ql);
  RG_LAUNCH(wsdr_cumprod_kernel, dim3(wsdr_blocks(episodes)), dim3(WSDR_THREADS), s, episode_offsets, episodes, rows, longest,
            a.w);
  RG_LAUNCH(wsdr_column_sums_kernel, dim3(wsdr_blocks(longest), a.G), dim3(WSDR_THREADS), s, a);
  RG_LAUNCH(wsdr_column_totals_kernel, dim3(wsdr_blocks(longest)), dim3(WSDR_THREADS), s, a);
  RG_LAUNCH(wsdr_returns_kernel, dim3(wsdr_blocks(episodes)), dim3(WSDR_THREADS), s, a);
  RG_LAUNCH(wsdr_sums_kernel, dim3(J + 1 + (J > 1 ? G : 0)), dim3(WSDR_THREADS), s, a);
  if (J > 1) RG_LAUNCH(wsdr_cov_kernel, dim3(J * (J + 1) / 2), dim3(WSDR_THREADS), s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
