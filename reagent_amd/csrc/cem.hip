// cem.hip — the cross-entropy-method planner over an ensemble of MDN-RNN world models (reagent/models/cem_planner.py).
//
// The reference evaluates a population of action sequences one trajectory, one step and one module call at a time
// (cem_planner.py:121-215).  The trajectories of an iteration are independent, so here an iteration is a batch: a workgroup
// owns a tile of 32 trajectories of ONE world model for the whole horizon (lstm.hip's shape), the step's input and the
// layers' activations stay in LDS, the layer products run on v_mfma_f32_32x32x2_f32 as k-ordered fp32 chains with the weights
// read in place from the members' parameters, and the gate arithmetic is rg_lstm_cell.h's (double, rounded once).
// gmm_linear is computed in column tiles; a row keeps its reward, its terminal logit, its mixture logits and the mu and
// sigma of the component it sampled, nothing of width (2S + 1)G + 2 lives in LDS.
//
// KEPT QUIRK: the reference calls mem_net(state, action) without a hidden state at every planning step, so h and c are
// ZERO at every step: W_hh contributes nothing, the forget gate multiplies a zero cell, and pre = x W_ih^T + b_ih + b_hh.
// The kernel skips the recurrent product and the forget gate's columns.
//
// rg_cem_group sorts the trajectories by their world model into tiles (a counting sort by one workgroup, in index order),
// rg_cem_sample draws the population, rg_cem_refit selects the elites and refits mean and var, rg_cem_tally is the discrete
// planner's per-first-action mean.  Every kernel returns at once when the planner state's done flag is set, so the host
// enqueues all iterations and reads back once.  No atomics, no flag a workgroup waits on; trip counts depend on the shapes
// alone; a trajectory's bits depend on its model's weights, its solution, the initial state and its own noise only.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"
#include "rg_philox.h"

namespace rg {

constexpr int CEM_THREADS = LSTM_THREADS;
constexpr int CEM_ZT_PITCH = RG_MDN_MAX_GAUSSIANS + 3;  // the mixture logits, the reward, the terminal logit; odd
constexpr int CEM_TN_ATTEMPTS = 32;
enum { CEM_DRAW_MODEL = 0, CEM_DRAW_MIX = 1, CEM_DRAW_TERM = 2, CEM_DRAW_EPS = 3, CEM_DRAW_TN = 4, CEM_DRAW_ACTION = 5 };

// ---- the noise recipe (include/reagent_hip.h states it) ----------------------------------------------------------------
__device__ __forceinline__ void cem_draw(uint64_t seed, int kind, int iteration, long n, uint32_t hi, uint32_t lo,
                                         uint32_t (&x)[4]) {
  // the key goes through vector registers: as a scalar the compiler would park the ten rounds' key schedule in scalar
  // registers for the whole kernel
  const uint64_t key = (uint64_t)(uint32_t)opaque((int)(uint32_t)seed) | ((uint64_t)(uint32_t)opaque((int)(uint32_t)(seed >> 32)) << 32);
  philox4x32_10(key, (uint64_t)n | ((uint64_t)(uint32_t)iteration << 20) | ((uint64_t)kind << 52), ((uint64_t)hi << 32) | lo, x);
}
__device__ __forceinline__ float cem_uniform(uint64_t seed, int kind, int iteration, long n, uint32_t hi, uint32_t lo) {
  uint32_t x[4];
  cem_draw(seed, kind, iteration, n, hi, lo, x);
  return (float)(x[0] >> 8) * 0x1p-24f;
}
// ln and cos(2 pi u) in double with their constants read from LDS, for the reason lstm_exp reads its own from there: the
// library's keep dozens of 64-bit constants that the compiler parks in scalar registers for the whole kernel.  nz: 1/3, 1/5,
// ..., 1/15 (the atanh series), sqrt(1/2), pi/2.  ec is lstm_exp's table: ec[1] + ec[2] = ln 2, ec[16 - n] = 1 / n!.
constexpr int CEM_NZ_COEFS = 9;
__device__ __forceinline__ void cem_noise_table(double* nz) {  // by one thread, before the workgroup's first barrier
  for (int k = 0; k < 7; ++k) nz[k] = 1.0 / (double)(2 * k + 3);
  nz[7] = 7.07106781186547524401e-01;
  nz[8] = 1.57079632679489661923e+00;
}
// ln x for a positive normal x: x = m 2^e with m in [sqrt(1/2), sqrt(2)), ln m = 2 atanh((m - 1) / (m + 1)) by its series to
// s^15 (|s| <= 0.172: the next term is under 4e-14 of the sum)
__device__ __forceinline__ double cem_log(double x, const double* ec, const double* nz) {
  int e;
  double m = frexp(x, &e);
  if (m < nz[7]) m *= 2.0, e -= 1;
  const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
  double p = nz[6];
#pragma unroll
  for (int k = 5; k >= 0; --k) p = fma(p, s2, nz[k]);
  const double lm = 2.0 * fma(p * s2, s, s);
  return fma((double)e, ec[1], fma((double)e, ec[2], lm));
}
// cos(2 pi u) for u in [0, 1): 4 u = q + r with q an integer and |r| <= 1/2 (exact), x = r pi / 2, and cos(q pi / 2 + x) is
// cos x, -sin x, -cos x or sin x by their series to x^12 and x^13 (|x| <= pi / 4: the next terms are under 4e-13)
__device__ __forceinline__ double cem_cos2pi(double u, const double* ec, const double* nz) {
  const double t = 4.0 * u, q = rint(t), x = (t - q) * nz[8], x2 = x * x;
  double c = ec[4], sn = ec[3];  // 1 / 12!, 1 / 13!
#pragma unroll
  for (int n = 10; n >= 2; n -= 2) c = fma(-c, x2, ec[16 - n]), sn = fma(-sn, x2, ec[15 - n]);
  c = fma(-c, x2, 1.0);
  sn = x * fma(-sn, x2, 1.0);
  const int qi = (int)q & 3;
  const double v = (qi & 1) ? sn : c;
  return (qi == 1 || qi == 2) ? -v : v;
}
// Box-Muller in double on two uniforms of one draw: u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ double cem_normal(uint64_t seed, int kind, int iteration, long n, uint32_t hi, uint32_t lo,
                                             const double* ec, const double* nz) {
  uint32_t x[4];
  cem_draw(seed, kind, iteration, n, hi, lo, x);
  const double u1 = ((double)x[0] + 1.0) * 0x1p-32, u2 = (double)x[1] * 0x1p-32;
  return sqrt(-2.0 * cem_log(u1, ec, nz)) * cem_cos2pi(u2, ec, nz);
}
__device__ __forceinline__ bool cem_done(const double* done) { return done && done[0] != 0.0; }
// floor(u * count) of a uniform in [0, 1), in double (exact); anything else reads as 0
__device__ __forceinline__ int cem_pick(float u, int count) {
  return (u >= 0.f && u < 1.f) ? (int)((double)u * (double)count) : 0;
}
// lstm_exp keeps a NaN (its clamp would drop it)
__device__ __forceinline__ double cem_exp(double x, const double* ec) { return x != x ? x : lstm_exp(x, ec); }

__global__ void cem_fill_noise_kernel(uint64_t seed, int iteration, int N, int T, int S, float* __restrict__ u_model,
                                      float* __restrict__ u_mix, float* __restrict__ eps, float* __restrict__ u_term) {
  __shared__ double ec[LSTM_EXP_COEFS], nz[CEM_NZ_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec), cem_noise_table(nz);
  __syncthreads();
  const long e = (long)blockIdx.x * CEM_THREADS + threadIdx.x;
  if (e >= (long)T * N * S) return;
  const int s = (int)(e % S);
  const long jn = e / S;
  const int n = (int)(jn % N), j = (int)(jn / N);
  eps[e] = (float)cem_normal(seed, CEM_DRAW_EPS, iteration, n, j, s, ec, nz);
  if (s == 0) {
    u_mix[jn] = cem_uniform(seed, CEM_DRAW_MIX, iteration, n, j, 0);
    u_term[jn] = cem_uniform(seed, CEM_DRAW_TERM, iteration, n, j, 0);
    if (j == 0) u_model[n] = cem_uniform(seed, CEM_DRAW_MODEL, iteration, n, 0, 0);
  }
}

// ---- grouping by world model --------------------------------------------------------------------------------------------
struct CemGroupArgs {
  const float* u_model;
  const double* done;
  int *rowmap, *tile_model;
  uint64_t seed;
  int iteration, N, M, tiles;
};

__device__ __forceinline__ int cem_model_of(const CemGroupArgs& a, int n) {
  const float u = a.u_model ? a.u_model[n] : cem_uniform(a.seed, CEM_DRAW_MODEL, a.iteration, n, 0, 0);
  return cem_pick(u, a.M);
}

// One workgroup: thread t owns the trajectories [t * chunk, (t + 1) * chunk).  Model m's trajectories fill, in index order,
// the tiles from start[m] on; a model's last tile is padded with -1, a model nobody drew gets no tile.
__global__ void RG_LAUNCH_BOUNDS(CEM_THREADS, 1) cem_group_kernel(const CemGroupArgs a) {
  __shared__ int cnt[CEM_THREADS * RG_CEM_MAX_MODELS];
  __shared__ int start[RG_CEM_MAX_MODELS + 1];
  if (cem_done(a.done)) return;
  const int t = threadIdx.x, M = a.M, N = a.N;
  const int chunk = (N + CEM_THREADS - 1) / CEM_THREADS;
  const int lo = t * chunk < N ? t * chunk : N, hi = lo + chunk < N ? lo + chunk : N;
  int* mine = cnt + t * RG_CEM_MAX_MODELS;
  for (int m = 0; m < RG_CEM_MAX_MODELS; ++m) mine[m] = 0;
  for (int n = lo; n < hi; ++n) mine[cem_model_of(a, n)] += 1;
  __syncthreads();
  if (t == 0) {
    int tile = 0;
    for (int m = 0; m < M; ++m) {
      start[m] = tile;
      int c = 0;
      for (int tt = 0; tt < CEM_THREADS; ++tt) {
        const int v = cnt[tt * RG_CEM_MAX_MODELS + m];
        cnt[tt * RG_CEM_MAX_MODELS + m] = c;
        c += v;
      }
      tile += (c + LSTM_ROWS - 1) / LSTM_ROWS;
    }
    for (int m = M; m <= RG_CEM_MAX_MODELS; ++m) start[m] = tile;
  }
  __syncthreads();
  for (int e = t; e < a.tiles * LSTM_ROWS; e += CEM_THREADS) a.rowmap[e] = -1;
  for (int e = t; e < a.tiles; e += CEM_THREADS) {
    int m = -1;
    for (int mm = 0; mm < M; ++mm)
      if (e >= start[mm] && e < start[mm + 1]) m = mm;
    a.tile_model[e] = m;
  }
  __syncthreads();
  for (int n = lo; n < hi; ++n) {
    const int m = cem_model_of(a, n);
    a.rowmap[start[m] * LSTM_ROWS + mine[m]] = n;
    mine[m] += 1;
  }
}

// ---- the rollout --------------------------------------------------------------------------------------------------------
struct CemRolloutArgs {
  const float* const* table;  // [M][3 L + 2]: per layer W_ih, b_ih, b_hh; gmm_linear's weight and bias
  const int *rowmap, *tile_model;
  const float* init_state;
  const void* pop;  // solutions [P, T, A] fp32, or (discrete) action indices [P, T] int32
  const float* gamma_pow;
  const float *u_mix, *eps, *u_term;
  const double* done;
  double* traj;
  float* trace;  // per (step, trajectory) a row of S + W + 2 floats: the entry state, z, the sampled index, not_terminal
  uint64_t seed;
  int iteration, N, E, T, S, A, G, H, L, terminal_effective, discrete;
};

constexpr int CEM_STAGE_PITCH = LSTM_TILE + 1;
// floats per (step, trajectory) row of the trace: the entry state, z [(2S + 1)G + 2], the sampled index, not_terminal
__device__ __forceinline__ int cem_trace_width(int S, int G) { return S + (2 * S + 1) * G + 4; }

// one 32 x 32 tile of src [32 rows, K] (LDS, pitch) times the rows of w starting at wrow (global, K floats each, one row per
// lane's column): the k-ordered chain; a masked column multiplies zeros
__device__ __forceinline__ f32x16 cem_tile(const float* src, int pitch, int K, int Kp, const float* wrow, bool col_ok, int col,
                                           int half) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
  for (int k = 0; k < Kp; k += 2) {
    const int kk = k + half;
    const bool ok = col_ok && kk < K;
    const float bv = wrow[kk < K ? kk : 0];
    acc = mfma_32x32x2_f32(src[col * pitch + kk], ok ? bv : 0.f, acc);
  }
  return acc;
}

__global__ void RG_LAUNCH_BOUNDS(CEM_THREADS, 1) cem_rollout_kernel(const CemRolloutArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS], nz[CEM_NZ_COEFS];
  __shared__ float zt[LSTM_ROWS * CEM_ZT_PITCH];
  __shared__ float stage_s[LSTM_WAVES * LSTM_ROWS * CEM_STAGE_PITCH];
  __shared__ int k_s[LSTM_ROWS], n_s[LSTM_ROWS];
  // the arguments the per-element code reads (pointers of the population, the noise, the trace ...) are read from an LDS copy
  // where they are used: as kernel arguments they, their null tests and their widened indices would sit in scalar registers
  // for the whole kernel, more than a wave has
  __shared__ CemRolloutArgs sa;
  if (cem_done(a.done)) return;
  const int model = a.tile_model[blockIdx.x];
  if (model < 0) return;
  if (threadIdx.x == 0) lstm_exp_table(ec), cem_noise_table(nz), sa = a;
  const int H = a.H, Hp = (a.H + LSTM_TILE - 1) / LSTM_TILE * LSTM_TILE, S = a.S, A = a.A, G = a.G, In = a.S + a.A, Inp = In + (In & 1), L = a.L;
  const int pitch_x = Inp + 1, pitch_h = Hp + 1, tiles = Hp / LSTM_TILE, GS = G * S;
  float* xs = (float*)smem;
  float* hbuf0 = xs + LSTM_ROWS * pitch_x;
  float* hbuf1 = hbuf0 + LSTM_ROWS * pitch_h;
  const float* const* tab = a.table + model * (3 * L + 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  float* stage = stage_s + wave * LSTM_ROWS * CEM_STAGE_PITCH;
  if (threadIdx.x < LSTM_ROWS) n_s[threadIdx.x] = a.rowmap[blockIdx.x * LSTM_ROWS + threadIdx.x];
  for (int e = threadIdx.x; e < LSTM_ROWS * pitch_x; e += CEM_THREADS) {
    const int c = e % pitch_x;
    xs[e] = (c >= A && c < In) ? a.init_state[c - A] : 0.f;
  }
  double acc_reward = 0.0;  // of row threadIdx.x, in the first 32 threads
  bool alive = true;
  for (int j = 0; j < a.T; ++j) {
    __syncthreads();  // the step before has written its next states; n_s and the exp table are there
    const int in_v = sa.S + sa.A;  // (In from LDS: the division below stays in vector registers)
    for (int e = threadIdx.x; e < LSTM_ROWS * in_v; e += CEM_THREADS) {
      const int r = e / in_v, c = e - r * in_v, n = n_s[r];
      if (c < sa.A) {
        float v = 0.f;
        if (n >= 0) {
          const long at = (long)(n / sa.E) * sa.T + j;
          v = sa.discrete ? (((const int*)sa.pop)[at] == c ? 1.f : 0.f) : ((const float*)sa.pop)[at * sa.A + c];
        }
        xs[r * pitch_x + c] = v;
      } else if (sa.trace && n >= 0) {
        sa.trace[((long)j * sa.N + n) * cem_trace_width(sa.S, sa.G) + (c - sa.A)] = xs[r * pitch_x + c];
      }
    }
    __syncthreads();
    // the LSTM layers from a zero state: i, g, o of W_ih alone
    const float* src = xs;
    int K = In, Kp = Inp, pitch = pitch_x;
    float* dst = hbuf0;
    for (int l = 0; l < L; ++l) {
      const float *w_ih = tab[3 * l], *b_ih = tab[3 * l + 1], *b_hh = tab[3 * l + 2];
      for (int tile = wave; tile < tiles; tile += LSTM_WAVES) {
        const int u = tile * LSTM_TILE + col;
        const bool u_ok = u < H;
        const int uc = u_ok ? u : H - 1;
        const LstmGates p = lstm_gate_products<false>(src, pitch, w_ih, H, K, Kp, uc, u_ok, col, half);
        const double bi0 = (double)b_ih[uc], bi1 = (double)b_hh[uc];
        const double bg0 = (double)b_ih[2 * H + uc], bg1 = (double)b_hh[2 * H + uc];
        const double bo0 = (double)b_ih[3 * H + uc], bo1 = (double)b_hh[3 * H + uc];
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
          const f32x4 qi = lstm_acc_quad(p.i, q), qg = lstm_acc_quad(p.g, q), qo = lstm_acc_quad(p.o, q);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int rl = lstm_acc_row(4 * q + jj, half);
            const double gi = lstm_sigmoid(((double)qi[jj] + bi0) + bi1, ec);
            const double gg = lstm_tanh(((double)qg[jj] + bg0) + bg1, ec);
            const double go = lstm_sigmoid(((double)qo[jj] + bo0) + bo1, ec);
            const float c = (float)(gi * gg);  // f * 0 + i * g
            const float h = (float)(go * lstm_tanh((double)c, ec));
            dst[rl * pitch_h + u] = u_ok ? h : 0.f;
          }
        }
      }
      __syncthreads();
      src = dst, K = H, Kp = Hp, pitch = pitch_h;
      dst = dst == hbuf0 ? hbuf1 : hbuf0;
    }
    // gmm_linear in three phases of column tiles: the last G + 2 columns (the mixture logits, the reward, the terminal
    // logit) and the rows' decisions; the mu columns; the sigma columns.  A wave stages its tile's z in LDS and each lane
    // then walks one row's 16 columns: a row keeps its sampled component's mu, then its next state, written over its state.
    const float* wg = tab[3 * L];
    const float* bg = tab[3 * L + 1];
    for (int phase = 0; phase < 3; ++phase) {
      const int base = phase == 0 ? 2 * GS : (phase == 1 ? 0 : GS);
      const int width = phase == 0 ? G + 2 : GS;
      for (int tile = wave; tile * LSTM_TILE < width; tile += LSTM_WAVES) {
        const int ct = tile * LSTM_TILE + col;
        const bool ok = ct < width;
        const int c = base + (ok ? ct : 0);
        const f32x16 acc = cem_tile(src, pitch, K, Kp, wg + c * H, ok, col, half);  // (W H floats below 2^24)
        const float b = bg[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[lstm_acc_row(r, half) * CEM_STAGE_PITCH + col] = __fadd_rn(acc[r], b);
        wave_lds_sync();
        const int rl = col, n = n_s[rl], nc = n < 0 ? 0 : n, k = k_s[rl];
        const long jn = (long)j * sa.N + nc;
        const int tw = cem_trace_width(sa.S, sa.G);
#pragma unroll 1
        for (int i = 0; i < LSTM_TILE / 2; ++i) {
          const int cl = 2 * i + half, cw = tile * LSTM_TILE + cl;
          if (cw < width) {
            const float z = stage[rl * CEM_STAGE_PITCH + cl];
            if (sa.trace && n >= 0) sa.trace[jn * tw + sa.S + base + cw] = z;
            if (phase == 0) {
              zt[rl * CEM_ZT_PITCH + cw] = z;
            } else {
              const int comp = cw / sa.S, s = cw - comp * sa.S;
              if (comp == k) {
                float* x = xs + rl * pitch_x + sa.A + s;
                if (phase == 1) {
                  *x = z;
                } else {
                  const double e = sa.eps ? (double)sa.eps[jn * sa.S + s] : (double)(float)cem_normal(sa.seed, CEM_DRAW_EPS, sa.iteration, nc, j, s, ec, nz);
                  *x = (float)((double)*x + cem_exp((double)z, ec) * e);
                }
              }
            }
          }
        }
        wave_lds_sync();
      }
      __syncthreads();
      if (phase == 0) {
        if (threadIdx.x < LSTM_ROWS) {
          const int r = threadIdx.x, n = n_s[r], nc = n < 0 ? 0 : n;
          const long jn = (long)j * sa.N + nc;
          const int tw = cem_trace_width(sa.S, sa.G);
          const float* z = zt + r * CEM_ZT_PITCH;
          double m = -(double)INFINITY;
          for (int g = 0; g < G; ++g) m = fmax(m, (double)z[g]);
          double se = 0.0;
          for (int g = 0; g < G; ++g) se += cem_exp((double)z[g] - m, ec);
          const double u = sa.u_mix ? (double)sa.u_mix[jn] : (double)cem_uniform(sa.seed, CEM_DRAW_MIX, sa.iteration, nc, j, 0);
          double cum = 0.0;
          int k = 0;
          for (int g = 0; g < G; ++g) {
            cum += cem_exp((double)z[g] - m, ec) / se;
            k += cum <= u ? 1 : 0;
          }
          k = k < G ? k : G - 1;
          int nt = 1;
          if (sa.terminal_effective) {
            const double ut = sa.u_term ? (double)sa.u_term[jn] : (double)cem_uniform(sa.seed, CEM_DRAW_TERM, sa.iteration, nc, j, 0);
            const double logit = (double)z[G + 1];
            nt = (logit == logit && ut < lstm_sigmoid(logit, ec)) ? 1 : 0;
          }
          if (alive) acc_reward += (double)__fmul_rn(z[G], sa.gamma_pow[j]);
          if (!nt) alive = false;
          k_s[r] = k;
          if (sa.trace && n >= 0) sa.trace[jn * tw + tw - 2] = (float)k, sa.trace[jn * tw + tw - 1] = (float)nt;
        }
        __syncthreads();
      }
    }
  }
  if (threadIdx.x < LSTM_ROWS && n_s[threadIdx.x] >= 0) sa.traj[n_s[threadIdx.x]] = acc_reward;
}

// the mean over a solution's E trajectories, in double and in index order
__global__ void cem_ensemble_mean_kernel(const double* __restrict__ traj, const double* done, int P, int E, double* __restrict__ out) {
  if (cem_done(done)) return;
  const int p = blockIdx.x * CEM_THREADS + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int e = 0; e < E; ++e) s += traj[(long)p * E + e];
  out[p] = s / (double)E;
}

// ---- the population -----------------------------------------------------------------------------------------------------
// np.minimum: a NaN wins
__device__ __forceinline__ double cem_npmin(double a, double b) { return (a != a || b != b) ? (a != a ? a : b) : fmin(a, b); }

__global__ void cem_sample_kernel(const double* __restrict__ ps, const double* __restrict__ lower, const double* __restrict__ upper,
                                  const double* __restrict__ tn_in, uint64_t seed, int iteration, int P, int D,
                                  double* __restrict__ sol, float* __restrict__ sol32) {
#pragma clang fp contract(off)
  __shared__ double ec[LSTM_EXP_COEFS], nz[CEM_NZ_COEFS];
  if (cem_done(ps + 2 * D)) return;
  if (threadIdx.x == 0) lstm_exp_table(ec), cem_noise_table(nz);
  __syncthreads();
  const long e = (long)blockIdx.x * CEM_THREADS + threadIdx.x;
  if (e >= (long)P * D) return;
  const int p = (int)(e / D), d = (int)(e % D);
  double tn;
  if (tn_in) {
    tn = tn_in[e];
  } else {
    bool got = false;
    tn = 0.0;
    for (int t = 0; t < CEM_TN_ATTEMPTS; ++t) {
      tn = cem_normal(seed, CEM_DRAW_TN, iteration, p, d, t, ec, nz);
      if (fabs(tn) <= 2.0) {
        got = true;
        break;
      }
    }
    if (!got) tn = fmin(fmax(tn, -2.0), 2.0);
  }
  const double m = ps[d], v = ps[D + d];
  const double lb = (m - lower[d]) / 2.0, ub = (upper[d] - m) / 2.0;
  const double cv = cem_npmin(cem_npmin(lb * lb, ub * ub), v);
  const double x = tn * sqrt(cv) + m;
  sol[e] = x;
  sol32[e] = (float)x;
}

__global__ void cem_sample_discrete_kernel(uint64_t seed, int iteration, int P, int T, int A, int* __restrict__ actions) {
  const long e = (long)blockIdx.x * CEM_THREADS + threadIdx.x;
  if (e >= (long)P * T) return;
  actions[e] = cem_pick(cem_uniform(seed, CEM_DRAW_ACTION, iteration, e / T, (uint32_t)(e % T), 0), A);
}

// ---- the refit ----------------------------------------------------------------------------------------------------------
// numpy's sort order as an unsigned key: ascending numbers (-0 and +0 equal), every NaN above them
__device__ __forceinline__ uint64_t cem_key(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) x = 0.0;
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// the sum of v over the workgroup, in every thread
__device__ __forceinline__ int cem_block_sum(int v, int* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < LSTM_WAVES; ++w) s += red[w];
  return s;
}

struct CemRefitArgs {
  const double *rewards, *sol;
  double* ps;  // mean [D], var [D], done, iterations run
  int* flags;  // [P]
  double alpha, epsilon;
  int P, D, elites;
};

// One workgroup.  The elites are the last `elites` entries of np.argsort(rewards): the threshold key is found bit by bit
// (64 counting passes), the ties at the threshold go to the highest indices.  Then a thread per dimension: mean and
// population variance over the elites in solution-index order, the update, and the done flag.
__global__ void RG_LAUNCH_BOUNDS(CEM_THREADS, 1) cem_refit_kernel(const CemRefitArgs a) {
#pragma clang fp contract(off)
  __shared__ int red[LSTM_WAVES];
  __shared__ int tie_s[CEM_THREADS];
  const int P = a.P, D = a.D, t = threadIdx.x;
  double* st = a.ps + 2 * D;
  if (st[0] != 0.0) return;
  uint64_t thr = 0;
  int remaining = a.elites;
  for (int b = 63; b >= 0; --b) {
    const uint64_t want = (thr >> b) | 1ull;
    int c = 0;
    for (int p = t; p < P; p += CEM_THREADS) c += (cem_key(a.rewards[p]) >> b) == want ? 1 : 0;
    c = cem_block_sum(c, red);
    if (c >= remaining) thr |= 1ull << b;
    else remaining -= c;
  }
  const int chunk = (P + CEM_THREADS - 1) / CEM_THREADS;
  const int lo = t * chunk < P ? t * chunk : P, hi = lo + chunk < P ? lo + chunk : P;
  int ties = 0;
  for (int p = lo; p < hi; ++p) ties += cem_key(a.rewards[p]) == thr ? 1 : 0;
  tie_s[t] = ties;
  __syncthreads();
  int seen = 0;  // the ties at higher indices than this thread's chunk
  for (int tt = t + 1; tt < CEM_THREADS; ++tt) seen += tie_s[tt];
  for (int p = hi - 1; p >= lo; --p) {
    const uint64_t k = cem_key(a.rewards[p]);
    int f = k > thr ? 1 : 0;
    if (k == thr) {
      f = seen < remaining ? 1 : 0;
      seen += 1;
    }
    a.flags[p] = f;
  }
  __syncthreads();
  const double ne = (double)a.elites;
  int open = 0;
  for (int d = t; d < D; d += CEM_THREADS) {
    double s = 0.0;
    for (int p = 0; p < P; ++p)
      if (a.flags[p]) s += a.sol[(long)p * D + d];
    const double nm = s / ne;
    double s2 = 0.0;
    for (int p = 0; p < P; ++p)
      if (a.flags[p]) {
        const double dd = a.sol[(long)p * D + d] - nm;
        s2 += dd * dd;
      }
    const double nv = s2 / ne;
    const double m = a.alpha * a.ps[d] + (1.0 - a.alpha) * nm;
    const double v = a.alpha * a.ps[D + d] + (1.0 - a.alpha) * nv;
    a.ps[d] = m, a.ps[D + d] = v;
    open += v <= a.epsilon ? 0 : 1;  // (a NaN keeps it open, as np.max(var) <= epsilon does)
  }
  open = cem_block_sum(open, red);
  if (t == 0) {
    st[1] += 1.0;
    if (open == 0) st[0] = 1.0;
  }
}

// ---- the discrete tally -------------------------------------------------------------------------------------------------
// out [3 A + 1]: per first action the count, the sum of the accumulated rewards in index order and their quotient; then
// np.nanargmax of the quotients (-1: all NaN)
__global__ void RG_LAUNCH_BOUNDS(CEM_THREADS, 1) cem_tally_kernel(const int* __restrict__ actions, int T, const double* __restrict__ rewards,
                                                                 int P, int A, double* __restrict__ out) {
  for (int c = threadIdx.x; c < A; c += CEM_THREADS) {
    double cnt = 0.0, s = 0.0;
    for (int p = 0; p < P; ++p)
      if (actions[(long)p * T] == c) cnt += 1.0, s += rewards[p];
    out[c] = cnt, out[A + c] = s, out[2 * A + c] = s / cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = -1;
    double bv = 0.0;
    for (int c = 0; c < A; ++c) {
      const double q = out[2 * A + c];
      if (q == q && (best < 0 || q > bv)) best = c, bv = q;
    }
    out[3 * A] = (double)best;
  }
}

static int cem_shape_check(int S, int A, int G, int H, int L) {
  if (S < 1 || A < 1 || G < 1 || H < 1 || L < 1) return RG_EINVAL;
  if (H > RG_LSTM_MAX_HIDDEN || L > RG_LSTM_MAX_LAYERS || G > RG_MDN_MAX_GAUSSIANS || S + A > RG_CEM_MAX_INPUT) return RG_EUNSUPPORTED;
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_cem_fill_noise(uint64_t seed, int iteration, int trajectories, int horizon, int state_dim, float* u_model, float* u_mix,
                      float* eps, float* u_term, rg_stream_t stream) {
  if (iteration < 0 || trajectories < 1 || horizon < 1 || state_dim < 1) return RG_EINVAL;
  if (trajectories >= RG_CEM_MAX_TRAJECTORIES || horizon > RG_CEM_MAX_HORIZON || state_dim > RG_CEM_MAX_INPUT) return RG_EUNSUPPORTED;
  if (!u_model || !u_mix || !eps || !u_term) return RG_EINVAL;
  const long n = (long)horizon * trajectories * state_dim;
  RG_LAUNCH(cem_fill_noise_kernel, dim3((unsigned)((n + CEM_THREADS - 1) / CEM_THREADS)), dim3(CEM_THREADS), (hipStream_t)stream,
            seed, iteration, trajectories, horizon, state_dim, u_model, u_mix, eps, u_term);
  return (int)hipGetLastError();
}

int rg_cem_rollout_tiles(int trajectories, int models) {
  if (trajectories < 1 || models < 1) return 0;
  return trajectories / LSTM_ROWS + models;
}

int rg_cem_group(const float* u_model, uint64_t seed, int iteration, int trajectories, int models, const double* done,
                 int* rowmap, int* tile_model, rg_stream_t stream) {
  if (iteration < 0 || trajectories < 1 || models < 1) return RG_EINVAL;
  if (trajectories >= RG_CEM_MAX_TRAJECTORIES || models > RG_CEM_MAX_MODELS) return RG_EUNSUPPORTED;
  if (!rowmap || !tile_model) return RG_EINVAL;
  CemGroupArgs a;
  a.u_model = u_model, a.done = done, a.rowmap = rowmap, a.tile_model = tile_model, a.seed = seed;
  a.iteration = iteration, a.N = trajectories, a.M = models, a.tiles = rg_cem_rollout_tiles(trajectories, models);
  RG_LAUNCH(cem_group_kernel, dim3(1), dim3(CEM_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

size_t rg_cem_rollout_lds_bytes(int state_dim, int action_dim, int hidden) {
  if (state_dim < 1 || action_dim < 1 || hidden < 1) return 0;
  const int in = state_dim + action_dim, inp = in + (in & 1);
  return ((size_t)LSTM_ROWS * (inp + 1) + 2 * lstm_tile_floats(hidden)) * sizeof(float);
}

int rg_cem_rollout(const float* const* table, int models, const int* rowmap, const int* tile_model, int tiles,
                   const float* init_state, const float* solutions, const int* action_idx, const float* gamma_pow,
                   const float* u_mix, const float* eps, const float* u_term, uint64_t seed, int iteration, const double* done,
                   int population, int ensemble, int horizon, int state_dim, int action_dim, int num_gaussians, int hidden,
                   int layers, int terminal_effective, double* traj, double* out, float* trace, rg_stream_t stream) {
  const int rc = cem_shape_check(state_dim, action_dim, num_gaussians, hidden, layers);
  if (rc != RG_OK) return rc;
  if (models < 1 || tiles < 1 || population < 1 || ensemble < 1 || horizon < 1 || iteration < 0) return RG_EINVAL;
  const int64_t n = (int64_t)population * ensemble;
  if (models > RG_CEM_MAX_MODELS || horizon > RG_CEM_MAX_HORIZON || n >= RG_CEM_MAX_TRAJECTORIES) return RG_EUNSUPPORTED;
  if (!table || !rowmap || !tile_model || !init_state || !gamma_pow || !out) return RG_EINVAL;
  if ((solutions == nullptr) == (action_idx == nullptr)) return RG_EINVAL;  // one form of the population
  if (ensemble > 1 && !traj) return RG_EINVAL;
  CemRolloutArgs a;
  a.table = table, a.rowmap = rowmap, a.tile_model = tile_model, a.init_state = init_state;
  a.pop = solutions ? (const void*)solutions : (const void*)action_idx, a.discrete = solutions ? 0 : 1;
  a.gamma_pow = gamma_pow, a.u_mix = u_mix, a.eps = eps, a.u_term = u_term, a.done = done;
  a.traj = ensemble > 1 ? traj : out, a.trace = trace;
  a.seed = seed, a.iteration = iteration, a.N = (int)n, a.E = ensemble, a.T = horizon, a.S = state_dim, a.A = action_dim;
  a.G = num_gaussians, a.H = hidden, a.L = layers, a.terminal_effective = terminal_effective;
  const size_t lds = rg_cem_rollout_lds_bytes(state_dim, action_dim, hidden);
  RG_ALLOW_LDS(cem_rollout_kernel, lds);
  RG_LAUNCH_DYN(cem_rollout_kernel, dim3(tiles), dim3(CEM_THREADS), lds, (hipStream_t)stream, a);
  if (ensemble > 1)
    RG_LAUNCH(cem_ensemble_mean_kernel, dim3((population + CEM_THREADS - 1) / CEM_THREADS), dim3(CEM_THREADS), (hipStream_t)stream,
              (const double*)traj, done, population, ensemble, out);
  return (int)hipGetLastError();
}

int rg_cem_sample(const double* planner_state, const double* lower, const double* upper, const double* tn, uint64_t seed,
                  int iteration, int population, int dims, double* solutions, float* solutions_f32, rg_stream_t stream) {
  if (population < 1 || dims < 1 || iteration < 0) return RG_EINVAL;
  if (population >= RG_CEM_MAX_TRAJECTORIES) return RG_EUNSUPPORTED;
  if (!planner_state || !lower || !upper || !solutions || !solutions_f32) return RG_EINVAL;
  const long n = (long)population * dims;
  RG_LAUNCH(cem_sample_kernel, dim3((unsigned)((n + CEM_THREADS - 1) / CEM_THREADS)), dim3(CEM_THREADS), (hipStream_t)stream,
            planner_state, lower, upper, tn, seed, iteration, population, dims, solutions, solutions_f32);
  return (int)hipGetLastError();
}

int rg_cem_sample_discrete(uint64_t seed, int iteration, int population, int horizon, int action_dim, int* actions,
                           rg_stream_t stream) {
  if (population < 1 || horizon < 1 || action_dim < 1 || iteration < 0) return RG_EINVAL;
  if (population >= RG_CEM_MAX_TRAJECTORIES || horizon > RG_CEM_MAX_HORIZON) return RG_EUNSUPPORTED;
  if (!actions) return RG_EINVAL;
  const long n = (long)population * horizon;
  RG_LAUNCH(cem_sample_discrete_kernel, dim3((unsigned)((n + CEM_THREADS - 1) / CEM_THREADS)), dim3(CEM_THREADS),
            (hipStream_t)stream, seed, iteration, population, horizon, action_dim, actions);
  return (int)hipGetLastError();
}

int rg_cem_refit(const double* rewards, const double* solutions, int population, int dims, int num_elites, double alpha,
                 double epsilon, double* planner_state, int* flags, rg_stream_t stream) {
  if (population < 1 || dims < 1 || num_elites < 1 || num_elites > population) return RG_EINVAL;
  if (population >= RG_CEM_MAX_TRAJECTORIES) return RG_EUNSUPPORTED;
  if (!rewards || !solutions || !planner_state || !flags) return RG_EINVAL;
  CemRefitArgs a;
  a.rewards = rewards, a.sol = solutions, a.ps = planner_state, a.flags = flags, a.alpha = alpha, a.epsilon = epsilon;
  a.P = population, a.D = dims, a.elites = num_elites;
  RG_LAUNCH(cem_refit_kernel, dim3(1), dim3(CEM_THREADS), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_cem_tally(const int* actions, int horizon, const double* rewards, int population, int action_dim, double* out,
                 rg_stream_t stream) {
  if (population < 1 || horizon < 1 || action_dim < 1) return RG_EINVAL;
  if (population >= RG_CEM_MAX_TRAJECTORIES) return RG_EUNSUPPORTED;
  if (!actions || !rewards || !out) return RG_EINVAL;
  RG_LAUNCH(cem_tally_kernel, dim3(1), dim3(CEM_THREADS), (hipStream_t)stream, actions, horizon, rewards, population, action_dim,
            out);
  return (int)hipGetLastError();
}

}  // extern "C"
