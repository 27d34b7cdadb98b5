// lstm.hip — one nn.LSTM layer over a whole sequence, forward and backward (the world model's recurrence, reagent/models/
// mdn_rnn.py:32-36, 72).  The recurrence couples hidden units but never batch rows, so a workgroup owns a tile of 32 batch
// rows for all T steps: one launch per layer and direction, no cooperative launch, no flag a workgroup waits on, no
// atomics.  The tile's h_{t-1} (forward), or d loss / d h and d loss / d c carried back from step t + 1 (backward), live in
// LDS; the four waves split the hidden units in tiles of 32 and a wave holds the i, f, g, o accumulators of the same 32
// units, so the cell update needs no exchange.  Products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation in k order); the gate arithmetic (sigmoid, tanh, the cell update and their derivatives) runs in double on the
// fp32 accumulators and is rounded once where it is stored.  Trip counts depend on H alone, a row's bits on that row alone.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_lstm_cell.h"  // the tile shape, lstm_gate_products / lstm_gates / lstm_cell, lstm_tanh, lstm_acc_row / lstm_acc_quad

namespace rg {

struct LstmFwdArgs {
  const float *xproj, *w_hh, *b_hh, *h0, *c0;
  float *h_all, *c_all, *gates;
  int T, B, H, Hp;
};

// Step t of a row tile: pre = xproj[t] + b_hh + h_{t-1} * W_hh^T, (i, f, o) = sigmoid, g = tanh, c_t = f * c_{t-1} + i * g,
// h_t = o * tanh(c_t).  h_{t-1} is read from one LDS image (pitch Hp + 1: the A fragment's 32 rows fall on 32 banks) while
// h_t is written to the other; units and rows past the end hold zeros there, so the K loop runs over Hp for every tile.
// c_{t-1} is what this same thread stored to c_all one step earlier (its own store: no fence needed).
__global__ void RG_LAUNCH_BOUNDS(LSTM_THREADS, 1) lstm_forward_kernel(const LstmFwdArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  const int H = a.H, Hp = a.Hp, B = a.B, pitch = Hp + 1, tiles = Hp / LSTM_TILE;
  float* cur = (float*)smem;
  float* nxt = cur + LSTM_ROWS * pitch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * LSTM_ROWS;
  for (int e = threadIdx.x; e < LSTM_ROWS * Hp; e += LSTM_THREADS) {
    const int r = e / Hp, u = e % Hp;
    const long row = row0 + r;
    cur[r * pitch + u] = (a.h0 && row < B && u < H) ? a.h0[row * H + u] : 0.f;
  }
  __syncthreads();
  for (int t = 0; t < a.T; ++t) {
    for (int tile = wave; tile < tiles; tile += LSTM_WAVES) {
      const int u = tile * LSTM_TILE + col;
      const bool u_ok = u < H;
      const int uc = u_ok ? u : H - 1;
      const LstmGates p = lstm_gate_products(cur, pitch, a.w_hh, H, H, Hp, uc, u_ok, col, half);
      double bias[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) bias[g] = a.b_hh ? (double)a.b_hh[g * H + uc] : 0.0;
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {  // four rows at a time: the double arithmetic below is compiled once, not sixteen times
        const f32x4 qi = lstm_acc_quad(p.i, q), qf = lstm_acc_quad(p.f, q), qg = lstm_acc_quad(p.g, q), qo = lstm_acc_quad(p.o, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rl = lstm_acc_row(4 * q + j, half);
          const long row = row0 + rl;
          const bool ok = u_ok && row < B;
          const long rowc = row < B ? row : B - 1;  // (addresses stay inside the arrays; the values are dropped)
          const long at = ((long)t * B + rowc) * H + uc;
          const float* xp = a.xproj + ((long)t * B + rowc) * 4 * H + uc;
          LstmCell e = lstm_gates(qi[j], qf[j], qg[j], qo[j], xp, H, bias, ec);
          const float cp = t == 0 ? (a.c0 ? a.c0[rowc * H + uc] : 0.f) : a.c_all[at - (long)B * H];
          lstm_cell(e, cp, ec);
          if (ok) {
            a.h_all[at] = e.h;
            a.c_all[at] = e.c;
            if (a.gates) {
              float* gp = a.gates + ((long)t * B + row) * 4 * H + u;
              gp[0] = (float)e.gi, gp[H] = (float)e.gf, gp[2 * H] = (float)e.gg, gp[3 * H] = (float)e.go;
            }
          }
          nxt[rl * pitch + u] = ok ? e.h : 0.f;
        }
      }
    }
    __syncthreads();
    float* s = cur;
    cur = nxt, nxt = s;
  }
}

struct LstmBwdArgs {
  const float *dh_all, *gates, *c_all, *c0, *w_hh;
  float *dgates, *dh0, *dc0;
  int T, B, H, Hp;
};

// Step t of a row tile, from the last step down.  Per element: dh = dh_all[t] + dh_rec, d_o = dh * tanh(c_t), dc = dc_next +
// dh * o * (1 - tanh(c_t)^2), d_i = dc * g, d_f = dc * c_{t-1}, d_g = dc * i, dc_next = dc * f, each times its gate's
// derivative: dgates[t] = d loss / d pre-activation.  Then dh_rec = dgates[t] * W_hh (K = 4H): the operand tile is 32 x 4H
// fp32, 128 KB at H = 256, so it is staged one gate (32 x H) at a time from the dgates rows the workgroup has just written
// (its own stores, after a barrier).  W_hh is read in place: lane n of the B fragment reads row k's element n (coalesced).
__global__ void RG_LAUNCH_BOUNDS(LSTM_THREADS, 1) lstm_backward_kernel(const LstmBwdArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double ec[LSTM_EXP_COEFS];
  if (threadIdx.x == 0) lstm_exp_table(ec);
  const int H = a.H, Hp = a.Hp, B = a.B, pitch = Hp + 1, tiles = Hp / LSTM_TILE;
  float* dhrec = (float*)smem;
  float* dc = dhrec + LSTM_ROWS * pitch;
  float* stage = dc + LSTM_ROWS * pitch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  const long row0 = (long)blockIdx.x * LSTM_ROWS;
  for (int e = threadIdx.x; e < LSTM_ROWS * pitch; e += LSTM_THREADS) dhrec[e] = 0.f, dc[e] = 0.f;
  __syncthreads();
  for (int t = a.T - 1; t >= 0; --t) {
    for (int e = threadIdx.x; e < LSTM_ROWS * Hp; e += LSTM_THREADS) {
      const int r = e / Hp, u = e % Hp;
      const long row = row0 + r;
      if (row < B && u < H) {
        const long at = ((long)t * B + row) * H + u;
        const long gat = ((long)t * B + row) * 4 * H + u;
        const double gi = a.gates[gat], gf = a.gates[gat + H], gg = a.gates[gat + 2 * H], go = a.gates[gat + 3 * H];
        const double cp = t == 0 ? (a.c0 ? (double)a.c0[row * H + u] : 0.0) : (double)a.c_all[at - (long)B * H];
        const double tc = lstm_tanh((double)a.c_all[at], ec);
        const double dh = (double)a.dh_all[at] + (double)dhrec[r * pitch + u];
        const double dct = (double)dc[r * pitch + u] + dh * go * (1.0 - tc * tc);
        dc[r * pitch + u] = (float)(dct * gf);
        a.dgates[gat] = (float)(dct * gg * gi * (1.0 - gi));
        a.dgates[gat + H] = (float)(dct * cp * gf * (1.0 - gf));
        a.dgates[gat + 2 * H] = (float)(dct * gi * (1.0 - gg * gg));
        a.dgates[gat + 3 * H] = (float)(dh * tc * go * (1.0 - go));
      }
    }
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    for (int gate = 0; gate < 4; ++gate) {
      for (int e = threadIdx.x; e < LSTM_ROWS * Hp; e += LSTM_THREADS) {
        const int r = e / Hp, u = e % Hp;
        const long row = row0 + r;
        stage[r * pitch + u] = (row < B && u < H) ? a.dgates[((long)t * B + row) * 4 * H + gate * H + u] : 0.f;
      }
      __syncthreads();
      const float* w = a.w_hh + (long)gate * H * H;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int tile = wave + q * LSTM_WAVES;
        if (tile < tiles) {  // (wave-uniform; at most 2 * LSTM_WAVES tiles: H <= RG_LSTM_MAX_HIDDEN)
          const int n = tile * LSTM_TILE + col;
          const bool n_ok = n < H;
          const int nc = n_ok ? n : H - 1;
#pragma unroll 4
          for (int k = 0; k < Hp; k += 2) {
            const int kk = k + half;
            const bool ok = n_ok && kk < H;
            const float bv = w[(long)(kk < H ? kk : 0) * H + nc];
            acc[q] = mfma_32x32x2_f32(stage[col * pitch + kk], ok ? bv : 0.f, acc[q]);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int tile = wave + q * LSTM_WAVES;
      if (tile < tiles) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dhrec[lstm_acc_row(r, half) * pitch + tile * LSTM_TILE + col] = acc[q][r];
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < LSTM_ROWS * Hp; e += LSTM_THREADS) {
    const int r = e / Hp, u = e % Hp;
    const long row = row0 + r;
    if (row < B && u < H) {
      if (a.dh0) a.dh0[row * H + u] = dhrec[r * pitch + u];
      if (a.dc0) a.dc0[row * H + u] = dc[r * pitch + u];
    }
  }
}

static int lstm_check(int seq_len, int batch, int hidden) {
  if (seq_len < 1 || batch < 1 || hidden < 1) return RG_EINVAL;
  if (hidden > RG_LSTM_MAX_HIDDEN) return RG_EUNSUPPORTED;
  if ((int64_t)seq_len * batch > 0x7fffffffLL / 4) return RG_EUNSUPPORTED;  // T * B rows go through rg_fc_* as an int
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_lstm_forward(const float* xproj, const float* w_hh, const float* b_hh, const float* h0, const float* c0, int seq_len,
                    int batch, int hidden, float* h_all, float* c_all, float* gates, rg_stream_t stream) {
  const int rc = lstm_check(seq_len, batch, hidden);
  if (rc != RG_OK) return rc;
  if (!xproj || !w_hh || !h_all || !c_all) return RG_EINVAL;
  LstmFwdArgs a;
  a.xproj = xproj, a.w_hh = w_hh, a.b_hh = b_hh, a.h0 = h0, a.c0 = c0;
  a.h_all = h_all, a.c_all = c_all, a.gates = gates;
  a.T = seq_len, a.B = batch, a.H = hidden, a.Hp = lstm_padded(hidden);
  const size_t lds = 2 * lstm_tile_floats(hidden) * sizeof(float);
  RG_ALLOW_LDS(lstm_forward_kernel, lds);
  RG_LAUNCH_DYN(lstm_forward_kernel, dim3((batch + LSTM_ROWS - 1) / LSTM_ROWS), dim3(LSTM_THREADS), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int rg_lstm_backward(const float* dh_all, const float* gates, const float* c_all, const float* c0, const float* w_hh,
                     int seq_len, int batch, int hidden, float* dgates, float* dh0, float* dc0, rg_stream_t stream) {
  const int rc = lstm_check(seq_len, batch, hidden);
  if (rc != RG_OK) return rc;
  if (!dh_all || !gates || !c_all || !w_hh || !dgates) return RG_EINVAL;
  LstmBwdArgs a;
  a.dh_all = dh_all, a.gates = gates, a.c_all = c_all, a.c0 = c0, a.w_hh = w_hh;
  a.dgates = dgates, a.dh0 = dh0, a.dc0 = dc0;
  a.T = seq_len, a.B = batch, a.H = hidden, a.Hp = lstm_padded(hidden);
  const size_t lds = 3 * lstm_tile_floats(hidden) * sizeof(float);
  RG_ALLOW_LDS(lstm_backward_kernel, lds);
  RG_LAUNCH_DYN(lstm_backward_kernel, dim3((batch + LSTM_ROWS - 1) / LSTM_ROWS), dim3(LSTM_THREADS), lds,
                (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
