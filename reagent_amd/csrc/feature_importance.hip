// feature_importance.hip — feature importance by perturbation of an FC Q-network
// (reagent/evaluation/feature_importance/feature_importance_perturbation.py), all variants of a batch in one sweep.  The
// reference permutes one raw feature (value and presence) over the rows, F times, and runs the preprocessor and the whole
// network on every copy.  After the preprocessor a permuted feature is a permuted block of normalized columns, so variant v
// is (perm[v], block v) and row (v, b) is derived from rows b and perm[v, b] of the ONE normalized batch x:
//
//   z0_v[b] = z0[b] + sum_{c in block v} (x[perm[v, b], c] - x[b, c]) W0[., c]        z0 = x W0^T + b0, shared by all variants
//
// and everything above layer 0 lives in LDS.  Neither a perturbed batch nor any activation of the V x B virtual rows is
// ever written: a workgroup leaves one double (A under RG_FI_PER_ACTION).
//
//   fi_sweep_kernel    a workgroup (4 waves) per (variant, 32-row tile): correction, the stack, the prediction, sum |delta|
//   fi_finish_kernel   importance[v, c] = (the tile partials in ascending order) / B, rounded once
//
// The tile is 32 rows by the LDS budget: an activation image is k-major [width][32] fp32 (the A fragment of
// v_mfma_f32_32x32x2_f32 is then 32 consecutive floats per half-wave), two of them for a 512-wide stack are 128 KB, and the
// weight slab (8 k x 544) is 17 KB: 145 KB of 160.  64 rows would need 256 KB for the images alone.
// Image element (k, row) lies at k * 32 + (row ^ (k & 31)): the epilogue's writes (a lane per k, one row at a time) and the
// fragment reads (a lane per row, one k per half-wave) both touch 32 different banks without a padding column.
// No atomics anywhere: two runs give the same bits.
#include <rg_platform.h>
#include "../../include/reagent_hip.h"
#include "rg_gemm.h"  // static_for, act_apply_n

namespace rg {

constexpr int FI_THREADS = 256, FI_WAVES = 4, FI_ROWS = 32, FI_BK = 8, FI_TILES = RG_FI_MAX_WIDTH / 32 / FI_WAVES;
constexpr int FI_MFMA_FROM = 32;  // a block this wide or wider takes the MFMA chain
static_assert(FI_TILES * FI_WAVES * 32 == RG_FI_MAX_WIDTH, "a wave's accumulators cover the widest layer");
static_assert(RG_FI_MAX_ACTIONS <= FI_THREADS && FI_ROWS <= FI_THREADS, "a thread per action / per row in the reduction");

struct FiArgs {
  rg_fi_net net;
  const float *x, *z0, *q, *mask;
  const int *perm, *blocks;
  long ldx, ldz0, ldq, ldmask;
  int reduce, B, max_width;
  int cap;   // k rows of an activation image (a multiple of 32)
  int sp;    // pitch of the weight slab: the widest layer rounded up to 32, 32 mod 64 (the two half-waves on disjoint banks)
  double* partials;
};

__device__ __forceinline__ int fi_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int fi_at(int k, int row) { return k * FI_ROWS + (row ^ (k & 31)); }
__device__ __forceinline__ int fi_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
__device__ __forceinline__ int fi_pad32(int v) { return (v + 31) & ~31; }
static inline int fi_round(int v, int m) { return (v + m - 1) / m * m; }

// acc[i] = tile (wave + 4 i) of src[32, K] . W[N, K]^T, i < the wave's tiles: per accumulator ONE chain of fp32 MFMAs in
// ascending k from +0 over the pairs (2j, 2j + 1), rg_fc_forward's RG_PREC_F32 order.  W (pitch ldw) passes through LDS in
// slabs of FI_BK k, k-major, loaded by all 256 threads as 16-byte pieces along k and held in registers while the slab
// before it is multiplied (two barriers per slab).  k past K and columns past N are zeros in the slab; src's rows K .. K
// rounded up to FI_BK must be zeros (every writer of an image pads to 32).
__device__ __forceinline__ void fi_product(const float* src, int K, const float* __restrict__ W, long ldw, int N, int Np,
                                           float* slab, int sp, f32x16 (&acc)[FI_TILES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), col = lane & 31, half = lane >> 5;
  const int mine = (Np / 32 - wave + FI_WAVES - 1) / FI_WAVES, nch = Np * (FI_BK / 4);
  const bool vec_ok = (ldw % 4) == 0 && ((((uintptr_t)W) & 15) == 0);
  f32x4 st[FI_TILES];  // Np * 2 pieces over 256 threads: at most 4 each
  auto load = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FI_TILES; ++i) {
      const int c = tid + i * FI_THREADS, row = c >> 1, gk = k0 + (c & 1) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c < nch && row < N && gk < K) {
        const float* p = W + (long)row * ldw + gk;
        if (vec_ok && gk + 4 <= K) {
          v = *(const f32x4*)p;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gk + e < K) v[e] = p[e];
        }
      }
      st[i] = v;
    }
  };
  auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FI_TILES; ++i) {
      const int c = tid + i * FI_THREADS, row = c >> 1, kc = c & 1;
      if (c < nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e) slab[(kc * 4 + e) * sp + row] = st[i][e];
      }
    }
  };
#pragma unroll
  for (int i = 0; i < FI_TILES; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  load(0);
  store();
  __syncthreads();  // (also publishes src, written before the call)
  for (int k0 = 0; k0 < K; k0 += FI_BK) {
    const bool more = k0 + FI_BK < K;
    if (more) load(k0 + FI_BK);
#pragma unroll
    for (int ks = 0; ks < FI_BK / 2; ++ks) {
      const int kk = 2 * ks + half, k = k0 + kk;
      const float av = src[fi_at(k, col)];
      static_for<0, FI_TILES>([&](auto i_c) __attribute__((always_inline)) {
        constexpr int i = decltype(i_c)::value;
        if (i < mine) acc[i] = mfma_32x32x2_f32(av, slab[kk * sp + (wave + FI_WAVES * i) * 32 + col], acc[i]);
      });
    }
    __syncthreads();
    if (more) {
      store();
      __syncthreads();
    }
  }
}

// dst (an image) = act(acc + add) over the wave's tiles, zeros at the columns N .. Np.  LAYER0: add is z0's element of the row
// (pitch ld, rows past the batch read the last row: their values are dropped at the end); otherwise add is the bias.
template <bool LAYER0>
__device__ __forceinline__ void fi_epilogue(const f32x16 (&acc)[FI_TILES], const float* __restrict__ add, long ld, long row0,
                                            int B, int N, int Np, int act, float* dst) {
  const int lane = threadIdx.x & 63, wave = wave_uniform(threadIdx.x >> 6), col = lane & 31, half = lane >> 5;
  const int mine = (Np / 32 - wave + FI_WAVES - 1) / FI_WAVES;
  static_for<0, FI_TILES>([&](auto i_c) __attribute__((always_inline)) {
    constexpr int i = decltype(i_c)::value;
    if (i < mine) {
      const int u = (wave + FI_WAVES * i) * 32 + col, uc = u < N ? u : N - 1;
      const float b = (!LAYER0 && add) ? add[uc] : 0.f;
      float o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (LAYER0) {
          const long row = row0 + fi_acc_row(r, half);
          o[r] = add[(row < B ? row : B - 1) * ld + uc] + acc[i][r];
        } else {
          o[r] = acc[i][r] + b;
        }
      }
      act_apply_n(o, act);
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[fi_at(u, fi_acc_row(r, half))] = u < N ? o[r] : 0.f;
    }
  });
}

__global__ void RG_LAUNCH_BOUNDS(FI_THREADS, 1) fi_sweep_kernel(const FiArgs a) {
  RG_DYN_LDS(smem);
  __shared__ double dd[FI_ROWS];
  float* cur = (float*)smem;
  float* nxt = cur + a.cap * FI_ROWS;
  float* slab = nxt + a.cap * FI_ROWS;
  const int tid = threadIdx.x, B = a.B, L = a.net.n_layers, D = a.net.dims[0], v = blockIdx.y;
  const long row0 = (long)blockIdx.x * FI_ROWS;
  int s = a.blocks[2 * v], e = a.blocks[2 * v + 1];
  s = fi_clamp(s, 0, D), e = fi_clamp(e, s, fi_clamp(s + a.max_width, s, D));  // (nobody on the host reads the device table: a block is cut to the row and to max_width columns here, as the header says)
  const int w = e - s;
  const int* perm = a.perm + (long)v * B;
  const float* W0 = a.net.w[0] + s;
  const int H1 = a.net.dims[1], H1p = fi_pad32(H1);
  f32x16 acc[FI_TILES];

  // ---- layer 0: h0 = act0(z0 + correction) into cur -------------------------------------------------------------------
  if (w >= FI_MFMA_FROM) {
    // the deltas as an image (k = the block's column, zeros up to a multiple of FI_BK), then the MFMA chain over the block
    const int wp = (w + FI_BK - 1) / FI_BK * FI_BK;
    for (int i = tid; i < FI_ROWS * wp; i += FI_THREADS) {
      const int r = i / wp, j = i % wp;
      const long row = row0 + r < B ? row0 + r : B - 1;
      const long pr = fi_clamp(perm[row], 0, B - 1);
      nxt[fi_at(j, r)] = j < w ? a.x[pr * a.ldx + s + j] - a.x[row * a.ldx + s + j] : 0.f;
    }
    fi_product(nxt, w, W0, D, H1, H1p, slab, a.sp, acc);
    fi_epilogue<true>(acc, a.z0, a.ldz0, row0, B, H1, H1p, a.net.acts[0], cur);
  } else {
    // a narrow block: the deltas [w][32] in the (idle) slab, then per output column one fmaf chain per row in ascending c
    float* dl = slab;
    for (int i = tid; i < FI_ROWS * w; i += FI_THREADS) {
      const int r = i / w, j = i % w;
      const long row = row0 + r < B ? row0 + r : B - 1;
      const long pr = fi_clamp(perm[row], 0, B - 1);
      dl[j * FI_ROWS + r] = a.x[pr * a.ldx + s + j] - a.x[row * a.ldx + s + j];
    }
    __syncthreads();
    for (int u = tid; u < H1p; u += FI_THREADS) {
      const int uc = u < H1 ? u : H1 - 1;
      const float* wrow = W0 + (long)uc * D;
      float o[FI_ROWS];
#pragma unroll
      for (int r = 0; r < FI_ROWS; ++r) o[r] = 0.f;
      for (int j = 0; j < w; ++j) {
        const float wv = wrow[j];
#pragma unroll
        for (int r = 0; r < FI_ROWS; ++r) o[r] = fmaf(dl[j * FI_ROWS + r], wv, o[r]);
      }
#pragma unroll
      for (int r = 0; r < FI_ROWS; ++r) {
        // (the row per lane: as scalars the 32 row offsets of this unrolled loop are hoisted and spill SGPRs)
        const long row = row0 + opaque(r) < B ? row0 + opaque(r) : B - 1;
        o[r] = a.z0[row * a.ldz0 + uc] + o[r];
      }
      act_apply_n(o, a.net.acts[0]);
#pragma unroll
      for (int r = 0; r < FI_ROWS; ++r) cur[fi_at(u, r)] = u < H1 ? o[r] : 0.f;
    }
    __syncthreads();  // (the slab is free again)
  }

  // ---- layers 1 .. L - 1, tile-resident ----------------------------------------------------------------------------------
  for (int l = 1; l < L; ++l) {
    const int K = a.net.dims[l], N = a.net.dims[l + 1], Np = fi_pad32(N);
    fi_product(cur, K, a.net.w[l], K, N, Np, slab, a.sp, acc);
    fi_epilogue<false>(acc, a.net.bias[l], 0, row0, B, N, Np, a.net.acts[l], nxt);
    float* sw = cur;
    cur = nxt, nxt = sw;
  }
  __syncthreads();

  // ---- the prediction and the tile's sum of |pred_v - pred_base| --------------------------------------------------------------
  const int A = a.net.dims[L];
  const long tile = (long)v * gridDim.x + blockIdx.x;
  if (a.reduce == RG_FI_PER_ACTION) {
    if (tid < A) {  // a thread per action, the rows in ascending order
      double sum = 0.0;
      for (int r = 0; r < FI_ROWS; ++r) {
        const long row = row0 + r;
        const double d = fabs((double)cur[fi_at(tid, r)] - (double)a.q[(row < B ? row : B - 1) * a.ldq + tid]);
        sum += row < B ? d : 0.0;
      }
      a.partials[tile * A + tid] = sum;
    }
    return;
  }
  if (tid < FI_ROWS) {  // a thread per row
    const long row = row0 + tid, rowc = row < B ? row : B - 1;
    const float* qr = a.q + rowc * a.ldq;
    double pv, pb;
    if (a.reduce == RG_FI_MAX) {
      float mv = cur[fi_at(0, tid)], mb = qr[0];
      for (int j = 1; j < A; ++j) {
        const float cv = cur[fi_at(j, tid)], cb = qr[j];
        mv = cv > mv ? cv : mv, mb = cb > mb ? cb : mb;
      }
      pv = mv, pb = mb;
    } else {  // (a product of two floats is exact in double: fused or not, the two sums are the same arithmetic)
      const float* mr = a.mask + rowc * a.ldmask;
      pv = 0.0, pb = 0.0;
      for (int j = 0; j < A; ++j) {
        const double m = mr[j];
        pv += m * (double)cur[fi_at(j, tid)], pb += m * (double)qr[j];
      }
    }
    dd[tid] = row < B ? fabs(pv - pb) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int r = 0; r < FI_ROWS; ++r) sum += dd[r];
    a.partials[tile] = sum;
  }
}

// a thread per output: its variant's partials in ascending tile order, divided by the batch in double, rounded once
__global__ void fi_finish_kernel(const double* __restrict__ partials, int tiles, int C, int outputs, double batch,
                                 float* __restrict__ importance) {
  const int o = blockIdx.x * FI_THREADS + threadIdx.x;
  if (o >= outputs) return;
  const double* mine = partials + (long)(o / C) * tiles * C + o % C;
  double sum = 0.0;
  for (int t = 0; t < tiles; ++t) sum += mine[(long)t * C];
  importance[o] = (float)(sum / batch);
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_fi_partials(int batch, int variants, int actions, int reduce) {
  if (batch < 1 || variants < 1 || actions < 1 || reduce < RG_FI_MAX || reduce > RG_FI_PER_ACTION) return 0;
  if (variants > 65535 || actions > RG_FI_MAX_ACTIONS) return 0;
  const int64_t n = (int64_t)variants * ((batch + FI_ROWS - 1) / FI_ROWS) * (reduce == RG_FI_PER_ACTION ? actions : 1);
  return n > 0x7fffffffLL ? 0 : (int)n;
}

int rg_fi_sweep(const rg_fi_net* net, const float* x, int64_t ldx, const float* z0, int64_t ldz0, const int32_t* perm,
                const int32_t* blocks, const float* q, int64_t ldq, const float* mask, int64_t ldmask, int reduce, int max_width,
                int batch, int variants, double* partials, rg_stream_t stream) {
  if (!net || !x || !z0 || !perm || !blocks || !q || !partials || batch < 1 || variants < 1 || max_width < 0) return RG_EINVAL;
  if (reduce < RG_FI_MAX || reduce > RG_FI_PER_ACTION || (reduce == RG_FI_MASKED && !mask)) return RG_EINVAL;
  const int L = net->n_layers;
  if (L < 1 || L > RG_FI_MAX_LAYERS) return RG_EINVAL;
  int widest = 0;
  for (int l = 0; l <= L; ++l) {
    if (net->dims[l] < 1) return RG_EINVAL;
    if (l >= 1 && net->dims[l] > widest) widest = net->dims[l];
  }
  for (int l = 0; l < L; ++l)
    if (!net->w[l] || net->acts[l] < RG_ACT_LINEAR || net->acts[l] > RG_ACT_SOFTPLUS) return RG_EINVAL;
  const int A = net->dims[L];
  if (ldx < net->dims[0] || ldz0 < net->dims[1] || ldq < A || (reduce == RG_FI_MASKED && ldmask < A)) return RG_EINVAL;
  if (widest > RG_FI_MAX_WIDTH || A > RG_FI_MAX_ACTIONS || net->dims[0] > RG_FI_MAX_INPUT || max_width > RG_FI_MAX_WIDTH ||
      variants > 65535)
    return RG_EUNSUPPORTED;
  if (rg_fi_partials(batch, variants, A, reduce) == 0) return RG_EUNSUPPORTED;
  FiArgs a;
  a.net = *net;
  a.x = x, a.z0 = z0, a.q = q, a.mask = mask, a.perm = (const int*)perm, a.blocks = (const int*)blocks;
  a.ldx = (long)ldx, a.ldz0 = (long)ldz0, a.ldq = (long)ldq, a.ldmask = (long)ldmask;
  a.reduce = reduce, a.B = batch, a.max_width = max_width, a.partials = partials;
  a.cap = fi_round(max_width >= FI_MFMA_FROM && max_width > widest ? max_width : widest, 32);
  const int np = fi_round(widest, 32);
  a.sp = (np % 64) == 0 ? np + 32 : np;
  // (the slab also holds a narrow block's deltas: up to 31 x 32)
  const int slab = FI_BK * a.sp > FI_ROWS * FI_MFMA_FROM ? FI_BK * a.sp : FI_ROWS * FI_MFMA_FROM;
  const size_t lds = ((size_t)2 * a.cap * FI_ROWS + slab) * sizeof(float);
  RG_ALLOW_LDS(fi_sweep_kernel, lds);
  RG_LAUNCH_DYN(fi_sweep_kernel, dim3((batch + FI_ROWS - 1) / FI_ROWS, variants), dim3(FI_THREADS), lds, (hipStream_t)stream,
                a);
  return (int)hipGetLastError();
}

int rg_fi_finish(const double* partials, int batch, int variants, int columns, float* importance, rg_stream_t stream) {
  if (!partials || !importance || batch < 1 || variants < 1 || columns < 1) return RG_EINVAL;
  if (variants > 65535 || columns > RG_FI_MAX_ACTIONS) return RG_EUNSUPPORTED;
  const int outputs = variants * columns;
  RG_LAUNCH(fi_finish_kernel, dim3((outputs + FI_THREADS - 1) / FI_THREADS), dim3(FI_THREADS), (hipStream_t)stream, partials,
            (batch + FI_ROWS - 1) / FI_ROWS, columns, outputs, (double)batch, importance);
  return (int)hipGetLastError();
}

}  // extern "C"
