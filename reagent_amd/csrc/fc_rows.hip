// fc_rows.hip — the exact-fp32 weight gradient of a linear layer from ROW-MAJOR operands over many rows:
//   dw[o, i] = sum_n dz[n, o] * x[n, i]      db[o] = sum_n dz[n, o]      (rg_fc_wgrad_rows)
// The reduced index is the row, and a row of dz or x is contiguous along its channels: rows n and n + 1 of a 32-channel
// strip ARE the A / B fragment of v_mfma_f32_32x32x2_f32 (lane l supplies dz[n + l / 32][o0 + l % 32] and x[n + l / 32][i0 + l % 32]).
// So nothing is transposed, neither by a launch before this one (rg_fc_wgrad's callers run two rg_transpose_cast per layer)
// nor on the way into LDS.
//
// Work split.  A workgroup of 256 threads owns one (row split, output tile of up to 128 x 128); its four waves hold one
// 64 x 64 quadrant each (2 x 2 MFMA tiles, 64 accumulator registers).  splits x tiles is held near the CU count (FR_TARGET_WGS),
// not at rg_fc_wgrad's 1 024: a 128 x 128 layer over 40 960 rows is 256 splits of 160 rows, 16 MB of partials in place of 64 MB.
//
// Data movement.  Per slab of FR_R = 32 rows the workgroup copies the tile's 128 columns of both operands into LDS row for
// row: 16-byte global loads (four per thread and operand, a row of the tile = 32 consecutive lanes = 512 contiguous bytes)
// held in registers across the previous slab's MFMA block, then 16-byte LDS stores.  All four waves read their fragments
// from that one image, so an operand byte is fetched once per workgroup.  The LDS pitch is 160 floats: a fragment read is
// two runs of 32 consecutive floats, one per half-wave, 160 floats = 32 banks (mod 64) apart, and a 16-byte store of 64
// consecutive lanes covers two rows of 512 contiguous bytes — neither meets a bank twice.  A pitch or a base that is not
// 16-byte aligned, and the chunk that straddles a ragged column edge, take 4-byte predicated loads; columns past the widths
// and rows past the split's end are staged as zeros, and an MFMA tile that lies wholly past a width is never issued.
//
// db is the column sum of the staged dz slab, taken from LDS by the workgroups of input tile 0 (thread c < 128 owns column
// c): no second pass over memory and no extra MFMA.
//
// Determinism.  Rows per split are a multiple of FR_R; inside a split every accumulator meets its rows in ascending order;
// with more than one split the partials [splits][out * in | out] lie in the workspace and fc_rows_finish_kernel adds them
// in ascending split order; with one split the main kernel writes dw and db itself.  No atomics; trip counts depend on the
// sizes alone.
//
// Reference semantics replaced: torch.nn.Linear's backward (autograd's AddmmBackward: grad_weight = grad_output^T . input,
// grad_bias = grad_output.sum(0)) for the linear layers of the sequence nets.
#include "rg_gemm.h"
#include "../../include/reagent_hip.h"

namespace rg {
namespace {

constexpr int FR_TILE = 128;               // columns of dz and of x per workgroup
constexpr int FR_R = RG_FC_ROWS_SLAB;      // rows per staged slab
constexpr int FR_PITCH = FR_TILE + 32;     // LDS row pitch in floats (see above)
constexpr int FR_THREADS = 256;
constexpr int FR_TARGET_WGS = 256;         // splits x tiles aimed at: one workgroup per CU of an MI355X
constexpr int FR_PER = FR_R * (FR_TILE / 4) / FR_THREADS;  // 16-byte chunks per thread, operand and slab
static_assert(FR_R % 2 == 0 && FR_R * (FR_TILE / 4) % FR_THREADS == 0, "a slab is whole k pairs and whole rounds of chunks");

struct RowsArgs {
  const float* dz;
  const float* x;
  long ld_dz, ldx;
  float* dw;        // where a split's dw goes: the output itself (one split) or the first partial slab
  float* db;        // likewise; null: no bias gradient
  long slab;        // floats between two splits' partials (0 with one split)
  int out_f, in_f, rows, rows_per_split, tiles_i;
};

struct RowsStage {
  f32x4 r[FR_PER];
};

// rows row0 .. row0 + FR_R of columns col0 .. col0 + 128 of src -> registers; zeros past row_end and past width
__device__ __forceinline__ void rows_load(RowsStage& s, const float* __restrict__ src, long ld, int col0, int width, long row0,
                                          long row_end, bool vec_ok, int tid) {
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int c = tid + i * FR_THREADS;
    const long grow = row0 + (c >> 5);
    const int gcol = col0 + (c & 31) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (grow < row_end && gcol < width) {
      const float* p = src + grow * ld + gcol;
      if (vec_ok && gcol + 4 <= width) {
        v = *(const f32x4*)p;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gcol + e < width) v[e] = p[e];
      }
    }
    s.r[i] = v;
  }
}

__device__ __forceinline__ void rows_store(const RowsStage& s, float* lds, int tid) {
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int c = tid + i * FR_THREADS;
    *(f32x4*)&lds[(c >> 5) * FR_PITCH + (c & 31) * 4] = s.r[i];
  }
}

// one slab of MFMA work of a wave: k pair ks = rows 2 ks, 2 ks + 1.  GUARD: some of the wave's four tiles lie past a width
template <bool GUARD>
__device__ __forceinline__ void rows_compute(const float* As, const float* Bs, int a0, int b0, int lane, const bool (&al)[2],
                                             const bool (&bl)[2], f32x16 (&acc)[2][2]) {
  const int lr = lane & 31, lk = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < FR_R / 2; ++ks) {
    float af[2], bf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      af[t] = As[(ks * 2 + lk) * FR_PITCH + a0 + t * 32 + lr];
      bf[t] = Bs[(ks * 2 + lk) * FR_PITCH + b0 + t * 32 + lr];
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
        if (!GUARD || (al[tm] && bl[tn])) acc[tm][tn] = mfma_32x32x2_f32(af[tm], bf[tn], acc[tm][tn]);
  }
}

__global__ void RG_LAUNCH_BOUNDS(FR_THREADS, 1) fc_rows_kernel(RowsArgs g) {
  __shared__ __attribute__((aligned(16))) float As[FR_R * FR_PITCH];  // dz slab: [row][output channel of the tile]
  __shared__ __attribute__((aligned(16))) float Bs[FR_R * FR_PITCH];  // x slab:  [row][input channel of the tile]

  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = (int)((g.out_f + FR_TILE - 1) / FR_TILE) * g.tiles_i;
  const int split = (int)blockIdx.x / tiles, tile = (int)blockIdx.x % tiles;
  const int o0 = (tile / g.tiles_i) * FR_TILE, i0 = (tile % g.tiles_i) * FR_TILE;
  const long row_begin = (long)split * g.rows_per_split;
  const long row_end = row_begin + g.rows_per_split < g.rows ? row_begin + g.rows_per_split : (long)g.rows;
  const int slabs = (int)((row_end - row_begin + FR_R - 1) / FR_R);

  const bool a_vec = ((g.ld_dz & 3) == 0) && ((((uintptr_t)g.dz) & 15) == 0);
  const bool b_vec = ((g.ldx & 3) == 0) && ((((uintptr_t)g.x) & 15) == 0);
  const int a0 = wm * 64, b0 = wn * 64;
  const bool al[2] = {o0 + a0 < g.out_f, o0 + a0 + 32 < g.out_f};
  const bool bl[2] = {i0 + b0 < g.in_f, i0 + b0 + 32 < g.in_f};
  const bool whole = al[1] && bl[1];
  const bool do_bias = g.db != nullptr && i0 == 0 && tid < FR_TILE;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum = 0.f;

  RowsStage sa, sb;
  rows_load(sa, g.dz, g.ld_dz, o0, g.out_f, row_begin, row_end, a_vec, tid);
  rows_load(sb, g.x, g.ldx, i0, g.in_f, row_begin, row_end, b_vec, tid);
  rows_store(sa, As, tid);
  rows_store(sb, Bs, tid);
  __syncthreads();
  for (int s = 0; s < slabs; ++s) {
    const bool more = s + 1 < slabs;
    if (more) {  // the next slab's loads are in flight during this slab's MFMA block
      const long next = row_begin + (long)(s + 1) * FR_R;
      rows_load(sa, g.dz, g.ld_dz, o0, g.out_f, next, row_end, a_vec, tid);
      rows_load(sb, g.x, g.ldx, i0, g.in_f, next, row_end, b_vec, tid);
      sched_fence();
    }
    if (do_bias) {
#pragma unroll
      for (int r = 0; r < FR_R; ++r) bsum += As[r * FR_PITCH + tid];  // rows past the end are zeros
    }
    if (whole) rows_compute<false>(As, Bs, a0, b0, lane, al, bl, acc);
    else if (al[0] && bl[0]) rows_compute<true>(As, Bs, a0, b0, lane, al, bl, acc);  // (a quadrant wholly past a width only keeps the barriers)
    __syncthreads();
    if (more) {
      rows_store(sa, As, tid);
      rows_store(sb, Bs, tid);
      __syncthreads();
    }
  }

  // D[i][j] of an MFMA tile: lane l, register r hold j = l % 32, i = (r % 4) + 8 (r / 4) + 4 (l / 32): a register of the wave
  // is four runs of 32 consecutive floats of dw
  float* dw = g.dw + (long)split * g.slab;
  const int lr = lane & 31, lh = lane >> 5;
  static_for<0, 2>([&](auto tm_c) __attribute__((always_inline)) {
    static_for<0, 2>([&](auto tn_c) __attribute__((always_inline)) {
      constexpr int tm = decltype(tm_c)::value, tn = decltype(tn_c)::value;
      const int col = i0 + b0 + tn * 32 + lr;
      if (al[tm] && col < g.in_f) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = o0 + a0 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (row < g.out_f) dw[(long)row * g.in_f + col] = acc[tm][tn][r];
        }
      }
    });
  });
  if (do_bias && o0 + tid < g.out_f) g.db[(long)split * g.slab + o0 + tid] = bsum;
}

// out[i] = partial 0 + partial 1 + ... in that order, for the n_w elements of dw and the n_b of db behind them in a slab;
// eight loads in flight, then eight ordered adds
__global__ void fc_rows_finish_kernel(const float* __restrict__ part, long slab, int splits, float* __restrict__ dw, long n_w,
                                      float* __restrict__ db, int n_b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_w + n_b) return;
  const float* p = part + i;
  float s = p[0];
  int k = 1;
  for (; k + 8 <= splits; k += 8) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = p[(long)(k + e) * slab];
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  }
  for (; k < splits; ++k) s += p[(long)k * slab];
  if (i < n_w) dw[i] = s;
  else db[i - n_w] = s;
}

struct RowsPlan {
  int tiles_o, tiles_i, splits, rows_per_split;
  long slab;  // floats of one split's partials: dw [out * in], then db [out]
};
bool rows_sizes_ok(int out_f, int in_f, int rows) {
  return out_f >= 1 && in_f >= 1 && rows >= 1 && out_f <= RG_FC_ROWS_MAX_WIDTH && in_f <= RG_FC_ROWS_MAX_WIDTH;
}
RowsPlan rows_plan(int out_f, int in_f, int rows) {
  RowsPlan p;
  p.tiles_o = (out_f + FR_TILE - 1) / FR_TILE;
  p.tiles_i = (in_f + FR_TILE - 1) / FR_TILE;
  const int tiles = p.tiles_o * p.tiles_i;
  long want = FR_TARGET_WGS / tiles;
  const long most = ((long)rows + FR_R - 1) / FR_R;  // a split has at least one slab
  if (want > most) want = most;
  if (want < 1) want = 1;
  const long per = (((long)rows + want - 1) / want + FR_R - 1) / FR_R * FR_R;
  p.rows_per_split = (int)(per < 0x7fffffc0L ? per : 0x7fffffc0L);  // (a multiple of FR_R that an int holds)
  p.splits = (int)(((long)rows + p.rows_per_split - 1) / p.rows_per_split);
  p.slab = (long)out_f * in_f + out_f;
  return p;
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_fc_wgrad_rows_workspace_bytes(int out_features, int in_features, int rows) {
  if (!rows_sizes_ok(out_features, in_features, rows)) return 0;
  const RowsPlan p = rows_plan(out_features, in_features, rows);
  return p.splits > 1 ? (size_t)p.splits * p.slab * sizeof(float) : 0;  // one split writes dw and db itself
}

int rg_fc_wgrad_rows(const float* dz, int64_t ld_dz, const float* x, int64_t ldx, float* dw, float* db, void* workspace,
                     size_t workspace_bytes, int out_features, int in_features, int rows, rg_stream_t stream) {
  if (!dz || !x || !dw || !rows_sizes_ok(out_features, in_features, rows)) return RG_EINVAL;
  if (ld_dz < out_features || ldx < in_features) return RG_EINVAL;
  const RowsPlan p = rows_plan(out_features, in_features, rows);
  const size_t need = p.splits > 1 ? (size_t)p.splits * p.slab * sizeof(float) : 0;
  if (need && (!workspace || workspace_bytes < need)) return RG_EWORKSPACE;
  const long n_w = (long)out_features * in_features;
  float* part = (float*)workspace;
  RowsArgs g;
  g.dz = dz; g.x = x; g.ld_dz = (long)ld_dz; g.ldx = (long)ldx;
  g.out_f = out_features; g.in_f = in_features; g.rows = rows;
  g.rows_per_split = p.rows_per_split; g.tiles_i = p.tiles_i;
  if (p.splits > 1) {
    g.dw = part; g.db = db ? part + n_w : nullptr; g.slab = p.slab;
  } else {
    g.dw = dw; g.db = db; g.slab = 0;
  }
  hipStream_t s = (hipStream_t)stream;
  RG_LAUNCH(fc_rows_kernel, dim3((unsigned)(p.splits * p.tiles_o * p.tiles_i)), dim3(FR_THREADS), s, g);
  if (p.splits > 1) {
    const long n = n_w + (db ? out_features : 0);
    RG_LAUNCH(fc_rows_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), s, (const float*)part, p.slab, p.splits, dw,
              n_w, db, db ? out_features : 0);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
