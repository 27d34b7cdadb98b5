// mlp_wgrad.hip — the weight gradient of a fused FullyConnected stack, bf16 (mlp_fused.hip) or split-bf16
// (mlp_fused_x3.hip), and of QR-DQN's grouped head (qr_grouped.hip): dW = dZ^T X from the operands the forward and backward
// kernels saved in MFMA-fragment order, cut into splits over the batch.  The cores (bf16; split-bf16 with three or two
// products per tile pair) over five workgroup tile shapes; three launch forms — one layer (rg_fc_wgrad_frag), one grouped
// layer (rg_group_head_wgrad), every layer of a stack in one launch (rg_mlp_wgrad_fused); the split reduces, the stack's with
// the bias gradients' column reduce and a scaled sum folded in; the host plan (shape, splits, launch entries and order).

#include "rg_mlp_frag.h"
#include "rg_reduce.h"
#include <cstdio>

namespace rg {

// workgroups per layer of the stack's weight-gradient launch (splits = this / tiles); the alternatives measured against it
// are in profiles/NOTES_r01_r05.md
constexpr int WGRAD_TARGET = 128;
constexpr int REDUCE_FLY = 16;       // split-reduce: fp32 partials requested per thread before the first add (multiple of 4)
constexpr int REDUCE_FLY_BF16 = 8;   // the same for the 32-byte bf16 tile records (even)

// ---- weight gradient from fragment-ordered operands ------------------------------------------
// dW[n][k] = sum_m dZ[m][n] X[m][k].  A = dz_frag tiles (lane = n), B = x_frag tiles (lane = k):
// per 32-row block and half, one MFMA per (n-tile, k-tile) pair.  Workgroup tile 256(n) x 256(k) — or another shape of
// <= 64 tiles, wgrad_shape_core — over 8 waves, each 4x2 MFMA tiles; operands staged HBM -> LDS by DMA (lane-linear
// 16-byte units, conflict-free reads), one 32-row block per stage, a ring of stages, one barrier per stage.
constexpr int WG_MB_STAGE = 1;                      // 32-row blocks per stage

struct WgradFragArgs {
  const bf16_t* a_frag;
  const bf16_t* b_frag;
  int NTa, NTb;       // tiles per 32-row block in each operand
  int MB;             // 32-row blocks in total (= the END of this entry's block range)
  int mb_base;        // first block of this entry's split 0 (0 but for the second class of an unevenly split layer)
  int mb_per_split;   // multiple of WG_MB_STAGE
  int splits;
  float* partial;     // [splits][N*K]
  long slab;
  int N, K;           // valid extents of dW
  // split-bf16 operands (x3 != 0): every stage carries the hi AND lo planes of both operands and a tile pair takes
  // three MFMAs — a_lo.b_hi + a_hi.b_lo + a_hi.b_hi into one accumulator (wgrad_x3_shape_core).  The kernel is bound by its
  // operand stream (§3.2), so the three products share ONE pass over the four planes instead of three passes over
  // two planes each (the round-2 first version: three partial slabs per split, 354 us per C2 launch).
  int x3;
  long a_lo, b_lo;    // element offsets of the lo planes
  int shape;          // workgroup tile shape (WG_SHAPE_*, wgrad_shape_core / wgrad_x3_shape_core); 0 = 8 x 8 tiles
  // How a split's partial tile leaves the workgroup.  0: fp32, row-major [N][K] (slab = N * K floats).  1 (round 5, the bf16
  // stack launch): bf16, one 2 KB record per 32 x 32 MFMA tile in ACCUMULATOR order — record (tn * NTb + tk), lane's 16 values
  // contiguous (32 bytes) — so a tile leaves as two 16-byte stores per lane instead of sixteen 4-byte ones and the launch
  // writes (and its reduce reads) half the bytes; slab = NTa * NTb * 512 floats' worth.  The reduce launch undoes the order.
  int part_mode;
};

// ---- workgroup tile shapes ------------------------------------------------------------------------------------------
// The kernel is bound by its operand stream L2 -> LDS (round 2-3 ablations), and a 256 x 256 tile streams 8 + 8 fragment
// tiles per 32-row block whatever the layer looks like: for dW0 [512 x 128] half of the B operand was a clamped re-read,
// for a thin output layer's dW [16 x 512] seven eighths of the A operand — 93 MB of the 804 MB a C2 launch moved into LDS
// were such junk, and both layers read their long operand through two tiles.  A workgroup now takes GA n-tiles x GB
// k-tiles (GA * GB <= 64 accumulator tiles over 8 waves = WN x WK, each TA x TB), chosen per layer by the host to minimise
// the bytes staged (wgrad_pick_shape):
//   8 x 8   (256 x 256)  square layers                      4 DMAs per thread and 32-row block
//   16 x 4  (512 x 128)  wide-out / narrow-in (dW0)          5   (dZ0 read by ONE tile)
//   4 x 16  (128 x 512)  narrow-out / wide-in                5
//   2 x 16, 1 x 16       thin output layers (<= 64 / <= 32 outputs): 5, with 2 / 1 accumulator tile(s) per wave
// A stage is (GA + GB) tiles x 2 KB, padded to whole 16-byte units per thread; stages of more than 32 KB ring through
// three slots (two in flight: measured equal to three in round 2), the 8 x 8 shape keeps four.
enum { WG_SHAPE_8x8 = 0, WG_SHAPE_16x4 = 1, WG_SHAPE_4x16 = 2, WG_SHAPE_2x16 = 3, WG_SHAPE_1x16 = 4, WG_N_SHAPES = 5 };

template <int GA_, int GB_, int WN_, int WK_> struct WgShape {
  static constexpr int GA = GA_, GB = GB_, WN = WN_, WK = WK_;
  static constexpr int TA = GA / WN, TB = GB / WK;
  static_assert(WN * WK == WG_THREADS / 64 && TA * WN == GA && TB * WK == GB && TA * TB <= 8, "wave layout");
  static constexpr int DMA = ((GA + GB) * 128 + WG_THREADS - 1) / WG_THREADS;  // 16-byte units per thread and stage
  static constexpr int STAGE_BYTES = DMA * WG_THREADS * 16;
  static constexpr int SLOTS = STAGE_BYTES <= 32 * 1024 ? 4 : 3;
  static constexpr int LDS_BYTES = SLOTS * STAGE_BYTES;
};
using WgS8x8 = WgShape<8, 8, 2, 4>;
using WgS16x4 = WgShape<16, 4, 4, 2>;
using WgS4x16 = WgShape<4, 16, 1, 8>;
using WgS2x16 = WgShape<2, 16, 1, 8>;
using WgS1x16 = WgShape<1, 16, 1, 8>;
constexpr int WG_SHAPED_LDS = 128 * 1024;  // max over the shapes (8x8: 4 x 32 KB; the 5-DMA shapes: 3 x 40 KB)
static_assert(WgS8x8::LDS_BYTES <= WG_SHAPED_LDS && WgS16x4::LDS_BYTES <= WG_SHAPED_LDS && WgS4x16::LDS_BYTES <= WG_SHAPED_LDS &&
              WgS2x16::LDS_BYTES <= WG_SHAPED_LDS && WgS1x16::LDS_BYTES <= WG_SHAPED_LDS, "dynamic LDS of the weight-gradient launches");

template <int N> __device__ __forceinline__ void wait_vmcnt() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}

// ---- what the two cores share: the accumulator clear and the fp32 epilogue.  (Compile-time tile indices in the clear:
// as plain loops inside a helper it cost the five-shape kernel 111 spilled registers.  The cores' prologues stay written
// out: shared, in two forms, they moved wgrad_grouped_kernel from 64 to 66 scalar registers.)
template <int TA, int TB> __device__ __forceinline__ void wgrad_clear(f32x16 (&acc)[TA][TB]) {
  static_for<0, TA * TB>([&](auto t_c) __attribute__((always_inline)) {
    constexpr int t = decltype(t_c)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t / TB][t % TB][r] = 0.f;
  });
}
// a split's partial tile leaves as fp32, row-major [N][K] (WgradFragArgs.part_mode 0); tn0 / tk0 = the wave's first n- / k-tile
template <int TA, int TB>
__device__ __forceinline__ void wgrad_store_f32(const WgradFragArgs& g, const f32x16 (&acc)[TA][TB], int tn0, int tk0, int lane, float* part) {
  const int lr = lane & 31, lg = lane >> 5;
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int j = 0; j < TB; ++j) {
      const int col = (tk0 + j) * 32 + lr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (tn0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
        if (row < g.N && col < g.K) part[(long)row * g.K + col] = acc[i][j][r];
      }
    }
}

// one workgroup: dW tile (n-group ng, k-group kg) of shape S over the 32-row blocks [mb_begin, mb_end), written to `part`
template <typename S>
__device__ __forceinline__ void wgrad_shape_core(const WgradFragArgs& g, int ng, int kg, int mb_begin, int mb_end, float* part,
                                                 char* smem) {
  constexpr int GA = S::GA, GB = S::GB, TA = S::TA, TB = S::TB, DMA = S::DMA, SLOTS = S::SLOTS, FLY = S::SLOTS - 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int wn = wave / S::WK, wk = wave % S::WK;
  const int ta0 = ng * GA, tb0 = kg * GB;
  const int na = (g.NTa - ta0 < GA) ? g.NTa - ta0 : GA, nb = (g.NTb - tb0 < GB) ? g.NTb - tb0 : GB;
  const bf16_t* ga_frag = g.a_frag;
  const bf16_t* gb_frag = g.b_frag;
  f32x16 acc[TA][TB];
  wgrad_clear(acc);
  // LDS image of a stage: tile t (A tiles 0 .. GA-1, then the B tiles, then padding) at t * 2 KB, lane-linear 16-byte
  // units — what the DMA writes (wave-uniform base + lane * 16).  Unit u = tid + i * 512 belongs to tile u / 128, which is
  // the same for the 64 lanes of a wave; out-of-range tiles / blocks read a clamped valid address (never used), so every
  // wave issues exactly DMA loads per stage and the vmcnt arithmetic below is exact.
  const int mb_last = mb_end - 1;
  // per DMA of a stage (compile-time i): this wave's tile is fixed, only the 32-row block moves — base pointer and block
  // stride are worked out once, from values already in registers (selecting between the A and the B operand's FIELDS of
  // the argument block inside the loop made the compiler index them through scratch)
  const int nta = g.NTa, ntb = g.NTb;
  const int within = tid & 127;  // (tid + i * 512) & 127: the same for every i
  const bf16_t* src0[DMA];
  long blk_stride[DMA];
  static_for<0, DMA>([&](auto i_c) __attribute__((always_inline)) {
    constexpr int i = decltype(i_c)::value;
    const int t = i * (WG_THREADS / 128) + (wave >> 1);  // tile of this wave's units (wave-uniform)
    const bool is_a = t < GA;
    const int ta = ta0 + (t < na ? t : na - 1);
    const int tb = tb0 + ((t - GA) < nb ? (t - GA < 0 ? 0 : t - GA) : nb - 1);
    const long tile = is_a ? (long)ta : (long)tb;
    const bf16_t* base = is_a ? ga_frag : gb_frag;
    src0[i] = base + tile * 1024 + within * 8;
    blk_stride[i] = (long)(is_a ? nta : ntb) * 1024;
  });
  auto issue = [&](int blk, int slot) {
    const int mb = blk < mb_last ? blk : mb_last;
    static_for<0, DMA>([&](auto i_c) __attribute__((always_inline)) {
      constexpr int i = decltype(i_c)::value;
      global_load_lds_b128(src0[i] + (long)mb * blk_stride[i], smem + slot * S::STAGE_BYTES + (wave * 64 + i * WG_THREADS) * 16);
    });
  };
  const bool wave_has_tiles = wn * TA < na && wk * TB < nb;  // a wave whose tiles are all padding skips its MFMAs
  // Round 4 (profiles/microbench/out/r04a/wgrad_phases.txt): an iteration of this loop took ~2700 cycles whatever the stage
  // held — 16 MFMAs per wave (1024 cycles per SIMD), the rest LDS latency, DMA issue and the barrier: the loop is bound
  // by its own per-iteration chain, not by the memory system (8 % of it waits for data).  So the fragments of the next
  // 16-row half are requested from LDS before the MFMAs of the current one.
  auto load_half = [&](int slot, int h, u16x8 (&af)[TA], u16x8 (&bf)[TB]) {
    const char* base = smem + slot * S::STAGE_BYTES + h * 1024 + lane * 16;
#pragma unroll
    for (int i = 0; i < TA; ++i) af[i] = *(const u16x8*)(base + (wn * TA + i) * 2048);
#pragma unroll
    for (int j = 0; j < TB; ++j) bf[j] = *(const u16x8*)(base + (GA + wk * TB + j) * 2048);
  };
  auto mma_half = [&](const u16x8 (&af)[TA], const u16x8 (&bf)[TB]) {
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TB; ++j) acc[i][j] = mfma_32x32x16_bf16(af[i], bf[j], acc[i][j]);
  };
  // the two halves of the block in `slot`
  auto compute = [&](int slot) __attribute__((always_inline)) {
    if (!wave_has_tiles) return;
    u16x8 af[2][TA], bf[2][TB];
    load_half(slot, 0, af[0], bf[0]);
    static_for<0, 2>([&](auto h_c) __attribute__((always_inline)) {
      constexpr int h = decltype(h_c)::value;
      if constexpr (h == 0) load_half(slot, 1, af[1], bf[1]);
      sched_fence();  // (without the fences the scheduler requests every half's fragments up front: 256 registers + scratch)
      mma_half(af[h], bf[h]);
      sched_fence();
    });
  };

  RG_PHASE_INIT();
  if (mb_begin < mb_end) {
    const int n_blk = mb_end - mb_begin;
    static_for<0, FLY>([&](auto f_c) __attribute__((always_inline)) { issue(mb_begin + decltype(f_c)::value, decltype(f_c)::value); });
    RG_PHASE(0);
    for (int t = 0; t < n_blk; ++t) {
      // FLY stages are outstanding: let the oldest land, then meet the other waves — past the barrier block t is complete
      // in LDS and every wave has finished reading block t-1, whose slot the DMA issued below overwrites
      wait_vmcnt<(FLY - 1) * DMA>();
      RG_PHASE(2);
      raw_barrier();
      RG_PHASE(3);
      issue(mb_begin + t + FLY, (t + FLY) % SLOTS);  // before the MFMAs: the requests leave a block time earlier
      compute(t % SLOTS);
      RG_PHASE(1);
    }
    wait_vmcnt<0>();
  }

  if (g.part_mode == 1) {
    typedef __attribute__((ext_vector_type(4))) unsigned pk4_t;
    bf16_t* pb = (bf16_t*)part;
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TB; ++j) {
        const int tn = ta0 + wn * TA + i, tk = tb0 + wk * TB + j;
        if (tn < nta && tk < ntb) {
          pk4_t* dst = (pk4_t*)(pb + ((long)tn * ntb + tk) * 1024 + lane * 16);
          const f32x16& c = acc[i][j];
          const pk4_t v0 = pk4_t{pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3]), pack_bf16x2(c[4], c[5]), pack_bf16x2(c[6], c[7])};
          const pk4_t v1 = pk4_t{pack_bf16x2(c[8], c[9]), pack_bf16x2(c[10], c[11]), pack_bf16x2(c[12], c[13]), pack_bf16x2(c[14], c[15])};
          dst[0] = v0;
          dst[1] = v1;
        }
      }
    RG_PHASE(4);
    RG_PHASE_FLUSH();
    return;
  }
  wgrad_store_f32(g, acc, ta0 + wn * TA, tb0 + wk * TB, lane, part);
  RG_PHASE(4);
  RG_PHASE_FLUSH();
}

// tiles per group of a shape, for the host plan and the workgroup decode (value-returning selects: reference outputs of a
// switch put four dwords of the five-shape kernel into scratch)
__host__ __device__ __forceinline__ int wgrad_shape_ga(int shape) {
  return shape == WG_SHAPE_16x4 ? 16 : shape == WG_SHAPE_4x16 ? 4 : shape == WG_SHAPE_2x16 ? 2 : shape == WG_SHAPE_1x16 ? 1 : 8;
}
__host__ __device__ __forceinline__ int wgrad_shape_gb(int shape) {
  return shape == WG_SHAPE_16x4 ? 4 : shape == WG_SHAPE_8x8 ? 8 : 16;
}

// Split-bf16 operands.  A stage is HALF a 32-row block (one 16-row MFMA chunk) of all four planes,
// [a_hi (GA tiles) | a_lo (GA) | b_hi (GB) | b_lo (GB)] x 1 KB — the same bytes, ring and DMA count per thread as the bf16
// core's stage of the same shape, twice the stages, three MFMAs per tile pair: per operand byte 1.5x the MFMA work of the
// bf16 kernel.  DMA i of a stage moves the 1 KB planes 8 i .. 8 i + 7, one per wave.
// TWO (x3 == 2, rg_mlp_frag.h: x3_dz_planes() == 1): the A operand (dZ) is ONE plane — a stage is [a_hi (GA) | b_hi (GB) | b_lo (GB)],
// two MFMAs per tile pair (a_hi.b_lo + a_hi.b_hi).
template <typename S, bool TWO = false>
__device__ __forceinline__ void wgrad_x3_shape_core(const WgradFragArgs& g, int ng, int kg, int mb_begin, int mb_end, float* part,
                                                    char* smem) {
  constexpr int GA = S::GA, GB = S::GB, TA = S::TA, TB = S::TB;
  constexpr int PA = TWO ? GA : 2 * GA;                     // A planes of a stage
  constexpr int DMA = TWO ? (PA + 2 * GB + 7) / 8 : S::DMA; // 1 KB planes, eight (one per wave) per DMA
  constexpr int STAGE_BYTES = TWO ? DMA * 8 * 1024 : S::STAGE_BYTES;
  constexpr int SLOTS = TWO ? (STAGE_BYTES <= 32 * 1024 ? 4 : 3) : S::SLOTS, FLY = SLOTS - 1;
  static_assert(SLOTS * STAGE_BYTES <= WG_SHAPED_LDS, "LDS of the two-product stage ring");
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int wn = wave / S::WK, wk = wave % S::WK;
  const int ta0 = ng * GA, tb0 = kg * GB;
  const int na = (g.NTa - ta0 < GA) ? g.NTa - ta0 : GA, nb = (g.NTb - tb0 < GB) ? g.NTb - tb0 : GB;
  f32x16 acc[TA][TB];
  wgrad_clear(acc);
  const int n_stage = 2 * (mb_end - mb_begin);
  // out-of-range tiles / stages read a clamped valid address (never used), so every wave has exactly DMA loads per stage;
  // base pointer and block stride of each are worked out once (see wgrad_shape_core)
  const int nta = g.NTa, ntb = g.NTb;
  const bf16_t* a_hi = g.a_frag;
  const bf16_t* b_hi = g.b_frag;
  const long a_lo = g.a_lo, b_lo = g.b_lo;
  const bf16_t* src0[DMA];
  long blk_stride[DMA];
#pragma unroll
  for (int i = 0; i < DMA; ++i) {
    const int q = i * 8 + wave;  // plane of this wave's DMA (wave-uniform)
    const bool is_a = q < PA;
    const int qa = q < GA ? q : q - GA;                  // tile within the A planes
    int qb = q - PA;                                     // within the B planes (hi, lo, padding)
    const bool b_is_lo = qb >= GB;
    qb = qb >= GB ? qb - GB : qb;
    qb = qb < 0 ? 0 : qb;
    const long tile = is_a ? (long)(ta0 + (qa < na ? qa : na - 1)) : (long)(tb0 + (qb < nb ? qb : nb - 1));
    const long plane = is_a ? (q >= GA ? a_lo : 0) : (b_is_lo ? b_lo : 0);
    const bf16_t* base = is_a ? a_hi : b_hi;
    src0[i] = base + plane + tile * 1024 + lane * 8;
    blk_stride[i] = (long)(is_a ? nta : ntb) * 1024;
  }
  auto issue = [&](int st, int slot) {
    const int sc = st < n_stage ? st : n_stage - 1;
    const long mb = mb_begin + (sc >> 1);
    const int h = sc & 1;
    static_for<0, DMA>([&](auto i_c) __attribute__((always_inline)) {
      constexpr int i = decltype(i_c)::value;
      global_load_lds_b128(src0[i] + mb * blk_stride[i] + h * 512, smem + slot * STAGE_BYTES + (i * 8 + wave) * 1024);
    });
  };
  const bool wave_has_tiles = wn * TA < na && wk * TB < nb;
  auto compute = [&](int slot) {
    if (!wave_has_tiles) return;
    const char* base = smem + slot * STAGE_BYTES + lane * 16;
    u16x8 ah[TA], al[TA], bh[TB], bl[TB];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      ah[i] = *(const u16x8*)(base + (wn * TA + i) * 1024);
      if (!TWO) al[i] = *(const u16x8*)(base + (GA + wn * TA + i) * 1024);
    }
#pragma unroll
    for (int j = 0; j < TB; ++j) {
      bh[j] = *(const u16x8*)(base + (PA + wk * TB + j) * 1024);
      bl[j] = *(const u16x8*)(base + (PA + GB + wk * TB + j) * 1024);
    }
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int j = 0; j < TB; ++j) {  // the small products first
        if (!TWO) acc[i][j] = mfma_32x32x16_bf16(al[i], bh[j], acc[i][j]);
        acc[i][j] = mfma_32x32x16_bf16(ah[i], bl[j], acc[i][j]);
        acc[i][j] = mfma_32x32x16_bf16(ah[i], bh[j], acc[i][j]);
      }
  };
  if (n_stage > 0) {
    static_for<0, FLY>([&](auto f_c) __attribute__((always_inline)) { issue(decltype(f_c)::value, decltype(f_c)::value); });
    for (int t = 0; t < n_stage; ++t) {
      wait_vmcnt<(FLY - 1) * DMA>();  // FLY stages outstanding: the oldest has landed
      raw_barrier();                  // ... for every wave, and all are done reading stage t-1, whose slot is refilled next
      issue(t + FLY, (t + FLY) % SLOTS);
      compute(t % SLOTS);
    }
    wait_vmcnt<0>();
  }
  wgrad_store_f32(g, acc, ta0 + wn * TA, tb0 + wk * TB, lane, part);
}

// the workgroup's core for its layer's tile shape and operand format (all arguments workgroup-uniform)
template <typename S>
__device__ __forceinline__ void wgrad_core(const WgradFragArgs& g, int ng, int kg, int mb_begin, int mb_end, float* part, char* smem) {
  if (g.x3 == 2) wgrad_x3_shape_core<S, true>(g, ng, kg, mb_begin, mb_end, part, smem);  // dZ as one plane (two products)
  else if (g.x3) wgrad_x3_shape_core<S>(g, ng, kg, mb_begin, mb_end, part, smem);
  else wgrad_shape_core<S>(g, ng, kg, mb_begin, mb_end, part, smem);
}
__device__ __forceinline__ void wgrad_dispatch(const WgradFragArgs& g, int ng, int kg, int mb_begin, int mb_end, float* part,
                                               char* smem) {
  switch (g.shape) {
    case WG_SHAPE_16x4: wgrad_core<WgS16x4>(g, ng, kg, mb_begin, mb_end, part, smem); break;
    case WG_SHAPE_4x16: wgrad_core<WgS4x16>(g, ng, kg, mb_begin, mb_end, part, smem); break;
    case WG_SHAPE_2x16: wgrad_core<WgS2x16>(g, ng, kg, mb_begin, mb_end, part, smem); break;
    case WG_SHAPE_1x16: wgrad_core<WgS1x16>(g, ng, kg, mb_begin, mb_end, part, smem); break;
    default: wgrad_core<WgS8x8>(g, ng, kg, mb_begin, mb_end, part, smem); break;
  }
}

__device__ __forceinline__ void wgrad_frag_body(const WgradFragArgs& g, int bid, char* smem) {
  const int shape = g.shape;
  const int GA = wgrad_shape_ga(shape), GB = wgrad_shape_gb(shape);
  const int n_groups = (g.NTa + GA - 1) / GA, k_groups = (g.NTb + GB - 1) / GB;
  // workgroups that read the same 32-row blocks (the tiles of one split) go to ONE XCD (hardware
  // places block b on XCD b % 8), so the second reader of a fragment hits that XCD's L2 instead of
  // HBM (PMC: 700 MB fetched per launch against 420 MB of unique operands without this)
  const int tiles = k_groups * n_groups;
  // the launch has tiles * 8 * ceil(splits / 8) workgroups per layer; those of a split past the end return at once
  const int xcd = bid & 7, slot = bid >> 3;
  const int split = (slot / tiles) * 8 + xcd, tile = slot % tiles;
  if (split >= g.splits) return;  // padding workgroups of a grouped launch (uniform for the workgroup)
  const int kg = tile % k_groups;
  const int ng = tile / k_groups;
  const int mb_begin0 = g.mb_base + split * g.mb_per_split;
  const int mb_begin = mb_begin0 < g.MB ? mb_begin0 : g.MB;
  const int mb_end = (mb_begin + g.mb_per_split < g.MB) ? mb_begin + g.mb_per_split : g.MB;
  wgrad_dispatch(g, ng, kg, mb_begin, mb_end, g.partial + (long)split * g.slab, smem);
}

__global__ void RG_LAUNCH_BOUNDS(512, 1) wgrad_frag_kernel(WgradFragArgs g) {
  RG_DYN_LDS(smem);
  wgrad_frag_body(g, (int)blockIdx.x, smem);
}

// Weight gradient of a GROUPED layer (QR-DQN's A x N output layer seen as A independent [N, K] layers, one per
// action; rows of the batch sorted by action, qr_grouped.hip): group a owns the rows [row_begin[a], row_begin[a + 1]), i.e.
// the 32-row blocks [row_begin[a] / 32, ceil(row_begin[a + 1] / 32)) of the activation fragments and the same blocks + a of
// the dZ fragments (where the backward launch put group a's copy of each block, the other groups' rows zeroed:
// grouped_dz_rows) — no row masks here.  The block range is cut into `splits` parts.  Workgroup = (group, k-group, split);
// partial slab index group * splits + split.  The ranges live in HBM (they depend on the sampled batch): no host round trip.
struct WgradGroupedArgs {
  WgradFragArgs g;       // a_frag: dZ fragments (NTa tiles of 32 columns), b_frag: activation fragments; N = rows of a group's dW
  const int* row_begin;  // [n_groups + 1], in rows of the grouped space
  int n_groups, splits;
};

__global__ void RG_LAUNCH_BOUNDS(512, 1) wgrad_grouped_kernel(WgradGroupedArgs G) {
  RG_DYN_LDS(smem);
  const int k_groups = (G.g.NTb + 7) / 8;
  const int bid = blockIdx.x;
  const int kg = bid % k_groups, s = (bid / k_groups) % G.splits, a = bid / (k_groups * G.splits);
  const int r0 = G.row_begin[a], r1 = G.row_begin[a + 1];
  const int mb0 = r0 >> 5, mb1 = r1 > r0 ? (r1 + 31) >> 5 : mb0;
  const int per = (mb1 - mb0 + G.splits - 1) / G.splits;
  int b0 = mb0 + s * per, b1 = b0 + per;
  if (b1 > mb1) b1 = mb1;
  if (b0 > mb1) b0 = mb1;
  float* part = G.g.partial + ((long)a * G.splits + s) * G.g.slab;
  WgradFragArgs g = G.g;
  g.a_frag += (long)a * g.NTa * 1024;  // this group's dZ blocks sit `a` blocks late (one block = NTa tiles of 2 KB)
  if (g.x3) wgrad_x3_shape_core<WgS8x8>(g, 0, kg, b0, b1, part, smem);  // split-bf16: both planes of dZ and of the activations
  else wgrad_shape_core<WgS8x8>(g, 0, kg, b0, b1, part, smem);
}

// out[a * slab + e] = sum_s partial[(a * splits + s) * slab + e]
__global__ void reduce_grouped_kernel(const float* __restrict__ partial, long slab, int splits, int n_groups,
                                      float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slab * n_groups) return;
  const long a = i / slab, e = i % slab;
  float s0 = 0.f, s1 = 0.f;
  int k = 0;
  for (; k + 1 < splits; k += 2) {
    s0 += stream_load(partial + (a * splits + k) * slab + e);
    s1 += stream_load(partial + (a * splits + k + 1) * slab + e);
  }
  if (k < splits) s0 += stream_load(partial + (a * splits + k) * slab + e);
  out[i] = s0 + s1;
}

// all layers of a stack in ONE launch (workgroups of the small layers fill the CUs the big ones
// leave idle; 4 launches + 4 reduces become 1 + 1)
// (an ENTRY is a layer, or one of the two classes of splits of an unevenly split layer: rg_mlp_wgrad_fused)
constexpr int WG_MAXV = FB_MAXL + 4;
struct WgradGroupArgs {
  int n;
  int wg_begin[WG_MAXV + 1];
  WgradFragArgs layer[WG_MAXV];
};

__global__ void RG_LAUNCH_BOUNDS(512, 1) wgrad_group_kernel(WgradGroupArgs G) {
  RG_DYN_LDS(smem);
  const int bid = blockIdx.x;
  WgradFragArgs g = G.layer[0];
  int base = 0;
#pragma unroll
  for (int i = 1; i < WG_MAXV; ++i)
    if (i < G.n && bid >= G.wg_begin[i]) {
      g = G.layer[i];
      base = G.wg_begin[i];
    }
  wgrad_frag_body(g, bid - base, smem);
}

struct ReduceGroupArgs {
  int n;
  long elem_begin[FB_MAXL + 1];  // in THREADS: one per element (row-major fp32 partials), 256 per 32 x 32 tile (part_mode 1)
  const float* partial[FB_MAXL];
  long slab[FB_MAXL];
  int splits[FB_MAXL];
  float* out[FB_MAXL];
  // part_mode 1 layers (WgradFragArgs.part_mode): bf16 partial tiles in accumulator order; N x K = valid extents of dW
  int mode[FB_MAXL], NTb[FB_MAXL], N[FB_MAXL], K[FB_MAXL];
};

// One 256-thread workgroup = one 32 x 32 tile: wave w sums the lane records (16 values, 32 contiguous bytes per split) of the
// w-th quarter of the splits — all of a quarter's records requested before the first is added (REDUCE_FLY_BF16 at a
// time): the launch runs on loads in flight, 148 workgroups of one wave each were 16 dependent round trips — the four
// quarter sums meet in LDS and are added in a fixed order.  Writes the row-major dW.
__device__ __forceinline__ void reduce_tiles_bf16(const float* part, long slab, int splits, float* out, int NTb, int N, int K,
                                                  long t, float (*red)[16][64]) {
  typedef __attribute__((ext_vector_type(4))) unsigned pk4_t;
  const int lane = (int)(t & 63), w = (int)((t >> 6) & 3);
  const long tile = t >> 8;
  const int tn = (int)(tile / NTb), tk = (int)(tile % NTb);
  const int lr = lane & 31, lg = lane >> 5;
  float s0[16], s1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) s0[r] = s1[r] = 0.f;
  const char* p = (const char*)part + (tile * 1024 + lane * 16) * 2;
  const long stride = slab * 4;  // bytes between the splits' slabs
  auto add = [&](float (&s)[16], const pk4_t a, const pk4_t b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s[2 * q] += __builtin_bit_cast(float, a[q] << 16);
      s[2 * q + 1] += __builtin_bit_cast(float, a[q] & 0xffff0000u);
      s[8 + 2 * q] += __builtin_bit_cast(float, b[q] << 16);
      s[8 + 2 * q + 1] += __builtin_bit_cast(float, b[q] & 0xffff0000u);
    }
  };
  const int per = (splits + 3) >> 2;
  int k = w * per;
  const int k_end = (k + per < splits) ? k + per : splits;
  constexpr int U = REDUCE_FLY_BF16;
  for (; k + U <= k_end; k += U) {
    pk4_t a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const pk4_t* rec = (const pk4_t*)(p + (k + u) * stride);
      a[u] = rec[0];
      b[u] = rec[1];
    }
#pragma unroll
    for (int u = 0; u < U; u += 2) {
      add(s0, a[u], b[u]);
      add(s1, a[u + 1], b[u + 1]);
    }
  }
  for (; k + 1 < k_end; k += 2) {
    const pk4_t* r0 = (const pk4_t*)(p + k * stride);
    const pk4_t* r1 = (const pk4_t*)(p + (k + 1) * stride);
    add(s0, r0[0], r0[1]);
    add(s1, r1[0], r1[1]);
  }
  if (k < k_end) {
    const pk4_t* r0 = (const pk4_t*)(p + k * stride);
    add(s0, r0[0], r0[1]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[w][r][lane] = s0[r] + s1[r];
  __syncthreads();
  const int col = tk * 32 + lr;
  if (col >= K) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // this wave finishes the accumulator registers 4 w .. 4 w + 3: rows 8 w + q + 4 lg of the tile
    const int r = 4 * w + q;
    const int row = tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
    if (row < N) out[(long)row * K + col] = (red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]);
  }
}

__device__ __forceinline__ void reduce_group_body(const ReduceGroupArgs& R, long i) {
  if (i >= R.elem_begin[R.n]) return;
  const float* part = R.partial[0];
  long slab = R.slab[0], base = 0;
  int splits = R.splits[0];
  float* out = R.out[0];
  int mode = R.mode[0], NTb = R.NTb[0], N = R.N[0], K = R.K[0];
#pragma unroll
  for (int k = 1; k < FB_MAXL; ++k)
    if (k < R.n && i >= R.elem_begin[k]) {
      part = R.partial[k]; slab = R.slab[k]; splits = R.splits[k]; out = R.out[k]; base = R.elem_begin[k];
      mode = R.mode[k]; NTb = R.NTb[k]; N = R.N[k]; K = R.K[k];
    }
  if (mode == 1) {  // (whole workgroups: a layer's range is 256 threads per tile)
    __shared__ float red[4][16][64];
    reduce_tiles_bf16(part, slab, splits, out, NTb, N, K, i - base, red);
    return;
  }
  const long e = i - base;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int k = 0;
#define RG_LDP(p) stream_load(p)  // the split partials are read exactly once
  // REDUCE_FLY loads in flight per thread (round 5; see reduce_tiles_bf16): 32 splits were 8 dependent round trips per wave.
  // Same four chains, same order of additions: bit-identical to the 4-deep loop below.
  for (; k + REDUCE_FLY <= splits; k += REDUCE_FLY) {
    float v[REDUCE_FLY];
#pragma unroll
    for (int u = 0; u < REDUCE_FLY; ++u) v[u] = RG_LDP(part + (long)(k + u) * slab + e);
#pragma unroll
    for (int u = 0; u < REDUCE_FLY; u += 4) {
      s0 += v[u];
      s1 += v[u + 1];
      s2 += v[u + 2];
      s3 += v[u + 3];
    }
  }
  for (; k + 3 < splits; k += 4) {
    s0 += RG_LDP(part + (long)k * slab + e);
    s1 += RG_LDP(part + (long)(k + 1) * slab + e);
    s2 += RG_LDP(part + (long)(k + 2) * slab + e);
    s3 += RG_LDP(part + (long)(k + 3) * slab + e);
  }
  for (; k < splits; ++k) s0 += part[(long)k * slab + e];
  out[e] = (s0 + s1) + (s2 + s3);
}

__global__ void reduce_group_kernel(ReduceGroupArgs R) { reduce_group_body(R, (long)blockIdx.x * blockDim.x + threadIdx.x); }

// The weight gradient's split reduce, the bias gradients' column reduce and (optionally) one scaled sum — the mean loss
// of a step — in ONE launch: blocks [0, elem_blocks) are reduce_group_kernel's, the next cols.block_begin[cols.n] are
// reduce_cols_group_kernel's, the last one is reduce_sum_kernel's (heads.hip), each with its own arithmetic unchanged:
// bit-identical to the three launches (5.6 + 4.6 us of launch-bound tails per C2 step).
struct ReduceTailArgs {
  ReduceGroupArgs splits;
  ReduceColsGroupArgs cols;
  int elem_blocks;
  const float* sum_in;
  int sum_n;
  int sum_run;  // > 1: sum_in holds per-wave sums, runs of sum_run of them are added in order first (rg_reduce.h: strided_sum_256_runs)
  float sum_scale;
  float* sum_out;
};

__global__ void reduce_tail_kernel(ReduceTailArgs T) {
  const int b = blockIdx.x;
  if (b < T.elem_blocks) {
    reduce_group_body(T.splits, (long)b * blockDim.x + threadIdx.x);
    return;
  }
  const int cb = b - T.elem_blocks;
  if (cb < T.cols.block_begin[T.cols.n]) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < FB_MAXL; ++i)
      if (i < T.cols.n && cb >= T.cols.block_begin[i]) l = i;
    reduce_cols_body(T.cols.partials[l], T.cols.S, T.cols.N[l], T.cols.out[l], cb - T.cols.block_begin[l]);
    return;
  }
  // reduce_sum_kernel (heads.hip): strided partial sums, block_sum_256's fixed order
  __shared__ float scratch[4];
  float acc = T.sum_run > 1 ? strided_sum_256_runs(T.sum_in, T.sum_n, T.sum_run, threadIdx.x)
                            : strided_sum_256(T.sum_in, T.sum_n, threadIdx.x);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) T.sum_out[0] = ((scratch[0] + scratch[1]) + (scratch[2] + scratch[3])) * T.sum_scale;
}

__global__ void reduce_splits2_kernel(const float* __restrict__ partials, long slab, int splits,
                                      float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += partials[(long)k * slab + i];
  out[i] = s;
}

}  // namespace rg

using namespace rg;

extern "C" {

struct WgradFragPlan {
  int NTa, NTb, MB, splits, mb_per_split;
  long slab;
  int shape, tiles;  // workgroup tile shape (WG_SHAPE_*) and the number of such tiles that cover dW
};
// workgroups per layer whose dW is ONE tile of its shape (dW0, thin output layers): their partial slab is the whole dW, so
// the 128 of the multi-tile layers would double the partial bytes they had as two tiles x 64 splits
constexpr int WGRAD_TARGET_THIN = 64;
// the shape that stages the fewest bytes for an NTa x NTb-tile dW: groups x 16-byte units per thread and 32-row block
// (the split-bf16 cores take the same shapes: their stage is the same bytes)
static int wgrad_pick_shape(int NTa, int NTb, int* tiles_out) {
  static const int dma[WG_N_SHAPES] = {WgS8x8::DMA, WgS16x4::DMA, WgS4x16::DMA, WgS2x16::DMA, WgS1x16::DMA};
  int best = WG_SHAPE_8x8, best_cost = 0, best_tiles = 0;
  for (int sh = 0; sh < WG_N_SHAPES; ++sh) {
    const int ga = wgrad_shape_ga(sh), gb = wgrad_shape_gb(sh);
    const int tiles = ((NTa + ga - 1) / ga) * ((NTb + gb - 1) / gb);
    const int cost = tiles * dma[sh];
    if (sh == WG_SHAPE_8x8 || cost < best_cost) { best = sh; best_cost = cost; best_tiles = tiles; }
  }
  *tiles_out = best_tiles;
  return best;
}
// splits and 32-row blocks per split of a layer from the workgroups wanted for it (xcd_rows: eight or more splits come in
// whole rows of eight, one per XCD — wgrad_frag_body)
static void wgrad_set_splits(WgradFragPlan& p, int want_wgs, bool xcd_rows) {
  int want = (want_wgs + p.tiles - 1) / p.tiles;
  const int max_splits = (p.MB + WG_MB_STAGE - 1) / WG_MB_STAGE;
  if (want > max_splits) want = max_splits;
  if (want < 1) want = 1;
  if (xcd_rows && want >= 8) want = want / 8 * 8;
  int per = (p.MB + want - 1) / want;
  per = (per + WG_MB_STAGE - 1) / WG_MB_STAGE * WG_MB_STAGE;
  p.mb_per_split = per;
  p.splits = (p.MB + per - 1) / per;
}
static WgradFragPlan wgrad_frag_plan(int out_f, int in_f, int batch) {
  WgradFragPlan p;
  p.NTa = (out_f + 31) / 32; p.NTb = (in_f + 31) / 32;
  p.MB = (batch + 127) / 128 * 4;
  p.shape = wgrad_pick_shape(p.NTa, p.NTb, &p.tiles);
  p.slab = (long)out_f * in_f;
  wgrad_set_splits(p, 256, false);  // ~one workgroup per CU
  return p;
}
// the launch arguments of a plan's layer: bf16 operands, fp32 row-major partials, all of the plan's blocks and splits — a
// caller with another operand format, partial form or block range sets those fields afterwards
static WgradFragArgs wgrad_args(const WgradFragPlan& p, const void* dz_frag, const void* x_frag, int out_f, int in_f,
                                float* partial, long slab) {
  WgradFragArgs g;
  g.a_frag = (const bf16_t*)dz_frag; g.b_frag = (const bf16_t*)x_frag;
  g.NTa = p.NTa; g.NTb = p.NTb; g.MB = p.MB; g.mb_base = 0; g.mb_per_split = p.mb_per_split; g.splits = p.splits;
  g.partial = partial; g.slab = slab; g.N = out_f; g.K = in_f;
  g.x3 = 0; g.a_lo = g.b_lo = 0; g.shape = p.shape; g.part_mode = 0;
  return g;
}

size_t rg_fc_wgrad_frag_workspace_bytes(int out_features, int in_features, int batch) {
  const WgradFragPlan p = wgrad_frag_plan(out_features, in_features, batch > 0 ? batch : 1);
  return (size_t)p.splits * p.slab * sizeof(float);
}

int rg_fc_wgrad_frag(const void* dz_frag, const void* x_frag, int out_features, int in_features, int batch,
                     float* dw, void* workspace, size_t workspace_bytes, rg_stream_t stream) {
  if (!dz_frag || !x_frag || !dw || out_features <= 0 || in_features <= 0 || batch <= 0) return RG_EINVAL;
  const WgradFragPlan p = wgrad_frag_plan(out_features, in_features, batch);
  if (!workspace || workspace_bytes < (size_t)p.splits * p.slab * sizeof(float)) return RG_EWORKSPACE;
  const WgradFragArgs g = wgrad_args(p, dz_frag, x_frag, out_features, in_features, (float*)workspace, p.slab);
  const int grid = p.tiles * ((p.splits + 7) / 8 * 8);
  const size_t lds = (size_t)WG_SHAPED_LDS;
  RG_ALLOW_LDS(wgrad_frag_kernel, lds);
  RG_LAUNCH_DYN(wgrad_frag_kernel, dim3(grid), dim3(WG_THREADS), lds, (hipStream_t)stream, g);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  RG_LAUNCH(reduce_splits2_kernel, dim3((unsigned)((p.slab + 255) / 256)), dim3(256), (hipStream_t)stream,
            (const float*)g.partial, p.slab, p.splits, dw, p.slab);
  return (int)hipGetLastError();
}

size_t rg_group_head_wgrad_workspace_bytes(int n_groups, int group_rows, int in_features, int splits) {
  return (size_t)n_groups * splits * group_rows * in_features * sizeof(float);
}

/* dw [n_groups * group_rows, in_features] of a grouped layer (qr_grouped.hip): group g's rows are the 32-row blocks
 * [row_begin[g] / 32, ceil(row_begin[g + 1] / 32)) of h_frag and the same blocks + g of dz_frag (wgrad_grouped_kernel) */
int rg_group_head_wgrad(const void* dz_frag, const void* h_frag, const int32_t* row_begin, int n_groups, int group_rows,
                        int in_features, int splits, int x3, int rows, float* dw, void* workspace, size_t workspace_bytes,
                        rg_stream_t stream) {
  if (!dz_frag || !h_frag || !row_begin || !dw || n_groups <= 0 || group_rows <= 0 || in_features <= 0 || splits <= 0 ||
      (x3 && rows <= 0))
    return RG_EINVAL;
  if (group_rows > 256) return RG_EUNSUPPORTED;  // one n-group of the 256 x 256 workgroup tile per action
  if (!workspace || workspace_bytes < rg_group_head_wgrad_workspace_bytes(n_groups, group_rows, in_features, splits))
    return RG_EWORKSPACE;
  WgradFragPlan p{};  // one 8 x 8 n-group per group; the block ranges (MB, mb_per_split: 0 here) come from row_begin, in the kernel
  p.NTa = (group_rows + 31) / 32; p.NTb = (in_features + 31) / 32; p.splits = splits; p.shape = WG_SHAPE_8x8;
  WgradGroupedArgs G;
  G.g = wgrad_args(p, dz_frag, h_frag, group_rows, in_features, (float*)workspace, (long)group_rows * in_features);
  // split-bf16: each operand is [hi plane | lo plane] over the `rows` rows of the grouped space (rg_frag_elems apart)
  G.g.x3 = x3 ? 1 : 0;
  G.g.a_lo = x3 ? (long)frag_elems(grouped_dz_rows(rows, n_groups), group_rows) : 0;
  G.g.b_lo = x3 ? (long)frag_elems(rows, in_features) : 0;
  G.row_begin = row_begin; G.n_groups = n_groups; G.splits = splits;
  const int k_groups = (G.g.NTb + 7) / 8;
  const size_t lds = (size_t)WgS8x8::LDS_BYTES;
  RG_ALLOW_LDS(wgrad_grouped_kernel, lds);
  RG_LAUNCH_DYN(wgrad_grouped_kernel, dim3(n_groups * splits * k_groups), dim3(WG_THREADS), lds, (hipStream_t)stream, G);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const long n = G.g.slab * n_groups;
  RG_LAUNCH(reduce_grouped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)stream,
            (const float*)workspace, G.g.slab, splits, n_groups, dw);
  return (int)hipGetLastError();
}

// ---- how many splits per layer --------------------------------------------------------------------------------------
// Round 4 (profiles/microbench/out/r04a: hbm_roof.txt, wgrad_model.txt).  The staging mechanism alone — the LDS-DMA ring of
// one workgroup per CU — draws 7.2 TB/s from HBM when every workgroup streams its own bytes (28 B/ns per CU) and 11.7 TB/s
// into LDS (46 B/ns per CU, 5.9 TB/s of unique bytes) when the tiles of a split sit on one XCD and find each other's operand
// in its L2; LDS fragment reads and MFMAs cost nothing on top, the partial tiles do: 67 MB of them, written when the
// workgroups of a round finish together, are 20 us.  The launch of rounds 1-3 gave every layer 128 workgroups: 512 of
// uneven length (a dW0 workgroup half as long as a hidden layer's) in dispatch order — the CU that drew dW0 then a hidden
// layer finished last, at 3/2 of a balanced schedule — and 86 MB of partials.  (A cost-model plan that makes all workgroups
// one round of the chip was measured slower in round 4: profiles/NOTES_r01_r05.md.)
// The plan's knobs, overridable from the environment so that tests can make a small stack meet the full-size plan:
// total = the CU count (what the uneven split below assumes one round of the chip to be), thin = the workgroups of a
// single-tile layer (WGRAD_TARGET_THIN), uneven = the single-tile block cost in percent of a multi-tile one's (125; 0 = every
// split of a layer the same length).
struct WgradTuning { int total, thin, uneven; };
static const WgradTuning& wgrad_tuning() {
  static const WgradTuning t = [] {
    WgradTuning v{0, WGRAD_TARGET_THIN, 125};
    if (const char* e = getenv("RG_WGRAD_UNEVEN")) v.uneven = atoi(e);
    if (const char* e = getenv("RG_WGRAD_THIN")) v.thin = atoi(e);
    if (const char* e = getenv("RG_WGRAD_TOTAL")) v.total = atoi(e);
    if (v.total <= 0) {
      int dev = 0;
      hipDeviceProp_t pr;
      v.total = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
                    ? pr.multiProcessorCount : 256;
    }
    return v;
  }();
  return t;
}

static WgradFragPlan wgrad_group_plan(int out_f, int in_f, int batch, int target_wgs) {
  WgradFragPlan p = wgrad_frag_plan(out_f, in_f, batch);
  if (p.tiles == 1 && p.shape != WG_SHAPE_8x8 && wgrad_tuning().thin < target_wgs) target_wgs = wgrad_tuning().thin;
  wgrad_set_splits(p, target_wgs, true);
  return p;
}

static void wgrad_stack_plan(const rg_mlp_desc* d, int batch, WgradFragPlan* out) {
  for (int l = 0; l < d->n_layers; ++l) out[l] = wgrad_group_plan(d->dims[l + 1], d->dims[l], batch, WGRAD_TARGET);
}

// floats a split's slab takes in the stack launch: N * K row-major, or NTa * NTb bf16 tile records of 2 KB (a thin layer's
// padded tiles can be the larger)
static long wgrad_slab_floats(const WgradFragPlan& p) {
  const long tiles = (long)p.NTa * p.NTb * 512;
  return tiles > p.slab ? tiles : p.slab;
}

size_t rg_mlp_wgrad_fused_workspace_bytes(const rg_mlp_desc* d, int batch) {
  if (!d || batch <= 0 || d->n_layers < 1 || d->n_layers > FB_MAXL) return 0;
  WgradFragPlan plan[FB_MAXL];
  wgrad_stack_plan(d, batch, plan);
  size_t total = 0;  // in floats; a layer's slab is the larger of its two partial forms (WgradFragArgs.part_mode)
  for (int l = 0; l < d->n_layers; ++l) total += (size_t)plan[l].splits * wgrad_slab_floats(plan[l]);
  return total * sizeof(float);
}

// ---- entries of the stack launch.  An entry is a layer, or one of the two CLASSES of splits of an unevenly split layer.
// Round 4: the layers whose workgroups run longest go first (workgroups are dispatched in id order, one per CU: with dW0's
// short ones first the launch ended at 3/2 of a balanced schedule).  Round 5: that order still leaves a staircase — at C2
// 256 hidden-layer workgroups of 64 blocks take every CU, then the 128 single-tile ones (dW0, the output layer: 32 blocks)
// run on half of the chip while the other half idles: 96 block times for 80 of work per CU.  The splits of the multi-tile
// layers are therefore cut UNEVENLY: a fraction f = (single-tile workgroups) / (multi-tile workgroups) of each layer's
// splits is shorter by what a single-tile workgroup costs (b blocks, weighted by WgradTuning::uneven percent: its stage is a
// single-reader stream, dearer per block), L1 = L - (1 - f) b, the others longer, L2 = L + f b.  Launch order L2 | L1 |
// single-tile: the CUs that drew an L1 workgroup are the ones that free up for a single-tile one, and every CU ends at ~L2.
// (pure integer / double arithmetic on the plans, the flags and the tuning: no HIP call.)  Returns the number of entries.
struct WgradEntry { int layer, mb_base, mb_end, per, splits, split_base; };
static int wgrad_launch_entries(const rg_mlp_desc* d, const WgradFragPlan* plan, const WgradTuning& T, WgradEntry* ent) {
  int n_ent = 0;
  // Applies to the launch it was measured on: every multi-tile layer's workgroups are ONE round of the chip and only
  // single-tile layers follow (C2's stack, either precision: 101 -> 94.7 us, split-bf16 221 -> 203).  Measured and NOT
  // extended (round 5, same box): counting a narrower multi-tile first layer among the followers (C4's critic, 512 x 288:
  // 116 -> 119 us), and any launch that shares the chip with another one (C3's trunk beside the head's weight gradient on
  // the second stream: 113.6 -> 122.6 us — the dispatch order this plan leans on is then not the launch's own; such
  // callers set rg_mlp_desc.wgrad_flags & 1).
  int n_multi = 0, n_single = 0;
  double single_blocks = 0.0;
  for (int l = 0; l < d->n_layers; ++l) {
    if (plan[l].tiles > 1) n_multi += plan[l].tiles * plan[l].splits;
    else { n_single += plan[l].splits; single_blocks += (double)plan[l].splits * plan[l].mb_per_split; }
  }
  const bool uneven = T.uneven > 0 && !(d->wgrad_flags & 1) && n_multi == T.total && n_single > 0 &&
                      n_single <= n_multi && d->n_layers + 2 <= WG_MAXV;
  const double f = uneven ? (double)n_single / n_multi : 0.0;
  const double b = uneven ? single_blocks / n_single * T.uneven / 100.0 : 0.0;
  for (int l = 0; l < d->n_layers; ++l) {
    const WgradFragPlan& p = plan[l];
    int s_short = (uneven && p.tiles > 1) ? ((int)(f * p.splits + 0.5) + 4) / 8 * 8 : 0;  // whole XCD rows of splits (wgrad_frag_body)
    // (an entry is kept in reserve for every layer still to come: the table has WG_MAXV slots)
    if (s_short <= 0 || s_short >= p.splits || n_ent + 2 + (d->n_layers - 1 - l) > WG_MAXV) s_short = 0;
    if (!s_short) {
      ent[n_ent++] = WgradEntry{l, 0, p.MB, p.mb_per_split, p.splits, 0};
      continue;
    }
    const int s_long = p.splits - s_short;
    const double fl = (double)s_short / p.splits;
    int L1 = (int)((double)p.MB / p.splits - (1.0 - fl) * b + 0.5);
    if (L1 < 1) L1 = 1;
    int L2 = (p.MB - s_short * L1 + s_long - 1) / s_long;
    const int cut = s_long * L2 < p.MB ? s_long * L2 : p.MB;
    L1 = (p.MB - cut + s_short - 1) / s_short;  // the short class covers exactly what is left
    ent[n_ent++] = WgradEntry{l, 0, cut, L2, s_long, 0};
    ent[n_ent++] = WgradEntry{l, cut, p.MB, L1 > 0 ? L1 : 1, s_short, s_long};
  }
  for (int i = 1; i < n_ent; ++i)  // stable insertion sort by descending blocks per split
    for (int j = i; j > 0 && ent[j].per > ent[j - 1].per; --j) { const WgradEntry t = ent[j]; ent[j] = ent[j - 1]; ent[j - 1] = t; }
  return n_ent;
}

/* dw[l] = dz_frag[l]^T act_frag[l] for every layer, one wgrad launch + one reduce launch */
int rg_mlp_wgrad_fused(const rg_mlp_desc* d, int batch, void* workspace, size_t workspace_bytes,
                       rg_stream_t stream) {
  if (!d || batch <= 0 || d->n_layers < 1 || d->n_layers > FB_MAXL) return RG_EINVAL;
  if (!workspace || workspace_bytes < rg_mlp_wgrad_fused_workspace_bytes(d, batch)) return RG_EWORKSPACE;
  WgradFragPlan plan[FB_MAXL];  // per layer: the ones the workspace size was worked out from
  wgrad_stack_plan(d, batch, plan);
  WgradEntry ent[WG_MAXV];  // in launch order
  const int n_ent = wgrad_launch_entries(d, plan, wgrad_tuning(), ent);
  if (getenv("RG_WGRAD_DEBUG")) {  // the launch plan, once per distinct shape (diagnostics: profiles/scripts)
    static int shown_batch = -1, shown_layers = -1;
    if (shown_batch != batch || shown_layers != d->n_layers) {
      shown_batch = batch; shown_layers = d->n_layers;
      for (int j = 0; j < n_ent; ++j)
        fprintf(stderr, "rg_mlp_wgrad_fused: entry %d layer %d (dW %d x %d, %d tile%s) blocks [%d, %d) in %d splits of %d\n", j, ent[j].layer,
                d->dims[ent[j].layer + 1], d->dims[ent[j].layer], plan[ent[j].layer].tiles, plan[ent[j].layer].tiles > 1 ? "s" : "",
                ent[j].mb_base, ent[j].mb_end, ent[j].splits, ent[j].per);
    }
  }
  // ---- the argument tables and the two launches
  // bf16 stacks: the splits' partial tiles as bf16 in accumulator order (half the bytes written here and read by the
  // reduce; error 2^-9 of a PARTIAL sum, far inside what bf16 operands cost the gradient).  Split-bf16 stacks: fp32.
  const int part_mode = d->x3 ? 0 : 1;
  WgradGroupArgs G;
  ReduceGroupArgs R;
  R.n = d->n_layers;
  float* part = (float*)workspace;
  long el = 0;
  for (int l = 0; l < FB_MAXL; ++l) {
    R.elem_begin[l] = el;
    if (l < d->n_layers) {
      if (!d->dz_frag[l] || !d->act_frag[l] || !d->dw[l]) return RG_EINVAL;
      const int out_f = d->dims[l + 1], in_f = d->dims[l];
      const WgradFragPlan& p = plan[l];
      const long slab = wgrad_slab_floats(p);
      R.partial[l] = part; R.slab[l] = slab; R.splits[l] = p.splits; R.out[l] = d->dw[l];
      R.mode[l] = part_mode; R.NTb[l] = p.NTb; R.N[l] = out_f; R.K[l] = in_f;
      part += (size_t)p.splits * slab;
      el += part_mode == 1 ? (long)p.NTa * p.NTb * 256 : p.slab;  // threads of the reduce launch: a workgroup per tile, or one per element
    } else {
      R.partial[l] = nullptr; R.slab[l] = 0; R.splits[l] = 0; R.out[l] = nullptr;
      R.mode[l] = 0; R.NTb[l] = 1; R.N[l] = 0; R.K[l] = 0;
    }
  }
  pad_begin_table(R.elem_begin, d->n_layers, el);
  G.n = n_ent;
  int wg = 0;
  for (int j = 0; j < WG_MAXV; ++j) {  // workgroup ranges in launch order
    G.wg_begin[j] = wg;
    if (j >= n_ent) {
      G.layer[j] = G.layer[0];
      continue;
    }
    const WgradEntry& e = ent[j];
    const int l = e.layer;
    const WgradFragPlan& p = plan[l];
    WgradFragArgs& g = G.layer[j];
    g = wgrad_args(p, d->dz_frag[l], d->act_frag[l], d->dims[l + 1], d->dims[l], (float*)R.partial[l] + (size_t)e.split_base * R.slab[l], R.slab[l]);
    g.MB = e.mb_end; g.mb_base = e.mb_base; g.mb_per_split = e.per; g.splits = e.splits;
    g.x3 = d->x3 ? (x3_dz_planes() == 1 ? 2 : 1) : 0;
    g.a_lo = d->x3 ? (long)frag_elems(batch, d->dims[l + 1]) : 0;
    g.b_lo = d->x3 ? (long)frag_elems(batch, d->dims[l]) : 0;
    g.part_mode = part_mode;
    wg += p.tiles * ((e.splits + 7) / 8 * 8);  // the tiles of a split on ONE XCD (wgrad_frag_body), eight splits abreast
  }
  G.wg_begin[WG_MAXV] = wg;
  const size_t lds = (size_t)WG_SHAPED_LDS;
  RG_ALLOW_LDS(wgrad_group_kernel, lds);
  RG_LAUNCH_DYN(wgrad_group_kernel, dim3(wg), dim3(WG_THREADS), lds, (hipStream_t)stream, G);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const int elem_blocks = (int)((el + 255) / 256);
  if (!d->db_partials && !d->sum_in) {
    RG_LAUNCH(reduce_group_kernel, dim3((unsigned)elem_blocks), dim3(256), (hipStream_t)stream, R);
    return (int)hipGetLastError();
  }
  // tails folded into this launch: the bias partials rg_mlp_backward_fused(defer_db) left in ITS workspace (layout as
  // there: [n_wg][dims[l+1]] per layer with a bias gradient, in layer order) and one scaled sum
  ReduceTailArgs T;
  T.splits = R;
  T.elem_blocks = elem_blocks;
  const int n_wg = padded_wgs(d, batch);
  const float* db_part[FB_MAXL] = {};
  const float* p = d->db_partials;
  for (int l = 0; p && l < d->n_layers; p += (size_t)n_wg * d->dims[l + 1], ++l)
    if (d->db[l]) db_part[l] = p;
  const int blocks = fill_reduce_cols(T.cols, n_wg, d->n_layers, db_part, d->db, d->dims + 1);
  if (d->sum_in && (!d->sum_out || d->sum_n <= 0)) return RG_EINVAL;
  T.sum_in = d->sum_in; T.sum_n = d->sum_n; T.sum_run = d->sum_run; T.sum_scale = (float)d->sum_scale; T.sum_out = d->sum_out;
  RG_LAUNCH(reduce_tail_kernel, dim3((unsigned)(elem_blocks + blocks + (d->sum_in ? 1 : 0))), dim3(256), (hipStream_t)stream, T);
  return (int)hipGetLastError();
}

}  // extern "C"
