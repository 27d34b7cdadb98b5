// mlp_fused.hip — the bf16 forward and backward of a FullyConnected stack: whole-network kernels that keep a 128-row
// activation tile resident in LDS across all layers (plain, grouped-output and dx-only forms; the paired online forward
// of a DQN step with its TD head) and the bias gradients' column reduce.  The weight gradient: mlp_wgrad.hip.
//
// Why (measured on MI355X, profiles/r01_run1): one GEMM launch per layer is bound by the HBM
// round trip of the [batch, 512] activation (67 MB bf16) between layers and by 2-byte epilogue
// stores, not by MFMA.  Here
//   * a workgroup (8 waves, 512 threads) owns 128 rows; the activation tile lives in LDS
//     (128 x (width+8) bf16 = 133 KB of the CU's 160 KB) and is rewritten in place layer by layer;
//   * each wave owns 32*TN output columns of a hidden layer (all 128 rows): its weight operand is
//     private, so weights are pre-staged in HBM in B-fragment order and stream L2 -> VGPR as
//     perfectly coalesced 1 KB wave loads, no LDS and no barrier on the weight path;
//   * what backward needs is stored straight from the accumulators in "C-fragment order"
//     (lane = column, 8 rows per lane per half-tile; 1 KB coalesced stores).  Both operands of the weight gradient (dZ
//     and X) leave in that order, which it reads as MFMA A/B fragments directly: no transposes, no 2-byte stores.
//
// Replaces: FullyConnectedNetwork.forward (reagent/models/fully_connected_network.py:157-163)
// and its autograd backward for stacks whose hidden layers share one width in {256, 512}.

#include "rg_mlp_frag.h"
#include "rg_reduce.h"
#include "rg_dqn_head_row.h"

namespace rg {

constexpr int GROUPED_RING = 8;      // weight chunks in flight per wave in the grouped whole-tile output's K loop

// NW waves per workgroup, each owning 32*TN columns of a hidden layer (hidden width = 32*TN*NW).
// NW = 4 (one wave per SIMD, up to 512 registers each): 16 accumulator tiles per wave and a weight
// ring deep enough to cover the L2 latency from a single wave.  NW = 8: two waves per SIMD.
template <int NW> struct MlpCfg {
  static constexpr int THREADS = NW * 64;
  static constexpr int RING = NW == 4 ? 8 : 2;
};

// Grouped forward, the LAST segment of a tile (mlp_fwd_fused_body): wave w sums column tile w of the group's [N, K] layer for all four
// row tiles in the software-pipelined main loop (one weight stream per wave, ring of 8 chunks), the 128 x N outputs are staged
// in the activation tile — dead once every wave has left its K loop — as 128 x P floats and leave as whole rows, a wave per row.
// (Its own function, with its own lane / wave derivations: written out inside the segment loop the 512-wide kernel spilled 45
// registers; called through a non-inlined function 70.)
template <int NW>
__device__ __forceinline__ void grouped_whole_tile_out(bf16_t* act, int pitch, int KC, const bf16_t* wf_out, const float* b_out,
                                                                 int N, int NTo, int out_act, int lo, int hi, int row_base,
                                                                 const int* scatter, int batch, float* out32, long ldo) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), lr = lane & 31, lg = lane >> 5;
  const int P = NTo * 32 + 4, np = N >> 2;
  f32x16 acc4[4][1];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc4[tm][0][r] = 0.f;
  const int col = wave * 32 + lr;
  float b = 0.f;
  if (wave < NTo) {
    if (b_out && col < N) b = b_out[col];  // (requested before the K loop)
    wide_mainloop<1, GROUPED_RING>(act, pitch, KC, wf_out + (long)wave * KC * 512, 0, acc4, lane, k_rotation(blockIdx.x, wave, KC));
  }
  RG_STAMP(16);
  __syncthreads();  // every wave is done reading the layer input
  RG_STAMP(17);
  float* stage = (float*)act;
  if (wave < NTo) {
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = acc4[tm][0][r] + b;
      act_apply_n(v, out_act);
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[(tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg) * P + col] = v[r];
    }
  }
  __syncthreads();
  RG_STAMP(18);
  for (int rel = lo + wave; rel < hi; rel += NW) {  // a wave per row: np <= 64 16-byte pieces
    int row = row_base + rel;
    if (scatter) row = scatter[row];  // back to batch order; padding rows (-1) are dropped
    if (row >= 0 && (scatter || row < batch) && lane < np)
      stream_store(*(const f32x4*)(stage + rel * P + lane * 4), (f32x4*)(out32 + (long)row * ldo + lane * 4));
  }
  RG_STAMP(19);
}

// PITCH (LDS row pitch in elements) is a template constant so that every LDS offset of the
// epilogue stores folds into an instruction immediate instead of a vector add per store.
// (Persistent workgroups — one per CU walking tile, tile + 256 with the next tile's input rows requested
// during the output layer — were measured: 78.8-79.3 us against 80.1 us per launch in
// profiles/microbench/fwd_phases, but 92 against 85 us inside the training step, where the static
// tile assignment loses the dispatcher's load balancing; the kernel stays one tile per workgroup.)
// GROUPED: the launch of a stack whose output layer takes per-tile weights (rg_mlp_desc.tile_key, qr_grouped.hip) is its
// own instantiation — the ordinary kernel does not carry its code paths (or their registers).
// PAIR: one pass of the paired online forward (mlp_fwd_pair_kernel, below): the same workgroup runs this body twice over the
// same LDS tile — `pass` 0 / 1, `on_state` = this pass reads `state` and saves, else `next_state` — with the thin output
// layer's weights copied to LDS in pass 0 only, the first pass's Q rows parked behind them, and the TD head
// (rg_dqn_head_row.h) in the row-store pass of the second output layer.
template <int TN, int NW, int PITCH, bool GROUPED, bool PAIR = false>
__device__ __forceinline__ void mlp_fwd_fused_body(const MlpArgs& a, const PairArgs* pp = nullptr, int pass = 0, bool on_state = false) {
  constexpr int THREADS = MlpCfg<NW>::THREADS, RING = MlpCfg<NW>::RING;
  static_assert(!PAIR || (!GROUPED && NW == 8), "the pair is the plain 8-wave kernel");
  const int save = PAIR ? (on_state ? 1 : 0) : a.save;
  RG_DYN_LDS(smem);
  bf16_t* act = (bf16_t*)smem;
  // (PAIR: an opaque copy per pass — what the two copies of the body derive from the lane is the same, and shared between
  // them those addresses would sit in registers across the hidden layers' main loops)
  const int tid = PAIR ? opaque((int)threadIdx.x) : (int)threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int lr = lane & 31, lg = lane >> 5;
  const int tile = GROUPED ? grouped_tile(blockIdx.x, (a.batch + FB_BM - 1) / FB_BM) : (int)blockIdx.x;
  if (GROUPED && tile * FB_BM >= round_up(a.batch, FB_BM)) return;  // padding blocks (workgroup-uniform)
  const int row_base = tile * FB_BM;
  constexpr int pitch = PITCH;
  const int k0p = round_up(a.dims[0], 32);
  RG_STAMP(0);
  if constexpr (PAIR) {
    const PairIO& io = pp->io[on_state ? 1 : 0];
    const void* x = io.x;
    const long ldx = io.ldx;
    if (io.x_is_f32)
      load_tile_to_lds<float, THREADS>(act, pitch, (const float*)x, ldx, row_base, a.batch, a.dims[0], k0p, tid);
    else
      load_tile_to_lds<bf16_t, THREADS>(act, pitch, (const bf16_t*)x, ldx, row_base, a.batch, a.dims[0], k0p, tid);
  } else if (a.rowmap) {  // grouped space: rows gathered through the map
    if (a.x_is_f32)
      load_tile_rows_mapped<float, THREADS>(act, pitch, (const float*)a.x, a.ldx, a.rowmap, row_base, a.dims[0], k0p, tid);
    else
      load_tile_rows_mapped<bf16_t, THREADS>(act, pitch, (const bf16_t*)a.x, a.ldx, a.rowmap, row_base, a.dims[0], k0p, tid);
  } else if (a.x2) {  // two panels (state | action): columns [0, x_split) from x (row r / x_tile), the rest from x2
    const int n2 = a.dims[0] - a.x_split;
    if (a.x_is_f32)  // each panel in its own element type (bf16 state rows from the sampler next to fp32 actions)
      load_tile_to_lds<float, THREADS>(act, pitch, (const float*)a.x, a.ldx, row_base, a.batch, a.x_split, a.x_split, tid, a.x_tile);
    else
      load_tile_to_lds<bf16_t, THREADS>(act, pitch, (const bf16_t*)a.x, a.ldx, row_base, a.batch, a.x_split, a.x_split, tid, a.x_tile);
    if (a.x2_is_f32)
      load_tile_to_lds<float, THREADS>(act + a.x_split, pitch, (const float*)a.x2, a.ldx2, row_base, a.batch, n2, k0p - a.x_split, tid);
    else
      load_tile_to_lds<bf16_t, THREADS>(act + a.x_split, pitch, (const bf16_t*)a.x2, a.ldx2, row_base, a.batch, n2, k0p - a.x_split, tid);
  } else if (a.x_is_f32)
    load_tile_to_lds<float, THREADS>(act, pitch, (const float*)a.x, a.ldx, row_base, a.batch, a.dims[0], k0p, tid);
  else
    load_tile_to_lds<bf16_t, THREADS>(act, pitch, (const bf16_t*)a.x, a.ldx, row_base, a.batch, a.dims[0], k0p, tid);
  __syncthreads();
  RG_STAMP(1);
  if (save == 1 && a.act_frag[0]) emit_frags_from_lds(act, pitch, k0p / 32, a.act_frag[0], tile * 4, wave, NW, lane);
  // a thin output layer's weights travel to LDS while the hidden layers compute (rg_mlp_frag.h: out_lds_prefetch)
  const bool out_lds = PAIR || (!GROUPED && a.out_lds);
  char* wo = (char*)(act + FB_BM * pitch);
  if (out_lds && pass == 0) out_lds_prefetch(a.wfrag[a.n_layers - 1], (a.dims[a.n_layers - 1] + 15) / 16, wo, wave, NW, lane);

  for (int l = 0; l < a.n_layers; ++l) {
    const int K = a.dims[l], N = a.dims[l + 1];
    const int KC = (K + 15) / 16;
    if (l < a.n_layers - 1) {  // hidden layer, N == 32 * TN * NW
      f32x16 acc[4][TN];
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
      const long nt_stride = (long)KC * 512;
      wide_mainloop<TN, RING>(act, pitch, KC, a.wfrag[l] + (long)(wave * TN) * nt_stride, nt_stride, acc, lane,
                              k_rotation(blockIdx.x, wave, KC), wave / (NW / 2));
      RG_STAMP(2 + 4 * l);
      unsigned PK[4][TN][8];
      unsigned* sign_dst = save ? a.act_sign[l + 1] : nullptr;  // plane base; the lane offset is applied at the store
      if constexpr (PAIR) {
        // ReLU hidden layers only (the launch checks): the pair carries two copies of this epilogue, and one per activation
        // kind on top of that puts the kernel's branches out of short range (a scratch slot for the long jumps)
        fwd_hidden_pack<TN, ACT_RELU>(acc, a.bias[l], save ? a.act_frag[l + 1] : nullptr, sign_dst, N / 32, tile * 4, wave, lane, PK);
      } else {
        RG_DISPATCH_ACT(a.acts[l], (fwd_hidden_pack<TN, A_>(acc, a.bias[l], fwd_save_dst(a, l),
                                                            sign_dst, N / 32, tile * 4, wave, lane, PK)));
      }
      RG_STAMP(3 + 4 * l);
      __syncthreads();  // every wave is done reading the layer input
      RG_STAMP(4 + 4 * l);
      store_packed_tiles<TN>(act, pitch, PK, wave, lane);
      if (out_lds) RG_WAIT_VMCNT(0);  // this wave's share of the output layer's weights has landed (long ago) ...
      __syncthreads();                // ... and after the barrier every wave's has
      RG_STAMP(5 + 4 * l);
    } else {  // output layer: 32x32 tiles spread over the waves, fp32 result to HBM
      const int NTo = (N + 31) / 32;
      const int out_act = a.acts[l];
      const bool stream_out = N > 64;
      // grouped output layer: the rows of the tile are cut into segments, one per group (rg_mlp_frag.h: next_segment; a
      // tile inside one group's range is one segment), and each segment's group selects the weight / bias slice; rows that
      // belong to no group have no output.  The plain layer is the one segment [0, 128) of "group 0".
      int seg_g = GROUPED ? a.tile_key[tile] : 0;
      RowSegment seg{0, 0, FB_BM};
      // (grouped: the lane-derived addresses of the segment loop are worked out HERE — hoisted out of that loop and above the
      // hidden layers' main loops they cost the 512-wide kernel 30 spilled registers)
      const int o_lane = GROUPED ? opaque(lane) : lane, o_tid = GROUPED ? opaque(tid) : tid;
      while (!GROUPED || next_segment(a.row_begin, a.n_groups, row_base, FB_BM, seg_g, seg)) {
        const int lane = o_lane, tid = o_tid, lr = lane & 31, lg = lane >> 5;
        const int grp = seg.grp;
        const bf16_t* wf_out = a.wfrag[l] + (GROUPED ? (long)grp * a.group_stride : 0);
        const float* b_out = a.bias[l] ? a.bias[l] + (GROUPED ? (long)grp * N : 0) : nullptr;
        const int tm0 = GROUPED ? seg.lo >> 5 : 0, tm1 = GROUPED ? (seg.hi + 31) >> 5 : 4;  // the segment's 32-row tiles
        // the bias of column tile 0, requested BEFORE the K loop: loaded at the point of use it put one more L2 round trip
        // (~2000 cycles) at the very end of every workgroup whose output is one column tile (16 Q-values, a critic's scalar)
        const float b_tile0 = (b_out && lr < N) ? b_out[lr] : 0.f;
        auto store_tile = [&](const f32x16& acc, int tm, int nt) {
          const int col = nt * 32 + lr;
          if (col < N) {
            const float b = nt == 0 ? b_tile0 : (b_out ? b_out[col] : 0.f);
            float ov[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ov[r] = acc[r] + b;
            act_apply_n(ov, out_act);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rel = tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
              if (GROUPED && (rel < seg.lo || rel >= seg.hi)) continue;  // another segment's row
              int row = row_base + rel;
              if (a.out_scatter) row = a.rowmap[row];  // back to batch order; padding rows (-1) are dropped
              if (row >= 0 && (a.out_scatter || row < a.batch)) {
                const float o = ov[r];
                // a wide output (QR-DQN's 200 quantiles per row: 54 MB per launch, read once by the loss head) streams
                // past the caches (same-box C3 step -1 %); a thin one is a few MB and its reader is next
                if (stream_out) stream_store(o, a.out32 + (long)row * a.ldo + col);
                else a.out32[(long)row * a.ldo + col] = o;
              }
            }
          }
        };
        // (A pipelined variant for 4..8 output column tiles — wave w running wide_mainloop<1> on column tile w, for all four
        // row tiles with a ring of 8 / 16 chunks — was measured on the C3 grouped forward in rounds 2 and 3: 171 us against
        // 169 us for this loop, C3 step 1.119 / 1.121 against 1.101 ms; its burst of output stores at the end costs more than
        // the re-read fragments.  Ablations of the 189 us target forward: head MFMAs removed -43 us, output stores -20..-28.)
        // PAIR: what the head needs of this thread's row (the row-store pass below: 4 lanes per row, dqn_head_lanes_kernel<4>'s
        // mapping) is requested HERE, before the output layer's K loop, like b_tile0 — the hidden layers' accumulators are dead
        f32x4 h_m4, h_qt4, h_ac4;
        float h_rew = 0.f, h_nt = 0.f, h_ge = 0.f;
        int h_b = 0;
        bool h_live = false;
        if constexpr (PAIR) {
          if (pass == 1) {
            const int it = wave * 64 + opaque(lane), row = row_base + (it >> 2);
            h_live = row < a.batch;
            h_b = h_live ? row : a.batch - 1;  // rows past the end: the last row's operands, nothing stored
            const long o = (long)h_b * 16 + (it & 3) * 4;
            h_m4 = *(const f32x4*)(pp->next_mask + o);
            h_qt4 = *(const f32x4*)(pp->qn_target + o);
            h_ac4 = *(const f32x4*)(pp->action + o);
            h_rew = pp->reward[h_b];
            h_nt = pp->not_terminal[h_b];
            if (pp->gamma_exponent) h_ge = pp->gamma_exponent[h_b];
          }
        }
        if (PAIR || (!GROUPED && NTo == 1 && NW == 8 && KC >= 8)) {
          // one column tile (<= 32 outputs, e.g. 16 Q-values): four 32x32 tiles for eight waves.  The loop is a chain
          // of L2 round trips (7 % of a workgroup's life with four waves idle), so two waves share a tile, each
          // summing half of K; the upper four hand their accumulators over through the activation tile, dead by then.
          const int tm = wave & 3, half = wave >> 2, kc_mid = (KC / 2 + 3) / 4 * 4;
          f32x16 acc = out_lds ? tile_kloop_ldsb(act, pitch, wo, tm, lane, half ? kc_mid : 0, half ? KC : kc_mid)
                               : tile_kloop(act, pitch, KC, wf_out, tm, 0, lane, half ? kc_mid : 0, half ? KC : kc_mid);
          RG_STAMP(16);
          __syncthreads();  // every wave is done reading the layer input
          RG_STAMP(17);
          // The 128 x N outputs leave as whole rows, 16 bytes per lane, through the (dead) activation tile — 8 wave stores of
          // 1 KB for 16 Q-values instead of 64 four-byte ones from the accumulators that each touch 32 half-lines (round 5's
          // A/B: profiles/NOTES_r01_r05.md).
          // Both halves of K put their partial sums into the staging area ([half][row][N] floats) and the row-store pass adds
          // them — (lower + upper) + bias, the order of the accumulator hand-off below — one barrier instead of two.
          // (everything the row store needs is worked out HERE, from an opaque copy of the lane: hoisted above the hidden layers'
          // main loops it cost the 512-wide kernel 5 spilled registers)
          const int o_ln = opaque(lane), o_lr = o_ln & 31, o_lg = o_ln >> 5;
          // two forms: rows of whole 16-byte pieces (N % 4 == 0), or — a dense output (ldo == N: e.g. a critic's single column)
          // and a full tile — the tile's 128 x N block as ONE contiguous run, whatever N is
          const bool aligned16 = (reinterpret_cast<uintptr_t>(a.out32) & 15) == 0;
          const bool dense_run = a.ldo == N && row_base + FB_BM <= a.batch;
          const bool rowstore = PAIR || (!a.out_scatter && aligned16 && (dense_run || ((N & 3) == 0 && (a.ldo & 3) == 0)));
          if (rowstore) {  // (workgroup-uniform)
            float* outs = (float*)act + half * (FB_BM * 32);
            float* bias_s = (float*)act + 2 * (FB_BM * 32);  // the bias (requested before the K loop) travels through LDS too
            if (o_lr < N) {
#pragma unroll
              for (int r = 0; r < 16; ++r) outs[(tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * o_lg) * N + o_lr] = acc[r];
              if (wave == 0 && o_lg == 0) bias_s[o_lr] = b_tile0;
            }
            __syncthreads();
            RG_STAMP(18);
            RG_STAMP(19);
            const float* lo_ = (const float*)act;
            const float* hi_ = lo_ + FB_BM * 32;
            if constexpr (PAIR) {  // N == 16 (the launch checks): thread it = row it / 4, float4 it % 4 of the tile's Q block
              const int it = wave * 64 + o_ln, rel = it >> 2, c4 = it & 3, row = row_base + rel;
              const f32x4 l4 = *(const f32x4*)(lo_ + it * 4), h4 = *(const f32x4*)(hi_ + it * 4);
              const f32x4 b4 = *(const f32x4*)(bias_s + c4 * 4);
              float o[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = (l4[e] + h4[e]) + b4[e];
              act_apply_n(o, out_act);
              const f32x4 mine = f32x4{o[0], o[1], o[2], o[3]};
              if (row < a.batch) *(f32x4*)(pp->io[on_state ? 1 : 0].out + (long)row * 16 + c4 * 4) = mine;
              // the first pass's Q rows wait behind the output layer's weights (8 KB; read back by the thread that wrote them)
              f32x4* park = (f32x4*)(wo + (size_t)KC * 512);
              if (pass == 0) {
                park[it] = mine;
              } else {
                const f32x4 other = park[it];
                const f32x4 q4 = on_state ? mine : other, qon4 = on_state ? other : mine;
                const float loss = dqn_head_lanes_row<4>(h_m4, h_qt4, pp->double_q ? qon4 : h_qt4, h_ac4, q4, c4, h_b, h_live, h_rew,
                                                         pp->reward_boosts, h_nt, pp->gamma, pp->gamma_exponent != nullptr, h_ge,
                                                         a.batch, pp->double_q, pp->loss_type, pp->dq, pp->next_q, pp->next_idx,
                                                         pp->q_sel);
                const float ws = dqn_head_wave_sum(loss);  // 16 rows: one of the 16 wave sums dqn_head_lanes_kernel<4> adds per partial
                if (o_ln == 0) pp->wave_sums[tile * NW + wave] = ws;
              }
            } else if (dense_run) {
              float* dst = a.out32 + (long)row_base * N;
              for (int it = wave * 64 + o_ln; it < (FB_BM * N) >> 2; it += THREADS) {
                const f32x4 l4 = *(const f32x4*)(lo_ + it * 4), h4 = *(const f32x4*)(hi_ + it * 4);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (l4[e] + h4[e]) + bias_s[(it * 4 + e) % N];
                act_apply_n(o, out_act);
                *(f32x4*)(dst + it * 4) = f32x4{o[0], o[1], o[2], o[3]};
              }
            }
            const int np = N >> 2;  // 16-byte pieces per row
            for (int it = wave * 64 + o_ln; !PAIR && !dense_run && it < FB_BM * np; it += THREADS) {  // (tid, rebuilt from the live lane: tid itself is dead by now)
              const int rel = it / np, c4 = it - rel * np;
              const int row = row_base + rel;
              if (row < a.batch) {
                const f32x4 l4 = *(const f32x4*)(lo_ + rel * N + c4 * 4), h4 = *(const f32x4*)(hi_ + rel * N + c4 * 4);
                const f32x4 b4 = *(const f32x4*)(bias_s + c4 * 4);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (l4[e] + h4[e]) + b4[e];
                act_apply_n(o, out_act);
                *(f32x4*)(a.out32 + (long)row * a.ldo + c4 * 4) = f32x4{o[0], o[1], o[2], o[3]};
              }
            }
          } else {
            float* hand = (float*)act + (tm * 64 + lane) * 16;
            if (half) {
#pragma unroll
              for (int r = 0; r < 16; r += 4) *(f32x4*)(hand + r) = f32x4{acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
            }
            __syncthreads();
            RG_STAMP(18);
            if (!half) {
#pragma unroll
              for (int r = 0; r < 16; r += 4) {
                const f32x4 o = *(const f32x4*)(hand + r);
                acc[r] += o[0]; acc[r + 1] += o[1]; acc[r + 2] += o[2]; acc[r + 3] += o[3];
              }
              RG_STAMP(19);
              store_tile(acc, tm, 0);
            }
          }
        } else if (GROUPED && NTo <= NW && a.stage_out) {
          // Grouped output layer, wide (QR-DQN: 200 quantiles per row).  Stored straight from the accumulators a wave
          // instruction writes two 128-byte row segments that start 32 * row bytes off a cache line (rows are 800 bytes):
          // partial lines, 54 MB of them per launch (-20..-28 us with the stores removed).  Here the output leaves as
          // whole rows, 16 bytes per lane: one 32-row tile at a time (wave w computes its column tile w) through a staging
          // area BEHIND the activation tile (32 x (32 NTo + 4) floats, 29 KB of the 30 KB the tile leaves of the CU's LDS).
          const int P = NTo * 32 + 4;  // floats per staged row
          const int np = N >> 2;       // 16-byte pieces per row
          // The per-row-tile loop below is a chain of L2 round trips: each of its four passes runs tile_kloop (4 weight
          // chunks in flight per wave, 8 dependent groups) and two barriers — ~45k of the workgroup's cycles for 8k of MFMAs.
          // The LAST segment of a tile (the only one of a tile inside one group's range: all but <= n_groups - 1 tiles of a
          // launch) leaves the activation tile dead after its K loop, so there: wave w sums column tile w for ALL FOUR row tiles
          // in the software-pipelined main loop (one weight stream per wave, ring of 8 chunks), and the 128 x N outputs are staged
          // in the dead activation tile (128 x P floats) and leave as whole rows — two barriers instead of eight.
          bool last_segment = false;
          if ((size_t)FB_BM * P * sizeof(float) <= (size_t)FB_BM * pitch * sizeof(bf16_t)) {
            int g2 = seg_g;
            RowSegment s2;
            last_segment = !next_segment(a.row_begin, a.n_groups, row_base, FB_BM, g2, s2);  // (workgroup-uniform)
          }
          if (last_segment) {
            grouped_whole_tile_out<NW>(act, pitch, KC, wf_out, b_out, N, NTo, out_act, seg.lo, seg.hi, row_base, a.out_scatter ? a.rowmap : nullptr,
                                       a.batch, a.out32, a.ldo);
            break;  // (the last segment)
          }
          float* stage = (float*)(act + FB_BM * pitch);
          for (int tm = tm0; tm < tm1; ++tm) {
            if (wave < NTo) {
              const f32x16 acc = tile_kloop(act, pitch, KC, wf_out, tm, wave, lane);
              const int col = wave * 32 + lr;
              const float b = (b_out && col < N) ? b_out[col] : 0.f;
              float v[16];
#pragma unroll
              for (int r = 0; r < 16; ++r) v[r] = acc[r] + b;
              act_apply_n(v, out_act);
#pragma unroll
              for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * lg) * P + col] = v[r];
            }
            __syncthreads();
            for (int it = tid; it < 32 * np; it += THREADS) {
              const int r = it / np, c4 = it - r * np;
              const int rel = tm * 32 + r;
              if (rel < seg.lo || rel >= seg.hi) continue;  // another segment's row
              int row = row_base + rel;
              if (a.out_scatter) row = a.rowmap[row];  // back to batch order; padding rows (-1) are dropped
              if (row >= 0 && (a.out_scatter || row < a.batch))
                stream_store(*(const f32x4*)(stage + r * P + c4 * 4), (f32x4*)(a.out32 + (long)row * a.ldo + c4 * 4));
            }
            __syncthreads();
          }
        } else {
          for (int t = wave; t < 4 * NTo; t += NW) {
            const int tm = t & 3, nt = t >> 2;
            if (tm < tm0 || tm >= tm1) continue;
            store_tile(tile_kloop(act, pitch, KC, wf_out, tm, nt, lane), tm, nt);
          }
        }
        if (!GROUPED) break;
      }
      RG_STAMP(2 + 4 * l);
    }
  }
}

// The online network's two forwards of a DQN step in one workgroup per 128-row tile: next_state (not saving) and state
// (saving), then the TD head for those rows (rg_dqn_online_pair_forward).  Half of the workgroups run (next_state, state),
// the other half (state, next_state): identical workgroups that start together stay in lockstep, and every CU storing its
// 128 KB of fragment records at the same moment is what the saving forward's PACK phases wait for
// (profiles/NOTES_r07.md); with the orders mixed about half of the CUs are in a saving pass at any moment.
#ifndef RG_PAIR_ORDER_SHIFT
#define RG_PAIR_ORDER_SHIFT 0  // which workgroups take which order: bit RG_PAIR_ORDER_SHIFT of the index (3: every XCD has both)
#endif
template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_fwd_pair_kernel(MlpArgs a, PairArgs p) {
  const bool state_first = (((int)blockIdx.x >> RG_PAIR_ORDER_SHIFT) & 1) != 0;  // (workgroup-uniform)
  // (two copies of the body, not a loop over the pass: in a loop the launch arguments both passes read are hoisted above it
  // and the scalar registers that hold them spill into vector registers the 512-wide kernel does not have)
  mlp_fwd_fused_body<TN, NW, PITCH, false, true>(a, &p, 0, state_first);
  __syncthreads();  // the row-store pass reads the (dead) activation tile the next pass loads its input into
  mlp_fwd_fused_body<TN, NW, PITCH, false, true>(a, &p, 1, !state_first);
}

template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_fwd_fused_kernel(MlpArgs a) {
  mlp_fwd_fused_body<TN, NW, PITCH, false>(a);
}
template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_fwd_grouped_kernel(MlpArgs a) {
  mlp_fwd_fused_body<TN, NW, PITCH, true>(a);
}

// DX_ONLY: a frozen stack — only the input gradient is produced, no dZ fragments are written (rg_mlp_desc.dx_only)
// GROUPED: the stack's output layer takes per-group weights (rg_mlp_desc.tile_key / row_begin): its own instantiation, the
// plain kernel does not carry the segment walk.  The grouped layer's step — dH = dZ . W_g per row's group — runs once per
// segment of the tile on a copy of the dZ tile with the other segments' rows zeroed (they add nothing to the shared
// accumulators); that copy is also what leaves as the segment's dZ fragments (group g's blocks g blocks late: fill_args /
// grouped_dz_rows) and what the segment's bias-gradient partial sums (row tile + g of db_part).  A tile that lies inside one
// group's range is one segment and uses the tile itself.
template <int TN, int NW, int PITCH, bool DX_ONLY, bool GROUPED = false>
__device__ __forceinline__ void mlp_bwd_fused_body(const MlpArgs& a) {
  constexpr int THREADS = MlpCfg<NW>::THREADS, RING = MlpCfg<NW>::RING;
  RG_DYN_LDS(smem);
  bf16_t* act = (bf16_t*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int lr = lane & 31, lg = lane >> 5;
  const int tile = GROUPED ? grouped_tile(blockIdx.x, (a.batch + FB_BM - 1) / FB_BM) : (int)blockIdx.x;
  if (tile * FB_BM >= round_up(a.batch, FB_BM)) return;  // padding blocks of a grouped launch (workgroup-uniform)
  const int row_base = tile * FB_BM;
  constexpr int pitch = PITCH;
  const int L = a.n_layers;
  const int nop = round_up(a.dims[L], 32);
  RG_BSTAMP(0);
  // The sign bits of H_l are requested ahead of step l's main loop so that its epilogue finds them in registers.  The FIRST
  // step's main loop is one or two K chunks long (K = the output width), too short to cover their HBM round trip
  // (bwd_phases: its pack 7.9k cycles against 6.1-6.8k for the other steps), so its request leaves before the dout tile's.
  auto request_signs = [&](int l, unsigned (&sg)[2 * TN]) {
    if (a.act_sign[l] != nullptr) {
      const u32x2* sp = (const u32x2*)(a.act_sign[l] + sign_offset(tile, wave, lane, TN, a.dims[l]));
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const u32x2 t = sp[i];
        sg[2 * i] = t[0];
        sg[2 * i + 1] = t[1];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2 * TN; ++i) sg[i] = 0u;
    }
  };
  unsigned sg_first[2 * TN];
  if (L >= 2) request_signs(L - 1, sg_first);
  // ... and when that step's K is ONE chunk (<= 16 outputs: Q-values, a critic's scalar) so do its weight fragments: the step is
  // then four LDS reads and 4 x TN MFMAs instead of an L2 round trip behind the tile's barrier (bwd_phases: 2.7k cycles).
  const bool first_one_chunk = !GROUPED && L >= 2 && a.dims[L] <= 16;
  u16x8 w_first[TN];
  if (first_one_chunk) {
    const bf16_t* wl = a.wfrag[L - 1] + (long)(wave * TN) * 512 + lane * 8;  // KC = 1: one 512-element record per n-tile
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) w_first[tn] = *(const u16x8*)(wl + tn * 512);
  }
  load_tile_to_lds<float, THREADS>(act, pitch, a.dout32, a.lddo, row_base, a.batch, a.dims[L], nop, tid);
  __syncthreads();
  RG_BSTAMP(1);
  if (!GROUPED) {
    if (!DX_ONLY) emit_frags_from_lds(act, pitch, nop / 32, a.dz_frag[L - 1], tile * 4, wave, NW, lane);
    if (a.db_part[L - 1] && tid < a.dims[L]) {
      float s = 0.f;
      for (int r = 0; r < FB_BM; ++r) s += bf16_to_f32(act[r * pitch + tid]);
      a.db_part[L - 1][(long)tile * a.dims[L] + tid] = s;
    }
  }
  RG_BSTAMP(2);

  for (int l = L - 1; l >= 1; --l) {
    // dH = dZ_l (LDS, width dims[l+1]) . W_l -> [128, dims[l]] ; dZ_{l-1} = dH * act'(H_l)
    const int K = a.dims[l + 1], N = a.dims[l];
    const int KC = (K + 15) / 16;
    f32x16 acc[4][TN];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
    const long nt_stride = (long)KC * 512;
    // sign bits of H_l, requested before the main loop so they are in registers at the epilogue
    unsigned sg[2 * TN];
    const bool use_sign = a.act_sign[l] != nullptr;
    if (l == L - 1) {
#pragma unroll
      for (int i = 0; i < 2 * TN; ++i) sg[i] = sg_first[i];
    } else {
      request_signs(l, sg);
    }
    // The grouped layer's FIRST segment (the only one of a tile inside a group's range) goes through the main loop like a
    // plain layer's tile — one call site, no loop around it (the software-pipelined loop inside a loop over segments spilled
    // 390-460 registers in the 512-wide kernel, accumulator tiles among them) — any further segment through
    // segment_accumulate.  What a segment contributes besides its products — its rows of dZ as fragments for the weight
    // gradient, its bias-gradient partial — is read from the dZ tile with the row range as a mask; only the MFMA operand of a
    // segment that is not the whole tile needs a copy with the other rows zeroed.
    const bool grouped_layer = GROUPED && l == L - 1;
    bf16_t* cp = act + masked_copy_offset<PITCH>(FB_BM * PITCH);
    int seg_g = grouped_layer ? a.tile_key[tile] : 0;
    RowSegment seg{0, 0, FB_BM};
    bool more = grouped_layer ? next_segment(a.row_begin, a.n_groups, row_base, FB_BM, seg_g, seg) : true;
    auto segment_side = [&]() -> const bf16_t* {  // -> the segment's MFMA operand
      const bool whole = seg.lo == 0 && seg.hi == FB_BM;
      if (!whole) {
        copy_rows_masked<THREADS, FB_BM>(act, cp, pitch, nop, seg.lo, seg.hi, tid);
        __syncthreads();
      }
      const bf16_t* src = whole ? act : cp;
      emit_frags_from_lds(src, pitch, nop / 32, a.dz_frag[L - 1], tile * 4 + seg.grp, wave, NW, lane, seg.lo >> 5,
                          (seg.hi + 31) >> 5);
      if (a.db_part[L - 1] && tid < a.dims[L]) {
        float s = 0.f;
        for (int r = seg.lo; r < seg.hi; ++r) s += bf16_to_f32(act[r * pitch + tid]);
        a.db_part[L - 1][(long)(tile + seg.grp) * a.dims[L] + tid] = s;
      }
      return src;
    };
    if (more) {
      const bf16_t* src = act;
      if (grouped_layer) src = segment_side();
      const bf16_t* wl = a.wfrag[l] + (grouped_layer ? (long)seg.grp * a.group_stride : 0);  // the group's slice of W^T
      if (first_one_chunk && l == L - 1) {
        const bf16_t* arow = src + lr * pitch + lg * 8;
        u16x8 af[4];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) af[tm] = *(const u16x8*)(arow + tm * 32 * pitch);
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mfma_main(af[tm], w_first[tn], acc[tm][tn]);
      } else {
        wide_mainloop<TN, RING>(src, pitch, KC, wl + (long)(wave * TN) * nt_stride, nt_stride, acc, lane,
                                k_rotation(blockIdx.x, wave, KC), wave / (NW / 2));
      }
    }
    if (grouped_layer) {
      while (more && next_segment(a.row_begin, a.n_groups, row_base, FB_BM, seg_g, seg)) {  // a boundary tile's other groups
        __syncthreads();  // every wave is done with the previous segment's copy
        const bf16_t* src = segment_side();
        segment_accumulate<4, TN>(src, pitch, KC, a.wfrag[l] + (long)seg.grp * a.group_stride + (long)(wave * TN) * nt_stride,
                                  nt_stride, acc, lane);
      }
    }
    float* dbp = a.db_part[l - 1] ? a.db_part[l - 1] + (long)tile * N : nullptr;
    RG_BSTAMP(3 + 4 * (L - 1 - l));
    unsigned PK[4][TN][8];
    if (use_sign) {
      RG_DISPATCH_ACT(a.acts[l - 1], (bwd_hidden_pack<TN, A_, true, !DX_ONLY>(acc, a.act_frag[l], sg, a.dz_frag[l - 1], dbp,
                                                                             N / 32, tile * 4, wave, lane, PK)));
    } else {
      RG_DISPATCH_ACT(a.acts[l - 1], (bwd_hidden_pack<TN, A_, false, !DX_ONLY>(acc, a.act_frag[l], sg, a.dz_frag[l - 1], dbp,
                                                                              N / 32, tile * 4, wave, lane, PK)));
    }
    RG_BSTAMP(4 + 4 * (L - 1 - l));
    __syncthreads();  // every wave is done reading dZ_l
    RG_BSTAMP(5 + 4 * (L - 1 - l));
    store_packed_tiles<TN>(act, pitch, PK, wave, lane);
    __syncthreads();
    RG_BSTAMP(6 + 4 * (L - 1 - l));
  }
  if (a.dx32) {  // gradient w.r.t. the network input (e.g. the critic's action input in SAC)
    const int K = a.dims[1], N = a.dims[0];
    const int KC = (K + 15) / 16, NTi = (N + 31) / 32, nt0 = a.dx_col0 / 32;  // only the tiles from dx_col0 on
    for (int t = wave; t < 4 * (NTi - nt0); t += NW) {
      const int tm = t & 3, nt = nt0 + (t >> 2);
      const f32x16 acc = tile_kloop(act, pitch, KC, a.wfrag[0], tm, nt, lane);
      const int col = nt * 32 + lr;
      if (col < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row_base + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
          if (row < a.batch) a.dx32[(long)row * a.lddx + col - a.dx_col0] = acc[r];
        }
      }
    }
  }
}

template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_bwd_fused_kernel(MlpArgs a) {
  mlp_bwd_fused_body<TN, NW, PITCH, false>(a);
}
template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_bwd_dx_kernel(MlpArgs a) {
  mlp_bwd_fused_body<TN, NW, PITCH, true>(a);
}
template <int TN, int NW, int PITCH>
__global__ void RG_LAUNCH_BOUNDS(NW * 64, 1) mlp_bwd_grouped_kernel(MlpArgs a) {
  mlp_bwd_fused_body<TN, NW, PITCH, false, true>(a);
}

__global__ void reduce_cols_group_kernel(ReduceColsGroupArgs G) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < FB_MAXL; ++i)
    if (i < G.n && (int)blockIdx.x >= G.block_begin[i]) l = i;
  reduce_cols_body(G.partials[l], G.S, G.N[l], G.out[l], (int)blockIdx.x - G.block_begin[l]);
}

// the three (hidden width, pitch) instantiations of a fused kernel template
#define RG_LAUNCH_FUSED_ARGS(KERNEL, hidden, pitch, grid, lds, stream, ...)                                     \
  do {                                                                                                       \
    const dim3 block_(FB_NW * 64);                                                                           \
    if ((hidden) == 256 && (pitch) == 264) {                                                                 \
      RG_ALLOW_LDS((KERNEL<256 / (32 * FB_NW), FB_NW, 264>), lds);                                           \
      RG_LAUNCH_DYN((KERNEL<256 / (32 * FB_NW), FB_NW, 264>), grid, block_, lds, (hipStream_t)stream, __VA_ARGS__); \
    } else if ((hidden) == 256) {                                                                            \
      RG_ALLOW_LDS((KERNEL<256 / (32 * FB_NW), FB_NW, 520>), lds);                                           \
      RG_LAUNCH_DYN((KERNEL<256 / (32 * FB_NW), FB_NW, 520>), grid, block_, lds, (hipStream_t)stream, __VA_ARGS__); \
    } else {                                                                                                 \
      RG_ALLOW_LDS((KERNEL<512 / (32 * FB_NW), FB_NW, 520>), lds);                                           \
      RG_LAUNCH_DYN((KERNEL<512 / (32 * FB_NW), FB_NW, 520>), grid, block_, lds, (hipStream_t)stream, __VA_ARGS__); \
    }                                                                                                        \
  } while (0)
#define RG_LAUNCH_FUSED(KERNEL, hidden, pitch, grid, lds, stream, args) RG_LAUNCH_FUSED_ARGS(KERNEL, hidden, pitch, grid, lds, stream, args)

}  // namespace rg

using namespace rg;

extern "C" {

int rg_mlp_fused_supported(const rg_mlp_desc* d) { return fused_supported(d) > 0; }

size_t rg_frag_elems(int rows, int cols) {
  return (size_t)((rows + 127) / 128 * 128) * (size_t)((cols + 31) / 32 * 32);
}

size_t rg_sign_bytes(int rows, int cols) { return rg_frag_elems(rows, cols) / 8; }

size_t rg_wfrag_elems(int out_features, int in_features) {
  return (size_t)((out_features + 31) / 32) * (size_t)((in_features + 15) / 16) * 512;
}

int rg_mlp_forward_fused(const rg_mlp_desc* d, const void* x, int x_dtype, int64_t ldx, int batch, float* out32,
                         int64_t ldo, int save, rg_stream_t stream) {
  const int tn = fused_supported(d);
  if (!tn) return RG_EUNSUPPORTED;
  if (!x || !out32 || batch <= 0) return RG_EINVAL;
  MlpArgs a;
  int rc = fill_args(d, batch, a, 0);
  if (rc) return rc;
  if (save < 0 || save > 2) return RG_EINVAL;
  if (save)
    for (int l = (save == 2 ? 1 : 0); l < d->n_layers; ++l)
      if (!d->act_frag[l]) return RG_EINVAL;  // (save = 2 writes it only where there is no usable sign plane)
  if (d->rowmap && (d->x2 || (d->x3 && !d->tile_key) || (batch % 128) != 0)) return RG_EUNSUPPORTED;
  if (d->tile_key && (!d->rowmap || !d->row_begin || d->n_groups <= 0)) return RG_EINVAL;
  if (d->x2 && (d->x_split <= 0 || d->x_split >= d->dims[0] || (d->x_split % 32) != 0)) return RG_EINVAL;
  if (d->x_tile > 1) {  // tiled state panel: forward only, batch order, plain output layer
    if (!d->x2) return RG_EINVAL;
    if (save || d->rowmap || d->tile_key) return RG_EUNSUPPORTED;
  }
  a.x = x; a.ldx = ldx; a.x_is_f32 = (x_dtype == RG_DT_F32); a.out32 = out32; a.ldo = ldo; a.save = save;
  if (d->x3) return x3_forward_launch(d, a, (hipStream_t)stream);
  size_t lds = (size_t)FB_BM * a.pitch * sizeof(bf16_t);
  const int n_tiles = (batch + FB_BM - 1) / FB_BM;
  const dim3 grid(d->tile_key ? (n_tiles + 7) / 8 * 8 : n_tiles);  // grouped: whole eighths of the tile list (grouped_tile)
  a.stage_out = a.out_lds = 0;
  {
    // a thin output layer (one column tile, the K-split path of the 8-wave kernel) reads its weights from LDS
    const int L = d->n_layers, KCo = (d->dims[L - 1] + 15) / 16;
    if (!d->tile_key && L >= 2 && d->dims[L] <= 16 && FB_NW == 8 && KCo >= 8 && (KCo & 1) == 0 &&
        lds + (size_t)KCo * 512 <= 160 * 1024) {
      a.out_lds = 1;
      lds += (size_t)KCo * 512;
    }
  }
  if (d->tile_key) {
    // a wide grouped output leaves as whole rows through a staging area behind the activation tile (mlp_fwd_fused_body)
    const int No = d->dims[d->n_layers], NTo = (No + 31) / 32;
    const size_t stage = (size_t)32 * (NTo * 32 + 4) * sizeof(float);
    if (No > 64 && (No & 3) == 0 && (ldo & 3) == 0 && (((uintptr_t)out32) & 15) == 0 && lds + stage <= 160 * 1024) {
      a.stage_out = 1;
      lds += stage;
    }
  }
  if (d->tile_key) RG_LAUNCH_FUSED(mlp_fwd_grouped_kernel, d->dims[1], a.pitch, grid, lds, stream, a);
  else RG_LAUNCH_FUSED(mlp_fwd_fused_kernel, d->dims[1], a.pitch, grid, lds, stream, a);
  return (int)hipGetLastError();
}

int rg_dqn_pair_wave_sums(int batch) { return (batch + FB_BM - 1) / FB_BM * FB_NW; }

int rg_dqn_online_pair_forward(const rg_mlp_desc* d, const void* state, int state_dtype, int64_t ld_state,
                               const void* next_state, int next_state_dtype, int64_t ld_next_state, int batch, float* q,
                               float* qn_online, const float* qn_target, const float* action, const float* next_mask,
                               const float* reward, const float* reward_boosts, const float* not_terminal, double gamma,
                               const float* gamma_exponent, int double_q, int loss_type, float* dq, float* loss_wave_sums,
                               float* next_q, int64_t* next_idx, float* q_sel, rg_stream_t stream) {
  if (!fused_supported(d)) return RG_EUNSUPPORTED;
  if (!state || !next_state || !q || !qn_online || !qn_target || !action || !next_mask || !reward || !not_terminal || !dq ||
      !loss_wave_sums || batch <= 0)
    return RG_EINVAL;
  if (loss_type != RG_LOSS_MSE && loss_type != RG_LOSS_HUBER) return RG_EINVAL;
  // the plain shape only: bf16 operands, one input panel in batch order, a plain 16-wide output layer whose weights fit
  // behind the activation tile (rg_mlp_forward_fused's out_lds condition) with the parked Q rows next to them
  const int L = d->n_layers, KCo = (d->dims[L - 1] + 15) / 16;
  if (d->x3 || d->x2 || d->x_tile > 1 || d->rowmap || d->tile_key || L < 2 || d->dims[L] != 16 || KCo < 8 || (KCo & 1)) return RG_EUNSUPPORTED;
  for (int l = 0; l + 1 < L; ++l)
    if (d->acts[l] != RG_ACT_RELU) return RG_EUNSUPPORTED;
  if (((uintptr_t)q | (uintptr_t)qn_online | (uintptr_t)qn_target | (uintptr_t)action | (uintptr_t)next_mask | (uintptr_t)dq) & 15)
    return RG_EUNSUPPORTED;
  MlpArgs a;
  int rc = fill_args(d, batch, a, 0);
  if (rc) return rc;
  for (int l = 0; l < L; ++l)
    if (!d->act_frag[l]) return RG_EINVAL;  // the state pass saves as rg_mlp_forward_fused(save = 1)
  const size_t park = (size_t)FB_BM * 16 * sizeof(float);
  const size_t lds = (size_t)FB_BM * a.pitch * sizeof(bf16_t) + (size_t)KCo * 512 + park;
  if (lds > 160 * 1024) return RG_EUNSUPPORTED;
  a.x = nullptr; a.ldx = 0; a.x_is_f32 = 0; a.out32 = nullptr; a.ldo = 16; a.save = 0;
  a.stage_out = 0; a.out_lds = 1;
  PairArgs p;
  p.io[0] = PairIO{next_state, (long)ld_next_state, qn_online, next_state_dtype == RG_DT_F32, 0};
  p.io[1] = PairIO{state, (long)ld_state, q, state_dtype == RG_DT_F32, 0};
  p.qn_target = qn_target; p.action = action; p.next_mask = next_mask; p.reward = reward;
  p.reward_boosts = reward_boosts; p.not_terminal = not_terminal; p.gamma_exponent = gamma_exponent; p.gamma = (float)gamma;
  p.double_q = double_q; p.loss_type = loss_type; p.dq = dq; p.wave_sums = loss_wave_sums; p.next_q = next_q;
  p.next_idx = next_idx; p.q_sel = q_sel;
  const dim3 grid((batch + FB_BM - 1) / FB_BM);
  RG_LAUNCH_FUSED_ARGS(mlp_fwd_pair_kernel, d->dims[1], a.pitch, grid, lds, stream, a, p);
  return (int)hipGetLastError();
}

size_t rg_mlp_backward_fused_workspace_bytes(const rg_mlp_desc* d, int batch) {
  if (!d || batch <= 0) return 0;
  size_t cols = 0;
  for (int l = 0; l < d->n_layers; ++l) cols += (size_t)d->dims[l + 1];
  // (a grouped output layer's partial rows are indexed workgroup + group: n_groups more rows of the LAST block)
  const size_t extra = d->n_groups > 0 ? (size_t)d->n_groups * d->dims[d->n_layers] : 0;
  return ((size_t)padded_wgs(d, batch) * cols + extra) * sizeof(float);
}

int rg_mlp_backward_fused(const rg_mlp_desc* d, const float* dout32, int64_t lddo, int batch, float* dx32,
                          int64_t lddx, void* workspace, size_t workspace_bytes, rg_stream_t stream) {
  // also a TRUNK: every layer hidden-wide, the "output" being the last hidden layer (dout32 = the gradient of its
  // pre-activation, [batch, H]) — what the grouped output layer of qr_grouped.hip hands back
  if (!fused_supported(d) && !fused_trunk(d)) return RG_EUNSUPPORTED;
  if (!dout32 || batch <= 0) return RG_EINVAL;
  MlpArgs a;
  int rc = fill_args(d, batch, a, 1);
  if (rc) return rc;
  bool want_db = false;
  for (int l = 0; l < d->n_layers; ++l) {
    if (!d->dx_only && !d->dz_frag[l]) return RG_EINVAL;
    if (l >= 1 && !d->act_frag[l]) return RG_EINVAL;
    if (d->db[l]) want_db = true;
  }
  if (dx32 && !d->wfrag_bwd[0]) return RG_EINVAL;
  if (d->dx_only && (!dx32 || want_db || d->tile_key)) return RG_EINVAL;
  if (d->tile_key && (!d->row_begin || d->n_groups <= 0 || d->dims[d->n_layers] > 256)) return RG_EINVAL;
  if (d->dx_col0 < 0 || d->dx_col0 >= d->dims[0] || (d->dx_col0 % 32) != 0) return RG_EINVAL;
  const int n_wg = padded_wgs(d, batch);
  if (want_db) {
    if (!workspace || workspace_bytes < rg_mlp_backward_fused_workspace_bytes(d, batch)) return RG_EWORKSPACE;
    float* p = (float*)workspace;
    for (int l = 0; l < d->n_layers; ++l) {
      a.db_part[l] = d->db[l] ? p : nullptr;
      p += (size_t)n_wg * d->dims[l + 1];
    }
  }
  a.dout32 = dout32; a.lddo = lddo; a.dx32 = dx32; a.lddx = lddx;
  if (d->x3) {
    rc = x3_backward_launch(d, a, (hipStream_t)stream);
  } else {
    size_t lds = (size_t)FB_BM * a.pitch * sizeof(bf16_t);
    const dim3 grid(d->tile_key ? (n_wg + 7) / 8 * 8 : n_wg);
    if (d->tile_key && a.pitch < 2 * 256 + 8) lds *= 2;  // a boundary tile's masked dZ copy lives behind a 264-wide tile
    if (d->dx_only) RG_LAUNCH_FUSED(mlp_bwd_dx_kernel, d->dims[1], a.pitch, grid, lds, stream, a);
    else if (d->tile_key) RG_LAUNCH_FUSED(mlp_bwd_grouped_kernel, d->dims[1], a.pitch, grid, lds, stream, a);
    else RG_LAUNCH_FUSED(mlp_bwd_fused_kernel, d->dims[1], a.pitch, grid, lds, stream, a);
    rc = (int)hipGetLastError();
  }
  if (rc) return rc;
  // a grouped output layer's bias gradient: per-group sums over each group's segments, a launch of its own either way
  // (a workgroup covers 128 rows of the grouped space in the bf16 kernel, 64 in the split-bf16 kernel)
  const int last = d->n_layers - 1;
  if (d->tile_key && a.db_part[last]) {
    grouped_bias_reduce_launch(a.db_part[last], d->row_begin, d->n_groups, d->dims[last + 1], d->db[last], d->x3 ? X3_BM : FB_BM,
                               (hipStream_t)stream);
    a.db_part[last] = nullptr;
  }
  // defer_db: the other partials stay in the workspace, rg_mlp_wgrad_fused (db_partials) sums them in its reduce launch (the
  // trunk's wait for the trunk's weight gradient, whose descriptor is this one's first n_layers - 1 layers — same layout)
  if (d->defer_db) return want_db ? (int)hipGetLastError() : RG_EINVAL;
  ReduceColsGroupArgs G;
  const int blocks = fill_reduce_cols(G, n_wg, d->n_layers, a.db_part, d->db, d->dims + 1);
  if (G.n > 0) RG_LAUNCH(reduce_cols_group_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, G);
  return (int)hipGetLastError();
}

}  // extern "C"
