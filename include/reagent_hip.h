/* reagent_hip.h — C ABI of libreagent_hip.so: the MI355X (gfx950) batch-RL training-step kernels.
 *
 * ReAgent (the reference) has no FFI on this path: every op is an eager torch call made from
 * Python.  This header therefore DEFINES the boundary; each entry point names the reference
 * code it replaces (paths relative to the ReAgent tree) so a maintainer can bind it from the
 * reference side with ctypes.
 *
 * Conventions
 *  - plain device pointers + sizes, no torch types; all matrices row-major, leading dimensions in
 *    ELEMENTS; every pointer is device memory unless the comment says host.
 *  - caller owns all memory (PyTorch caching allocator); nothing is allocated or freed here.
 *  - work is enqueued on `stream` only; no entry point synchronises.
 *  - return 0 on success, negative RG_E* for argument errors detected on the host before any
 *    launch, positive = hipError_t of a failed launch.  Never throws, never exits.
 *  - `precision`: RG_PREC_F32 = fp32 operands on v_mfma_f32_32x32x2_f32 (exact fp32, parity mode);
 *    RG_PREC_BF16 = bf16 operands on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The
 *    element type of every `void*` activation/weight operand is float resp. bf16 accordingly.
 */
#ifndef REAGENT_HIP_H_
#define REAGENT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rg_stream_t; /* hipStream_t */

enum { RG_OK = 0, RG_EINVAL = -1, RG_EALIGN = -2, RG_EUNSUPPORTED = -3, RG_EWORKSPACE = -4 };
enum { RG_PREC_F32 = 0, RG_PREC_BF16 = 1, RG_PREC_BF16X3 = 2 /* fused stack only: rg_mlp_desc.x3 */ };
enum { RG_DT_F32 = 0, RG_DT_BF16 = 1 };
enum {
  RG_ACT_LINEAR = 0, RG_ACT_RELU = 1, RG_ACT_LEAKY_RELU = 2, RG_ACT_TANH = 3, RG_ACT_SIGMOID = 4,
  RG_ACT_SOFTPLUS = 5 /* reagent/models/fully_connected_network.py:37-44 ACTIVATION_MAP */
};
enum {
  RG_LOSS_MSE = 0, RG_LOSS_HUBER = 1, /* reagent/training/dqn_trainer_base.py:146-155 */
  RG_LOSS_BCE_LOGITS = 2 /* ABI 13, rg_pdqn_head only: F.binary_cross_entropy_with_logits,
                          * reagent/training/parametric_dqn_trainer.py:55-61 */
};

const char* rg_strerror(int code);
int rg_abi_version(void);

/* ---- FullyConnected layer ops ------------------------------------------------------------ */

/* y = act(x · w^T + bias).  Replaces nn.Linear + activation,
 * reagent/models/fully_connected_network.py:101-153.
 * x [batch, in] (ldx), w [out, in] (ldw, nn.Linear layout), bias [out] fp32 or NULL.
 * Outputs (each nullable): y [batch, out] compute type; y32 [batch, out] fp32 (both use ldy);
 * yt [out, batch] (ldyt) transposed copy in compute type (input of rg_fc_wgrad / mask of
 * rg_fc_dgrad). */
int rg_fc_forward(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                  void* y, float* y32, int64_t ldy, void* yt, int64_t ldyt, int batch,
                  int out_features, int in_features, int act, int precision, rg_stream_t stream);

/* dx = (dz · w) ⊙ act'(h_below).  Replaces autograd's AddmmBackward (input grad) +
 * Relu/Tanh/...Backward of the layer below.
 * dz [batch, out] (lddz); wt = w^T [in, out] (ldwt); ht = saved transposed output of the layer
 * below [in, batch] (ldht) or NULL when that "layer" is the network input / linear.
 * Outputs (nullable): dx [batch, in] compute type, dx32 fp32 (lddx), dxt [in, batch] (lddxt). */
int rg_fc_dgrad(const void* dz, int64_t lddz, const void* wt, int64_t ldwt, const void* ht,
                int64_t ldht, int act_below, void* dx, float* dx32, int64_t lddx, void* dxt,
                int64_t lddxt, int batch, int in_features, int out_features, int precision,
                rg_stream_t stream);

/* dw [out, in] (contiguous fp32) = dz^T · x ; db [out] = column sums of dz (nullable).
 * Replaces autograd's AddmmBackward (weight + bias grads).  Inputs are the TRANSPOSED
 * copies: dzt [out, batch] (lddzt), xt [in, batch] (ldxt).  Deterministic: fixed split of
 * the batch axis, partial slabs in `workspace`, ordered second-stage sum. */
size_t rg_fc_wgrad_workspace_bytes(int out_features, int in_features, int batch, int precision);
int rg_fc_wgrad(const void* dzt, int64_t lddzt, const void* xt, int64_t ldxt, float* dw, float* db,
                void* workspace, size_t workspace_bytes, int out_features, int in_features,
                int batch, int precision, rg_stream_t stream);

/* src [rows, cols] (ld_src, dtype src_dt) -> dst [rows, cols] (ld_dst) and/or
 * dst_t [cols, rows] (ld_t), both of dtype dst_dt.  Used to stage fp32 master weights /
 * network inputs into the compute type and its transposed twin. */
int rg_transpose_cast(const void* src, int src_dt, int64_t ld_src, int rows, int cols, void* dst,
                      int64_t ld_dst, void* dst_t, int64_t ld_t, int dst_dt, rg_stream_t stream);

/* nn.LayerNorm(n) between a Linear and its activation — FullyConnectedNetwork's use_layer_norm option
 * (reagent/models/fully_connected_network.py:128-130).  z [batch, n] fp32 = the Linear's output (rg_fc_forward with
 * RG_ACT_LINEAR); y (nullable, element type y_dtype) and / or y32 (nullable) = act(((z - mean) / sqrt(var + eps)) *
 * gamma + beta) with the row's mean and biased variance; mean / rstd [batch] (nullable) are what the backward reads. */
int rg_layer_norm_forward(const float* z, int64_t ldz, const float* gamma, const float* beta, double eps, int act,
                          int batch, int n, void* y, int y_dtype, int64_t ldy, float* y32, int64_t ldy32, float* mean,
                          float* rstd, rg_stream_t stream);
/* g [batch, n] = d loss / d (LayerNorm output, i.e. with the activation's derivative already applied): writes
 * dz (nullable, dz_dtype) and / or dz32 = d loss / d z, dgamma [n] and dbeta [n] (overwritten; per-workgroup partials in
 * `workspace`, summed in a fixed order). */
size_t rg_layer_norm_backward_workspace_bytes(int batch, int n);
int rg_layer_norm_backward(const float* g, int64_t ldg, const float* z, int64_t ldz, const float* mean, const float* rstd,
                           const float* gamma, int batch, int n, void* dz, int dz_dtype, int64_t lddz, float* dz32,
                           int64_t lddz32, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                           rg_stream_t stream);

/* nn.BatchNorm1d(n) on a layer's INPUT — FullyConnectedNetwork's use_batch_norm option (SlateBatchNorm1d on
 * [batch, features], reagent/models/fully_connected_network.py:48-64,107-108).  x, y [batch, n] fp32.
 * training != 0: y = (x - mean_b) / sqrt(var_b + eps) * gamma + beta with the batch mean and BIASED variance, which are
 *   kept in save_mean / save_rstd [n] for the backward; running_mean / running_var (nullable) move by `momentum`
 *   toward the batch mean and the UNBIASED variance (torch.nn.functional.batch_norm), `stat_updates` times (1; 2 for a
 *   module the reference evaluates twice on the same batch, actor.py:215-231; 0 leaves them alone).  `workspace` holds the
 *   fixed-order fp64 column partials (rg_batch_norm_workspace_bytes).
 * training == 0: the running statistics normalise; save_* and workspace are not touched.  gamma / beta nullable. */
size_t rg_batch_norm_workspace_bytes(int batch, int n);
int rg_batch_norm_forward(const float* x, int64_t ldx, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, int training, int stat_updates, double momentum, double eps, int batch, int n, float* y,
                          int64_t ldy, float* save_mean, float* save_rstd, void* workspace, size_t workspace_bytes,
                          rg_stream_t stream);
/* g = d loss / d y.  training != 0: mean / rstd are the forward's save_mean / save_rstd and
 *   dx = gamma * rstd * (g - mean_b(g) - xhat * mean_b(g * xhat)); training == 0: mean = running_mean, rstd null,
 *   running_var + eps give the scale and dx = gamma * rstd * g.  dgamma = sum_b g * xhat, dbeta = sum_b g
 *   (each nullable, overwritten); dx nullable. */
int rg_batch_norm_backward(const float* g, int64_t ldg, const float* x, int64_t ldx, const float* gamma,
                           const float* mean, const float* rstd, const float* running_var, int training, double eps,
                           int batch, int n, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, rg_stream_t stream);

/* nn.Dropout(p) after a layer's activation (fully_connected_network.py:139-141), training mode.
 * generate != 0: keep [batch * n] bytes ~ Bernoulli(1 - p) from Philox4x32-10 keyed by `seed`, counter (element / 4,
 *   offset) — a different `offset` per call gives an independent mask — and y = x * keep / (1 - p).
 * generate == 0: `keep` is read (the backward pass: x = d loss / d y, y = d loss / d x).  x may alias y. */
int rg_dropout(const float* x, int64_t ldx, int batch, int n, double p, int generate, uint64_t seed, uint64_t offset,
               uint8_t* keep, float* y, int64_t ldy, rg_stream_t stream);

/* dz = dy * act'(z) written through the activation output y = act(z), fp32 [rows, cols]: turns the
 * gradient w.r.t. a non-linear OUTPUT layer (FullyConnectedActor's tanh head,
 * reagent/models/actor.py:71-75) into the pre-activation gradient the backward entry points take. */
int rg_act_backward(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, int act, float* dz,
                    int64_t ld_dz, int rows, int cols, rg_stream_t stream);

/* ---- fused FullyConnected stack (bf16 throughput path) ------------------------------------ */

/* Whole-network kernels for stacks whose hidden layers share one width in {256, 512}, input
 * width <= 512 and output width <= 256 (rg_mlp_fused_supported): a 128-row activation tile stays
 * in LDS across all layers; weights stream from HBM/L2 in MFMA B-fragment order
 * (rg_stage_weights_frag); what backward needs is saved in MFMA C-fragment order
 * (rg_frag_elems(batch, width) bf16 elements per saved matrix), which rg_fc_wgrad_frag
 * consumes directly as MFMA operands.  Replaces FullyConnectedNetwork.forward
 * (reagent/models/fully_connected_network.py:157-163) and its autograd backward. */
#define RG_MLP_MAX_LAYERS 6
typedef struct {
  int32_t n_layers;
  int32_t dims[RG_MLP_MAX_LAYERS + 1];        /* dims[0] = input features, dims[l+1] = out of layer l */
  int32_t acts[RG_MLP_MAX_LAYERS];            /* RG_ACT_* per layer; backward takes d loss / d PRE-activation of the last layer (rg_act_backward) */
  const void* wfrag_fwd[RG_MLP_MAX_LAYERS];   /* rg_stage_weights_frag outputs */
  const void* wfrag_bwd[RG_MLP_MAX_LAYERS];
  const float* bias[RG_MLP_MAX_LAYERS];
  void* act_frag[RG_MLP_MAX_LAYERS];          /* [l] = saved INPUT of layer l, C-fragment order */
  void* dz_frag[RG_MLP_MAX_LAYERS];           /* [l] = d loss / d pre-activation output of layer l */
  void* act_sign[RG_MLP_MAX_LAYERS];          /* optional, [l] (l >= 1) = one bit per element of act_frag[l]
                                               * (value > 0), rg_sign_bytes(batch, dims[l]) bytes, written by a
                                               * saving forward; when layer l-1 is ReLU / leaky ReLU the backward
                                               * reads these 16 B per lane instead of act_frag[l] */
  float* db[RG_MLP_MAX_LAYERS];               /* backward output: bias gradients [dims[l+1]] (nullable) */
  const float* w[RG_MLP_MAX_LAYERS];          /* fp32 master weights [dims[l+1], dims[l]] (stage_weights_fused) */
  float* dw[RG_MLP_MAX_LAYERS];               /* weight gradients, same shape (wgrad_fused) */
  int32_t x3;                                 /* 0: bf16 operands.  1: split-bf16 ("bf16x3", RG_PREC_BF16X3) — every
                                               * operand x is carried as hi = bf16(x), lo = bf16(x - hi) and a product
                                               * is hi*hi + hi*lo + lo*hi on the bf16 MFMA pipe with fp32 accumulation
                                               * (~2^-16 relative per product: fp32-class results).  All
                                               * fragment buffers (wfrag_*, act_frag, dz_frag) then hold TWO planes, hi
                                               * then lo, i.e. twice the element counts rg_*_elems report; the kernels
                                               * work on 64-row tiles (both planes of the activation tile share the LDS) */
  int32_t dx_only;                            /* backward: 1 = only the input gradient is wanted (a frozen network, e.g.
                                               * SAC's critics in the actor step, sac_trainer.py:262-279): dz_frag is
                                               * neither required nor written and no weight gradient may follow */
  /* Two-panel network input (FullyConnectedCritic: cat(state, action), reagent/models/critic.py:79-92) without
   * materialising the concatenation: when x2 != NULL the forward reads input columns [0, x_split) from its `x`
   * argument and columns [x_split, dims[0]) from x2 (row pitch ldx2, element type x2_dtype); x_split a multiple of 32. */
  const void* x2;
  int64_t ldx2;
  int32_t x_split;
  /* backward: dx32 receives d loss / d input columns [dx_col0, dims[0]) only (dx32[0] is column dx_col0; a
   * multiple of 32) — SAC's actor step needs the action columns of the critic's input gradient, not the state's */
  int32_t dx_col0;
  int32_t x2_dtype;                           /* element type of x2 (RG_DT_*): the panels may differ — network-ready bf16
                                               * state rows from the sampler next to fp32 actions */
  int32_t wgrad_flags;                        /* ABI 10 (was reserved, 0).  rg_mlp_wgrad_fused: bit 0 = this launch shares the chip
                                               * with another launch on a second stream (the QR-DQN trunk beside the grouped
                                               * head's weight gradient): every split of a layer keeps the same length — the
                                               * uneven plan leans on the launch's own dispatch order */
  /* forward only: row r of the batch the kernels work on reads input row rowmap[r] of x (-1: an all-zero row);
   * `batch` is then the length of rowmap.  Lets a stack run in "grouped space" (rows sorted by a key and padded to
   * whole 128-row tiles, qr_grouped.hip) without materialising the permuted input. */
  const int32_t* rowmap;
  /* Grouped OUTPUT layer (qr_grouped.hip): with tile_key != NULL the last layer is one of n_groups layers
   * [dims[L], dims[L-1]] chosen per ROW of the grouped space: group g owns the rows [row_begin[g], row_begin[g + 1])
   * (ABI 9; rows past row_begin[n_groups] belong to no group and have no output), tile_key[tile] = the first group with rows
   * in a 128-row tile (-1: none) — a tile that spans several groups runs the layer once per group on that group's rows.
   * wfrag_fwd[L-1] / wfrag_bwd[L-1] / bias[L-1] point at group 0 and advance by group_stride_fwd /
   * group_stride_bwd elements / dims[L] per group (rg_group_weights_stage lays them out so).  out_scatter != 0
   * writes output row r of the forward to out32[rowmap[r]] (rows with rowmap[r] < 0 are dropped).  The backward
   * reduces the last layer's bias gradient per group (db[L-1]: [n_groups * dims[L]]; its workspace holds n_groups more
   * partial rows for that layer) and leaves the last layer's weight gradient to rg_group_head_wgrad; dz_frag[L-1], its
   * operand, is a fragment matrix of rows + 32 * n_groups rows: group g's 32-row blocks are written g blocks late, a
   * block two groups share once per group with the other group's rows zeroed.
   * ABI 8: also for split-bf16 stacks (x3): per group [hi plane | lo plane], the strides cover both. */
  const int32_t* tile_key;
  const int32_t* row_begin;
  int32_t n_groups;
  int32_t out_scatter;
  int64_t group_stride_fwd, group_stride_bwd;
  /* ABI 6 — the step's launch-bound tails folded into the weight gradient's reduce launch.
   * defer_db != 0: rg_mlp_backward_fused leaves the bias-gradient partials in its workspace and launches no column
   *   reduce; rg_mlp_wgrad_fused, handed that workspace in db_partials, sums them into db[] in the launch that sums its
   *   own split partials (same arithmetic, one launch instead of two).  With a grouped output layer (ABI 9) the last
   *   layer's per-group reduce is still launched by rg_mlp_backward_fused; the other layers' partials wait for the
   *   rg_mlp_wgrad_fused call on the trunk (the first n_layers - 1 layers: same workspace layout).
   * sum_in != NULL: that launch also writes sum_out[0] = sum_scale * sum(sum_in[0 .. sum_n)) — the mean loss of a step
   *   from the loss head's per-workgroup partials (rg_reduce_sum's arithmetic). */
  int32_t defer_db;
  int32_t sum_n;
  const float* db_partials;
  const float* sum_in;
  float* sum_out;
  double sum_scale;
  /* ABI 12: sum_run > 1 — sum_in holds sum_n per-wave sums (rg_dqn_online_pair_forward's loss_wave_sums); each run of
   * sum_run of them is first added in order into one value (what rg_dqn_head adds into one partial per 256 rows) and the
   * values are then summed as above: the same adds in the same order as rg_dqn_head's partials.  0 / 1: as before. */
  int32_t sum_run;
  /* ABI 13 — tiled two-panel forward (forward only): with x2 != NULL and x_tile = M > 1, `batch` counts TILED rows and
   * batch row r reads columns [0, x_split) from row r / M of x (ceil(batch / M) rows) and the remaining columns from row r
   * of x2: the network input cat(state.repeat_interleave(M, 0), candidates) of a parametric DQN step
   * (FeatureData.get_tiled_batch, reagent/core/types.py:349-365, and FullyConnectedCritic's cat, reagent/models/critic.py:79-92,
   * as reagent/training/parametric_dqn_trainer.py:134-140 evaluates them) without either being written.  Same bits as the
   * two-panel forward on the materialised tiled state.  0 / 1: as before.  RG_EINVAL without x2; RG_EUNSUPPORTED with
   * save != 0, rowmap, tile_key or rg_dqn_online_pair_forward. */
  int32_t x_tile;
} rg_mlp_desc; /* host struct */

int rg_mlp_fused_supported(const rg_mlp_desc* d);
size_t rg_frag_elems(int rows, int cols);                  /* bf16 elements of a C-fragment matrix */
size_t rg_sign_bytes(int rows, int cols);                  /* bytes of an act_sign plane */
size_t rg_wfrag_elems(int out_features, int in_features);  /* bf16 elements of a B-fragment weight */
/* w [out, in] fp32 (nn.Linear layout) -> wfrag_fwd (rg_wfrag_elems(out,in)) and/or
 * wfrag_bwd = fragments of w^T (rg_wfrag_elems(in,out)); zero padded. */
int rg_stage_weights_frag(const float* w, int out_features, int in_features, void* wfrag_fwd,
                          void* wfrag_bwd, rg_stream_t stream);
/* out32 [batch, dims[L]] = network(x); x [batch, dims[0]] row-major of dtype x_dtype (RG_DT_*).
 * save = 1 additionally writes act_frag[0..L-1] and the act_sign planes (everything backward + wgrad read).
 * save = 2 writes only what a dx_only backward reads: the act_sign planes, and act_frag[l] of the layers whose
 * activation gradient is not a sign test (tanh, sigmoid, softplus) — for a ReLU stack 16 B per lane per layer
 * instead of the activations themselves. */
int rg_mlp_forward_fused(const rg_mlp_desc* d, const void* x, int x_dtype, int64_t ldx, int batch,
                         float* out32, int64_t ldo, int save, rg_stream_t stream);
/* Given dout32 = d loss / d out32: writes dz_frag[0..L-1] (needs act_frag[1..L-1] from a saving
 * forward of the same batch) and the bias gradients d->db[l] (column sums of dZ_l, reduced
 * deterministically from per-workgroup partials in `workspace`); dx32 (nullable) = d loss / d x,
 * fp32 [batch, dims[0]].  With d->dx_only only dx32 is produced (see rg_mlp_desc). */
size_t rg_mlp_backward_fused_workspace_bytes(const rg_mlp_desc* d, int batch);
int rg_mlp_backward_fused(const rg_mlp_desc* d, const float* dout32, int64_t lddo, int batch,
                          float* dx32, int64_t lddx, void* workspace, size_t workspace_bytes,
                          rg_stream_t stream);
/* dw [out, in] fp32 = dz^T x from C-fragment operands dz_frag (batch x out) and x_frag
 * (batch x in).  Deterministic split over the batch. */
size_t rg_fc_wgrad_frag_workspace_bytes(int out_features, int in_features, int batch);
int rg_fc_wgrad_frag(const void* dz_frag, const void* x_frag, int out_features, int in_features,
                     int batch, float* dw, void* workspace, size_t workspace_bytes,
                     rg_stream_t stream);

/* Whole-stack variants: every layer's weights staged by ONE launch (d->w -> d->wfrag_fwd, and
 * d->wfrag_bwd when need_bwd), every layer's weight gradient by ONE wgrad launch + ONE reduce
 * (d->dz_frag, d->act_frag -> d->dw).  The weight gradient is a deterministic split over the batch (same inputs, same
 * bits); the workspace holds the splits' partial tiles — fp32 for split-bf16 stacks, bf16 in accumulator-tile order for
 * bf16 stacks (round 5: half the bytes; 2^-9 of a PARTIAL sum, far inside what bf16 operands cost the gradient) — and is
 * sized by rg_mlp_wgrad_fused_workspace_bytes for either form.  Split-bf16 stacks multiply BOTH planes of dZ (three
 * MFMAs per tile pair: fp32-class gradients) unless the library runs with RG_X3_DZ_PLANES=1 (dZ as one plane, two
 * MFMAs, ~2e-3 relative on dW: an opt-in). */
int rg_mlp_stage_weights_fused(const rg_mlp_desc* d, int need_bwd, rg_stream_t stream);
size_t rg_mlp_wgrad_fused_workspace_bytes(const rg_mlp_desc* d, int batch);
int rg_mlp_wgrad_fused(const rg_mlp_desc* d, int batch, void* workspace, size_t workspace_bytes,
                       rg_stream_t stream);

/* Optimizer step fused with weight staging for a fused stack: rg_adam_step on the flat parameter slab
 * of the online network, rg_soft_update of the equally laid out target slab (target NULL = none), and
 * the bf16 re-staging of the updated weights into wfrag_fwd / wfrag_bwd (online) and target_wfrag_fwd
 * — same arithmetic per element as the separate entry points, one launch instead of four.
 * w_off / b_off: element offsets of layer l's weight [dims[l+1], dims[l]] and bias [dims[l+1]] inside
 * the slabs.  The fragment buffers must have been staged once (their padding is not rewritten in
 * wfrag_bwd); any of the three fragment pointers of a layer may be NULL. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* target;
  int32_t n_layers;
  int32_t dims[RG_MLP_MAX_LAYERS + 1];
  int64_t w_off[RG_MLP_MAX_LAYERS];
  int64_t b_off[RG_MLP_MAX_LAYERS];
  void* wfrag_fwd[RG_MLP_MAX_LAYERS];
  void* wfrag_bwd[RG_MLP_MAX_LAYERS];
  void* target_wfrag_fwd[RG_MLP_MAX_LAYERS];
  int32_t x3;  /* ABI 6: split-bf16 stacks — every fragment buffer is [hi plane | lo plane] (rg_mlp_desc.x3), both
                * planes of all three fragment sets are re-staged: lo = bf16(w - hi) as rg_mlp_stage_weights_fused */
  int32_t group_rows[RG_MLP_MAX_LAYERS]; /* ABI 7: group_rows[l] > 0 = layer l is a GROUPED layer (QR-DQN's A x N output
                * layer, reagent/training/qrdqn_trainer.py:108-194, as dims[l+1] / group_rows[l] independent
                * [group_rows[l], dims[l]] layers): its three fragment buffers are laid out as rg_group_weights_stage
                * writes them (group g at g * rg_group_wfrag_elems elements; ABI 8: with x3 a group's set is
                * [hi plane | lo plane], twice that). */
  /* ABI 7, replayed steps (a captured HIP graph must not need launch arguments that change from step to step):
   * sched_pre_ticked != 0 (_sched entry point only): the step is already counted in sched[0] — by the sampler launch of the
   * same step, rg_replay_dqn_batch_pooled — so the coefficients of step sched[0] apply and no rg_sched_tick follows;
   * post_tick != NULL: *post_tick = (*post_tick + 1) % post_tick_mod when the launch is done with it (the cursor of the
   * index pool the next step's sampler reads). */
  int32_t sched_pre_ticked;
  int32_t post_tick_mod;
  int64_t* post_tick;
} rg_mlp_update_desc; /* host struct */
int rg_mlp_update_fused(const rg_mlp_update_desc* d, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                        double grad_scale, double tau, rg_stream_t stream);

/* ---- replay buffer ------------------------------------------------------------------------ */

/* n-step bookkeeping of ReplayBuffer.sample_transition_batch,
 * reagent/replay_memory/circular_replay_buffer.py:652-663,676-678,741-747,759-774.
 * indices [B] int64; terminal [C] uint8; reward [C] fp32; decays [update_horizon] fp32 host-
 * computed gamma**k (so the product order matches the reference bit for bit).
 * Outputs: steps [B] int64; next_indices [B] int64; out_terminal [B] uint8; out_reward [B] fp32. */
int rg_replay_nstep(const int64_t* indices, const uint8_t* terminal, const float* reward,
                    const float* decays, int64_t capacity, int update_horizon, int batch,
                    int64_t* steps, int64_t* next_indices, uint8_t* out_terminal,
                    float* out_reward, rg_stream_t stream);

/* One launch gathers up to RG_MAX_GATHER_COLS dense columns
 * (`store[key][stack_indices]` of circular_replay_buffer.py:749-757 + sample_to_output :133-141).
 * For column c: dst_c[b, e, s] = src_c[(idx_c[b] - (stack-1) + s) mod capacity, e]
 * with e in [0,row_elems_c), elem_bytes_c in {1,2,4,8}; stack==1 degenerates to a row copy. */
#define RG_MAX_GATHER_COLS 16
typedef struct {
  const void* src;        /* [capacity, row_elems] */
  void* dst;              /* [batch, row_elems, stack] */
  const int64_t* indices; /* [batch] */
  int32_t row_elems;
  int32_t elem_bytes;
  /* optional normalize-on-gather epilogue (fp32 source columns, stack == 1): `norm` points to
   * row_elems rg_norm_col descriptors on the device (one per element, 1:1 ops — no ENUM), applied
   * with presence = 1 while the row streams through (Preprocessor.forward fused into the gather);
   * out_dtype RG_DT_F32 or RG_DT_BF16 selects the element type of dst. */
  const void* norm;
  const float* norm_quantiles;
  int32_t out_dtype;
  int32_t reserved;
} rg_gather_col;
int rg_replay_gather(const rg_gather_col* cols /*host*/, int ncols, int64_t capacity, int stack,
                     int batch, rg_stream_t stream);

/* ---- sum tree for prioritized replay ------------------------------------------------------ */

/* Device-resident SumTree (reagent/replay_memory/sum_tree.py:30-189) backing
 * PrioritizedReplayBuffer (reagent/replay_memory/prioritized_replay_buffer.py:30-185).
 * `tree`: rg_sumtree_nodes(capacity) doubles in heap order (level d at offset 2^d - 1, leaves at
 * level depth = rg_sumtree_depth(capacity) = ceil(log2(capacity))), zero-initialised by the caller.
 * Updates of <= 32 pairs (or with claim == NULL) repeat the reference's delta accumulation exactly;
 * larger batches write the leaves and rebuild node = left + right level by level (identical
 * whenever the sums are exact in fp64, last-place differences otherwise). */
int rg_sumtree_depth(int64_t capacity);
size_t rg_sumtree_nodes(int64_t capacity);
/* SumTree.set for n (index, value) pairs applied in order (a later pair overrides an earlier one on
 * the same index), set_priority :146-157.  `claim`: int32 [2^depth] all -1, scratch for n > 32
 * (returned all -1); nullable -> the in-order single-thread walk is used for any n.
 * Indices outside [0, capacity) are skipped, never dereferenced (the reference raises IndexError; the host
 * wrapper raises it too whenever the indices are host data). */
int rg_sumtree_set(double* tree, int depth, int64_t capacity, const int64_t* indices, const double* values,
                   int n, int* claim, rg_stream_t stream);
/* SumTree.sample :97-131 for n query values in [0, 1] (each scaled by the root, then the
 * reference's descent); stratified_sample :133-153 = queries drawn one per segment by the caller. */
int rg_sumtree_sample(const double* tree, int depth, const double* query01, int n,
                      int64_t* out_indices, rg_stream_t stream);
/* leaf values: out32 (float32, get_priority :159-180) and/or out64; either nullable; 0 for an index outside
 * [0, capacity) */
int rg_sumtree_get(const double* tree, int depth, int64_t capacity, const int64_t* indices, int n,
                   float* out32, double* out64, rg_stream_t stream);

/* DiscreteDqnInputMaker (reagent/gym/preprocessors/trainer_preprocessor.py:72-97,118-158):
 * action / next_action [B] int64 -> one-hot fp32 [B, A] (next_action rows zeroed where terminal),
 * not_terminal [B] = 1 - terminal, action_probability [B] = exp(log_prob) (nullable). */
int rg_make_dqn_input(const int64_t* action, const int64_t* next_action, const uint8_t* terminal,
                      const float* log_prob, int batch, int num_actions, float* action_onehot,
                      float* next_action_onehot, float* not_terminal, float* action_probability,
                      rg_stream_t stream);
/* Sparse replay elements — IDListMetadata / IDScoreListMetadata.sample_to_output (circular_replay_buffer.py:144-274).
 * A feature's lists sit in padded slots ids [capacity, width] (+ scores [capacity, width]) with lens [capacity].
 * rg_ragged_offsets: offsets [batch] = exclusive prefix sums of lens[indices[b]], total [1] = their sum.
 * rg_ragged_copy: ids_out (and scores_out when scores != NULL) receive the sampled rows back to back at `offsets`. */
int rg_ragged_offsets(const int32_t* lens, const int64_t* indices, int batch, int32_t* offsets, int32_t* total,
                      rg_stream_t stream);
int rg_ragged_copy(const int64_t* ids, const float* scores, int width, const int32_t* lens, const int64_t* indices,
                   const int32_t* offsets, int batch, int64_t* ids_out, float* scores_out, rg_stream_t stream);
/* PolicyNetworkInputMaker.__call__ (gym/preprocessors/trainer_preprocessor.py:161-227, dense path) in one launch:
 * action_out / next_action_out [B, A] = rescale_actions(training/utils.py:13-29) from the environment's range to the
 * training range, next_action rows of terminal transitions zeroed; not_terminal [B] = 1 - terminal;
 * action_probability [B] (nullable) = exp(log_prob).  ranges [4 * A] = prev_min | prev_max | new_min | new_max per
 * action dimension.  Same operation order and roundings as the torch expression it replaces. */
int rg_make_policy_input(const float* action, int64_t lda, const float* next_action, int64_t ldna, const uint8_t* terminal,
                         const float* log_prob, const float* ranges, int batch, int action_dim, float* action_out,
                         float* next_action_out, float* not_terminal, float* action_probability, rg_stream_t stream);

/* ---- dense feature normalization ---------------------------------------------------------- */

/* Preprocessor.forward, reagent/preprocessing/preprocessor.py:115-170 (+ _preprocess_* :197-525).
 * One descriptor per OUTPUT column (ENUM features expand to several).  x [B, n_in] fp32 (ldx),
 * presence [B, n_in] uint8 (ldp).  out [B, n_out] fp32 (ldo).
 * p0..p3 per op:  CONTINUOUS mean,stddev | BOXCOX shift,lambda,mean,stddev | ENUM value |
 * QUANTILE q_offset,q_count (into `quantiles`),-,- | CONTINUOUS_ACTION min_serving,scaling,min_training */
enum {
  RG_NORM_BINARY = 0, RG_NORM_PROBABILITY = 1, RG_NORM_CONTINUOUS = 2, RG_NORM_BOXCOX = 3,
  RG_NORM_ENUM = 4, RG_NORM_QUANTILE = 5, RG_NORM_CONTINUOUS_ACTION = 6,
  RG_NORM_DISCRETE_ACTION = 7, RG_NORM_DO_NOT_PREPROCESS = 8, RG_NORM_CLIP_LOG = 9
};
typedef struct {
  int32_t op;
  int32_t in_col;
  float p0, p1, p2, p3;
} rg_norm_col;
int rg_normalize_dense(const float* x, int64_t ldx, const uint8_t* presence, int64_t ldp,
                       const rg_norm_col* cols /*device*/, int n_out, const float* quantiles,
                       float* out, int64_t ldo, int batch, rg_stream_t stream);

/* ---- offline table -> training batch ------------------------------------------------------- */

/* The post-timeline dataset (column schema of select_relevant_columns,
 * reagent/data/oss_data_fetcher.py:293-336) as one device array per column.  rg_table_dqn_batch
 * replaces the data loader's row fetch plus DiscreteDqnBatchPreprocessor.forward
 * (reagent/preprocessing/batch_preprocessor.py:35-66) for a batch of row indices, in one launch:
 * Preprocessor.forward on state / next_state (cols / quantiles as for rg_normalize_dense, n_out
 * output columns), one-hot action / next_action (next_action == n_actions -> all zeros), not_terminal
 * = max of possible_next_actions_mask, pass-through columns.  Nullable table columns: presence
 * (= all present), time_diff / step (= 1), action_probability (= 1), mdp_id / sequence_number (= 0),
 * possible_actions_mask (= all ones).  Nullable outputs: time_diff, step, action_probability, mdp_id,
 * sequence_number, possible_actions_mask.  Masks and presence are bytes (0 / 1). */
typedef struct {
  const float* state_features;                 /* [n_rows, n_features] */
  const uint8_t* state_features_presence;      /* [n_rows, n_features] */
  const float* next_state_features;
  const uint8_t* next_state_features_presence;
  const int64_t* action;                       /* [n_rows] index into the action names */
  const int64_t* next_action;                  /* [n_rows], n_actions = no next action */
  const float* reward;                         /* [n_rows] */
  const float* action_probability;
  const int64_t* time_diff;
  const int64_t* step;
  const int64_t* mdp_id;
  const int64_t* sequence_number;
  const uint8_t* possible_actions_mask;        /* [n_rows, n_actions] */
  const uint8_t* possible_next_actions_mask;
  int64_t n_rows;
  int32_t n_features;
  int32_t n_actions;
} rg_dqn_table; /* host struct */
typedef struct {
  void* state;                                 /* [batch, n_out] fp32 or bf16 (state_dtype) */
  void* next_state;
  float* action;                               /* [batch, n_actions] one-hot */
  float* next_action;
  float* reward;                               /* [batch] */
  float* time_diff;
  float* step;
  float* not_terminal;
  float* possible_actions_mask;                /* [batch, n_actions] */
  float* possible_next_actions_mask;
  float* action_probability;
  int64_t* mdp_id;
  int64_t* sequence_number;
  int32_t state_dtype;                         /* RG_DT_F32 / RG_DT_BF16 */
  int32_t reserved;
} rg_dqn_batch_out; /* host struct */
int rg_table_dqn_batch(const rg_dqn_table* table, const int64_t* indices, int batch, const rg_norm_col* cols,
                       int n_out, const float* quantiles, const rg_dqn_batch_out* out, rg_stream_t stream);
/* The replay store as the DQN step reads it (stack_size 1, dense fp32 observations; gym schema of
 * SURVEY.md §8 a1).  rg_replay_dqn_batch = ReplayBuffer.sample_transition_batch
 * (reagent/replay_memory/circular_replay_buffer.py:614-706: n-step steps / next index / terminal /
 * discounted reward, state and next_state rows) + DiscreteDqnInputMaker
 * (reagent/gym/preprocessors/trainer_preprocessor.py:100-158: one-hots, next_action zeroed on terminal,
 * not_terminal, exp(log_prob), masks at idx / next idx or ones) in ONE launch, optionally with
 * Preprocessor.forward on both state matrices (cols = n_features 1:1 descriptors, all present; NULL =
 * raw fp32 rows).  Bit-identical to rg_replay_nstep + rg_replay_gather + rg_make_dqn_input.
 * RG_EUNSUPPORTED (n_features % 4, > 512 features, unaligned rows): use those three instead. */
typedef struct {
  const float* observation;            /* [capacity, n_features] */
  const int64_t* action;               /* [capacity] */
  const float* reward;                 /* [capacity] */
  const uint8_t* terminal;             /* [capacity] */
  const float* log_prob;               /* [capacity], nullable (action_probability = 1) */
  const float* possible_actions_mask;  /* [capacity, n_actions], nullable (all ones) */
  const int64_t* mdp_id;               /* nullable */
  const int64_t* sequence_number;      /* nullable */
  const float* decays;                 /* [update_horizon] gamma**k, as for rg_replay_nstep */
  int64_t capacity;
  int32_t n_features;
  int32_t n_actions;
  int32_t update_horizon;
  int32_t reserved;
} rg_replay_view; /* host struct */
int rg_replay_dqn_batch(const rg_replay_view* view, const int64_t* indices, int batch, const rg_norm_col* cols,
                        const float* quantiles, const rg_dqn_batch_out* out, rg_stream_t stream);
/* ABI 7: the same launch for a replayed step: index_pool [pool rows][batch] int64, the row sampled is *cursor (device; advanced
 * by the step's rg_mlp_update_fused_sched through rg_mlp_update_desc.post_tick); pre_tick_sched (nullable): the device-resident
 * Adam schedule whose step count this launch advances (sched[0] += 1, see rg_mlp_update_desc.sched_pre_ticked). */
int rg_replay_dqn_batch_pooled(const rg_replay_view* view, const int64_t* index_pool, const int64_t* cursor,
                               double* pre_tick_sched, int batch, const rg_norm_col* cols, const float* quantiles,
                               const rg_dqn_batch_out* out, rg_stream_t stream);

/* ABI 11.  The continuous-action twin of rg_replay_dqn_batch: ReplayBuffer.sample_transition_batch
 * (reagent/replay_memory/circular_replay_buffer.py:614-706, stack_size 1, dense fp32 observations and [capacity, action_dim]
 * fp32 actions) + PolicyNetworkInputMaker (reagent/gym/preprocessors/trainer_preprocessor.py:175-227: rescale_actions of action
 * and next_action into the training range, next_action rows of terminal transitions zero, not_terminal = 1 - terminal,
 * action_probability = exp(log_prob)) in ONE launch, optionally with Preprocessor.forward on both state matrices.
 * Bit-identical to rg_replay_nstep + rg_replay_gather + rg_make_policy_input (same operations, same roundings).
 * ranges [4 * action_dim] (device) = prev_min | prev_max | new_min | new_max, as for rg_make_policy_input.
 * RG_EUNSUPPORTED (n_features % 4, > 512 features, unaligned rows): use those three instead. */
typedef struct {
  const float* observation;  /* [capacity, n_features] */
  const float* action;       /* [capacity, action_dim] */
  const float* reward;       /* [capacity] */
  const uint8_t* terminal;   /* [capacity] */
  const float* log_prob;     /* [capacity], nullable (action_probability = 1) */
  const float* decays;       /* [update_horizon] gamma**k, as for rg_replay_nstep */
  const float* ranges;       /* [4 * action_dim] */
  int64_t capacity;
  int32_t n_features;
  int32_t action_dim;
  int32_t update_horizon;
  int32_t reserved;
} rg_policy_replay_view; /* host struct */
typedef struct {
  void* state;                /* [batch, n_features] fp32 or bf16 (state_dtype) */
  void* next_state;
  float* action;              /* [batch, action_dim] rescaled */
  float* next_action;         /* [batch, action_dim] rescaled, zero rows for terminal transitions */
  float* reward;              /* [batch] n-step discounted sum */
  float* not_terminal;        /* [batch] */
  float* action_probability;  /* [batch], nullable */
  int32_t state_dtype;        /* RG_DT_F32 / RG_DT_BF16 */
  int32_t reserved;
} rg_policy_batch_out; /* host struct */
int rg_replay_policy_batch(const rg_policy_replay_view* view, const int64_t* indices, int batch, const rg_norm_col* cols,
                           const float* quantiles, const rg_policy_batch_out* out, rg_stream_t stream);

/* *bad_flag (device int, zeroed by the caller) becomes 1 if a sampled row holds an action outside
 * [0, n_actions) or a next_action outside [0, n_actions] (F.one_hot would raise), 2 if an index is
 * outside [0, n_rows). */
int rg_table_check_actions(const rg_dqn_table* table, const int64_t* indices, int batch, int* bad_flag,
                           rg_stream_t stream);

/* ---- loss heads --------------------------------------------------------------------------- */

/* DQN TD head: boost_rewards (reagent/training/dqn_trainer_base.py:216-241),
 * compute_discount_tensor (reagent/training/dqn_trainer.py:166-177),
 * get_max_q_values_with_target (dqn_trainer_base.py:33-77), compute_td_loss tail
 * (dqn_trainer.py:201-238) and d loss / d q, fused in one pass over the batch.
 * q, qn_online, qn_target [B, A] fp32 contiguous; action, next_mask [B, A] fp32
 * (next_mask = possible_next_actions_mask when maxq_learning, next_action when SARSA);
 * reward, not_terminal [B] fp32; reward_boosts [A] fp32 or NULL;
 * discount = gamma, or gamma ** gamma_exponent[b] when gamma_exponent != NULL (time_diff / step).
 * Outputs: dq [B, A] fp32 = d(mean loss)/d q; loss_partials [rg_dqn_head_partials(B)] fp32 whose
 * ordered sum / B is the loss (rg_reduce_sum finishes it); next_q [B], next_idx [B] int64 and
 * q_sel [B] (nullable) for logging/tests. */
int rg_dqn_head_partials(int batch);
int rg_dqn_head(const float* q, const float* qn_online, const float* qn_target, const float* action,
                const float* next_mask, const float* reward, const float* reward_boosts,
                const float* not_terminal, double gamma, const float* gamma_exponent, int batch,
                int num_actions, int double_q, int loss_type, float* dq, float* loss_partials,
                float* next_q, int64_t* next_idx, float* q_sel, rg_stream_t stream);

/* ABI 12 — the online network's two forwards of a DQN step and the TD head in ONE launch (bf16 fused stacks with a
 * 16-wide output): a workgroup takes rows [128 t, 128 t + 128) of next_state (not saving; -> qn_online) AND of state
 * (saving as rg_mlp_forward_fused(save = 1) does; -> q) — alternate workgroups in alternate order, so that the saving
 * passes' store bursts do not all fall on the same moment — and finishes with rg_dqn_head's arithmetic for those rows,
 * reading qn_target (the target network's forward runs before this launch) and the head's other operands as rg_dqn_head
 * does.  Every output (q, qn_online, the saved fragments and sign planes, dq, next_q, next_idx, q_sel) has the bits of
 * rg_mlp_forward_fused x 2 + rg_dqn_head.  The loss leaves as one sum per wave, loss_wave_sums
 * [rg_dqn_pair_wave_sums(B)] (16 rows each, rg_dqn_head's lane order): rg_mlp_wgrad_fused (rg_mlp_desc.sum_run = 16) or
 * rg_reduce_sum_runs(run = 16) finishes it with the adds of rg_dqn_head + rg_reduce_sum.
 * q, qn_online, qn_target, action, next_mask, dq: [B, 16] fp32 contiguous, 16-byte aligned.  RG_EUNSUPPORTED for
 * anything else (split-bf16, grouped or two-panel stacks, other widths): callers then run the three launches. */
int rg_dqn_pair_wave_sums(int batch);
int rg_dqn_online_pair_forward(const rg_mlp_desc* d, const void* state, int state_dtype, int64_t ld_state,
                               const void* next_state, int next_state_dtype, int64_t ld_next_state, int batch, float* q,
                               float* qn_online, const float* qn_target, const float* action, const float* next_mask,
                               const float* reward, const float* reward_boosts, const float* not_terminal, double gamma,
                               const float* gamma_exponent, int double_q, int loss_type, float* dq, float* loss_wave_sums,
                               float* next_q, int64_t* next_idx, float* q_sel, rg_stream_t stream);

/* ABI 13 — parametric DQN (Q(s, a) over a per-state list of M = max_num_actions candidate actions).
 * rg_tile_concat: out[r, :x_cols] = x[r / x_tile, :], out[r, x_cols:] = x2[r, :] for r < rows — the critic input
 * cat(next_state.get_tiled_batch(M), possible_next_actions) (reagent/core/types.py:349-365 repeat_interleave,
 * reagent/models/critic.py:79-92 cat; parametric_dqn_trainer.py:134-140) for the engines that do not read two panels in
 * place (x_tile = 1: the plain cat(state, action) of :166).  fp32 row-major with the given pitches; a pure copy, 16-byte
 * accesses where pitch and base allow. */
int rg_tile_concat(const float* x, int64_t ldx, const float* x2, int64_t ldx2, int rows, int x_tile, int x_cols, int x2_cols,
                   float* out, int64_t ldo, rg_stream_t stream);
/* rg_pdqn_head: get_max_q_values_with_target (reagent/training/dqn_trainer_base.py:33-77), the TD target with its
 * discount, the loss and d(mean loss)/dq (reagent/training/parametric_dqn_trainer.py:112-171) in one pass over the batch.
 * q [B] = q_network(state, action).  maxq != 0: qn_online_all (read with double_q only), qn_target_all [B * M] = the two
 * networks on the tiled next state, next_mask [B, M]; the values are penalised by -1e9 * (1 - mask) in fp32 as the
 * reference does, the first maximal index wins (double_q: of the online values, the target value at that index is read),
 * a fully masked row selects index 0 and yields the penalised value.  maxq == 0 (SARSA): qn_target_all [B] is the target
 * network's value of (next_state, next_action), the others NULL.  reward, not_terminal [B];
 * discount = gamma, or gamma ** gamma_exponent[b] when gamma_exponent != NULL (time_diff / step), as for rg_dqn_head.
 * target = reward + (not_terminal * discount) * next_q.  loss_type: RG_LOSS_MSE, RG_LOSS_HUBER, RG_LOSS_BCE_LOGITS.
 * Outputs: target [B], dq [B], loss_partials [rg_pdqn_head_partials(B)] whose ordered sum / B is the loss
 * (rg_reduce_sum finishes it), next_q [B], next_idx [B] int64 (nullable). */
int rg_pdqn_head_partials(int batch);
int rg_pdqn_head(const float* q, const float* qn_online_all, const float* qn_target_all, const float* next_mask,
                 const float* reward, const float* not_terminal, double gamma, const float* gamma_exponent, int batch,
                 int max_num_actions, int maxq, int double_q, int loss_type, float* target, float* dq,
                 float* loss_partials, float* next_q, int64_t* next_idx, rg_stream_t stream);

/* ABI 14 — SlateQ (reagent/training/slate_q_trainer.py): a state has C candidate documents [B, C, D] with a presence
 * mask [B, C] (one byte per entry: torch.bool storage) and a value [B, C]; a slate is K indices into them [B, K] int64.
 * rg_slate_gather: DocList.select_slate (reagent/core/types.py:277-284) with _get_docs_value's value * mask
 * (slate_q_trainer.py:162-164).  out_features[b * K + k, :D] (row pitch ldo: the candidate panel of the critic's forward
 * or of rg_tile_concat; NULL: the weights alone) = features[b, index[b, k], :], out_weight[b, k] = value * mask of that
 * document.  Where
 * not_terminal (nullable, [B]) is 0 every index of the row is read as 0 (_action_docs, :112-117; `index` itself is not
 * written).  An index outside [0, C) is a caller error, as it is for torch's indexing: it is CLAMPED into range, so no
 * address outside the arrays is ever formed.  features is contiguous; 16-byte accesses where D, the bases and ldo allow,
 * scalars elsewhere.  count_mask (nullable, count_n bytes) with count_out: the same launch counts the non-zero bytes —
 * the true entries of reward_mask — into count_out[0], the device scalar rg_slateq_head reads.
 * rg_slate_topk: _get_maxq_topk (:145-160).  score[b, c] = q_all[b, c] * w[b, c], w = value * mask, or with
 * single_selection softmax over the C candidates of value * mask (max-subtracted, divided by the row sum).  next_index
 * [B, K] = the K largest scores' indices in descending order, of equal scores the LOWER index first (torch.topk leaves
 * that open; this is torch.sort(descending=True, stable=True)); q_sel [B, K] = q_all at them.  Inputs finite.
 * 1 <= K <= C <= RG_SLATE_MAX_CANDIDATES, RG_EINVAL beyond.
 * rg_slateq_head: train_step_gen :204-259 after the forwards.  q, qn, wn, reward [B, K] fp32 (online critic on the logged
 * slate, target critic on the next slate, value * mask of the next slate's documents), reward_mask [B, K] bytes,
 * not_terminal [B].  next_q[b] = sum_k qn * (single_selection ? softmax over the K items of wn : wn); without single
 * selection divided by min(sum_c norm_mask[b, c], slate_size) (:169-175; norm_mask [B, C] bytes is the current or the
 * next state's mask, by next_slate_value_norm_method); times not_terminal.  target = reward + discount * next_q,
 * discount = gamma, or powf(gamma, time_diff[b] / discount_time_scale) when time_diff != NULL (the division in fp32, the
 * power correctly rounded to fp32).
 * F.mse_loss: with single selection over the n_selected[0] elements where reward_mask is set (dq = 0 elsewhere),
 * otherwise over all B * K.  n_selected is DEVICE memory (rg_slate_gather's count_out): no host synchronisation.
 * Outputs: target, dq [B, K], next_q [B], loss_partials [rg_slateq_head_partials(B)] whose ordered sum is the loss
 * (already divided by the element count; rg_reduce_sum with scale 1 finishes it). */
#define RG_SLATE_MAX_CANDIDATES 1024
int rg_slate_gather(const float* features, const uint8_t* mask, const float* value, const int64_t* index,
                    const float* not_terminal, int batch, int num_candidates, int slate_size, int feature_dim,
                    float* out_features, int64_t ldo, float* out_weight, const uint8_t* count_mask, int64_t count_n,
                    int32_t* count_out, rg_stream_t stream);
int rg_slate_topk(const float* q_all, const float* value, const uint8_t* mask, int batch, int num_candidates, int slate_size,
                  int single_selection, int64_t* next_index, float* q_sel, rg_stream_t stream);
int rg_slateq_head_partials(int batch);
int rg_slateq_head(const float* q, const float* qn, const float* wn, const float* reward, const uint8_t* reward_mask,
                   const float* not_terminal, double gamma, const float* time_diff, double discount_time_scale,
                   int single_selection, const uint8_t* norm_mask, int num_candidates, int slate_size,
                   const int32_t* n_selected, int batch, int num_items, float* target, float* dq, float* loss_partials,
                   float* next_q, rg_stream_t stream);

/* ABI 15 — policy gradient (reagent/training/reinforce_trainer.py, reagent/training/ppo_trainer.py) on PACKED
 * trajectories: N rows, trajectory t the rows [offsets[t], offsets[t + 1]), offsets [T + 1] int32 in DEVICE memory,
 * ascending, offsets[T] = N.
 * rg_pg_returns: per trajectory discounted_returns(clamp(reward, max = reward_clip), gamma)
 * (reagent/training/utils.py:42-54, reinforce_trainer.py:106-108, ppo_trainer.py:225-227) — run = reward[t] + gamma * run
 * from the trajectory's end, gamma rounded to fp32, multiply and add rounded separately: the reference's bits; gamma == 0
 * is the copy the reference makes.  Then normalize != 0: whiten(x, subtract_mean) (utils.py:32-39: the population
 * standard deviation + EPS, EPS = float64's epsilon added in fp32); normalize == 0 and subtract_mean != 0: x - x.mean()
 * (reinforce_trainer.py:113-114).  Then clamp_min != 0: clamp(min = 0) (:115-116).  Mean and variance are summed in
 * double.  A wave per trajectory; an empty trajectory writes nothing; rows outside [offsets[0], offsets[T]) are not
 * written; offsets outside [0, N] are clamped into it.  RG_EINVAL for T < 1 or N < 0.
 * rg_pg_head: one launch over N rows.  scores [N, A] fp32 (row pitch ld_scores) = the scorer's output;
 * possible_actions_mask (nullable, [N, A] fp32 contiguous): scores + (1 - mask) * -1e10 is formed first as
 * FullyConnectedDQN.forward does (reagent/models/dqn.py:60-62) — NULL where the scores already carry it.  action [N, A]
 * (pitch ld_action, in elements) a one-hot in fp32 or int64 (action_is_int64): its first arg-max is the logged action a
 * (reagent/gym/policies/samplers/discrete_sampler.py:67-71).  z = scores / temperature, logp = z - logsumexp(z),
 * p = softmax(z), l = logp[a], H = -sum p * logp (terms with p = 0 count 0), adv = returns - values (values NULL: returns).
 *   RG_PG_REINFORCE (reinforce_trainer.py:105,132)       loss = -adv * l                      g = -adv
 *   RG_PG_REINFORCE_OFF_POLICY (:124-130), clip = clip_param, d = l - old_log_prob, e = exp(min(d, log clip)):
 *                                                          loss = -adv * e                      g = d <= log clip ? -adv * e : 0
 *   RG_PG_PPO (ppo_trainer.py:127-152), clip = ppo_epsilon, rho = exp(l - old_log_prob):
 *                                   loss = -min(adv * rho, adv * clamp(rho, 1 - clip, 1 + clip))
 *                                   g = -adv * rho where the unclipped term is the smaller or rho is inside the clip, else 0
 * every mode: loss -= entropy_weight * H.  Outputs: dscores[i, j] = g * (1[j = a] - p_j) / temperature + entropy_weight *
 * p_j * (logp_j + H) / temperature (pitch ld_dscores); with values: dvalues[i] = 2 * value_scale * (v - returns) and the
 * value loss value_scale * (v - returns)^2 (value_scale = 1 / N: MSELoss "mean", 1: "sum"); log_prob = l, ratio = e or rho
 * (1 on policy), advantage [N] (each nullable); policy_partials, value_partials [rg_pg_head_partials(N, A)] whose ordered
 * sums are the two summed losses (rg_reduce_sum finishes them; no atomics: two runs give the same bits).
 * A group of 1 / 4 / 16 / 64 lanes per row for A <= 4 / 16 / 64 / 256, four consecutive actions per lane, 16-byte
 * accesses where pitch and base allow.  The row's arithmetic runs in double on the fp32 inputs (temperature, clip,
 * entropy_weight and value_scale as the doubles they are passed as) and is rounded once where it is stored.  RG_EINVAL for A < 1, A > RG_PG_MAX_ACTIONS, N < 1, a missing old_log_prob. */
#define RG_PG_MAX_ACTIONS 256
enum { RG_PG_REINFORCE = 0, RG_PG_REINFORCE_OFF_POLICY = 1, RG_PG_PPO = 2 };
int rg_pg_returns(const float* reward, const int32_t* offsets, int num_trajectories, int64_t n, double gamma,
                  double reward_clip, int normalize, int subtract_mean, int clamp_min, float* out, rg_stream_t stream);
int rg_pg_head_partials(int n, int num_actions);
int rg_pg_head(const float* scores, int64_t ld_scores, const float* possible_actions_mask, const void* action,
               int action_is_int64, int64_t ld_action, const float* returns, const float* values, const float* old_log_prob,
               double temperature, int mode, double clip, double entropy_weight, double value_scale, int n, int num_actions,
               float* dscores, int64_t ld_dscores, float* dvalues, float* log_prob, float* ratio, float* advantage,
               float* policy_partials, float* value_partials, rg_stream_t stream);

/* ABI 16 — LinUCB contextual bandit (reagent/training/cb/linucb_trainer.py, reagent/models/linear_regression.py).
 * rg_linucb_accumulate: LinUCBTrainer.update_params (linucb_trainer.py:50-75) on device-resident state, one main launch
 * and one finishing launch, no host synchronisation.  x [batch, dim] fp32 contiguous (action NULL), or x [batch, arms, dim]
 * with action [batch] int64: the chosen arm's row is read in place (add_chosen_arm_features, reagent/training/cb/utils.py:
 * 41-53, without the gathered copy), each index clamped into [0, arms).  y [batch]; weight [batch] or NULL (every weight 1).
 * State, updated in place: cur_avg_A [dim, dim], cur_avg_b [dim], cur_sum_weight [1] fp32, cur_num_obs [1] int64.
 * The main launch forms per-workgroup partials of S_A = sum_b w x x^T (v_mfma_f32_32x32x2_f32 on (w * x, x); only the
 * 32 x 32 tiles on or above the diagonal), S_b = sum_b (w * y) x and s_w = sum_b w over slices of the batch.  The finishing
 * launch adds the partials in slice order, mirrors the triangle and applies :64-75 in the reference's fp32 operation order
 * (no contraction): cur_num_obs += batch; cur_sum_weight += s_w; cur_avg = cur_avg * (1 - s_w / cur_sum_weight) + S /
 * cur_sum_weight.  cur_avg_A leaves exactly symmetric (the entries above the diagonal are the ones read).  No atomics: two
 * runs give the same bits.  workspace: rg_linucb_workspace_bytes(batch, dim) bytes (0 for arguments the call refuses).
 * RG_EINVAL for dim < 1, dim > RG_LINUCB_MAX_DIM, batch < 1, a null pointer, arms < 1 with an action, a short workspace.
 * rg_linucb_score: LinearRegressionUCB._forward_no_coefs_check (linear_regression.py:213-234) over x [n, dim] (n = B *
 * arms rows): pred_label = x . coefs; pred_sigma = sqrt(x^T inv_avg_A x / sum_weight[0]) (batch_quadratic_form, :41-51;
 * sum_weight read from DEVICE memory), exactly 0 and not computed for ucb_alpha == 0; ucb = pred_label + ucb_alpha *
 * pred_sigma.  x * inv_avg_A stays in MFMA accumulators: nothing of size [n, dim] is written.  nan_partials
 * [rg_linucb_score_partials(n)] int32: rows with a NaN sigma per workgroup.  A finishing launch adds them in order into
 * nan_count [1] (plain stores, no atomics) and, for arms > 0, writes best_arm [n / arms] int64 = the arg-max of ucb over
 * each row's arms under arm_presence ([n] bytes, nonzero = present; NULL = all), the lowest index among equals
 * (get_model_actions, reagent/training/cb/utils.py:113-139, randomize_ties = False), the first present NaN before any
 * number; arm 0 for a row with no arm present or with every present arm at -inf (a present -inf counts as an absent arm).
 * RG_EINVAL for n < 1, dim < 1, dim > RG_LINUCB_MAX_DIM, arms < 0, n not a multiple of arms, a null pointer. */
#define RG_LINUCB_MAX_DIM 512
size_t rg_linucb_workspace_bytes(int batch, int dim);
int rg_linucb_accumulate(const float* x, const int64_t* action, int arms, const float* y, const float* weight, int batch,
                         int dim, float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs,
                         void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_linucb_score_partials(int n);
int rg_linucb_score(const float* x, const float* coefs, const float* inv_avg_A, const float* sum_weight, double ucb_alpha,
                    int n, int dim, int arms, const uint8_t* arm_presence, float* pred_label, float* pred_sigma, float* ucb,
                    int32_t* nan_partials, int32_t* nan_count, int64_t* best_arm, rg_stream_t stream);

/* ABI 17 — disjoint LinUCB: one ridge regression per arm (reagent/training/cb/disjoint_linucb_trainer.py,
 * reagent/models/disjoint_linucb_predictor.py).
 * rg_dlinucb_accumulate: DisjointLinUCBTrainer.cb_training_step (disjoint_linucb_trainer.py:88-101: a Python loop of
 * update_params, :46-76, over the arms) for ALL arms in one main and one finishing launch, no host synchronisation.
 * x [n, dim] fp32 contiguous, y [n], weight [n] or NULL (every weight 1): the arms' sub-batches back to back in arm order;
 * row_offsets [arms + 1] int64 in DEVICE memory: arm a's rows are [row_offsets[a], row_offsets[a + 1]) (forced into
 * 0 <= begin <= end <= n where they are not; an empty range is legal).  max_arm_rows is a HOST hint, the longest sub-batch:
 * it sizes the grid and the workspace and never decides which rows count (the last slice of an arm runs to the arm's end).
 * State, updated in place: cur_A [arms, dim, dim], cur_b [arms, dim] fp32, cur_num_obs [arms] int64.  The main launch forms,
 * per (tile on or above the diagonal, slice of the arm's rows, arm), partials of S_A = sum w x x^T (v_mfma_f32_32x32x2_f32 on
 * (w * x, x)) and S_b = sum (w * y) x; a workgroup whose slice is empty writes zeros.  The finishing launch adds an arm's
 * slices in order, mirrors the triangle, and does cur_A[a] += S_A, cur_b[a] += S_b (one fp32 add each; cur_A[a] leaves
 * exactly symmetric: the entries above the diagonal are the ones read) and cur_num_obs[a] += n_a.  No atomics: two runs give
 * the same bits.  Where an arm's rows are cut into slices depends on dim alone, so an arm's result depends only on its own
 * rows — not on where they lie in the packed batch, on the other arms or (while the hint is not too short and the launch has
 * under 2^20 workgroups) on max_arm_rows: a call with arms = 1 on one arm's rows and that arm's slice of the state gives the
 * bits of the packed call.  workspace: rg_dlinucb_workspace_bytes(max_arm_rows, arms, dim) bytes (0 for arguments the call
 * refuses).  n == 0 is legal and changes nothing.  RG_EINVAL for dim < 1, dim > RG_LINUCB_MAX_DIM, arms < 1, arms > 65535,
 * n < 0, max_arm_rows < 0, a null pointer (weight excepted; x and y too where n == 0), a short workspace.
 * rg_dlinucb_score: DisjointLinearRegressionUCB.forward (disjoint_linucb_predictor.py:149-174, with
 * batch_quadratic_form_multi_arms, :17-31) over x [batch, dim]: mean[r, a] = x_r . coefs[a] (coefs [arms, dim]);
 * sigma[r, a] = sqrt(x_r^T inv_A[a] x_r) (inv_A [arms, dim, dim]; no division by a weight, no NaN check: a negative form is
 * NaN, silently); ucb = mean + float(ucb_alpha) * sigma, one multiply and one add.  ucb_alpha == 0: inv_A is not read, sigma
 * is exactly 0 and ucb has the bits of mean.  ucb [batch, arms] is required; mean and sigma [batch, arms] may be NULL.
 * best_arm [batch] int64 (or NULL), from the same launch: the arg-max of ucb over the arms arm_presence ([batch, arms] bytes,
 * nonzero = present; NULL = all) marks present, the lowest index among equals, a NaN before any number (rg_linucb_score's
 * rule), arm 0 for a row with no arm present or with every present arm at -inf (get_model_actions,
 * reagent/training/cb/utils.py:113-139).  A workgroup stages its rows of x in LDS once and reuses them for every arm;
 * x * inv_A[a] stays in MFMA accumulators.  One launch.
 * RG_EINVAL for batch < 1, arms < 1, dim < 1, dim > RG_LINUCB_MAX_DIM, batch * arms >= 2^31, a null x / coefs / inv_A / ucb,
 * arm_presence without best_arm. */
size_t rg_dlinucb_workspace_bytes(int max_arm_rows, int arms, int dim);
int rg_dlinucb_accumulate(const float* x, const float* y, const float* weight, const int64_t* row_offsets, int n, int arms,
                          int max_arm_rows, int dim, float* cur_A, float* cur_b, int64_t* cur_num_obs, void* workspace,
                          size_t workspace_bytes, rg_stream_t stream);
int rg_dlinucb_score(const float* x, const float* coefs, const float* inv_A, double ucb_alpha, int batch, int dim, int arms,
                     const uint8_t* arm_presence, float* mean, float* sigma, float* ucb, int64_t* best_arm,
                     rg_stream_t stream);

/* ABI 18 — deep-represent LinUCB: an MLP's output under a LinUCB layer (reagent/models/deep_represent_linucb.py,
 * reagent/training/cb/deep_represent_linucb_trainer.py).
 * rg_linucb_solve: LinearRegressionUCB._calculate_coefs (reagent/models/linear_regression.py:157-199, one process) on
 * device-resident state in ONE launch of one workgroup, no host synchronisation, for 1 <= dim <= RG_LINUCB_SOLVE_MAX_DIM.
 * The deep model runs it on every training step (deep_represent_linucb.py:148-151: cur_avg_A is non-zero after every
 * update_params).  Fold (reduce_avg, :54-89) in the reference's fp32 operation order, no contraction, bit for bit:
 * total = cur_sum_weight + sum_weight; avg_A = (avg_A * sum_weight + cur_avg_A * cur_sum_weight) / total, likewise avg_b;
 * num_obs += cur_num_obs; sum_weight += cur_sum_weight.  A_ext = avg_A + float(l2_reg_lambda) * I / sum_weight (the diagonal
 * gets (lambda * 1) / sum_weight in fp32, the rest of avg_A is taken as it is).  inv_avg_A = A_ext^-1 by Gauss-Jordan
 * elimination without pivoting (A_ext is symmetric positive definite for lambda > 0): the matrix lives in the registers of
 * a 16 x 16 grid of threads (entry (i, j) with thread (i % 16, j % 16); 1, 4, 16 or 64 entries a thread for dim <= 16 / 32 /
 * 64 / 128); every step publishes the pivot row and column through LDS (2.5 KB) and costs one barrier.  coefs = inv_avg_A * avg_b; coefs_valid_for_avg_A = avg_A;
 * cur_avg_A, cur_avg_b, cur_sum_weight and cur_num_obs leave exactly zero.  status [1] int32 is STICKY: set to 1 where a
 * pivot is not positive or not finite (the call still runs all dim steps and writes finite-or-NaN values; a caller that
 * finds it set recomputes on the host from the folded avg_A and clears it), never written otherwise.  No atomics: two runs
 * give the same bits.  RG_EINVAL for dim < 1, dim > RG_LINUCB_SOLVE_MAX_DIM, a null pointer.
 * rg_drlinucb_head: what DeepRepresentLinearRegressionUCB.forward (deep_represent_linucb.py:136-152, 165) and
 * DeepRepresentLinUCBTrainer.cb_training_step (deep_represent_linucb_trainer.py:81-89) do after the MLP, and autograd's
 * backward of it.  mlp_out [batch, h] fp32 (pitch ld_mlp_out); v [h + 1] = linear_layer.weight[0] (nn_e2e) or _coefs.
 * Always written: z [batch, h + 1] contiguous = [1, mlp_out] (mlp_out_with_ones: what forward returns and
 * rg_linucb_accumulate / rg_linucb_score read), lin [batch] = z . v, pred_label [batch] = act(lin) (act an RG_ACT_* code,
 * the FC epilogues' functions).  label == NULL is the forward-only mode: nothing else is written and no finishing launch
 * follows.  With label [batch] (weight [batch] or NULL: every weight 1), loss_type RG_CB_LOSS_MSE (p - y)^2, RG_CB_LOSS_MAE
 * |p - y|, RG_CB_LOSS_BCE -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) (F.binary_cross_entropy):
 * row_loss [batch] = loss_r * w_r; loss [1] = sum_r row_loss / batch; with g_r = 2 (p - y), sign(p - y) (sign(0) = 0),
 * (p - y) / max(p (1 - p), 1e-12) and dlin_r = g_r * (w_r / batch) * act'(lin_r): dmlp_out [batch, h] (pitch ld_dmlp_out)
 * = dlin_r * v[1:], and, where dv is not NULL (nn_e2e), dv [h + 1] = sum_r dlin_r * z_r.  The main launch leaves
 * per-workgroup partials (loss_partials [P], dv_partials [P, h + 1], P = rg_drlinucb_head_partials(batch, h)); a finishing
 * launch adds them in a fixed order (in double) into loss and dv.  No atomics: two runs give the same bits.  1 / 4 / 16 /
 * 64 lanes per row for h <= 4 / 16 / 64 / more.  RG_EINVAL for batch < 1, h < 1, h + 1 > RG_LINUCB_MAX_DIM, a pitch below
 * h, an unknown act or loss_type, a null mlp_out / v / z / lin / pred_label, and with a label a null row_loss / dmlp_out /
 * loss_partials / loss, or dv without dv_partials.
 * rg_drlinucb_activate: a[i] = act(a[i]) and (b not NULL) b[i] = act(b[i]) for i < n, one launch: the output activation on
 * pred_label and ucb after rg_linucb_score (deep_represent_linucb.py:165-166, 202-204).  RG_EINVAL for n < 1, a null a, an
 * unknown act. */
#define RG_LINUCB_SOLVE_MAX_DIM 128
enum { RG_CB_LOSS_MSE = 0, RG_CB_LOSS_MAE = 1, RG_CB_LOSS_BCE = 2 };
int rg_linucb_solve(int dim, double l2_reg_lambda, float* avg_A, float* avg_b, float* sum_weight, int64_t* num_obs,
                    float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs, float* inv_avg_A,
                    float* coefs, float* coefs_valid_for_avg_A, int32_t* status, rg_stream_t stream);
int rg_drlinucb_head_partials(int batch, int h);
int rg_drlinucb_head(const float* mlp_out, int64_t ld_mlp_out, const float* v, const float* label, const float* weight,
                     int act, int loss_type, int batch, int h, float* z, float* lin, float* pred_label, float* row_loss,
                     float* dmlp_out, int64_t ld_dmlp_out, float* loss_partials, float* dv_partials, float* loss, float* dv,
                     rg_stream_t stream);
int rg_drlinucb_activate(float* a, float* b, int n, int act, rg_stream_t stream);

/* ABI 19 — offline policy evaluation inside the contextual-bandit training loop: the replay estimator of Li et al.
 * (arXiv 1003.0146, Algorithm 3), reagent/evaluation/cb/policy_evaluator.py, base_evaluator.py, utils.py.
 * rg_cb_eval_ingest: BaseOfflineEval.ingest_batch (base_evaluator.py:147-169) = PolicyEvaluator._process_all_data
 * (policy_evaluator.py:22-35), add_importance_weights (evaluation/cb/utils.py:9-47) and _process_used_data
 * (policy_evaluator.py:38-68), plus sum_weight_since_update_local += ... (reagent/training/cb/base_trainer.py:127-129), in
 * one main and one finishing launch on device-resident state, no atomics, no host synchronisation.  action, model_action
 * [batch] int64 (model_action is rg_linucb_score's best_arm as it is); reward [batch] fp32; weight [batch] or NULL (every
 * weight 1); action_log_probability [batch] or NULL; arm_presence [batch, arms] bytes (nonzero = present) or NULL.  Per row,
 * every operation rounded to fp32 on its own: size = the row's count of present arms (arms without arm_presence);
 * p = exp(logp), or 1.0f / size without log-probabilities; iw = 1.0f / p (two IEEE divisions); with clip != 0
 * iw = iw > float(max_importance_weight) ? that : iw (torch.clamp(max=): a NaN passes); importance_weight = (action ==
 * model_action ? 1.0f : 0.0f) * iw — a multiplication: 0 * inf is NaN, as in the reference; effective_weight = w *
 * importance_weight (what rg_linucb_accumulate / rg_drlinucb_head take as their weight); acc = importance_weight > 0.
 * The nine one-element fp32 buffers each receive their sum over the batch, in the order of the arguments: w; w * reward;
 * w * size; eff * reward; (w * acc) * reward; w * acc; eff; (w * acc) * size; and w again into sum_weight_since_update.
 * The main launch leaves per-workgroup (256 rows) partials in double in `partials` (8 * rg_cb_eval_ingest_partials(batch)
 * doubles); the finishing launch adds them in a fixed order and adds each total to its buffer with ONE rounding to fp32:
 * two runs give the same bits.  KEPT QUIRK of the reference: without arm_presence its `sizes` [B, 1] times
 * `weights.squeeze()` [B] broadcasts to [B, B], so the two size sums are `batch` times too large (B * arms * sum w); they are
 * here too.  With arm_presence they are the plain sums.  RG_EINVAL for batch < 1, arms < 1, a null action / model_action /
 * reward / importance_weight / effective_weight / partials / state pointer. */
int rg_cb_eval_ingest_partials(int batch);
int rg_cb_eval_ingest(const int64_t* action, const int64_t* model_action, const float* reward, const float* weight,
                      const float* action_log_probability, const uint8_t* arm_presence, int batch, int arms,
                      int clip, double max_importance_weight, float* importance_weight, float* effective_weight,
                      double* partials, float* sum_weight_all_data, float* sum_reward_weighted_all_data,
                      float* sum_size_weighted_all_data, float* sum_reward_importance_weighted_accepted,
                      float* sum_reward_weighted_accepted, float* sum_weight_accepted,
                      float* sum_importance_weight_accepted, float* sum_size_weighted_accepted,
                      float* sum_weight_since_update, rg_stream_t stream);

/* ABI 20 — rg_linucb_solve_blocked: rg_linucb_solve's contract, word for word, for 1 <= dim <= RG_LINUCB_MAX_DIM (the
 * deep-represent model's solve where its last layer is 128 to 511 wide).  Fold (reduce_avg) in the reference's fp32
 * operation order, bit for bit, an elementwise launch; A_ext = avg_A + (float(l2_reg_lambda) * 1) / sum_weight on the
 * diagonal; inv_avg_A = A_ext^-1; coefs = inv_avg_A * avg_b; coefs_valid_for_avg_A = avg_A; cur_avg_A, cur_avg_b,
 * cur_sum_weight and cur_num_obs leave exactly zero; inv_avg_A leaves EXACTLY symmetric (the tiles on or above the
 * diagonal are computed and mirrored).  The route is a blocked Cholesky factorisation in 32 x 32 blocks, n = ceil(dim / 32),
 * on three P x P fp32 matrices (P = 32 n) in `workspace` (rg_linucb_solve_blocked_workspace_bytes(dim) = 12 P^2 bytes; 0
 * for a dim the call refuses): A_ext padded with the identity, L^T with A_ext = L L^T (only the lower triangle of A_ext is
 * read) and W = L^-1.  n + 3 launches, ordered by the stream alone (no cooperative launch, no flag a workgroup waits on):
 * the fold; one launch per block column k in which every workgroup factors the diagonal block S_kk = A_kk - sum_{j<k}
 * L_kj L_kj^T for itself (unblocked, in LDS) and inverts the factor by substitution (W_kk), then one workgroup each forms
 * a panel block L_gk = (A_gk - sum_{j<k} L_gj L_kj^T) W_kk^T (g > k) or a block of row k of the block substitution
 * W_kg = -W_kk sum_{g<=j<k} L_kj W_jg (g < k); inv = W^T W over the upper tiles; coefs and the fold's one-element
 * buffers.  The block products run on v_mfma_f32_32x32x2_f32, their steps dealt to the workgroup's four waves and the
 * four partial tiles added in wave order: trip counts depend on dim alone, no atomics, two runs give the same bits.
 * status [1] int32 is STICKY: set to 1 where a pivot of a diagonal block is not positive or not finite (the call still
 * runs every launch and writes finite-or-NaN values), never written otherwise.  RG_EINVAL for dim < 1, dim >
 * RG_LINUCB_MAX_DIM, a null pointer, a workspace that is short or not 4-byte aligned. */
size_t rg_linucb_solve_blocked_workspace_bytes(int dim);
int rg_linucb_solve_blocked(int dim, double l2_reg_lambda, float* avg_A, float* avg_b, float* sum_weight, int64_t* num_obs,
                            float* cur_avg_A, float* cur_avg_b, float* cur_sum_weight, int64_t* cur_num_obs,
                            float* inv_avg_A, float* coefs, float* coefs_valid_for_avg_A, int32_t* status, void* workspace,
                            size_t workspace_bytes, rg_stream_t stream);

/* ABI 21 — counterfactual policy evaluation (CPE) of the discrete DQN trainers on a device-resident EvaluationDataPage:
 * reagent/evaluation/evaluation_data_page.py, doubly_robust_estimator.py, sequential_doubly_robust_estimator.py, cpe.py.
 * Common to the five entry points: no atomics; trip counts come from the arguments (an episode's from its clamped offsets);
 * sums are double and added in a fixed order, so two runs give the same bits; every fp32 operation named below is rounded
 * on its own (no contraction); RG_EINVAL for a null pointer that is not marked "or NULL" and for a size out of range.
 *
 * rg_cpe_page_rows: the row arithmetic of EvaluationDataPage.create_from_tensors_dqn (:334-378, 408-433), one launch per
 * validation batch.  q [batch, A] = the model outputs the policy acts on; q_cpe, reward_est [batch, M * A] = q_network_cpe
 * (state), reward_network(state), M = 1 + the number of extra metrics (q_cpe may be NULL where M == 1); action [batch, A]
 * (one-hot, as floats); possible_actions_mask [batch, A] or NULL (every action possible); reward [batch]; reward_boosts [A] or
 * NULL.  logged_rewards = reward + sum_a action * boost (boost_rewards, dqn_trainer_base.py:216-241); model_propensities
 * [batch, A] = masked_softmax(q, mask, temperature) (core/torch_utils.py:62-73, the NaN-to-0 rule of a fully masked row
 * included; the same row code as rg_cpe_head's propensities); eval_action_idxs [batch] int64 = get_max_q_values(q, mask)[1]
 * (first maximal q + -1e9 * (1 - mask); the same row code as rg_dqn_head's); model_rewards_for_logged_action [batch] = sum_a
 * reward_est[:, a] * action; model_metrics_for_logged_action, model_metrics_values_for_logged_action [batch, M - 1] = the same
 * sum over columns i A .. (i + 1) A of reward_est and q_cpe, i = 1 .. M - 1 (both unused where M == 1).  Sums over actions run
 * left to right in fp32.
 *
 * rg_cpe_episode_values: EvaluationDataPage.compute_values_for_mdps (:523-540) on a page sorted by (mdp_id, sequence_number).
 * Episode e is rows episode_offsets[e] .. episode_offsets[e + 1] - 1 ([episodes + 1] int32 in device memory, clamped to
 * [0, rows] and to begin <= end before use).  One lane per episode walks it backwards: values[x] = column[x] + values[x + 1] *
 * fp32(pow(gamma, double(sequence_number[x + 1] - sequence_number[x]))), the multiply and the add rounded separately; the
 * episode's last row is column's.  column and values have pitches ld and ld_values (in floats), so a metric column of
 * logged_metrics is scanned in place; sequence_number [rows] int64.  pow is the device library's double pow: it and the
 * host's math.pow are each within an ulp in double, so the two fp32 factors agree unless the true value lies within 2^-29
 * (relative) of an fp32 rounding tie; nothing closer is claimed.
 *
 * rg_cpe_dr_rows: the row quantities of DoublyRobustEstimator (doubly_robust_estimator.py:219-239, 266-304) and of
 * SequentialDoublyRobustEstimator (sequential_doubly_robust_estimator.py:29-68).  model_propensities, action_mask [rows, A]
 * contiguous; model_rewards, model_values [rows, A] with row pitches (a metric's columns are read in place); logged_propensities
 * [rows]; logged_rewards and model_rewards_for_logged_action [rows] with pitches.  Per row, over actions left to right in fp32:
 * target_propensity = sum p * mask; dm = sum p * model_rewards; state_value = sum p * model_values; q_logged = sum model_values
 * * mask; then importance_weight = target_propensity / logged_propensity; ips = iw * r; dr = iw * (r - mr_logged) + dm.
 * dm_ips_dr is [3, rows] (dm, ips, dr), so the bootstrap reads the three together.  partials: 5 * rg_cpe_dr_partials(rows)
 * doubles (per workgroup of 256 rows); a finishing launch adds them in order into totals [5] (double): sum logged_rewards,
 * sum dm, sum mr_logged, sum ips, sum dr.
 *
 * rg_cpe_sdr: the sequential-DR recurrence (:70-95), one lane per episode, backwards, fp32, g = fp32(gamma):
 * d = state_value[j] + importance_weight[j] * ((r[j] + g * d) - q_logged[j]); e = e * g + r[j], both from 0.  doubly_robust,
 * episode_value [episodes].  Offsets as in rg_cpe_episode_values.
 *
 * rg_cpe_bootstrap: bootstrapped_std_error_of_mean (cpe.py:176-191) of up to RG_CPE_BOOTSTRAP_MAX_COLUMNS columns at once.
 * values [columns, n] fp32 with row pitch ld.  THE DRAW RECIPE: draw j (0 <= j < sample_size) of resample k (0 <= k <
 * num_samples) takes word j % 4 of the Philox4x32-10 block with key (lo32(seed), hi32(seed)) and counter (c0, c1, c2, c3) =
 * (j / 4, 0, k, 0) (ten rounds, multipliers 0xD2511F53 on c0 and 0xCD9E8D57 on c2, key increments 0x9E3779B9 and 0xBB67AE85;
 * round: c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))); index = (word * n) >> 32 in 64-bit
 * arithmetic, in [0, n) by construction; index i is drawn with probability within n / 2^32 of 1 / n.  One index stream
 * serves every column.  One workgroup per resample (one wave where sample_size <= 256, else four), a fixed assignment of draws
 * to lanes, per-lane double sums, a fixed-order tree; means [columns, num_samples] (double) = sum / sample_size (sample_size == 0: NaN, as np.mean of nothing).  A
 * finishing launch writes std [columns] (double): the population standard deviation (ddof 0) of each column's means, two
 * passes in a fixed order.  RG_EINVAL for columns outside 1 .. RG_CPE_BOOTSTRAP_MAX_COLUMNS, n < 1, ld < n, sample_size < 0,
 * num_samples < 1. */
#define RG_CPE_BOOTSTRAP_MAX_COLUMNS 4
int rg_cpe_page_rows(const float* q, const float* q_cpe, const float* reward_est, const float* action,
                     const float* possible_actions_mask, const float* reward, const float* reward_boosts, double temperature,
                     int batch, int num_actions, int num_metrics, float* logged_rewards, float* model_propensities,
                     int64_t* eval_action_idxs, float* model_rewards_for_logged_action,
                     float* model_metrics_for_logged_action, float* model_metrics_values_for_logged_action,
                     rg_stream_t stream);
int rg_cpe_episode_values(const float* column, int64_t ld, const int64_t* sequence_number, const int32_t* episode_offsets,
                          int episodes, int rows, double gamma, float* values, int64_t ld_values, rg_stream_t stream);
int rg_cpe_dr_partials(int rows);
int rg_cpe_dr_rows(const float* model_propensities, const float* action_mask, const float* model_rewards,
                   int64_t ld_model_rewards, const float* model_values, int64_t ld_model_values,
                   const float* logged_propensities, const float* logged_rewards, int64_t ld_logged_rewards,
                   const float* model_rewards_for_logged_action, int64_t ld_model_rewards_for_logged_action, int rows,
                   int num_actions, float* target_propensity, float* importance_weight, float* dm_ips_dr,
                   float* state_value, float* q_logged, double* partials, double* totals, rg_stream_t stream);
int rg_cpe_sdr(const float* state_value, const float* importance_weight, const float* logged_rewards,
               int64_t ld_logged_rewards, const float* q_logged, const int32_t* episode_offsets, int episodes, int rows,
               double gamma, float* doubly_robust, float* episode_value, rg_stream_t stream);
int rg_cpe_bootstrap(const float* values, int64_t ld, int columns, int n, int sample_size, int num_samples, uint64_t seed,
                     double* means, double* std, rg_stream_t stream);

/* ABI 22 — the weighted sequential doubly-robust and MAGIC estimators' row and episode arithmetic on a sorted, device-resident
 * EvaluationDataPage (reagent/evaluation/weighted_sequential_doubly_robust_estimator.py:27-155, 275-353; arXiv 1604.00923
 * sections 5, 7, 8).  Everything of the reference's estimate() except the quadratic program over the j-step weights, which
 * stays on the host: rg_cpe_wsdr leaves j_step_returns, infinite_step_returns, the covariance of the j-step returns and the
 * mean episode value in `out`, J + G + J * J + 1 doubles, read back once.
 *
 * Inputs.  model_propensities, action_mask [rows, A] contiguous; model_values [rows, A] with row pitch ld_model_values (a
 * metric's columns are read in place); logged_propensities [rows]; logged_rewards [rows] with pitch ld_logged_rewards (a
 * set_metric_as_reward page's column); all fp32 in device memory.  episode_offsets [episodes + 1] int32 in device memory as in
 * rg_cpe_episode_values (clamped to [0, rows] and to begin <= end before use; an episode longer than `longest` is cut to it).
 * longest = T, the longest episode.  j_steps [J] and subset_offsets [G + 1] int32 are HOST arrays, copied into the launch
 * arguments: j_steps already reduced to -1 .. T - 1 (the reference's inf is T - 1), J <= RG_CPE_WSDR_MAX_J_STEPS; subset g is
 * episodes subset_offsets[g] .. subset_offsets[g + 1] - 1 (non-decreasing, inside [0, episodes]; G <= RG_CPE_WSDR_MAX_SUBSETS;
 * n_g = its length).  An episode in no subset (:118-119's float interval can leave the last one out) still counts in the whole
 * set.  J == 1 (weighted DR) takes no subsets (subset_offsets and G are ignored) and computes no covariance: `out` is then
 * j_step_returns[0], the mean episode value at out[1], and its whole-set column sums are added over min(episodes, 32) even
 * runs of episodes in run order.
 *
 * All arithmetic is double on the fp32 inputs, each operation rounded on its own (no contraction), no atomics, a fixed order
 * of adds: two runs give the same bits.  Padding is virtual: a step t >= len_e has reward, state value and logged q 0 and raw
 * weight 0; nothing of size episodes * T is stored.  The launches, all on `stream`, nothing synchronised in between:
 *  1. rows, a thread per row, over actions left to right: ratio = (sum p * mask) / logged_p; sv = sum p * mv; ql = sum mv * mask.
 *  2. cumulative weights, a lane per episode, forwards: w_raw[row] = product of ratio up to that row (:72-73).
 *  3. column sums, a thread per step t (neighbouring lanes read neighbouring rows of one episode), a grid row per subset:
 *     S[g, t] = sum of w_raw over the subset's episodes longer than t, in episode order; then S[t] = sum_g S[g, t] in subset
 *     order plus the left-out episodes in episode order, and disc[t] = pow(gamma, (double)t) (:86-88, np.logspace).
 *  4. returns, a lane per episode walking its rows once.  With a set's column sums S and size n (normalize_importance_weights,
 *     :275-289): wn[t] = self_normalize ? (S[t] == 0 ? 1 / n : w_raw[t] / S[t]) : w_raw[t] / n; wprev[0] = 1 / n, wprev[t] =
 *     wn[t - 1]; P_t = sum_{s <= t} disc[s] * (wn[s] * r[s] - wn[s] * ql[s] + wprev[s] * sv[s]), s ascending, P_-1 = 0;
 *     ret[j, e] = P_min(j_steps[j], len - 1) + (j_steps[j] + 1 < len ? disc[j + 1] * wprev[j + 1] * sv[j + 1] : 0)
 *     (calculate_step_return, :291-343).  ret is [J + 1, episodes]; its last row is the episode value sum_t disc[t] * r[t].
 *     inf_ret[e] is the same with j = T - 1 and the episode's own subset's S[g, .] and n_g; 0 for an episode in no subset.
 *  5. moments: j_step_returns[j] = sum_e ret[j, e]; infinite_step_returns[g] = sum_{e in g} inf_ret[e]; the mean of the
 *     episode-value row; C[j, k] = sum_e (ret[j, e] - m_j) (ret[k, e] - m_k) / (episodes - 1) with m = the row means, as
 *     np.cov does it (:228).  One workgroup per sum and per pair k >= j: a strided lane sum in episode order (lane i adds
 *     i, i + 256, ...), a fixed LDS tree; C[k, j] is the same double as C[j, k].  episodes == 1 gives 0 / 0 = NaN as np.cov.
 * out = j_step_returns [J], infinite_step_returns [G], C [J, J] row-major, mean episode value [1] (J == 1: [2], see above).
 * workspace: rg_cpe_wsdr_workspace_bytes(rows, episodes, longest, J, G) bytes of device memory, 0 for arguments rg_cpe_wsdr
 * refuses.  RG_EINVAL for a null pointer, J, G, episodes or rows < 1 (G only where J > 1), J or G beyond its maximum, episodes >
 * rows, longest < 1 or > rows, num_actions < 1, a j_step outside -1 .. T - 1, subset offsets that decrease or leave [0,
 * episodes], a pitch below its row, a workspace too small. */
#define RG_CPE_WSDR_MAX_J_STEPS 32
#define RG_CPE_WSDR_MAX_SUBSETS 32
size_t rg_cpe_wsdr_workspace_bytes(int rows, int episodes, int longest, int num_j_steps, int num_subsets);
int rg_cpe_wsdr(const float* model_propensities, const float* action_mask, const float* model_values, int64_t ld_model_values,
                const float* logged_propensities, const float* logged_rewards, int64_t ld_logged_rewards,
                const int32_t* episode_offsets, int rows, int num_actions, int episodes, int longest, double gamma,
                int self_normalize, const int32_t* j_steps, int num_j_steps, const int32_t* subset_offsets, int num_subsets,
                void* workspace, size_t workspace_bytes, double* ret, double* out, rg_stream_t stream);

/* Batch-constrained q-learning (reagent/training/dqn_trainer.py:209-215 with
 * get_valid_actions_from_imitator, reagent/training/imitator_training.py:12-25): mask [B, A] (in place)
 * *= (softmax(imitator_logits)[b, a] / max_a softmax(imitator_logits)[b, :] >= drop_threshold). */
int rg_bcq_filter(const float* imitator_logits, int batch, int num_actions, double drop_threshold, float* mask,
                  rg_stream_t stream);

/* CPE heads of the DQN step, _calculate_cpes (reagent/training/dqn_trainer_base.py:338-452) with
 * masked_softmax (reagent/core/torch_utils.py:62-73): reward-network MSE and CPE q-network loss on the
 * logged action's column of each of the M metrics, and both output gradients.
 * reward_est, q_cpe, q_cpe_tgt_next [B, M*A] fp32 = reward_network(state), q_network_cpe(state),
 * q_network_cpe_target(next_state); next_scores [B, A] = q_network(next_state) (after the q step);
 * next_mask [B, A] = possible_next_actions_mask (maxq) or next_action (SARSA); action [B, A] one-hot;
 * reward [B] (unboosted), extra_metrics [B, M-1] or NULL (M == 1); discount as in rg_dqn_head.
 * Outputs: d_reward_est, d_q_cpe [B, M*A] = d(mean loss)/d output; reward_partials, cpe_partials
 * [rg_dqn_head_partials(B)] whose ordered sums / (B*M) are the two losses; propensities_out [B, A]
 * (nullable) = model propensities of the next states. */
int rg_cpe_head(const float* reward_est, const float* q_cpe, const float* q_cpe_tgt_next,
                const float* next_scores, const float* next_mask, const float* action,
                const float* reward, const float* extra_metrics, const float* not_terminal, double gamma,
                const float* gamma_exponent, double temperature, int batch, int num_actions,
                int num_metrics, int loss_type, float* d_reward_est, float* d_q_cpe,
                float* reward_partials, float* cpe_partials, float* propensities_out,
                rg_stream_t stream);

/* C51 head, reagent/training/c51_trainer.py:98-187 (+ CategoricalDQN.log_dist,
 * reagent/models/categorical_dqn.py:36-38).  q / qn_online / qn_target [B, A*N] fp32 = logits viewed
 * (B, A, N); qn_online NULL = select the next action with the target net.  next_mask [B, A] =
 * possible_next_actions_mask (maxq != 0) or next_action (SARSA); support [N] = linspace(qmin, qmax, N).
 * Outputs: dq [B, A*N] = d loss / d logits; loss_partials [B] whose sum is the loss; all_q [B, A]
 * (nullable) = expected values of the current distributions.  Limits: N <= 1024, A <= 256. */
int rg_c51_head(const float* q, const float* qn_online, const float* qn_target, const float* action,
                const float* next_mask, const float* reward, const float* reward_boosts,
                const float* not_terminal, double gamma, const float* gamma_exponent, const float* support,
                double qmin, double qmax, int batch, int num_actions, int num_atoms, int maxq, float* dq,
                float* loss_partials, float* all_q, rg_stream_t stream);

/* Dueling aggregation, reagent/models/dueling_q_network.py:96-107: value [B, num_atoms], advantage [B, A * num_atoms]
 * viewed (B, A, N) (num_atoms = 1 for plain DQN): q = value + advantage - mean over (actions, atoms) of advantage;
 * rg_dueling_split is its adjoint (dadvantage = dq - mean(dq), dvalue[b, n] = sum over actions of dq[b, a, n]). */
int rg_dueling_combine(const float* value, int64_t ldv, const float* advantage, int64_t lda, int batch,
                       int num_actions, int num_atoms, float* q, int64_t ldq, rg_stream_t stream);
int rg_dueling_split(const float* dq, int64_t lddq, int batch, int num_actions, int num_atoms, float* dadvantage,
                     int64_t ldda, float* dvalue, int64_t lddv, rg_stream_t stream);

/* ---- QR-DQN with a grouped output layer (qr_grouped.hip; reagent/training/qrdqn_trainer.py:108-160) ---------
 * The [A * N, H] output layer is treated as A layers [N, H] ("groups"); the batch rows are sorted by the action
 * whose quantiles are needed — "grouped space", dense (ABI 9: no padding between the groups, ceil(batch / 128) tiles) or with
 * each action's rows padded to whole 128-row tiles (rounds 2-3), described by
 *   rowmap    [128 * n_tiles] int32 : batch row of each grouped row, -1 for padding
 *   tile_key  [n_tiles] int32       : first group with rows in each tile, -1 for none
 *   row_begin [n_groups + 1] int32  : first grouped row of each group ([n_groups] = end of the last group's range)
 * all built on the device.  Forward and input gradient of the grouped layer run inside the fused stack kernels
 * (rg_mlp_desc.rowmap / tile_key); h_frag below is the saved input of the stack's last layer (act_frag[L-1]) and
 * dz_frag the dz_frag[L-1] that backward wrote.
 * rg_group_weights_stage : w [n_groups * group_rows, in] fp32 -> per-group B fragments of W_g (forward) and of
 *                          W_g^T (input gradient); rg_group_wfrag_elems(...) bf16 elements per group.
 * rg_wide_head_mean      : wbar [n_groups, in], bbar [n_groups] = mean over each group's rows of w and b — the
 *                          per-action mean over quantiles is the linear layer (wbar, bbar) (fp32, row order).
 * rg_qr_select_action    : key[b] = arg max_a (q[b,a] - 1e9 (1 - mask[b,a])) (maxq != 0, :210-214) or the position of
 *                          the 1 in mask[b,:] (SARSA, mask = next_action), num_actions for an all-zero row.
 * rg_qr_compact_head     : quantile-Huber loss (:143-160, :217-218) of z [grouped rows] against
 *                          T = reward (+ boost of action row_key[rowmap[r]], ABI 9) + gamma^e * not_terminal * zt[rowmap[r], :];
 *                          dz [padded_rows, lddz] (padding rows and columns zero), loss_partials [padded_rows];
 *                          tile_losses (nullable) [padded_rows / 128] = their sums per 128-row tile.  num_atoms <= 256.
 *                          O(N log N) per row (sorted targets + prefix sums), not the N x N pair loop.
 * rg_group_head_wgrad    : dw [n_groups * group_rows, in] = per group dz^T h over the group's rows. */
/* rg_group_rows: the grouped space of `key` [batch] int32 in [0, n_groups] (n_groups = "no group": dropped) — a
 * stable counting sort (rows keep batch order inside a group).  dense != 0 (ABI 9): the groups follow each other without
 * padding, n_tiles >= ceil(batch / 128); dense == 0: every group starts on a tile, n_tiles >= ceil(batch / 128) + n_groups. */
size_t rg_group_rows_workspace_bytes(int batch, int n_groups);
int rg_group_rows(const int32_t* key, int batch, int n_groups, int n_tiles, int dense, int32_t* rowmap, int32_t* tile_key,
                  int32_t* row_begin, void* workspace, size_t workspace_bytes, rg_stream_t stream);
size_t rg_group_wfrag_elems(int group_rows, int in_features, int transposed);
/* ABI 8: x3 != 0 = split-bf16 — a group's fragment set is [hi plane | lo plane] (lo = bf16(w - hi)), 2 *
 * rg_group_wfrag_elems(...) elements per group; rg_mlp_desc.group_stride_* then counts both planes. */
int rg_group_weights_stage(const float* w, int n_groups, int group_rows, int in_features, int x3, void* wfrag_fwd,
                           void* wfrag_bwd, rg_stream_t stream);
int rg_wide_head_mean(const float* w, const float* b, int n_groups, int group_rows, int in_features, float* wbar,
                      float* bbar, rg_stream_t stream);
/* ABI 7: the same, and the means also written as the forward B fragments of the [n_groups, in] mean layer (the slots
 * rg_stage_weights_frag(wbar, n_groups, in, wfrag_fwd, NULL) fills for rows < n_groups; wfrag_fwd staged once before) */
/* ABI 8: x3 != 0 also writes the lo plane (rg_wfrag_elems(n_groups, in) elements behind the hi plane) */
int rg_wide_head_mean_staged(const float* w, const float* b, int n_groups, int group_rows, int in_features, float* wbar,
                             float* bbar, void* wfrag_fwd, int x3, rg_stream_t stream);
int rg_qr_select_action(const float* q, int64_t ldq, const float* mask, int batch, int num_actions, int maxq,
                        int32_t* key, rg_stream_t stream);
/* ABI 7: rg_qr_select_action + rg_group_rows(key, n_groups = num_actions) in the launches of the latter (the key is
 * evaluated by the counting launch and written to `key`): two launches instead of four for the grouped space of a*
 * (qrdqn_trainer.py:210-214) or of the logged action */
int rg_qr_select_group_rows(const float* q, int64_t ldq, const float* mask, int batch, int num_actions, int maxq,
                            int32_t* key, int n_tiles, int dense, int32_t* rowmap, int32_t* tile_key, int32_t* row_begin,
                            void* workspace, size_t workspace_bytes, rg_stream_t stream);
int rg_qr_compact_head(const float* z, int64_t ldz, const float* zt, int64_t ldzt, const int32_t* rowmap,
                       const int32_t* row_key, int padded_rows, const float* reward, const float* reward_boosts,
                       const float* not_terminal, double gamma, const float* gamma_exponent,
                       const float* quantiles, int batch, int num_atoms, float* dz, int64_t lddz,
                       float* loss_partials, float* tile_losses, rg_stream_t stream);
size_t rg_group_head_wgrad_workspace_bytes(int n_groups, int group_rows, int in_features, int splits);
/* ABI 8: x3 != 0 = split-bf16 operands, each [hi plane | lo plane] over `rows` (the grouped space's row count: the lo
 * planes start rg_frag_elems(rows + 32 * n_groups, group_rows) / rg_frag_elems(rows, in_features) elements in), three MFMAs
 * per product.  ABI 9: group g reads the blocks [row_begin[g] / 32, ceil(row_begin[g + 1] / 32)) of h_frag and the same
 * blocks + g of dz_frag (rg_mlp_desc: how the backward launch writes them) */
int rg_group_head_wgrad(const void* dz_frag, const void* h_frag, const int32_t* row_begin, int n_groups,
                        int group_rows, int in_features, int splits, int x3, int rows, float* dw, void* workspace,
                        size_t workspace_bytes, rg_stream_t stream);

/* Discrete CRR heads, reagent/training/discrete_crr_trainer.py.  All matrices [B, A] fp32 contiguous.
 * rg_crr_critic_head = compute_target_q_values (:191-206) + compute_td_loss (:208-212) for one or two
 * critics: target = reward (+ sum_a action * reward_boosts) + gamma * not_terminal * min_k sum_a
 * Qk_target(s', a) * softmax(next_logits)_a ; loss_k = mean((sum_a Qk(s, a) * action - target)^2).
 * q2 / q2_next_target / dq2 / partials2 are all NULL for a single critic.  target_out [B] nullable.
 * partials*: rg_crr_partials(B) floats whose sum / B is the loss.
 * rg_crr_actor_head = compute_actor_loss (:214-285): q = q1_network(state) AFTER its optimizer step,
 * logits = actor scores, logged_prob [B] = extras.action_probability (read only if entropy_coeff > 0).
 * dlogits = d actor_loss / d logits; plain_partials sum / B = actor_loss_without_reg;
 * entropy_partials sum / B = the entropy term (actor_loss = plain + entropy_coeff * entropy). */
int rg_crr_partials(int batch);
int rg_crr_critic_head(const float* q1, const float* q2, const float* q1_next_target, const float* q2_next_target,
                       const float* next_logits, const float* action, const float* reward,
                       const float* reward_boosts, const float* not_terminal, double gamma, int batch,
                       int num_actions, float* target_out, float* dq1, float* dq2, float* partials1,
                       float* partials2, rg_stream_t stream);
int rg_crr_actor_head(const float* q, const float* logits, const float* action, const float* logged_prob,
                      double beta, double max_weight, double entropy_coeff, double clip_limit, int batch,
                      int num_actions, float* dlogits, float* plain_partials, float* entropy_partials,
                      rg_stream_t stream);

/* QR-DQN head, reagent/training/qrdqn_trainer.py:108-160 (+ argmax_with_mask :210-214, huber
 * :217-218, quantiles :70-73).  q / qn_online / qn_target [B, A*N] fp32 = network outputs viewed
 * (B, A, N); qn_online NULL = select the next action with the target net (double_q off).
 * next_mask [B, A] = possible_next_actions_mask (maxq != 0) or next_action (SARSA).
 * Outputs: dq [B, A*N] = d loss / d q; loss_partials [B] whose sum is the loss; all_q [B, A]
 * (nullable) = mean over atoms of q (the trainer's logged `all_q_values`).  The (N, B, N) pair
 * tensor of the reference is never materialised.  Limits: N <= 1024, A <= 256. */
int rg_qr_head(const float* q, const float* qn_online, const float* qn_target, const float* action,
               const float* next_mask, const float* reward, const float* reward_boosts,
               const float* not_terminal, double gamma, const float* gamma_exponent,
               const float* quantiles, int batch, int num_actions, int num_atoms, int maxq, float* dq,
               float* loss_partials, float* all_q, rg_stream_t stream);

/* ---- SAC: Gaussian policy head and loss heads ---------------------------------------------- */

/* GaussianFullyConnectedActor.forward, reagent/models/actor.py:215-231 (+ get_log_prob :233-261),
 * given the FC output loc_scale [B, 2A] (ldls) and the N(0,1) draw `noise` [B, A] the reference
 * takes from torch.randn_like (:217): action [B, A] (lda) = clamp(tanh(loc + noise*exp(scale_log))),
 * log_prob [B] (nullable), squashed_mean [B, A] (nullable). */
int rg_gaussian_head_forward(const float* loc_scale, int64_t ldls, const float* noise, int batch,
                             int action_dim, float* action, int64_t lda, float* log_prob,
                             float* squashed_mean, rg_stream_t stream);
/* get_log_prob(state, squashed_action) for a given action, actor.py:233-261. */
int rg_gaussian_log_prob(const float* loc_scale, int64_t ldls, const float* action, int64_t lda,
                         int batch, int action_dim, float* log_prob, rg_stream_t stream);
/* Backward of rg_gaussian_head_forward: g_action [B, A] (nullable) and g_log_prob [B] (nullable) are
 * d loss / d action and d loss / d log_prob; d_loc_scale [B, 2A] = d loss / d loc_scale. */
int rg_gaussian_head_backward(const float* loc_scale, int64_t ldls, const float* noise,
                              const float* g_action, int64_t ldga, const float* g_log_prob, int batch,
                              int action_dim, float* d_loc_scale, int64_t lddls, rg_stream_t stream);
/* Same with the action-embedding KLD term's gradient (sac_trainer.py:282-306) folded in: kld_coef (nullable) [2A] =
 * (c0, c1) from rg_sac_kld; the term's gradient c0_d + c1_d x reaches the action (kld_on_mean == 0) or, through
 * the squashed mean x = clamp(tanh(loc)), loc alone (kld_on_mean != 0). */
int rg_gaussian_head_backward_kld(const float* loc_scale, int64_t ldls, const float* noise, const float* g_action,
                                  int64_t ldga, const float* g_log_prob, int batch, int action_dim,
                                  float* d_loc_scale, int64_t lddls, const float* kld_coef, int kld_on_mean,
                                  rg_stream_t stream);
/* The KLD term itself, sac_trainer.py:282-306: per action dimension d, m = mean over the batch of x[:, d] and v its
 * unbiased variance (x = the sampled action, or with squash != 0 clamp(tanh(x)) of the actor's loc output: the
 * squashed mean); kld = 0.5 * sum_d ((v + (m - emb_mean)^2) / emb_var - 1 + log emb_var - log v).
 * Writes coef [2A] (the gradient coefficients above, `weight` folded in), kld_terms [A] (scratch: per-dimension
 * terms), kld [1] (nullable) and adds weight * kld to loss_inout [1] (nullable: the actor loss mean). */
int rg_sac_kld(const float* x, int64_t ldx, int squash, int batch, int action_dim, const float* emb_mean,
               const float* emb_var, double weight, float* coef, float* kld_terms, float* kld, float* loss_inout,
               rg_stream_t stream);

/* Critic segment of SACTrainer.train_step_gen, reagent/training/sac_trainer.py:217-248:
 * y = r + gamma * (min(q1_t, q2_t) - alpha * clamp(log_prob', -2, 2)) * not_done (y = r if gamma == 0);
 * loss_i = mse(q_i, y), dq_i = d loss_i / d q_i.  All per-transition arrays are [B] fp32; alpha is a
 * device fp64 scalar; q2* may be NULL (single critic).  *_partials: [rg_sac_partials(B)]. */
int rg_sac_partials(int batch);
int rg_sac_critic_head(const float* q1, const float* q2, const float* q1_target, const float* q2_target,
                       const float* log_prob_next, const float* reward, const float* not_terminal,
                       double gamma, const double* alpha, int batch, float* target, float* dq1,
                       float* dq2, float* loss1_partials, float* loss2_partials, rg_stream_t stream);
/* Actor segment, sac_trainer.py:254-280: loss = mean(alpha*clamp(log_prob,-2,2) - min(q1a, q2a));
 * outputs d loss / d log_prob, d loss / d q1a, d loss / d q2a, loss partials and partial sums of
 * (clamp(log_prob) + target_entropy) for the temperature segment (:311-320). */
int rg_sac_actor_head(const float* log_prob, const float* q1_actor, const float* q2_actor, const double* alpha,
                      double target_entropy, int batch, const float* v_cur, int crr_mode, double crr_p0,
                      double crr_clamp, int backprop_log_prob, float* g_log_prob, float* dq1_actor,
                      float* dq2_actor, float* loss_partials, float* entropy_partials, rg_stream_t stream);
/* grad[0] = d alpha_loss / d log_alpha = -mean(clamp(log_prob) + target_entropy); alpha_loss
 * (nullable) = -(log_alpha * mean(...)).  fp64 like the reference's log_alpha (:124-126). */
int rg_sac_alpha_grad(const float* entropy_partials, int batch, const double* log_alpha, double* grad,
                      double* alpha_loss, rg_stream_t stream);
/* TD3 target-policy smoothing, reagent/training/td3_trainer.py:141-146:
 * out[b, :A] (row pitch ld_out) = clamp(next_actor[b] + clamp(noise[b] * noise_variance, noise_clip_lo,
 * noise_clip_hi), lo, hi)   (the reference's `noise.clamp(*self.noise_clip_range)`);
 * noise [B, A] contiguous ~ N(0, 1). */
int rg_td3_target_action(const float* next_actor, int64_t ld_a, const float* noise, double noise_variance,
                         double noise_clip_lo, double noise_clip_hi, double lo, double hi, float* out,
                         int64_t ld_out, int batch, int action_dim, rg_stream_t stream);

/* torch.optim.Adam arithmetic in fp64; exp_param_out (nullable) = exp(param) (alpha = exp(log_alpha)). */
int rg_adam_step_f64(double* param, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t n,
                     double lr, double beta1, double beta2, double eps, double bias_correction1,
                     double bias_correction2_sqrt, double* exp_param_out, rg_stream_t stream);
/* out[b, c] = a[b, c] + b[b, c] (b nullable) on strided [batch, cols] views (sums the two critics'
 * action-input gradients). */
int rg_add_cols(const float* a, int64_t lda, const float* b, int64_t ldb, int batch, int cols,
                float* out, int64_t ldo, rg_stream_t stream);

/* out[0] = scale * sum_i in[i], summed in index order by one workgroup (deterministic). */
int rg_reduce_sum(const float* in, int n, float scale, float* out, rg_stream_t stream);
/* ABI 12: the same over values that are ordered sums of runs of `run` consecutive inputs (the last run may be short):
 * rg_reduce_sum_runs(wave sums of rg_dqn_online_pair_forward, n, 16, ..) == rg_reduce_sum(rg_dqn_head's partials, ..). */
int rg_reduce_sum_runs(const float* in, int n, int run, float scale, float* out, rg_stream_t stream);

/* ---- optimizer ---------------------------------------------------------------------------- */

/* torch.optim.Adam single-tensor step (torch/optim/adam.py _single_tensor_adam, the arithmetic
 * behind reagent/optimizer/uninferrable_optimizers.py:23-33) over one flat fp32 slab.
 * bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t) are computed by the
 * caller in double like the reference does.  grad_scale multiplies g first (1/world for DP). */
int rg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 double lr, double beta1, double beta2, double eps, double weight_decay,
                 double bias_correction1, double bias_correction2_sqrt, double grad_scale,
                 rg_stream_t stream);

/* Graph-safe Adam steps.  A captured HIP graph bakes launch ARGUMENTS in, and bias_correction1/2 change every
 * step: the `_sched` variants read them (and lr) from a device-resident schedule instead, so one captured
 * step replays as step t, t+1, ...  Layout of `sched` (doubles, written by the host):
 *   [0] steps applied so far   [1] lr   [2] n = table entries   [3] reserved
 *   [4 + 2(t-1)], [5 + 2(t-1)] = 1 - beta1^t, sqrt(1 - beta2^t) for t = 1..n (steps past n use entry n; the
 *   host extends the table until both have reached 1.0), computed in double as for the scalar entry points.
 * A launch applies step [0] + 1; rg_sched_tick (one thread: [0] += 1) is enqueued after the last launch of
 * that step.  Arithmetic per element is that of rg_adam_step / rg_mlp_update_fused / rg_adam_step_f64 with the
 * same coefficients: identical bits. */
int rg_adam_step_sched(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       double beta1, double beta2, double eps, double weight_decay, double grad_scale,
                       const double* sched, rg_stream_t stream);
int rg_mlp_update_fused_sched(const rg_mlp_update_desc* d, double beta1, double beta2, double eps,
                              double weight_decay, double grad_scale, double tau, const double* sched,
                              rg_stream_t stream);
int rg_adam_step_f64_sched(double* param, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t n,
                           double beta1, double beta2, double eps, const double* sched,
                           double* exp_param_out, rg_stream_t stream);
int rg_sched_tick(double* sched, rg_stream_t stream);
/* ABI 11: the ticks of up to RG_MAX_TICKS DISTINCT schedules in one launch (a SAC step updates four optimizers — three networks and
 * the temperature — each with its own schedule: one launch at the end of the step instead of four between its segments).
 * `scheds` is a host array of n device pointers. */
#define RG_MAX_TICKS 8
int rg_sched_tick_many(double* const* scheds, int n, rg_stream_t stream);

/* SoftUpdate.step, reagent/optimizer/soft_update.py:60-70: tgt = tau*src + (1-tau)*tgt */
int rg_soft_update(float* target, const float* source, int64_t n, double tau, rg_stream_t stream);

/* World model: MDN-RNN (reagent/models/mdn_rnn.py, reagent/training/world_model/mdnrnn_trainer.py).  Additive symbols: the
 * ABI number does not move.  All fp32 (RG_PREC_F32 throughout), every array contiguous unless a pitch is named.
 *
 * rg_lstm_forward: one layer of nn.LSTM(num_layers = L), sequence first, unidirectional, gate order i, f, g, o
 * (mdn_rnn.py:32-36, :72), all seq_len steps in one launch.  xproj [T, B, 4H] = x * W_ih^T + b_ih for all steps at once
 * (rg_fc_forward over T * B rows, RG_ACT_LINEAR); w_hh [4H, H]; b_hh [4H] or NULL; h0, c0 [B, H] or NULL (zeros).
 *   pre = xproj[t] + b_hh + h_{t-1} * w_hh^T;  i, f, o = sigmoid, g = tanh;  c_t = f * c_{t-1} + i * g;  h_t = o * tanh(c_t)
 * Outputs: h_all, c_all [T, B, H]; gates [T, B, 4H] after their non-linearities, or NULL for a forward that saves nothing
 * for a backward (same h_all bits).  A workgroup owns 32 batch rows for the whole sequence (h_{t-1} in LDS, two images);
 * its four waves own the hidden units in tiles of 32, each holding the four gates' accumulators of its units.  The product
 * is a k-ordered fp32 fma chain over H (v_mfma_f32_32x32x2_f32, zero-padded to a multiple of 32); the gate arithmetic runs
 * in double on it and is rounded once per stored value; tanh(c_t) is taken of the stored fp32 c_t.  A row's bits depend on
 * that row alone, trip counts on H alone; no atomics.
 *
 * rg_lstm_backward: the same layer in reverse (autograd's backward of the lines above).  dh_all [T, B, H] = the gradient
 * arriving from above at every step (the gradient with respect to the final h_n, where there is one, added into its last
 * step by the caller); gates, c_all, c0, w_hh as the forward had them.  Outputs: dgates [T, B, 4H] = d loss / d pre; dh0,
 * dc0 [B, H] (nullable).  The weight, bias and input gradients are the caller's: dW_ih = dgates^T * x and db_ih = db_hh =
 * the column sums (rg_fc_wgrad over T * B rows), dW_hh = dgates[1:]^T * h_all[:-1] (plus dgates[0]^T * h0), dx = dgates *
 * W_ih (rg_fc_dgrad).  Per step: the element-wise part in double, then dh_rec = dgates[t] * w_hh on the fp32 MFMA, K = 4H,
 * staged through LDS one gate at a time.
 *
 * Both: RG_EINVAL for seq_len, batch or hidden < 1 or a null pointer not marked nullable; RG_EUNSUPPORTED for hidden >
 * RG_LSTM_MAX_HIDDEN or seq_len * batch >= 2^29. */
#define RG_LSTM_MAX_HIDDEN 256
#define RG_LSTM_MAX_LAYERS 4 /* the host's limit on num_hidden_layers (a launch is one layer) */
int rg_lstm_forward(const float* xproj, const float* w_hh, const float* b_hh, const float* h0, const float* c0, int seq_len,
                    int batch, int hidden, float* h_all, float* c_all, float* gates, rg_stream_t stream);
int rg_lstm_backward(const float* dh_all, const float* gates, const float* c_all, const float* c0, const float* w_hh,
                     int seq_len, int batch, int hidden, float* dgates, float* dh0, float* dc0, rg_stream_t stream);

/* rg_mdn_head: the mixture-density head over n = T * B rows.  z [n, (2S + 1) G + 2] (pitch ldz) = gmm_linear's output:
 * mus [G, S], log sigmas [G, S], mixture logits [G], reward, not_terminal logit (mdn_rnn.py:75-92).  next_state [n, S],
 * reward [n], not_terminal [n].  With rows = n - first_row (fit_only_one_next_step passes (T - 1) * B: the last step):
 *   gmm = next_state_loss_weight * mean over the rows of -log sum_g pi_g N(next_state | mu_g, sigma_g)  (gmm_loss, :188-233)
 *   bce = not_terminal_loss_weight * mean binary_cross_entropy_with_logits(z[-1], not_terminal)
 *   mse = reward_loss_weight * mean (z[-2] - reward)^2
 *   loss = gmm / (S + 2) + bce + mse with divide_by_state_dim, gmm + bce + mse without  (mdnrnn_trainer.py:164-177)
 * Outputs: losses [4] = gmm, bce, mse, loss; dz [n, .] (pitch lddz) = d loss / d z, rows before first_row exactly zero;
 * sigmas [n, G, S] = exp(log sigma) and logpi [n, G] = log_softmax(logits) for all n rows (each nullable).  partials:
 * 3 * rg_mdn_head_partials(n) doubles of scratch.  One wave per row; a row's arithmetic is double on the fp32 inputs,
 * rounded once where it is stored; the three sums leave as per-workgroup partials in double and a finishing launch adds
 * them in a fixed order and rounds once.  No atomics: two runs give the same bits.
 * rg_mdn_outputs: the same sigmas and logpi (bit for bit) without targets: what MDNRNN.forward returns.
 * rg_mdn_gmm_nll: gmm_loss(batch, mus, sigmas, logpi, reduce = False) on its own arguments as they are (sigmas, not their
 * logarithms; logpi not normalised again): nll [n] = -log_prob.
 * All: RG_EINVAL for n, G or S < 1, a null pointer not marked nullable, a pitch below the row, first_row outside [0, n);
 * RG_EUNSUPPORTED for G > RG_MDN_MAX_GAUSSIANS or S > RG_MDN_MAX_STATE_DIM. */
#define RG_MDN_MAX_GAUSSIANS 32
#define RG_MDN_MAX_STATE_DIM 512
int rg_mdn_head_partials(int n);
int rg_mdn_head(const float* z, int64_t ldz, const float* next_state, const float* reward, const float* not_terminal,
                double next_state_loss_weight, double not_terminal_loss_weight, double reward_loss_weight,
                int divide_by_state_dim, int first_row, int n, int num_gaussians, int state_dim, float* dz, int64_t lddz,
                float* sigmas, float* logpi, double* partials, float* losses, rg_stream_t stream);
int rg_mdn_outputs(const float* z, int64_t ldz, int n, int num_gaussians, int state_dim, float* sigmas, float* logpi,
                   rg_stream_t stream);
int rg_mdn_gmm_nll(const float* batch, const float* mus, const float* sigmas, const float* logpi, int n, int num_gaussians,
                   int state_dim, float* nll, rg_stream_t stream);

/* World model: Seq2Reward (reagent/models/seq2reward_model.py, reagent/training/world_model/seq2reward_trainer.py,
 * compress_model_trainer.py).  Additive symbols: the ABI number does not move.  All fp32, every array contiguous.
 *
 * rg_lstm_fanout_step: one LSTM layer, ONE time step, over n = parents * fanout child rows of a prefix tree: the planning
 * step get_Q (seq2reward_trainer.py:31-64) without the enumeration's repeated prefixes.  Child r takes h_prev and c_prev
 * [parents, H] (c_prev NULL: zeros) from row r / fanout, and its input projection x * W_ih^T + b_ih from row r % table_rows
 * of proj [table_rows, 4H] when table_rows > 0 (layer 0: the projection of a one-hot action is a row of the projected
 * identity, and with table_rows = fanout = A child r's action is r % A), or from row r of proj [n, 4H] when table_rows = 0
 * (upper layers: rg_fc_forward on the layer below's child h).  Writes h, c [n, H].  The tile shape and arithmetic are
 * rg_lstm_forward's (32 rows per workgroup, the k-ordered v_mfma_f32_32x32x2_f32 chain over H, gates in double, rounded
 * once): a child's bits are those of rg_lstm_forward with seq_len = 1 on the materialised h0 / c0 / xproj rows.
 * RG_EINVAL for parents, fanout or hidden < 1, table_rows < 0 or a null pointer other than c_prev and b_hh;
 * RG_EUNSUPPORTED for hidden > RG_LSTM_MAX_HIDDEN or n >= 2^29.
 *
 * rg_seq2reward_plan_max: acc[r] = h[r] . w + bias[0] over the leaf rows h [groups * group_size, H] (lstm_linear,
 * seq2reward_model.py:63: accumulated in double in index order, rounded once), q[g] = the max over group g's group_size
 * consecutive leaves (seq2reward_trainer.py:60-62 with groups = B * A and group_size = P / A: the leaves of one first
 * action).  A NaN among a group's leaves gives NaN, as torch.max does.  One wave per group, any group_size.
 * RG_EINVAL for groups, group_size or hidden < 1 or a null pointer; RG_EUNSUPPORTED for groups * group_size >= 2^29.
 *
 * rg_seq2reward_head: the training head over B rows (seq2reward_model.py:62-68, seq2reward_trainer.py:216-245).  h_all
 * [T, B, H] = the top layer's hidden states; valid_step [B] int64, CLAMPED into [1, T] inside the kernel (the reference
 * indexes with it as it is and faults outside that range); reward [T, B]; gamma_pow [T] = fp32(gamma ** i).
 *   pred[b] = h_all[v - 1, b] . w + bias[0]                              (double in index order, rounded once: acc_reward [B])
 *   target[b] = sum_{i < v} reward[i, b] * gamma_pow[i]                  (an fp32 product, then a sequential fp32 sum)
 *   loss = mean_b (pred - target)^2
 * Outputs: acc_reward [B]; dh_all [T, B, H] = d loss / d h_all, written entirely (zero except at step v - 1 of each row);
 * dw [H], dbias [1], loss [1] from per-workgroup double partials (partials: (H + 2) * rg_seq2reward_head_partials(B)
 * doubles) added in a fixed order by a finishing launch.  With valid_step NULL: the last step of every row.  With dh_all
 * NULL: acc_reward alone, the forward of Seq2RewardNetwork (reward, gamma_pow, dw, dbias, partials and loss are not read or
 * written and may be NULL).
 * RG_EINVAL for seq_len, batch or hidden < 1 or a null pointer the mode needs; RG_EUNSUPPORTED for seq_len * batch >= 2^29.
 *
 * rg_step_ce_head: nn.CrossEntropyLoss(mean) of logits [B, K] against valid_step - 1 (seq2reward_trainer.py:261-267), the
 * step clamped into [1, K]: loss [1], dlogits [B, K] = (softmax - onehot) / B, and (nullable) softmax [B, K]
 * (get_step_prediction, :21-27).  With valid_step NULL: the softmax alone.  A 32-lane group per row, in double, rounded once;
 * partials: rg_step_ce_head_partials(B) doubles, added in a fixed order by a finishing launch.
 * RG_EINVAL for batch or classes < 1 or a null pointer the mode needs; RG_EUNSUPPORTED for classes > RG_STEP_CE_MAX_CLASSES.
 * No atomics anywhere: two runs give the same bits. */
#define RG_STEP_CE_MAX_CLASSES 32
int rg_lstm_fanout_step(const float* h_prev, const float* c_prev, const float* proj, int table_rows, const float* w_hh,
                        const float* b_hh, int parents, int fanout, int hidden, float* h, float* c, rg_stream_t stream);
int rg_seq2reward_plan_max(const float* h, const float* w, const float* bias, int groups, int group_size, int hidden, float* q,
                           rg_stream_t stream);
int rg_seq2reward_head_partials(int batch);
int rg_seq2reward_head(const float* h_all, const int64_t* valid_step, const float* reward, const float* gamma_pow,
                       const float* w, const float* bias, int seq_len, int batch, int hidden, float* acc_reward, float* dh_all,
                       float* dw, float* dbias, double* partials, float* loss, rg_stream_t stream);
int rg_step_ce_head_partials(int batch);
int rg_step_ce_head(const float* logits, const int64_t* valid_step, int batch, int classes, float* dlogits, float* softmax,
                    double* partials, float* loss, rg_stream_t stream);

/* World model: the cross-entropy-method planner (reagent/models/cem_planner.py).  Additive symbols: the ABI number does not
 * move.  Everything is on the caller's stream; no atomics, no flag a workgroup waits on: two runs give the same bits.
 *
 * The planner state `planner_state` is 2 D + 2 doubles on the device: mean [D], var [D], done (0 or 1), iterations run.
 * Every entry point that takes it (or `done`, a pointer to its done slot, nullable) returns at once, writing nothing, when
 * done is set: the host enqueues all cem_num_iterations iterations and reads back once (cem_planner.py:233-256's `break`
 * becomes "later iterations do nothing").
 *
 * NOISE.  A draw is Philox4x32-10 (rg_philox.h) with key = seed, counter words (c0, c1) = the low and high half of
 *   n | iteration << 20 | kind << 52      (n < 2^20: the trajectory solution * E + member, or the solution for kinds 4, 5)
 * and (c2, c3) = (lo, hi), four 32-bit outputs x0 .. x3:
 *   kind 0  u_model[n]        (hi, lo) = (0, 0)            kind 3  eps[step, n, s]     (hi, lo) = (step, s)
 *   kind 1  u_mix[step, n]    (hi, lo) = (step, 0)         kind 4  tn[solution, d]     (hi, lo) = (d, attempt)
 *   kind 2  u_term[step, n]   (hi, lo) = (step, 0)         kind 5  action[solution, step]  (hi, lo) = (step, 0)
 * A uniform is fp32 (x0 >> 8) * 2^-24, in [0, 1).  A standard normal is Box-Muller in double,
 * sqrt(-2 ln((x0 + 1) 2^-32)) cos(2 pi x1 2^-32), rounded once to fp32 for eps and kept in double for tn.  An integer draw
 * is floor(u * count) in double.  tn is a standard normal truncated to [-2, 2] by rejection: attempt t = 0 .. 31 of an
 * element, the first inside is taken; after 32 the last is clamped.  rg_cem_fill_noise writes u_model [N], u_mix [T, N],
 * eps [T, N, S], u_term [T, N] exactly as rg_cem_group and rg_cem_rollout would draw them in place (their noise arguments
 * NULL); with the buffers passed the results have the same bits.
 *
 * rg_cem_group: each trajectory's world model floor(u_model[n] * models) (cem_planner.py:137), then a counting sort by one
 * workgroup: rowmap [tiles * 32] lists, per tile of 32 rows, trajectories of ONE model in index order (-1: padding),
 * tile_model [tiles] that model (-1: an unused tile); tiles = rg_cem_rollout_tiles(N, models) = N / 32 + models.  A model
 * that draws no trajectory gets no tile.
 *
 * rg_cem_rollout: acc_rewards_of_all_solutions (:121-190) of population solutions x ensemble trajectories in one launch, a
 * workgroup per tile for all `horizon` steps.  table [models][3 layers + 2] holds device pointers to each member's
 * rnn.weight_ih_l*, bias_ih_l*, bias_hh_l* and gmm_linear's weight and bias, read in place.  Per step x = cat([action_j,
 * state]) (actions first, MDNRNN's order); the action is row j of solutions [P, horizon, A] fp32, or the one-hot of
 * action_idx [P, horizon] (exactly one of the two is given).
 * KEPT QUIRK: h and c are ZERO at every planning step (the reference passes no hidden state to mem_net, :197), so W_hh and
 * the forget gate contribute nothing: pre = x W_ih^T + b_ih + b_hh, c = i * g, h = o * tanh(c), per layer; the products are
 * k-ordered fp32 chains on v_mfma_f32_32x32x2_f32, the gate arithmetic is rg_lstm_forward's (double, rounded once).
 * z = gmm_linear(h).  The mixture index is the inverse CDF over softmax(z[2GS .. 2GS + G)) in index order against u_mix
 * (the count of cumulative sums <= u, at most G - 1); next_state = fp32(mu_k + exp(z_sigma_k) * eps), in double, rounded once;
 * not_terminal = (u_term < sigmoid(z[-1])) when terminal_effective, else 1.  The reward z[-2] of step j enters as the fp32
 * product z[-2] * gamma_pow[j] (gamma_pow [horizon] = fp32(gamma ** j) from the host), summed in double in step order; the
 * step at which a terminal is sampled counts, nothing after it does.  A stopped trajectory stays in its tile's barriers
 * and products, masked.  out [population]: the trajectory's sum for ensemble == 1; for ensemble > 1 the mean over the
 * solution's trajectories in double in index order (traj [N] is then the per-trajectory workspace).  DEPARTURE: the
 * reference assigns the length-E array to a scalar slot (:186) and raises for E > 1.
 * trace (nullable; for tests) [T, N, S + W + 2] with W = (2S + 1)G + 2 holds per step and trajectory the state it entered
 * with, its z row, the sampled index and not_terminal (as floats).  When NULL the launch writes out (and traj) alone.
 * RG_EUNSUPPORTED for hidden > RG_LSTM_MAX_HIDDEN, layers > RG_LSTM_MAX_LAYERS, num_gaussians > RG_MDN_MAX_GAUSSIANS,
 * state_dim + action_dim > RG_CEM_MAX_INPUT, models > RG_CEM_MAX_MODELS, horizon > RG_CEM_MAX_HORIZON or
 * population * ensemble >= RG_CEM_MAX_TRAJECTORIES.  rg_cem_rollout_lds_bytes is the launch's dynamic LDS request.
 *
 * rg_cem_sample: solutions [P, D] = tn * sqrt(constrained_variance(mean, var)) + mean in double (:217-222, :235-242; lower
 * and upper are the bounds tiled to D), and their fp32 copy (:243-247).  tn [P, D] (nullable) replaces the draw.
 * rg_cem_sample_discrete: actions [P, horizon] = floor(u * A): random.choices over the enumerated product (:275-278)
 * without the enumeration.
 *
 * rg_cem_refit (:249-255), one workgroup: the elites are the last num_elites entries of np.argsort(rewards) (a NaN ranks
 * above every number; of equal rewards the higher index ranks higher); per dimension their mean and population variance
 * in double in solution-index order; mean = alpha mean + (1 - alpha) new_mean, the same for var; iterations run += 1; done
 * is set when max(var) <= epsilon.  flags [P] is workspace (1: an elite).  RG_EINVAL for num_elites outside [1, P].
 *
 * rg_cem_tally (:287-296): out [3 A + 1] = per first action actions[p, 0] the count, the sum of rewards in index order and
 * their quotient (0 / 0 = NaN: never drawn), then np.nanargmax of the quotients (-1: every quotient is NaN). */
#define RG_CEM_MAX_MODELS 16
#define RG_CEM_MAX_HORIZON 64
#define RG_CEM_MAX_INPUT 512
#define RG_CEM_MAX_TRAJECTORIES (1 << 20)
int rg_cem_fill_noise(uint64_t seed, int iteration, int trajectories, int horizon, int state_dim, float* u_model, float* u_mix,
                      float* eps, float* u_term, rg_stream_t stream);
int rg_cem_rollout_tiles(int trajectories, int models);
int rg_cem_group(const float* u_model, uint64_t seed, int iteration, int trajectories, int models, const double* done,
                 int* rowmap, int* tile_model, rg_stream_t stream);
size_t rg_cem_rollout_lds_bytes(int state_dim, int action_dim, int hidden);
int rg_cem_rollout(const float* const* table, int models, const int* rowmap, const int* tile_model, int tiles,
                   const float* init_state, const float* solutions, const int* action_idx, const float* gamma_pow,
                   const float* u_mix, const float* eps, const float* u_term, uint64_t seed, int iteration, const double* done,
                   int population, int ensemble, int horizon, int state_dim, int action_dim, int num_gaussians, int hidden,
                   int layers, int terminal_effective, double* traj, double* out, float* trace, rg_stream_t stream);
int rg_cem_sample(const double* planner_state, const double* lower, const double* upper, const double* tn, uint64_t seed,
                  int iteration, int population, int dims, double* solutions, float* solutions_f32, rg_stream_t stream);
int rg_cem_sample_discrete(uint64_t seed, int iteration, int population, int horizon, int action_dim, int* actions,
                           rg_stream_t stream);
int rg_cem_refit(const double* rewards, const double* solutions, int population, int dims, int num_elites, double alpha,
                 double epsilon, double* planner_state, int* flags, rg_stream_t stream);
int rg_cem_tally(const int* actions, int horizon, const double* rewards, int population, int action_dim, double* out,
                 rg_stream_t stream);

/* Synthetic reward (reagent/models/synthetic_reward.py, reagent/training/reward_network_trainer.py).  Additive symbols: the
 * ABI number does not move.  All fp32 unless said, on the caller's stream; no atomics, no flag a workgroup waits on: two runs
 * give the same bits.
 *
 * rg_ngram_concat: ngram() over cat(state, action) (synthetic_reward.py:177-205, called at :399-403) in one launch.  state
 * [T, B, S] and action [T, B, A] with row pitches ld_state / ld_action (elements between consecutive (t, b) rows), out
 * [T, B, (S + A) * n] with row pitch ld_out, n = context_size odd.  For window slot i < n:
 *   out[t, b, i * (S + A) + f] = cat(state, action)[t + i - n / 2, b, f]   when that step lies in [0, T), else 0.0f
 * (the reference's ngram_padding is a zero tensor, not a parameter).  A pure copy: the inputs' bits.  n = 1 is the plain
 * cat(state, action).  Total in n: a window wholly outside the sequence is zeros (the reference raises from narrow() when
 * n / 2 > T).  RG_EINVAL for an even or non-positive n, a size below 1, a pitch below its row or a null pointer;
 * RG_EUNSUPPORTED for T * B >= 2^29 or (S + A) * n >= 2^31.
 *
 * rg_step_reward_head: SyntheticRewardNet.forward behind the trunk (synthetic_reward.py:245-266) fused with the nets' last
 * Linear(P, 1) + activation (:301-302, :389-390, :450-452) and _get_loss_function's wrapper
 * (reward_network_trainer.py:27-66).  h [T, B, P] contiguous = the trunk's output, w [P], bias [1], act an RG_ACT_* code;
 * valid_step [B] int64, CLAMPED into [1, T] inside the kernel (the reference's _gen_mask asserts the range on the host,
 * :220-222); target [B]; loss_type an RG_SRW_LOSS_* code.
 *   z[t, b] = h[t, b, :] . w + bias                (double; lanes stride over P, a fixed butterfly adds them)
 *   r[t, b] = act(z);   mask[b, t] = (t >= T - v_b);   pred[b] = sum_t mask * r   (double, in t order, rounded once)
 *   MSE (pred - target)^2; SmoothL1 with beta 1; L1; BCE: pred and target divided by v_b first, both logs clamped at -100 as
 *   nn.BCELoss does, and a pred / v outside [0, 1] gives NaN for that row where torch raises.
 *   kept[b] = !(has_threshold && apply_threshold) || fp32 target (BCE: target / v_b in fp32) <= (float)threshold: the
 *   reference gates the filter on pred.requires_grad, so the caller sets apply_threshold in training and clears it in
 *   validation.  loss = sum of the kept rows' losses / n_kept; with no row kept the loss is NaN and n_kept = 0 (the
 *   reference asserts on the host), dh, dw and dbias zero.
 * Outputs: output [B, T] (r transposed, as the reference returns it), mask [B, T], predicted_reward [B]; with target: loss
 * [1], n_kept [1] int32; with dh: dh [T, B, P] = d loss / d h written entirely (+0 rows where the mask or the filter drops
 * them), dw [P], dbias [1] from per-workgroup double partials added in a fixed order, every output rounded once.  The L1
 * gradient at a zero residual is 0; BCE's is (p - y) / max(p (1 - p), 1e-12) / v, torch's.  target NULL: the three forward
 * outputs alone (loss, n_kept, workspace may be NULL); dh NULL: no gradients (dw, dbias may be NULL).  The forward outputs
 * have the same bits in every mode.  workspace: rg_step_reward_head_partials(B) * (P + 3) + (T + 1) * B doubles.  Three
 * launches at most: the rows, the partials' sum (which makes n_kept), dh.
 * RG_EINVAL for a size below 1, an act or loss_type outside its codes, a null pointer the mode needs; RG_EUNSUPPORTED for
 * T * B >= 2^29. */
enum { RG_SRW_LOSS_MSE = 0, RG_SRW_LOSS_SMOOTH_L1 = 1, RG_SRW_LOSS_L1 = 2, RG_SRW_LOSS_BCE = 3 };
int rg_ngram_concat(const float* state, int64_t ld_state, const float* action, int64_t ld_action, int seq_len, int batch,
                    int state_dim, int action_dim, int context_size, float* out, int64_t ld_out, rg_stream_t stream);
int rg_step_reward_head_partials(int batch);
int rg_step_reward_head(const float* h, const float* w, const float* bias, int act, const int64_t* valid_step,
                        const float* target, int loss_type, int has_threshold, double threshold, int apply_threshold,
                        int seq_len, int batch, int width, float* output, float* mask, float* predicted_reward, float* loss,
                        int32_t* n_kept, float* dh, float* dw, float* dbias, double* workspace, rg_stream_t stream);

/* Counterfactual-evaluation reward models (reagent/training/cfeval/, reagent/models/probabilistic_fully_connected_network.py).
 * Additive symbols: the ABI number does not move.  All fp32 unless said, on the caller's stream; no atomics, no flag a
 * workgroup waits on; per-workgroup partials in double, added in a fixed order by a finishing launch; every output rounded
 * once; two runs give the same bits.
 *
 * The Bayes-by-backprop kernels walk a SEGMENT TABLE: up to RG_BBB_MAX_SEGMENTS flat parameter tensors (a layer's weights and
 * its biases are a segment each, so eight layers), passed by value, so the number of launches does not depend on depth.  A
 * workgroup takes RG_BBB_CHUNK consecutive elements of one segment.
 *
 * rg_bbb_sample: LinearBBB.forward's weight draw and both log-densities (probabilistic_fully_connected_network.py:87-105)
 * for every segment, and log_prior() / log_post() (:175-188) over them.  Per element, in double on the fp32 inputs:
 *   sigma = log(1 + exp(rho))   (as rho + log1p(exp(-rho)) for rho > 0, log1p(exp(rho)) otherwise: finite and positive for
 *                                every rho in [-700, 3e38], where the reference's fp32 form is inf above 88 and 0 below -17)
 *   w     = fp32(mu + sigma * eps)
 *   log_prior += log Normal(0, prior_var).pdf(w)      (the ROUNDED w; prior_var is the prior's SCALE: the reference's quirk)
 *   log_post  += log Normal(mu, sigma).pdf(w)
 * eps: with draw = 0 read from seg.eps (the explicit-noise path); with draw = 1 drawn and written to seg.eps:
 * Philox4x32-10 (rg_philox.h) with key = seed, counter words (c0, c1) = the element's index in its segment (low, high),
 * c2 = the sample index, c3 = the segment's index in the table; the first two output words make u1 = (x0 + 1) / 2^32 in
 * (0, 1] and u2 = x1 / 2^32 in [0, 1), eps = fp32(sqrt(-2 ln u1) cos(2 pi u2)) with the arithmetic in double.
 * rg_bbb_fill_noise writes exactly that eps and nothing else.  Outputs: seg.w, seg.eps (draw), log_prior [1], log_post [1]
 * (fp32, rounded once) and terms[0] = log_prior, terms[1] = log_post as doubles for rg_bbb_elbo_head.  workspace:
 * 2 * rg_bbb_chunks(table) doubles.  Two launches.
 *
 * rg_bbb_elbo_head: sample_elbo's likelihood and loss (:190-213) for one sample.  out [B] (the network's one output column,
 * pitch ld_out), target [B]:
 *   log_like = sum_r log Normal(out_r, noise_tol).pdf(target_r)           (double per row, fixed order)
 *   acc      = (accumulate ? acc : 0) + scale * (log_post - log_prior - log_like, log_prior, log_post, log_like)
 *   result[0 .. 3] = fp32(acc)      (the loss and its three terms; scale = 1 / num_samples, accumulate on every sample but
 *                                    the first: the Monte-Carlo means of :205-210)
 *   dout_r   = scale * (out_r - target_r) / noise_tol^2                   (d loss / d out; may be NULL)
 * terms: rg_bbb_sample's two doubles; acc: 4 doubles the caller keeps between samples; workspace:
 * rg_bbb_elbo_head_partials(B) doubles.  Two launches.
 *
 * rg_bbb_grad: autograd's chain rule back into mu and rho (one launch), after the network's backward left
 * seg.dw = d (-log_like) / d w (times the head's scale).  Per element, in double:
 *   g     = dw + scale * (w / prior_var^2 - (w - mu) / sigma^2)
 *   dmu   = g                       (the posterior's mean is w_mu.data: detached in the reference, :101-102, kept)
 *   drho  = sigmoid(rho) * (g * eps + scale * ((w - mu)^2 / sigma^3 - 1 / sigma))
 * written to seg.dmu / seg.drho, added to them with accumulate (the host loop over num_samples).
 *
 * rg_bandit_reward_head: BanditRewardNetTrainer behind the [B, A] forward (cfeval/bandit_reward_network_trainer.py:57-61,
 * :48-55, :63-75 and the loss wrapper of reward_network_trainer.py:27-66).  q [B, A] (pitch ld_q), action [B, A] (pitch
 * ld_action), reward [B], action_prob [B] or NULL:
 *   idx_r  = argmax(action[r, :]) by torch.argmax's rule: the first maximum, a NaN ranking above everything
 *   pred_r = q[r, idx_r];  l_r = MSE, SmoothL1 (beta 1) or L1 of (pred_r, reward_r)  (RG_SRW_LOSS_* codes; BCE: RG_EINVAL)
 *   weight_r = 1 / action_prob_r (1 without action_prob)
 *   kept_r = !(has_threshold && apply_threshold) || reward_r <= (float)threshold
 *   loss = sum_kept weight_r l_r / n_kept;  unweighted_loss = sum_kept l_r / n_kept;  n_kept int32
 *   dq[r, c] = weight_r * dl_r / n_kept at c = idx_r of a kept row, +0 everywhere else (written whole; may be NULL)
 * With no row kept the losses are NaN, n_kept = 0 and dq zero (rg_step_reward_head's convention).  The L1 gradient at a
 * zero residual is 0.  predicted_reward [B] is always written.  workspace: rg_bandit_reward_head_workspace(B) doubles.  Two
 * launches: the rows, then the partials' sum in every workgroup (the same order: the same bits) and dq.
 *
 * RG_EINVAL for a null pointer a mode needs, a size below 1, more than RG_BBB_MAX_SEGMENTS segments, a non-positive
 * prior_var or noise_tol, a loss code outside MSE / SmoothL1 / L1; RG_EUNSUPPORTED for a segment of 2^31 elements or more. */
#define RG_BBB_MAX_SEGMENTS 16
#define RG_BBB_CHUNK 1024
typedef struct rg_bbb_segment {
  const float* mu;
  const float* rho;
  float* w;        /* the sampled tensor: written by rg_bbb_sample, read by rg_bbb_grad */
  float* eps;      /* the noise: read (draw = 0) or written (draw = 1) by rg_bbb_sample, read by rg_bbb_grad */
  const float* dw; /* rg_bbb_grad: d (-log_like) / d w */
  float* dmu;      /* rg_bbb_grad's outputs */
  float* drho;
  int64_t n;
} rg_bbb_segment;
typedef struct rg_bbb_table {
  int32_t n_segments;
  int32_t reserved;
  rg_bbb_segment seg[RG_BBB_MAX_SEGMENTS];
} rg_bbb_table;
int rg_bbb_chunks(const rg_bbb_table* table);
int rg_bbb_fill_noise(const rg_bbb_table* table, uint64_t seed, int sample, rg_stream_t stream);
int rg_bbb_sample(const rg_bbb_table* table, double prior_var, int draw, uint64_t seed, int sample, float* log_prior,
                  float* log_post, double* terms, double* workspace, rg_stream_t stream);
int rg_bbb_elbo_head_partials(int batch);
int rg_bbb_elbo_head(const float* out, int64_t ld_out, const float* target, int batch, double noise_tol, double scale,
                     int accumulate, const double* terms, double* acc, float* result, float* dout, double* workspace,
                     rg_stream_t stream);
int rg_bbb_grad(const rg_bbb_table* table, double prior_var, double scale, int accumulate, rg_stream_t stream);
int rg_bandit_reward_head_workspace(int batch);
int rg_bandit_reward_head(const float* q, int64_t ld_q, const float* action, int64_t ld_action, const float* reward,
                          const float* action_prob, int loss_type, int has_threshold, double threshold, int apply_threshold,
                          int batch, int num_actions, float* predicted_reward, float* loss, float* unweighted_loss,
                          int32_t* n_kept, float* dq, int64_t ld_dq, double* workspace, rg_stream_t stream);

/* ---- multi-head self-attention over short sequences (attention.hip) ----------------------------------------------------
 * nn.MultiheadAttention's core between its projections, with no mask, as PETransformerEncoderLayer calls it
 * (reagent/models/synthetic_reward.py:160-166).  q, k, v, ctx and the gradients are fp32 [seq_len * batch, embed] views, row
 * t * batch + b, each with its own pitch (q | k and dq | dk may be the halves of one [N, 2 * embed] buffer); head h owns
 * columns h * hd .. (h + 1) * hd, hd = embed / nhead.
 *
 * rg_attn_forward: ctx = softmax(q k^T / sqrt(hd)) v per (b, head); p (nullable) [batch, nhead, seq_len, seq_len] contiguous =
 * the probabilities, which the backward reads.  Dot products and the soft-max (row maximum subtracted) in double on the fp32
 * inputs, p and ctx rounded once; a wave owns a (b, head) pair, nothing is added across waves, no atomics: two runs give the
 * same bits.  rg_attn_backward: dv = p^T dctx, dp = dctx v^T, ds = p * (dp - rowsum(dp * p)), dq = ds k / sqrt(hd),
 * dk = ds^T q / sqrt(hd), every output written entirely and rounded once.
 * RG_EINVAL for embed % nhead != 0, a pitch below embed or a missing pointer; RG_EUNSUPPORTED for seq_len >
 * RG_ATTN_MAX_SEQ_LEN (a score row is one wavefront, a lane per key), embed / nhead > RG_ATTN_MAX_HEAD_DIM, embed >
 * RG_ATTN_MAX_EMBED, seq_len * batch >= 2^29 or batch * nhead >= 2^29. */
#define RG_ATTN_MAX_SEQ_LEN 64
#define RG_ATTN_MAX_HEAD_DIM 128
#define RG_ATTN_MAX_EMBED 512
int rg_attn_forward(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int seq_len, int batch,
                    int embed, int nhead, float* ctx, int64_t ld_ctx, float* p, rg_stream_t stream);
int rg_attn_backward(const float* dctx, int64_t ld_dctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                     int64_t ldv, const float* p, int seq_len, int batch, int embed, int nhead, float* dq, int64_t ld_dq,
                     float* dk, int64_t ld_dk, float* dv, int64_t ld_dv, rg_stream_t stream);
/* out = act((a + b) + pe[row / batch]) on strided fp32 [seq_len * batch, cols] views in one launch: b and pe [>= seq_len,
 * cols] (pitch ld_pe) nullable, act RG_ACT_LINEAR or RG_ACT_RELU; each element is fp32 adds in that order.
 * rg_residual_join_backward: dx = (((g0 + g1) + g2) + g3) where out > 0 (out: the join's saved relu output, nullable: no
 * mask; g1 .. g3 nullable), 0 elsewhere, a NaN in out passing the sum. */
int rg_residual_join(const float* a, int64_t lda, const float* b, int64_t ldb, const float* pe, int64_t ld_pe, int seq_len,
                     int batch, int cols, int act, float* out, int64_t ldo, rg_stream_t stream);
int rg_residual_join_backward(const float* out, int64_t ldo, const float* g0, int64_t ld0, const float* g1, int64_t ld1,
                              const float* g2, int64_t ld2, const float* g3, int64_t ld3, int64_t rows, int cols, float* dx,
                              int64_t ld_dx, rg_stream_t stream);

/* ---- Seq2Slate behind its encoder: embedding join, Frechet-sort likelihood and ranking (seq2slate.hip) --------------------
 * Rows of the encoder's matrices are ordered (s, b): row s * batch + b of an fp32 [seq_len * batch, embed] view, as
 * rg_attn_* reads them; candidate c of the reference's index space is c + 2 (0 = padding, 1 = the decoder's start symbol).
 *
 * rg_s2s_embed_join: src_embed[(s, b), :] = (sqrt(state_cols) * state_embed[b] | sqrt(cand_cols) * cand_embed[(s, b)]), the
 * two Embedders' scalings with encode's repeat / reshape / cat (reagent/models/seq2slate.py:317-328, 776-796) in one launch;
 * state_embed [batch, state_cols], cand_embed [seq_len * batch, cand_cols]; each element is one fp32 multiply by the root
 * rounded to fp32.  rg_s2s_embed_join_backward: d_state_embed[b] = sqrt(state_cols) * sum_s d_src_embed[(s, b), :state_cols]
 * (fp32 adds in ascending s, then one multiply), d_cand_embed = sqrt(cand_cols) * the right-hand slice.
 *
 * rg_frechet_head: PER_SEQ_LOG_PROB_MODE of a FRECHET_SORT net behind its encoder (decode, seq2slate.py:807-818;
 * per_symbol_to_per_seq_probs, reagent/model_utils/seq2slate_utils.py:147-160) and Seq2SlateTrainer's loss
 * (reagent/training/ranking/seq2slate_trainer.py:119-149, helper.py:10-18).  mem = the last encoder layer's output, w [embed]
 * and bias [1] = encoder_scorer; tgt_out_idx [batch, tgt_len] int64 (pitch ld_idx), offset by 2, distinct in a row (a repeated
 * index gives that row p = 1e-40 and no gradient; nothing is read or written through an index).
 *   score[b, c] = w . mem[(c, b)] + bias;  pi_t = softmax of the scores over the candidates not chosen before step t;
 *   p[b] = max(prod_t pi_t(a_t), 1e-40) (an fp32 subnormal: kept, not flushed);  log_prob = log p;  impt = p / logged;
 *   clamped = impt (RG_IPS_CLAMP_NONE), clamp(impt, 0, clamp_max) (UNIVERSAL), where(impt > clamp_max, 0, impt) (AGGRESSIVE);
 *   sums[0] = mean(-clamped * (reward - baseline)), sums[1] = mean(-impt * reward), sums[2] = mean(-clamped * reward)
 * (baseline nullable: zeros).  With dscore .. dbias given (all four or none): d sums[0] / d score [batch, seq_len] =
 * g_b * p_b * sum_{t : c remaining at t} (1[c = a_t] - pi_t(c)) with g_b = d sums[0] / d p_b by autograd's rule through each
 * clamp (1e-40: where the product is at or above it; UNIVERSAL: where 0 <= impt <= clamp_max; AGGRESSIVE: where not
 * impt > clamp_max), and from it dmem [seq_len * batch, embed] (written whole), dw [embed] and dbias [1].  logged null (then
 * reward .. sums and the gradients must be null too): log_prob and p alone.  Everything is double on the fp32 inputs, each
 * output rounded once; a wave owns a row, workgroups leave partials in workspace (rg_frechet_head_workspace doubles) which a
 * second launch adds in workgroup order: no atomics, two runs give the same bits.
 *
 * rg_frechet_rank: RANK_MODE in one launch.  scores [batch, seq_len] given, or (scores null) computed from mem, w and bias as
 * above.  RG_FRECHET_RANK_ENCODER (_encoder_rank): argsort of the scores, descending; RG_FRECHET_RANK_GREEDY (_greedy_rank):
 * argsort of the first step's soft-max, descending; both with ties to the lower index, one-hot ranked_per_symbol_probs and
 * ranked_per_seq_probs = 1.  RG_FRECHET_RANK_SAMPLED (_autoregressive_rank, greedy=False): tgt_len draws without
 * replacement, each from its step's pi_t by inversion of the cumulative sum (double, ascending candidate order) at a
 * Philox4x32-10 uniform, key = seed, counter = (row, step); the probabilities are the pi_t rows and ranked_per_seq_probs their
 * product at the drawn indices, clamped at 1e-40.  The reference draws with torch.multinomial: the law is the same, the
 * stream is not.  ranked_tgt_out_idx [batch, tgt_len] int64 (offset by 2), ranked_per_symbol_probs [batch, tgt_len,
 * seq_len + 2] (columns 0 and 1 zero), ranked_per_seq_probs [batch], all contiguous and written whole.
 *
 * The soft-max's exponential holds its argument at -745: a remaining candidate more than 745 below the step's maximum weighs
 * 4.9e-324 where the float64 statement has 0, which no sum, no rounded output and no draw sees.
 *
 * RG_EINVAL for tgt_len > seq_len, a pitch below its width, a missing pointer or an unknown method / mode; RG_EUNSUPPORTED
 * for seq_len > RG_S2S_MAX_SEQ_LEN (a lane per candidate), embed (for the joins: state_cols + cand_cols) > RG_S2S_MAX_EMBED or
 * seq_len * batch >= 2^29. */
#define RG_S2S_MAX_SEQ_LEN 64
#define RG_S2S_MAX_EMBED 512
enum { RG_IPS_CLAMP_NONE = 0, RG_IPS_CLAMP_UNIVERSAL = 1, RG_IPS_CLAMP_AGGRESSIVE = 2 };
enum { RG_FRECHET_RANK_ENCODER = 0, RG_FRECHET_RANK_GREEDY = 1, RG_FRECHET_RANK_SAMPLED = 2 };
int rg_s2s_embed_join(const float* state_embed, int64_t ld_state, const float* cand_embed, int64_t ld_cand, int seq_len, int batch,
                      int state_cols, int cand_cols, float* src_embed, int64_t ld_out, rg_stream_t stream);
int rg_s2s_embed_join_backward(const float* d_src_embed, int64_t ld_d, int seq_len, int batch, int state_cols, int cand_cols,
                               float* d_state_embed, int64_t ld_dstate, float* d_cand_embed, int64_t ld_dcand,
                               rg_stream_t stream);
size_t rg_frechet_head_workspace(int batch, int embed);
int rg_frechet_head(const float* mem, int64_t ld_mem, const float* w, const float* bias, const int64_t* tgt_out_idx,
                    int64_t ld_idx, const float* logged, const float* reward, const float* baseline, int clamp_method,
                    double clamp_max, int seq_len, int tgt_len, int batch, int embed, float* log_prob, float* p, float* impt,
                    float* clamped, float* sums, float* dscore, int64_t ld_dscore, float* dmem, int64_t ld_dmem, float* dw,
                    float* dbias, double* workspace, rg_stream_t stream);
int rg_frechet_rank(const float* scores, int64_t ld_scores, const float* mem, int64_t ld_mem, const float* w, const float* bias,
                    int mode, uint64_t seed, int seq_len, int tgt_len, int batch, int embed, int64_t* ranked_tgt_out_idx,
                    float* ranked_per_symbol_probs, float* ranked_per_seq_probs, rg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REAGENT_HIP_H_ */
