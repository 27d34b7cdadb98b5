// mlp_update.hip — a fused FullyConnected stack's fp32 master weights -> the fragment-ordered bf16 (or split-bf16) operands
// its kernels read (mlp_fused.hip, mlp_fused_x3.hip, qr_grouped.hip): the staging launches, and the optimizer step fused with
// re-staging — Adam (rg_optim.h), the target network's soft update and both networks' fragment stores in one launch.

#include "rg_mlp_frag.h"
#include "rg_reduce.h"

namespace rg {

struct StageGroupArgs {
  int n;
  int x3;  // also write the lo planes (bf16(w - hi)) behind the hi planes
  long begin[FB_MAXL + 1];
  const float* w[FB_MAXL];
  int N[FB_MAXL], K[FB_MAXL];
  bf16_t* wf[FB_MAXL];
  bf16_t* wb[FB_MAXL];
};

__global__ void stage_group_kernel(StageGroupArgs G) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G.begin[G.n]) return;
  const float* w = G.w[0];
  int N = G.N[0], K = G.K[0];
  bf16_t* wf = G.wf[0];
  bf16_t* wb = G.wb[0];
  long base = 0;
#pragma unroll
  for (int k = 1; k < FB_MAXL; ++k)
    if (k < G.n && i >= G.begin[k]) {
      w = G.w[k]; N = G.N[k]; K = G.K[k]; wf = G.wf[k]; wb = G.wb[k]; base = G.begin[k];
    }
  stage_weight_elem(w, N, K, wf, wb, i - base, G.x3);
}

__global__ void stage_weights_frag_kernel(const float* __restrict__ w, int N, int K, bf16_t* __restrict__ wf,
                                          bf16_t* __restrict__ wb) {
  const int NTf = (N + 31) / 32, KCf = (K + 15) / 16;
  const int NTb = (K + 31) / 32, KCb = (N + 15) / 16;
  const long tf = (long)NTf * KCf * 512, tb = (long)NTb * KCb * 512;
  const long total = tf > tb ? tf : tb;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    stage_weight_elem(w, N, K, wf, wb, i);
  }
}

// ---- optimizer step fused with weight staging ----------------------------------------------------
// After the backward pass a DQN step runs Adam on the online network, the soft update of the target
// network and the bf16 re-staging of both networks' weights: four launches of ~5-8 us each for
// 600 K parameters (they are launch-bound, not bandwidth-bound).  This kernel walks the flat
// parameter slab (coalesced on the five fp32 arrays) and does all of it per element: the Adam and
// soft-update arithmetic of rg_optim.h, then, for weight elements, the bf16 value goes to its three
// fragment slots (online forward / backward, target forward; 2-byte scattered stores into 1.2 MB).
struct UpdateArgs {
  int n;
  long total;  // slab elements
  int N[FB_MAXL], K[FB_MAXL];
  long w_off[FB_MAXL], b_off[FB_MAXL];
  bf16_t* wf[FB_MAXL];
  bf16_t* wb[FB_MAXL];
  bf16_t* twf[FB_MAXL];
  float* p;
  const float* g;
  float* m;
  float* v;
  float* t;
  AdamCoef c;
  float tau, one_minus_tau;
  const double* sched;  // device-resident Adam schedule (rg_optim.h) or null: coefficients as launch arguments
  // split-bf16 stacks: every fragment buffer is [hi plane | lo plane], lo = bf16(x - hi) (stage_weight_elem); the lo
  // plane of layer l starts wfrag_elems(N, K) (forward, target) / wfrag_elems(K, N) (backward) elements in
  int x3;
  // grouped layers (qr_grouped.hip: QR-DQN's A x N output layer as A independent [Ng, K] layers): Ng[l] > 0 = the rows
  // of layer l fall into groups of Ng, group g's fragments start g * per_f[l] (forward, target) / g * per_b[l] (backward)
  // elements in — what rg_group_weights_stage writes (split-bf16: a group's set is [hi plane | lo plane], per_* covers both).
  int Ng[FB_MAXL];
  long per_f[FB_MAXL], per_b[FB_MAXL];
  // replayed steps (runtime._GraphedLoop): the sampler launch has already counted this step in sched[0]
  // (sched_pre_ticked), and this launch advances the index pool's cursor for the next one — workgroup 0, when it is
  // done; no other workgroup of this launch touches it
  int pre_ticked;
  long long* post_tick;
  int post_tick_mod;
};

// the three fragment slots of W[n][k] (online forward / backward, target forward), both planes in split-bf16 mode —
// element for element what stage_weight_elem writes
__device__ __forceinline__ void update_store_frags(const UpdateArgs& U, int l, int n, int k, float pn, float tn) {
  int N = U.N[l];
  const int K = U.K[l];
  long gf = 0, gb = 0;
  if (U.Ng[l] > 0) {  // this row's group, its row inside the group
    const int g = n / U.Ng[l];
    n -= g * U.Ng[l];
    N = U.Ng[l];
    gf = g * U.per_f[l];
    gb = g * U.per_b[l];
  }
  const int KCf = (K + 15) / 16, KCb = (N + 15) / 16;
  const long jf = gf + ((((long)(n >> 5) * KCf + (k >> 4)) * 64) + ((n & 31) + 32 * ((k & 15) >> 3))) * 8 + (k & 7);
  const long tf = (long)((N + 31) / 32) * KCf * 512, tb = (long)((K + 31) / 32) * KCb * 512;
  const bf16_t ph = f32_to_bf16(pn), th = f32_to_bf16(tn);
  if (U.wf[l]) {
    U.wf[l][jf] = ph;
    if (U.x3) U.wf[l][tf + jf] = f32_to_bf16(pn - bf16_to_f32(ph));
  }
  if (U.twf[l]) {
    U.twf[l][jf] = th;
    if (U.x3) U.twf[l][tf + jf] = f32_to_bf16(tn - bf16_to_f32(th));
  }
  if (U.wb[l]) {
    const long jb = gb + ((((long)(k >> 5) * KCb + (n >> 4)) * 64) + ((k & 31) + 32 * ((n & 15) >> 3))) * 8 + (n & 7);
    U.wb[l][jb] = ph;
    if (U.x3) U.wb[l][tb + jb] = f32_to_bf16(pn - bf16_to_f32(ph));
  }
}

__global__ void mlp_update_kernel(UpdateArgs U) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= U.total) return;
  // which tensor of the slab does element i belong to?  (alignment gaps between tensors: none)
  int l = -1, is_w = 0;
  long rel = 0;
#pragma unroll
  for (int k = 0; k < FB_MAXL; ++k) {
    if (k < U.n) {
      const long wn = (long)U.N[k] * U.K[k];
      if (i >= U.w_off[k] && i < U.w_off[k] + wn) { l = k; is_w = 1; rel = i - U.w_off[k]; }
      if (i >= U.b_off[k] && i < U.b_off[k] + U.N[k]) { l = k; is_w = 0; rel = i - U.b_off[k]; }
    }
  }
  if (l < 0) return;
  if (U.post_tick && i == 0) U.post_tick[0] = (U.post_tick[0] + 1) % U.post_tick_mod;
  const AdamCoef coef = sched_coef(U.c, U.sched, U.pre_ticked);
  float mi = U.m[i], vi = U.v[i];
  const float pn = adam_element(coef, U.p[i], U.g[i], mi, vi);
  U.p[i] = pn;
  U.m[i] = mi;
  U.v[i] = vi;
  float tn = 0.f;
  if (U.t) {
    tn = soft_update_element(U.tau, U.one_minus_tau, pn, U.t[i]);
    U.t[i] = tn;
  }
  if (!is_w) return;
  const int K = U.K[l];
  // B-fragment slot of W[n][k] (forward) and of W^T[k][n] (backward); padding slots were zeroed by
  // the first staging and are never touched
  update_store_frags(U, l, (int)(rel / K), (int)(rel % K), pn, tn);
}

// Tiled form of the update for weight matrices whose rows can be read in 32-byte pieces (in_features a
// multiple of 8, slab offset a multiple of 4): a workgroup owns a 32 (out) x 32 (in) tile, every thread
// four consecutive in-features of one row.  Against one element per thread this turns
//   * the fp32 traffic (p, g, m, v, target) into float4 requests,
//   * the forward fragments (online and target) into one 8-byte store per thread (half a fragment
//     record), and
//   * the backward fragments (W^T: 8 consecutive OUT-features of one in-feature are a record) into one
//     16-byte store per thread after a transpose through LDS, instead of 2-byte stores 16 bytes apart.
// The arithmetic is adam_element / soft_update_element on the same values: bit-identical results.
constexpr int UT_ROWS = 32, UT_COLS = 32, UT_PITCH = UT_COLS + 2;  // pitch: 17 dwords, conflict-free columns

struct UpdateTileArgs {
  UpdateArgs u;
  int tile_begin[FB_MAXL + 1];  // first workgroup of each layer's tiles; [n] = first "rest" workgroup
  int tiled[FB_MAXL];           // layer's weight handled by tiles
  long rest_begin[2 * FB_MAXL + 1];  // prefix sums of the element ranges left to the per-element path
};

__device__ __forceinline__ void update_one(const UpdateArgs& U, const AdamCoef& coef, long i, float& pn, float& tn) {
  float mi = U.m[i], vi = U.v[i];
  pn = adam_element(coef, U.p[i], U.g[i], mi, vi);
  U.p[i] = pn;
  U.m[i] = mi;
  U.v[i] = vi;
  tn = 0.f;
  if (U.t) {
    tn = soft_update_element(U.tau, U.one_minus_tau, pn, U.t[i]);
    U.t[i] = tn;
  }
}

__global__ void mlp_update_tiles_kernel(UpdateTileArgs T) {
  const UpdateArgs& U = T.u;
  __shared__ bf16_t tile[UT_ROWS * UT_PITCH];
  __shared__ bf16_t tile_lo[UT_ROWS * UT_PITCH];  // split-bf16: lo plane of the tile
  const int wg = blockIdx.x, tid = threadIdx.x;
  const AdamCoef coef = sched_coef(U.c, U.sched, U.pre_ticked);
  if (U.post_tick && wg == 0 && tid == 0) U.post_tick[0] = (U.post_tick[0] + 1) % U.post_tick_mod;
  if (wg >= T.tile_begin[U.n]) {
    // everything the tiles do not cover (biases; weights with odd shapes): one element per thread
    const long j = (long)(wg - T.tile_begin[U.n]) * blockDim.x + tid;
    int r = -1;
    for (int q = 0; q < 2 * U.n; ++q)
      if (j >= T.rest_begin[q] && j < T.rest_begin[q + 1]) r = q;
    if (r < 0) return;
    const int l = r >> 1, is_w = r & 1;
    const long rel = j - T.rest_begin[r];
    float pn, tn;
    update_one(U, coef, (is_w ? U.w_off[l] : U.b_off[l]) + rel, pn, tn);
    if (!is_w) return;
    const int K = U.K[l];
    update_store_frags(U, l, (int)(rel / K), (int)(rel % K), pn, tn);
    return;
  }
  int l = 0;
  for (int q = 1; q < U.n; ++q)
    if (wg >= T.tile_begin[q]) l = q;
  const int N = U.N[l], K = U.K[l];
  const int tiles_k = (K + UT_COLS - 1) / UT_COLS;
  const int tw = wg - T.tile_begin[l];
  const int n0 = (tw / tiles_k) * UT_ROWS, k0 = (tw % tiles_k) * UT_COLS;
  const int r = tid >> 3, c = (tid & 7) * 4;  // row of the tile, first of this thread's 4 in-features
  const int n = n0 + r, k = k0 + c;
  const bool live = n < N && k < K;  // K % 8 == 0: a piece is entirely inside or outside
  float pn[4], tn[4], pl[4] = {0.f, 0.f, 0.f, 0.f}, tl[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const long i = U.w_off[l] + (long)n * K + k;
    f32x4 P = *(const f32x4*)(U.p + i), G = *(const f32x4*)(U.g + i), M = *(const f32x4*)(U.m + i);
    f32x4 V = *(const f32x4*)(U.v + i), Tg = U.t ? *(const f32x4*)(U.t + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float mi = M[e], vi = V[e];
      pn[e] = adam_element(coef, P[e], G[e], mi, vi);
      P[e] = pn[e];
      M[e] = mi;
      V[e] = vi;
      tn[e] = 0.f;
      if (U.t) {
        tn[e] = soft_update_element(U.tau, U.one_minus_tau, pn[e], Tg[e]);
        Tg[e] = tn[e];
      }
    }
    *(f32x4*)(U.p + i) = P;
    *(f32x4*)(U.m + i) = M;
    *(f32x4*)(U.v + i) = V;
    if (U.t) *(f32x4*)(U.t + i) = Tg;
    const int KCf = (K + 15) / 16;
    int nl = n;  // row inside its group (grouped layer) / the row itself
    long gf = 0;
    if (U.Ng[l] > 0) {
      const int g = n / U.Ng[l];
      nl = n - g * U.Ng[l];
      gf = g * U.per_f[l];
    }
    const long jf = gf + ((((long)(nl >> 5) * KCf + (k >> 4)) * 64) + ((nl & 31) + 32 * ((k & 15) >> 3))) * 8 + (k & 7);
    // lo plane of the forward fragments (split-bf16): behind the layer's — a grouped layer: the group's — hi plane
    const long tf = (long)(((U.Ng[l] > 0 ? U.Ng[l] : N) + 31) / 32) * KCf * 512;
    if (U.wf[l]) *(uint2*)(U.wf[l] + jf) = uint2{pack_bf16x2(pn[0], pn[1]), pack_bf16x2(pn[2], pn[3])};
    if (U.twf[l]) *(uint2*)(U.twf[l] + jf) = uint2{pack_bf16x2(tn[0], tn[1]), pack_bf16x2(tn[2], tn[3])};
    if (U.x3) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pl[e] = pn[e] - bf16_to_f32(f32_to_bf16(pn[e]));
        tl[e] = tn[e] - bf16_to_f32(f32_to_bf16(tn[e]));
      }
      if (U.wf[l]) *(uint2*)(U.wf[l] + tf + jf) = uint2{pack_bf16x2(pl[0], pl[1]), pack_bf16x2(pl[2], pl[3])};
      if (U.twf[l]) *(uint2*)(U.twf[l] + tf + jf) = uint2{pack_bf16x2(tl[0], tl[1]), pack_bf16x2(tl[2], tl[3])};
    }
  }
  if (!U.wb[l]) return;  // workgroup-uniform
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    tile[r * UT_PITCH + c + e] = live ? f32_to_bf16(pn[e]) : (bf16_t)0;
    if (U.x3) tile_lo[r * UT_PITCH + c + e] = live ? f32_to_bf16(pl[e]) : (bf16_t)0;
  }
  __syncthreads();
  // W^T fragments: thread -> (in-feature kk, group of 8 out-features); a record = 8 consecutive n
  const int kk = tid & 31, ng = tid >> 5;
  const int kt = k0 + kk, nt = n0 + ng * 8;
  if (ng < UT_ROWS / 8 && kt < K && nt < N) {  // N may end inside a record: those slots are padding and stay zero-written
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (nt + e < N) ? tile[(ng * 8 + e) * UT_PITCH + kk] : (bf16_t)0;
    // grouped layer (Ng % 8 == 0, checked by the host): a record of 8 out-features lies inside one group
    const int grp = U.Ng[l] > 0 ? nt / U.Ng[l] : 0;
    const int ntl = nt - grp * (U.Ng[l] > 0 ? U.Ng[l] : 0);
    const int KCb = ((U.Ng[l] > 0 ? U.Ng[l] : N) + 15) / 16;
    const long jb = grp * (U.Ng[l] > 0 ? U.per_b[l] : 0) +
                    ((((long)(kt >> 5) * KCb + (ntl >> 4)) * 64) + ((kt & 31) + 32 * ((ntl & 15) >> 3))) * 8;
    *(u32x4*)(U.wb[l] + jb) = u32x4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16),
                                    (unsigned)h[4] | ((unsigned)h[5] << 16), (unsigned)h[6] | ((unsigned)h[7] << 16)};
    if (U.x3) {
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (nt + e < N) ? tile_lo[(ng * 8 + e) * UT_PITCH + kk] : (bf16_t)0;
      const long tb = (long)((K + 31) / 32) * KCb * 512;
      *(u32x4*)(U.wb[l] + tb + jb) = u32x4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16),
                                           (unsigned)h[4] | ((unsigned)h[5] << 16), (unsigned)h[6] | ((unsigned)h[7] << 16)};
    }
  }
}

}  // namespace rg

using namespace rg;

extern "C" {

int rg_stage_weights_frag(const float* w, int out_features, int in_features, void* wfrag_fwd, void* wfrag_bwd,
                          rg_stream_t stream) {
  if (!w || out_features <= 0 || in_features <= 0 || (!wfrag_fwd && !wfrag_bwd)) return RG_EINVAL;
  const size_t tf = rg_wfrag_elems(out_features, in_features), tb = rg_wfrag_elems(in_features, out_features);
  const size_t total = tf > tb ? tf : tb;
  long blocks = (long)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  RG_LAUNCH(stage_weights_frag_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, w, out_features,
            in_features, (bf16_t*)wfrag_fwd, (bf16_t*)wfrag_bwd);
  return (int)hipGetLastError();
}

/* all layers' weights of a stack -> fragment order in one launch */
int rg_mlp_stage_weights_fused(const rg_mlp_desc* d, int need_bwd, rg_stream_t stream) {
  if (!d || d->n_layers < 1 || d->n_layers > FB_MAXL) return RG_EINVAL;
  StageGroupArgs G;
  G.n = d->n_layers;
  G.x3 = d->x3;
  long off = 0;
  for (int l = 0; l < FB_MAXL; ++l) {
    G.begin[l] = off;
    if (l < d->n_layers) {
      if (!d->w[l] || !d->wfrag_fwd[l]) return RG_EINVAL;
      const int N = d->dims[l + 1], K = d->dims[l];
      G.w[l] = d->w[l]; G.N[l] = N; G.K[l] = K;
      G.wf[l] = (bf16_t*)d->wfrag_fwd[l];
      G.wb[l] = need_bwd ? (bf16_t*)d->wfrag_bwd[l] : nullptr;
      const size_t tf = rg_wfrag_elems(N, K), tb = G.wb[l] ? rg_wfrag_elems(K, N) : 0;
      off += (long)(tf > tb ? tf : tb);
    } else {
      G.w[l] = nullptr; G.N[l] = G.K[l] = 0; G.wf[l] = G.wb[l] = nullptr;
    }
  }
  pad_begin_table(G.begin, d->n_layers, off);
  RG_LAUNCH(stage_group_kernel, dim3((unsigned)((off + 255) / 256)), dim3(256), (hipStream_t)stream, G);
  return (int)hipGetLastError();
}

static int mlp_update_launch(const rg_mlp_update_desc* d, double lr, double beta1, double beta2, double eps,
                             double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                             double grad_scale, double tau, const double* sched, rg_stream_t stream) {
  if (!d || d->n_layers < 1 || d->n_layers > FB_MAXL || !d->param || !d->grad || !d->exp_avg || !d->exp_avg_sq ||
      bias_correction1 == 0.0 || (d->target && (tau < 0.0 || tau > 1.0)))
    return RG_EINVAL;
  UpdateArgs U;
  U.n = d->n_layers;
  long total = 0;
  for (int l = 0; l < FB_MAXL; ++l) {
    if (l < d->n_layers) {
      const int K = d->dims[l], N = d->dims[l + 1];
      U.N[l] = N; U.K[l] = K;
      U.w_off[l] = d->w_off[l]; U.b_off[l] = d->b_off[l];
      U.wf[l] = (bf16_t*)d->wfrag_fwd[l]; U.wb[l] = (bf16_t*)d->wfrag_bwd[l]; U.twf[l] = (bf16_t*)d->target_wfrag_fwd[l];
      const int Ng = d->group_rows[l];
      if (Ng < 0 || (Ng > 0 && N % Ng != 0)) return RG_EINVAL;
      U.Ng[l] = Ng;
      // a group's fragment set: [hi plane] (bf16) or [hi plane | lo plane] (split-bf16), what rg_group_weights_stage writes
      U.per_f[l] = Ng > 0 ? (long)wfrag_elems(Ng, K) * (d->x3 ? 2 : 1) : 0;
      U.per_b[l] = Ng > 0 ? (long)wfrag_elems(K, Ng) * (d->x3 ? 2 : 1) : 0;
      const long we = d->w_off[l] + (long)N * K, be = d->b_off[l] + N;
      total = we > total ? we : total;
      total = be > total ? be : total;
    } else {
      U.N[l] = U.K[l] = 0; U.w_off[l] = U.b_off[l] = 0; U.wf[l] = U.wb[l] = U.twf[l] = nullptr;
      U.Ng[l] = 0; U.per_f[l] = U.per_b[l] = 0;
    }
  }
  U.total = total;
  U.p = d->param; U.g = d->grad; U.m = d->exp_avg; U.v = d->exp_avg_sq; U.t = d->target;
  const double step_size = lr / bias_correction1;
  U.c = AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay,
                 (float)(-step_size), (float)bias_correction2_sqrt, (float)grad_scale};
  U.tau = (float)tau; U.one_minus_tau = (float)(1.0 - tau);
  U.sched = sched;
  U.pre_ticked = (sched && d->sched_pre_ticked) ? 1 : 0;
  U.post_tick = (long long*)d->post_tick;
  U.post_tick_mod = d->post_tick_mod > 0 ? d->post_tick_mod : 1;
  if (d->sched_pre_ticked && !sched) return RG_EINVAL;
  U.x3 = d->x3 ? 1 : 0;
  // weights with 32-byte-addressable rows go to the tiled kernel, the rest of the slab to its
  // per-element workgroups (same launch)
  UpdateTileArgs T;
  T.u = U;
  int wgs = 0, any_tiled = 0;
  long rest = 0;
  for (int l = 0; l < FB_MAXL; ++l) {
    T.tile_begin[l] = wgs;
    T.tiled[l] = 0;
    if (l < d->n_layers) {
      const int K = U.K[l], N = U.N[l];
      const bool ok = (K % 8) == 0 && (U.Ng[l] % 8) == 0 && (U.w_off[l] % 4) == 0 && ((((uintptr_t)U.p | (uintptr_t)U.g | (uintptr_t)U.m |
                                                                  (uintptr_t)U.v | (uintptr_t)U.t) & 15) == 0) &&
                      ((((uintptr_t)U.wf[l] | (uintptr_t)U.wb[l] | (uintptr_t)U.twf[l]) & 15) == 0);
      if (ok) {
        T.tiled[l] = 1;
        any_tiled = 1;
        wgs += ((N + UT_ROWS - 1) / UT_ROWS) * ((K + UT_COLS - 1) / UT_COLS);
      }
      T.rest_begin[2 * l] = rest;
      rest += N;  // bias
      T.rest_begin[2 * l + 1] = rest;
      if (!ok) rest += (long)N * K;
    } else {
      T.rest_begin[2 * l] = T.rest_begin[2 * l + 1] = rest;
    }
  }
  pad_begin_table(T.tile_begin, d->n_layers, wgs);
  pad_begin_table(T.rest_begin, 2 * d->n_layers, rest);
  if (!any_tiled) {
    RG_LAUNCH(mlp_update_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, U);
    return (int)hipGetLastError();
  }
  const int rest_wgs = (int)((rest + 255) / 256);
  RG_LAUNCH(mlp_update_tiles_kernel, dim3((unsigned)(wgs + rest_wgs)), dim3(256), (hipStream_t)stream, T);
  return (int)hipGetLastError();
}

int rg_mlp_update_fused(const rg_mlp_update_desc* d, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                        double grad_scale, double tau, rg_stream_t stream) {
  return mlp_update_launch(d, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale,
                           tau, nullptr, stream);
}

int rg_mlp_update_fused_sched(const rg_mlp_update_desc* d, double beta1, double beta2, double eps,
                              double weight_decay, double grad_scale, double tau, const double* sched,
                              rg_stream_t stream) {
  if (!sched) return RG_EINVAL;
  return mlp_update_launch(d, 0.0, beta1, beta2, eps, weight_decay, 1.0, 1.0, grad_scale, tau, sched, stream);
}

}  // extern "C"
