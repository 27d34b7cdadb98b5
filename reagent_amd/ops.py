"""Thin tensor-level wrappers over the C ABI (one function per entry point of reagent_hip.h).

All tensors must be on the GPU; leading dimensions are taken from ``stride(0)``.  Nothing here
falls back to torch math.  ``profile()`` optionally brackets every C-ABI call with HIP events on
the stream the kernels are enqueued on (bench.py's per-kernel roofline numbers come from that).
"""
import contextlib
import ctypes
import os
from typing import List, Optional, Tuple

import torch

from . import _lib as L

BF16 = torch.bfloat16
F32 = torch.float32


def compute_dtype(precision: int) -> torch.dtype:
    return F32 if precision == L.PREC_F32 else BF16


def dt_code(dtype: torch.dtype) -> int:
    if dtype == F32:
        return L.DT_F32
    if dtype == BF16:
        return L.DT_BF16
    raise L.ReagentHipError(f"unsupported dtype {dtype}")


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D tensor"
    return t.stride(0)


def _chk_dev(*ts):
    for t in ts:
        if t is not None:
            L.require_cuda(t)


# ---- optional per-call timing -----------------------------------------------------------------
class CallProfile:
    """(entry point, meta) -> HIP-event durations in ms, on torch's current stream."""

    def __init__(self):
        self.records: List[Tuple[str, dict, torch.cuda.Event, torch.cuda.Event]] = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, meta, s, e in self.records:
            key = (name, tuple(sorted(meta.items())))
            d = out.setdefault(key, {"name": name, "meta": meta, "calls": 0, "ms": 0.0})
            d["calls"] += 1
            d["ms"] += s.elapsed_time(e)
        return sorted(out.values(), key=lambda d: -d["ms"])


_prof: Optional[CallProfile] = None


@contextlib.contextmanager
def profile():
    global _prof
    prev, _prof = _prof, CallProfile()
    try:
        yield _prof
    finally:
        _prof = prev


def _run(name: str, meta: dict, call):
    if _prof is None:
        L.check(call(), name)
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = call()
    e.record()
    L.check(rc, name)
    _prof.records.append((name, meta, s, e))


def profiling() -> bool:
    return _prof is not None


@contextlib.contextmanager
def profile_span(name: str, meta: dict):
    """events around a region that is not one C-ABI call (the RCCL all-reduce of the gradient slab); no-op unless
    a profile() pass is active"""
    if _prof is None:
        yield
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    yield
    e.record()
    _prof.records.append((name, meta, s, e))


# ---- FullyConnected ---------------------------------------------------------------------------
def fc_forward(x, w, bias, act: int, precision: int, y=None, y32=None, yt=None):
    """y = act(x @ w.T + bias); any of y (compute type), y32 (fp32), yt (transposed) may be given."""
    _chk_dev(x, w, bias, y, y32, yt)
    batch, in_f = x.shape
    out_f = w.shape[0]
    ldy = _ld(y) if y is not None else (_ld(y32) if y32 is not None else out_f)
    if y is not None and y32 is not None:
        assert _ld(y) == _ld(y32)
    _run("rg_fc_forward", dict(M=batch, N=out_f, K=in_f, prec=precision),
         lambda: L.lib().rg_fc_forward(L.ptr(x), _ld(x), L.ptr(w), _ld(w), L.ptr(bias), L.ptr(y), L.ptr(y32),
                                       ldy, L.ptr(yt), _ld(yt) if yt is not None else 0, batch, out_f, in_f,
                                       act, precision, L.stream_ptr()))


def fc_dgrad(dz, wt, ht, act_below: int, precision: int, dx=None, dx32=None, dxt=None):
    _chk_dev(dz, wt, ht, dx, dx32, dxt)
    batch, out_f = dz.shape
    in_f = wt.shape[0]
    lddx = _ld(dx) if dx is not None else (_ld(dx32) if dx32 is not None else in_f)
    _run("rg_fc_dgrad", dict(M=batch, N=in_f, K=out_f, prec=precision),
         lambda: L.lib().rg_fc_dgrad(L.ptr(dz), _ld(dz), L.ptr(wt), _ld(wt), L.ptr(ht),
                                     _ld(ht) if ht is not None else 0, act_below, L.ptr(dx), L.ptr(dx32), lddx,
                                     L.ptr(dxt), _ld(dxt) if dxt is not None else 0, batch, in_f, out_f,
                                     precision, L.stream_ptr()))


def fc_wgrad_workspace_bytes(out_f, in_f, batch, precision) -> int:
    return int(L.lib().rg_fc_wgrad_workspace_bytes(out_f, in_f, batch, precision))


def fc_wgrad(dzt, xt, dw, db, workspace, precision: int):
    """dw[out,in] (contiguous fp32) = dz^T x, db[out] = sum_b dz; inputs are transposed copies."""
    _chk_dev(dzt, xt, dw, db, workspace)
    out_f, batch = dzt.shape
    in_f = xt.shape[0]
    assert dw.is_contiguous() and dw.dtype == F32
    _run("rg_fc_wgrad", dict(M=out_f, N=in_f, K=batch, prec=precision),
         lambda: L.lib().rg_fc_wgrad(L.ptr(dzt), _ld(dzt), L.ptr(xt), _ld(xt), L.ptr(dw), L.ptr(db),
                                     L.ptr(workspace), workspace.numel() * workspace.element_size(), out_f,
                                     in_f, batch, precision, L.stream_ptr()))


def act_backward(dy, y, act: int, dz):
    """dz = dy * act'(z) through the activation output y (all fp32 [rows, cols], unit column stride)"""
    _chk_dev(dy, y, dz)
    rows, cols = dy.shape
    assert dy.dtype == y.dtype == dz.dtype == F32 and dy.stride(1) == y.stride(1) == dz.stride(1) == 1
    _run("rg_act_backward", dict(rows=rows, cols=cols),
         lambda: L.lib().rg_act_backward(L.ptr(dy), _ld(dy), L.ptr(y), _ld(y), act, L.ptr(dz), _ld(dz), rows, cols,
                                         L.stream_ptr()))


def td3_target_action(next_actor, noise, noise_variance, noise_clip_range, lo, hi, out):
    """out (a [B, A] view, e.g. the action columns of the critic input) = smoothed target action"""
    _chk_dev(next_actor, noise, out)
    B, A = next_actor.shape
    assert noise.is_contiguous() and noise.shape == (B, A) and next_actor.stride(1) == 1 and out.stride(1) == 1
    _run("rg_td3_target_action", dict(B=B, A=A),
         lambda: L.lib().rg_td3_target_action(L.ptr(next_actor), _ld(next_actor), L.ptr(noise), float(noise_variance),
                                              float(noise_clip_range[0]), float(noise_clip_range[1]), float(lo), float(hi), L.ptr(out), _ld(out), B, A,
                                              L.stream_ptr()))


def tile_concat(x, x2, out, x_tile: int = 1):
    """out[r] = cat(x[r // x_tile], x2[r]) (fp32; out may be a [rows, S + A] view of a wider workspace): the critic input
    on the tiled next state, or with x_tile = 1 the plain cat(state, action)"""
    _chk_dev(x, x2, out)
    R, A = x2.shape
    S = x.shape[1]
    assert x.dtype == x2.dtype == out.dtype == F32 and x_tile >= 1
    assert x.shape[0] == (R + x_tile - 1) // x_tile and out.shape == (R, S + A)
    _run("rg_tile_concat", dict(R=R, S=S, A=A, M=int(x_tile)),
         lambda: L.lib().rg_tile_concat(L.ptr(x), _ld(x), L.ptr(x2), _ld(x2), R, int(x_tile), S, A, L.ptr(out), _ld(out),
                                        L.stream_ptr()))


def transpose_cast(src, dst=None, dst_t=None):
    _chk_dev(src, dst, dst_t)
    rows, cols = src.shape
    out = dst if dst is not None else dst_t
    _run("rg_transpose_cast", dict(rows=rows, cols=cols),
         lambda: L.lib().rg_transpose_cast(L.ptr(src), dt_code(src.dtype), _ld(src), rows, cols, L.ptr(dst),
                                           _ld(dst) if dst is not None else 0, L.ptr(dst_t),
                                           _ld(dst_t) if dst_t is not None else 0, dt_code(out.dtype),
                                           L.stream_ptr()))


# ---- layer norm (use_layer_norm of FullyConnectedNetwork) ------------------------------------------------------
def layer_norm_forward(z32, gamma, beta, eps, act: int, y=None, y32=None, mean=None, rstd=None):
    _chk_dev(z32, gamma, beta, y, y32, mean, rstd)
    B, n = z32.shape
    _run("rg_layer_norm_forward", dict(B=B, n=n),
         lambda: L.lib().rg_layer_norm_forward(L.ptr(z32), _ld(z32), L.ptr(gamma), L.ptr(beta), float(eps), act, B, n,
                                               L.ptr(y), dt_code(y.dtype) if y is not None else 0,
                                               _ld(y) if y is not None else 0, L.ptr(y32),
                                               _ld(y32) if y32 is not None else 0, L.ptr(mean), L.ptr(rstd), L.stream_ptr()))


def layer_norm_backward(g32, z32, mean, rstd, gamma, dgamma, dbeta, workspace, dz=None, dz32=None):
    _chk_dev(g32, z32, mean, rstd, gamma, dgamma, dbeta, workspace, dz, dz32)
    B, n = z32.shape
    assert dgamma.is_contiguous() and dbeta.is_contiguous()
    _run("rg_layer_norm_backward", dict(B=B, n=n),
         lambda: L.lib().rg_layer_norm_backward(L.ptr(g32), _ld(g32), L.ptr(z32), _ld(z32), L.ptr(mean), L.ptr(rstd),
                                                L.ptr(gamma), B, n, L.ptr(dz), dt_code(dz.dtype) if dz is not None else 0,
                                                _ld(dz) if dz is not None else 0, L.ptr(dz32),
                                                _ld(dz32) if dz32 is not None else 0, L.ptr(dgamma), L.ptr(dbeta),
                                                L.ptr(workspace), workspace.numel() * workspace.element_size(),
                                                L.stream_ptr()))



# ---- batch norm / dropout (use_batch_norm, dropout_ratio of FullyConnectedNetwork; fcopts.hip) ------------------
def batch_norm_workspace(batch: int, n: int, device) -> torch.Tensor:
    nbytes = L.lib().rg_batch_norm_workspace_bytes(batch, n)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def batch_norm_forward(x32, gamma, beta, running_mean, running_var, training: bool, momentum, eps, y32, save_mean=None,
                       save_rstd=None, workspace=None, stat_updates: int = 1):
    _chk_dev(x32, gamma, beta, running_mean, running_var, y32, save_mean, save_rstd, workspace)
    B, n = x32.shape
    assert x32.dtype == y32.dtype == F32 and x32.stride(1) == y32.stride(1) == 1
    _run("rg_batch_norm_forward", dict(B=B, n=n),
         lambda: L.lib().rg_batch_norm_forward(L.ptr(x32), _ld(x32), L.ptr(gamma), L.ptr(beta), L.ptr(running_mean),
                                               L.ptr(running_var), int(bool(training)), int(stat_updates), float(momentum),
                                               float(eps), B, n,
                                               L.ptr(y32), _ld(y32), L.ptr(save_mean), L.ptr(save_rstd), L.ptr(workspace),
                                               workspace.numel() * workspace.element_size() if workspace is not None else 0,
                                               L.stream_ptr()))


def batch_norm_backward(g32, x32, gamma, mean, rstd, running_var, training: bool, eps, workspace, dx32=None, dgamma=None,
                        dbeta=None):
    _chk_dev(g32, x32, gamma, mean, rstd, running_var, workspace, dx32, dgamma, dbeta)
    B, n = x32.shape
    assert g32.dtype == x32.dtype == F32 and g32.stride(1) == x32.stride(1) == 1
    _run("rg_batch_norm_backward", dict(B=B, n=n),
         lambda: L.lib().rg_batch_norm_backward(L.ptr(g32), _ld(g32), L.ptr(x32), _ld(x32), L.ptr(gamma), L.ptr(mean),
                                                L.ptr(rstd), L.ptr(running_var), int(bool(training)), float(eps), B, n,
                                                L.ptr(dx32), _ld(dx32) if dx32 is not None else 0, L.ptr(dgamma),
                                                L.ptr(dbeta), L.ptr(workspace),
                                                workspace.numel() * workspace.element_size(), L.stream_ptr()))


def dropout(x32, p: float, keep, y32, seed: int = 0, offset: int = 0, generate: bool = True):
    """y = x * keep / (1 - p); generate: draw `keep` (uint8 [B * n]) from (seed, offset), else read it (backward)"""
    _chk_dev(x32, keep, y32)
    B, n = x32.shape
    assert x32.dtype == y32.dtype == F32 and keep.dtype == torch.uint8 and keep.numel() >= B * n and keep.is_contiguous()
    _run("rg_dropout", dict(B=B, n=n),
         lambda: L.lib().rg_dropout(L.ptr(x32), _ld(x32), B, n, float(p), int(bool(generate)), int(seed) & (2**64 - 1),
                                    int(offset) & (2**64 - 1), L.ptr(keep), L.ptr(y32), _ld(y32), L.stream_ptr()))

# ---- replay -----------------------------------------------------------------------------------
def replay_nstep(indices, terminal_u8, reward, decays, capacity, horizon, steps, next_indices,
                 out_terminal, out_reward):
    _chk_dev(indices, terminal_u8, reward, decays, steps, next_indices, out_terminal, out_reward)
    _run("rg_replay_nstep", dict(B=indices.numel()),
         lambda: L.lib().rg_replay_nstep(L.ptr(indices), L.ptr(terminal_u8), L.ptr(reward), L.ptr(decays),
                                         capacity, horizon, indices.numel(), L.ptr(steps),
                                         L.ptr(next_indices), L.ptr(out_terminal), L.ptr(out_reward),
                                         L.stream_ptr()))


def replay_gather(cols, capacity: int, stack: int, batch: int):
    """cols: list of (src [C, ...], dst, indices[int64 B][, norm]) tensors; one launch per <=16 columns.
    norm = (col_table_dev, quantiles_dev): normalize-on-gather epilogue (dst dtype fp32 or bf16)."""
    for i in range(0, len(cols), L.MAX_GATHER_COLS):
        chunk = cols[i : i + L.MAX_GATHER_COLS]
        arr = (L.GatherCol * len(chunk))()
        nbytes = 0
        for j, item in enumerate(chunk):
            src, dst, idx = item[:3]
            norm = item[3] if len(item) > 3 else None
            _chk_dev(src, dst, idx)
            assert src.is_contiguous() and dst.is_contiguous() and idx.dtype == torch.int64
            row_elems = 1
            for s in src.shape[1:]:
                row_elems *= s
            arr[j].src = src.data_ptr()
            arr[j].dst = dst.data_ptr()
            arr[j].indices = idx.data_ptr()
            arr[j].row_elems = row_elems
            arr[j].elem_bytes = src.element_size()
            if norm is not None:
                assert src.dtype == F32 and stack == 1
                arr[j].norm = norm[0].data_ptr()
                arr[j].norm_quantiles = norm[1].data_ptr()
                arr[j].out_dtype = dt_code(dst.dtype)
            nbytes += row_elems * (src.element_size() + dst.element_size()) * stack + 8
        _run("rg_replay_gather", dict(B=batch, bytes_per_row=nbytes),
             lambda: L.lib().rg_replay_gather(arr, len(chunk), capacity, stack, batch, L.stream_ptr()))


def sumtree_set(tree, depth: int, capacity: int, indices, values, claim=None):
    """SumTree.set for every (index, value) pair, in order (sum_tree.py:159-189)."""
    _chk_dev(tree, indices, values, claim)
    assert tree.dtype == torch.float64 and values.dtype == torch.float64 and indices.dtype == torch.int64
    _run("rg_sumtree_set", dict(n=indices.numel()),
         lambda: L.lib().rg_sumtree_set(L.ptr(tree), depth, capacity, L.ptr(indices), L.ptr(values), indices.numel(),
                                        L.ptr(claim), L.stream_ptr()))


def sumtree_sample(tree, depth: int, query01, out_indices):
    """SumTree.sample for a batch of query values in [0, 1] (sum_tree.py:97-131)."""
    _chk_dev(tree, query01, out_indices)
    assert tree.dtype == torch.float64 and query01.dtype == torch.float64 and out_indices.dtype == torch.int64
    _run("rg_sumtree_sample", dict(n=query01.numel()),
         lambda: L.lib().rg_sumtree_sample(L.ptr(tree), depth, L.ptr(query01), query01.numel(), L.ptr(out_indices),
                                           L.stream_ptr()))


def sumtree_get(tree, depth: int, capacity: int, indices, out32=None, out64=None):
    _chk_dev(tree, indices, out32, out64)
    assert tree.dtype == torch.float64 and indices.dtype == torch.int64
    _run("rg_sumtree_get", dict(n=indices.numel()),
         lambda: L.lib().rg_sumtree_get(L.ptr(tree), depth, capacity, L.ptr(indices), indices.numel(), L.ptr(out32),
                                        L.ptr(out64), L.stream_ptr()))


def make_dqn_input(action, next_action, terminal, log_prob, num_actions, action_1h, next_action_1h,
                   not_terminal, action_probability=None):
    _chk_dev(action, next_action, terminal, log_prob, action_1h, next_action_1h, not_terminal,
             action_probability)
    _run("rg_make_dqn_input", dict(B=action.numel()),
         lambda: L.lib().rg_make_dqn_input(L.ptr(action), L.ptr(next_action), L.ptr(terminal), L.ptr(log_prob),
                                           action.numel(), num_actions, L.ptr(action_1h), L.ptr(next_action_1h),
                                           L.ptr(not_terminal), L.ptr(action_probability), L.stream_ptr()))


def ragged_gather(ids, scores, lens, indices):
    """(offsets int32 [B], ids int64 [total], scores float32 [total] or None): the sampled rows of a padded-slot ragged
    column back to back (IDListMetadata / IDScoreListMetadata.sample_to_output).  One host read: the total length."""
    _chk_dev(ids, scores, lens, indices)
    B, dev = indices.numel(), ids.device
    offsets = torch.empty(B, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    _run("rg_ragged_offsets", dict(B=B),
         lambda: L.lib().rg_ragged_offsets(L.ptr(lens), L.ptr(indices), B, L.ptr(offsets), L.ptr(total), L.stream_ptr()))
    n = int(total.item())  # the output's length is data dependent, as in the reference
    ids_out = torch.empty(n, dtype=torch.int64, device=dev)
    scores_out = torch.empty(n, dtype=torch.float32, device=dev) if scores is not None else None
    if n:
        _run("rg_ragged_copy", dict(B=B),
             lambda: L.lib().rg_ragged_copy(L.ptr(ids), L.ptr(scores), ids.shape[1], L.ptr(lens), L.ptr(indices), L.ptr(offsets),
                                            B, L.ptr(ids_out), L.ptr(scores_out), L.stream_ptr()))
    return offsets, ids_out, scores_out


def make_policy_input(action, next_action, terminal, log_prob, ranges, action_out, next_action_out, not_terminal,
                      action_probability=None):
    """PolicyNetworkInputMaker's arithmetic in one launch; ranges [4, A] = prev_min, prev_max, new_min, new_max"""
    _chk_dev(action, next_action, terminal, log_prob, ranges, action_out, next_action_out, not_terminal, action_probability)
    B, A = action.shape
    assert action.stride(1) == 1 and next_action.stride(1) == 1 and action_out.is_contiguous() and next_action_out.is_contiguous()
    assert ranges.is_contiguous() and ranges.numel() == 4 * A and terminal.element_size() == 1
    _run("rg_make_policy_input", dict(B=B, A=A),
         lambda: L.lib().rg_make_policy_input(L.ptr(action), action.stride(0), L.ptr(next_action), next_action.stride(0),
                                              L.ptr(terminal), L.ptr(log_prob), L.ptr(ranges), B, A, L.ptr(action_out),
                                              L.ptr(next_action_out), L.ptr(not_terminal), L.ptr(action_probability),
                                              L.stream_ptr()))


def normalize_dense(x, presence_u8, cols_dev, n_out, quantiles, out):
    _chk_dev(x, presence_u8, cols_dev, quantiles, out)
    _run("rg_normalize_dense", dict(B=x.shape[0], n_out=n_out),
         lambda: L.lib().rg_normalize_dense(L.ptr(x), _ld(x), L.ptr(presence_u8),
                                            _ld(presence_u8) if presence_u8 is not None else 0,
                                            L.ptr(cols_dev), n_out, L.ptr(quantiles), L.ptr(out), _ld(out),
                                            x.shape[0], L.stream_ptr()))


def table_dqn_batch(table, indices, cols_dev, n_out, quantiles, out: dict):
    """out: name -> device tensor for every field of rg_dqn_batch_out (a missing name = NULL)"""
    _chk_dev(indices, cols_dev, quantiles, *out.values())
    assert indices.dtype == torch.int64 and indices.is_contiguous()
    o = L.DqnBatchOut()
    for name in L.BATCH_OUT_FIELDS:
        t = out.get(name)
        assert t is None or t.is_contiguous()
        setattr(o, name, t.data_ptr() if t is not None else None)
    o.state_dtype = dt_code(out["state"].dtype)
    assert out["next_state"].dtype == out["state"].dtype
    B = indices.numel()
    _run("rg_table_dqn_batch", dict(B=B, n_out=n_out, F=table.num_features, A=table.num_actions),
         lambda: L.lib().rg_table_dqn_batch(ctypes.byref(table.desc()), L.ptr(indices), B, L.ptr(cols_dev), n_out,
                                            L.ptr(quantiles), ctypes.byref(o), L.stream_ptr()))


class PooledIndices:
    """The indices of a REPLAYED step (runtime._GraphedLoop): row `cursor[0]` (device int64) of `pool` [rows, batch]; the
    sampler launch also counts the step in the device-resident Adam schedule `sched` (nullable), the step's one-launch update
    advances the cursor (rg_replay_dqn_batch_pooled / rg_mlp_update_desc.sched_pre_ticked, post_tick)."""

    def __init__(self, pool, cursor, sched=None):
        assert pool.dtype == torch.int64 and pool.dim() == 2 and pool.is_contiguous() and cursor.dtype == torch.int64
        self.pool, self.cursor, self.sched = pool, cursor, sched

    def numel(self):
        return self.pool.shape[1]


def replay_dqn_batch(view: "L.ReplayView", indices, cols_dev, quantiles, out: dict) -> bool:
    """one-launch sample + input maker (+ normalize); False = shape not supported by the fused kernel"""
    pooled = indices if isinstance(indices, PooledIndices) else None
    if pooled is not None:
        _chk_dev(pooled.pool, pooled.cursor, pooled.sched, cols_dev, quantiles, *out.values())
    else:
        _chk_dev(indices, cols_dev, quantiles, *out.values())
        assert indices.dtype == torch.int64 and indices.is_contiguous()
    o = L.DqnBatchOut()
    for name in L.BATCH_OUT_FIELDS:
        t = out.get(name)
        assert t is None or t.is_contiguous()
        setattr(o, name, t.data_ptr() if t is not None else None)
    o.state_dtype = dt_code(out["state"].dtype)
    B = indices.numel()
    rc = [0]

    def call():
        if pooled is not None:
            rc[0] = L.lib().rg_replay_dqn_batch_pooled(ctypes.byref(view), pooled.pool.data_ptr(), pooled.cursor.data_ptr(),
                                                       L.ptr(pooled.sched), B, L.ptr(cols_dev), L.ptr(quantiles),
                                                       ctypes.byref(o), L.stream_ptr())
        else:
            rc[0] = L.lib().rg_replay_dqn_batch(ctypes.byref(view), L.ptr(indices), B, L.ptr(cols_dev), L.ptr(quantiles),
                                                ctypes.byref(o), L.stream_ptr())
        return 0 if rc[0] == L.EUNSUPPORTED else rc[0]

    F_, A_, H_ = view.n_features, view.n_actions, view.update_horizon
    es = out["state"].element_size()
    # algorithmic bytes per transition: rows in (2 F fp32) and out (2 F), n-step window, action / log_prob /
    # index reads, masks in (if stored) and out, one-hots and scalars out
    nbytes = (2 * F_ * 4 + 2 * F_ * es + 5 * H_ + 2 * 8 + 4 + 8 + (2 * A_ * 4 if view.possible_actions_mask else 0)
              + 4 * A_ * 4 + 3 * 4)
    _run("rg_replay_dqn_batch", dict(B=B, bytes_per_row=nbytes), call)
    return rc[0] == 0


def replay_policy_batch(view: "L.PolicyReplayView", indices, cols_dev, quantiles, out: dict) -> bool:
    """one-launch sample + PolicyNetworkInputMaker (+ normalize) — rg_replay_policy_batch; False = shape not supported by the
    fused kernel (the caller takes rg_replay_nstep + rg_replay_gather + rg_make_policy_input)"""
    _chk_dev(indices, cols_dev, quantiles, *out.values())
    assert indices.dtype == torch.int64 and indices.is_contiguous()
    o = L.PolicyBatchOut()
    for name in L.POLICY_OUT_FIELDS:
        t = out.get(name)
        assert t is None or t.is_contiguous()
        setattr(o, name, t.data_ptr() if t is not None else None)
    o.state_dtype = dt_code(out["state"].dtype)
    B = indices.numel()
    rc = [0]

    def call():
        rc[0] = L.lib().rg_replay_policy_batch(ctypes.byref(view), L.ptr(indices), B, L.ptr(cols_dev), L.ptr(quantiles),
                                               ctypes.byref(o), L.stream_ptr())
        return 0 if rc[0] == L.EUNSUPPORTED else rc[0]

    F_, A_, H_ = view.n_features, view.action_dim, view.update_horizon
    es = out["state"].element_size()
    # algorithmic bytes per transition: state rows in (2 F fp32) and out (2 F), action rows in and out (4 A fp32), the n-step
    # window (terminal byte + reward per slot), index, log_prob, three scalars out
    nbytes = 2 * F_ * 4 + 2 * F_ * es + 4 * A_ * 4 + 5 * H_ + 8 + 4 + 3 * 4
    _run("rg_replay_policy_batch", dict(B=B, bytes_per_row=nbytes), call)
    return rc[0] == 0


def table_check_actions(table, indices) -> int:
    _chk_dev(indices)
    flag = torch.zeros(1, dtype=torch.int32, device=indices.device)
    _run("rg_table_check_actions", dict(B=indices.numel()),
         lambda: L.lib().rg_table_check_actions(ctypes.byref(table.desc()), L.ptr(indices), indices.numel(),
                                                L.ptr(flag), L.stream_ptr()))
    return int(flag.item())


# ---- heads ------------------------------------------------------------------------------------
def bcq_filter(imitator_logits, drop_threshold: float, mask):
    """mask *= (softmax(logits) / rowmax >= drop_threshold), in place"""
    _chk_dev(imitator_logits, mask)
    B, A = mask.shape
    assert imitator_logits.shape == (B, A) and imitator_logits.dtype == F32 and mask.dtype == F32
    assert imitator_logits.is_contiguous() and mask.is_contiguous()
    _run("rg_bcq_filter", dict(B=B, A=A),
         lambda: L.lib().rg_bcq_filter(L.ptr(imitator_logits), B, A, float(drop_threshold), L.ptr(mask), L.stream_ptr()))


def dqn_head_partials(batch: int) -> int:
    return int(L.lib().rg_dqn_head_partials(batch))


def dqn_pair_wave_sums(batch: int) -> int:
    return int(L.lib().rg_dqn_pair_wave_sums(batch))


DQN_PAIR_RUN = 16  # wave sums per loss partial of dqn_head (256 rows, 16 rows per wave at 16 actions)


def dqn_head(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma,
             gamma_exponent, double_q, loss_type, dq, loss_partials, next_q=None, next_idx=None,
             q_sel=None):
    _chk_dev(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal,
             gamma_exponent, dq, loss_partials, next_q, next_idx, q_sel)
    batch, A = q.shape
    for t in (q, qn_online, qn_target, action, next_mask, dq):
        assert t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A)
    for t in (reward, not_terminal, gamma_exponent):
        assert t is None or (t.is_contiguous() and t.dtype == F32 and t.numel() == batch)
    _run("rg_dqn_head", dict(B=batch, A=A),
         lambda: L.lib().rg_dqn_head(L.ptr(q), L.ptr(qn_online), L.ptr(qn_target), L.ptr(action),
                                     L.ptr(next_mask), L.ptr(reward), L.ptr(reward_boosts),
                                     L.ptr(not_terminal), float(gamma), L.ptr(gamma_exponent), batch, A,
                                     int(double_q), loss_type, L.ptr(dq), L.ptr(loss_partials), L.ptr(next_q),
                                     L.ptr(next_idx), L.ptr(q_sel), L.stream_ptr()))


def pdqn_head_partials(batch: int) -> int:
    return int(L.lib().rg_pdqn_head_partials(batch))


def pdqn_head(q, qn_online_all, qn_target_all, next_mask, reward, not_terminal, gamma, gamma_exponent, double_q, loss_type,
              target, dq, loss_partials, next_q, next_idx=None):
    """next_mask given: maxq learning over next_mask.shape[1] candidates per state (qn_*_all hold B * M values; the online
    values are read with double_q only); next_mask None: SARSA, qn_target_all holds the B values of the logged next action"""
    _chk_dev(q, qn_online_all, qn_target_all, next_mask, reward, not_terminal, gamma_exponent, target, dq, loss_partials,
             next_q, next_idx)
    B = q.numel()
    maxq = next_mask is not None
    M = next_mask.shape[1] if maxq else 1
    if maxq:
        assert next_mask.is_contiguous() and next_mask.dtype == F32 and next_mask.shape == (B, M)
        assert double_q is False or qn_online_all is not None
    for t, n in ((q, B), (qn_online_all, B * M), (qn_target_all, B * M), (reward, B), (not_terminal, B), (gamma_exponent, B),
                 (target, B), (dq, B), (next_q, B)):
        assert t is None or (t.is_contiguous() and t.dtype == F32 and t.numel() == n)
    assert next_idx is None or (next_idx.is_contiguous() and next_idx.dtype == torch.int64 and next_idx.numel() == B)
    assert loss_partials.dtype == F32 and loss_partials.numel() >= pdqn_head_partials(B)
    _run("rg_pdqn_head", dict(B=B, M=M),
         lambda: L.lib().rg_pdqn_head(L.ptr(q), L.ptr(qn_online_all) if maxq else None, L.ptr(qn_target_all),
                                      L.ptr(next_mask), L.ptr(reward), L.ptr(not_terminal), float(gamma),
                                      L.ptr(gamma_exponent), B, M, int(maxq), int(bool(double_q)), loss_type, L.ptr(target),
                                      L.ptr(dq), L.ptr(loss_partials), L.ptr(next_q), L.ptr(next_idx), L.stream_ptr()))


def _u8(t):
    """a bool / uint8 tensor as its bytes (torch.bool storage is one byte per entry)"""
    if t is None:
        return None
    assert t.dtype in (torch.bool, torch.uint8) and t.is_contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def slate_gather(features, mask, value, index, out_features, out_weight, not_terminal=None, count_mask=None, count_out=None):
    """out_features[b * K + k] = features[b, index[b, k]] (a [B * K, D] view, e.g. of a wider workspace), out_weight[b, k] =
    (value * mask)[b, index[b, k]]; rows with not_terminal == 0 read document 0 (index is left as it is).  out_features None:
    the weights alone.  count_mask with count_out (int32 [1]): the launch also counts count_mask's true entries into count_out"""
    _chk_dev(features, mask, value, index, out_features, out_weight, not_terminal, count_mask, count_out)
    B, C, D = features.shape
    K = index.shape[1]
    assert features.dtype == value.dtype == out_weight.dtype == F32
    assert features.is_contiguous() and value.is_contiguous() and value.shape == (B, C) and mask.shape == (B, C)
    assert index.dtype == torch.int64 and index.is_contiguous() and index.shape == (B, K)
    assert out_features is None or (out_features.dtype == F32 and out_features.shape == (B * K, D))
    assert out_weight.is_contiguous() and out_weight.numel() == B * K
    assert not_terminal is None or (not_terminal.dtype == F32 and not_terminal.is_contiguous() and not_terminal.numel() == B)
    assert (count_mask is None) == (count_out is None)
    assert count_out is None or (count_out.dtype == torch.int32 and count_out.numel() >= 1)
    m, cm = _u8(mask), _u8(count_mask)
    _run("rg_slate_gather", dict(B=B, C=C, K=K, D=D),
         lambda: L.lib().rg_slate_gather(L.ptr(features), L.ptr(m), L.ptr(value), L.ptr(index), L.ptr(not_terminal), B, C, K, D,
                                         L.ptr(out_features), _ld(out_features) if out_features is not None else 0,
                                         L.ptr(out_weight), L.ptr(cm),
                                         cm.numel() if cm is not None else 0, L.ptr(count_out), L.stream_ptr()))


def slate_topk(q_all, value, mask, single_selection: bool, next_index, q_sel):
    """next_index [B, K] = the K candidates with the largest q_all * (value * mask, or its softmax over the candidates with
    single_selection), descending, the lower index first among equal scores; q_sel = q_all at them"""
    _chk_dev(q_all, value, mask, next_index, q_sel)
    B, C = value.shape
    K = next_index.shape[1]
    assert q_all.dtype == value.dtype == q_sel.dtype == F32 and next_index.dtype == torch.int64
    assert q_all.is_contiguous() and q_all.numel() == B * C and value.is_contiguous() and mask.shape == (B, C)
    assert next_index.is_contiguous() and next_index.shape == (B, K) and q_sel.is_contiguous() and q_sel.numel() == B * K
    m = _u8(mask)
    _run("rg_slate_topk", dict(B=B, C=C, K=K),
         lambda: L.lib().rg_slate_topk(L.ptr(q_all), L.ptr(value), L.ptr(m), B, C, K, int(bool(single_selection)),
                                       L.ptr(next_index), L.ptr(q_sel), L.stream_ptr()))


def slateq_head_partials(batch: int) -> int:
    return int(L.lib().rg_slateq_head_partials(batch))


def slateq_head(q, qn, wn, reward, reward_mask, not_terminal, gamma, time_diff, discount_time_scale, single_selection: bool,
                norm_mask, slate_size, n_selected, target, dq, loss_partials, next_q):
    """the SlateQ TD head over [B, K] items; time_diff None: the discount is gamma.  single_selection reads reward_mask and
    the device count n_selected (int32 [1]), otherwise norm_mask [B, C] and slate_size form the divisor.  The ordered sum of
    loss_partials is the loss"""
    _chk_dev(q, qn, wn, reward, reward_mask, not_terminal, time_diff, norm_mask, n_selected, target, dq, loss_partials, next_q)
    B, K = reward.shape
    for t, n in ((q, B * K), (qn, B * K), (wn, B * K), (reward, B * K), (not_terminal, B), (time_diff, B), (target, B * K),
                 (dq, B * K), (next_q, B)):
        assert t is None or (t.is_contiguous() and t.dtype == F32 and t.numel() == n)
    assert reward_mask is None or reward_mask.shape == (B, K)
    assert norm_mask is None or (norm_mask.dim() == 2 and norm_mask.shape[0] == B)
    assert n_selected is None or n_selected.dtype == torch.int32
    assert loss_partials.dtype == F32 and loss_partials.numel() >= slateq_head_partials(B)
    rm, nm = _u8(reward_mask), _u8(norm_mask)
    C = norm_mask.shape[1] if norm_mask is not None else 0
    _run("rg_slateq_head", dict(B=B, K=K),
         lambda: L.lib().rg_slateq_head(L.ptr(q), L.ptr(qn), L.ptr(wn), L.ptr(reward), L.ptr(rm), L.ptr(not_terminal),
                                        float(gamma), L.ptr(time_diff), float(discount_time_scale or 0.0),
                                        int(bool(single_selection)), L.ptr(nm), C, int(slate_size), L.ptr(n_selected), B, K,
                                        L.ptr(target), L.ptr(dq), L.ptr(loss_partials), L.ptr(next_q), L.stream_ptr()))


def pg_returns(reward, offsets, gamma, reward_clip, normalize: bool, subtract_mean: bool, clamp_min: bool, out):
    """out [N] = per packed trajectory [offsets[t], offsets[t + 1]) the discounted reward-to-go of clamp(reward, max =
    reward_clip), whitened (normalize) or mean-subtracted (subtract_mean alone), clamped at 0 from below (clamp_min).
    offsets: int32 [T + 1] on the device, ascending, offsets[T] = N"""
    _chk_dev(reward, offsets, out)
    N, T = reward.numel(), offsets.numel() - 1
    assert reward.dtype == out.dtype == F32 and reward.is_contiguous() and out.is_contiguous() and out.numel() >= N
    assert offsets.dtype == torch.int32 and offsets.is_contiguous()
    _run("rg_pg_returns", dict(N=N, T=T),
         lambda: L.lib().rg_pg_returns(L.ptr(reward), L.ptr(offsets), T, N, float(gamma), float(reward_clip),
                                       int(bool(normalize)), int(bool(subtract_mean)), int(bool(clamp_min)), L.ptr(out),
                                       L.stream_ptr()))


def pg_head_partials(n: int, num_actions: int) -> int:
    return int(L.lib().rg_pg_head_partials(n, num_actions))


def pg_head(scores, action, returns, values, old_log_prob, temperature, mode: int, clip, entropy_weight, value_scale, dscores,
            dvalues, log_prob, ratio, advantage, policy_partials, value_partials, possible_actions_mask=None):
    """the categorical policy head over [N, A] scores (see rg_pg_head): mode is L.PG_REINFORCE / PG_REINFORCE_OFF_POLICY
    (clip = clip_param) / PG_PPO (clip = ppo_epsilon); action a one-hot in fp32 or int64; possible_actions_mask [N, A] fp32
    where the scores do not carry the -1e10 penalty yet.  The ordered sums of the partials are the two summed losses"""
    _chk_dev(scores, action, returns, values, old_log_prob, dscores, dvalues, log_prob, ratio, advantage, policy_partials,
             value_partials, possible_actions_mask)
    N, A = scores.shape
    assert scores.dtype == dscores.dtype == F32 and dscores.shape == (N, A) and action.shape == (N, A)
    assert action.dtype in (F32, torch.int64) and action.stride(1) == 1
    for t in (returns, values, old_log_prob, dvalues, log_prob, ratio, advantage):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.numel() == N)
    P = pg_head_partials(N, A)
    assert policy_partials.dtype == F32 and policy_partials.numel() >= P
    assert value_partials is None or (value_partials.dtype == F32 and value_partials.numel() >= P)
    m = possible_actions_mask
    assert m is None or (m.dtype == F32 and m.is_contiguous() and m.shape == (N, A))
    _run("rg_pg_head", dict(N=N, A=A, mode=mode),
         lambda: L.lib().rg_pg_head(L.ptr(scores), _ld(scores), L.ptr(m), L.ptr(action), int(action.dtype == torch.int64),
                                    _ld(action), L.ptr(returns), L.ptr(values), L.ptr(old_log_prob), float(temperature),
                                    int(mode), float(clip), float(entropy_weight), float(value_scale), N, A, L.ptr(dscores),
                                    _ld(dscores), L.ptr(dvalues), L.ptr(log_prob), L.ptr(ratio), L.ptr(advantage),
                                    L.ptr(policy_partials), L.ptr(value_partials), L.stream_ptr()))


# ---- world model (MDN-RNN) --------------------------------------------------------------------------------------
def _lstm_check(T, B, H):
    if H > L.LSTM_MAX_HIDDEN:
        raise NotImplementedError(f"LSTM kernels: hidden size {H} is not supported (1 .. {L.LSTM_MAX_HIDDEN})")
    if T * B >= 1 << 29:
        raise NotImplementedError(f"LSTM kernels: seq_len * batch = {T * B} is not supported (below 2^29)")
    assert T >= 1 and B >= 1 and H >= 1


def _f32_flat(t, numel):
    assert t is None or (t.dtype == F32 and t.is_contiguous() and t.numel() == numel), "expected a contiguous fp32 tensor"


def lstm_forward(xproj, w_hh, b_hh, h0, c0, h_all, c_all, gates=None):
    """one LSTM layer over the whole sequence (see rg_lstm_forward): xproj [T, B, 4H] = x @ W_ih.T + b_ih, w_hh [4H, H];
    b_hh, h0, c0 may be None (zeros); gates=None saves nothing for a backward"""
    _chk_dev(xproj, w_hh, b_hh, h0, c0, h_all, c_all, gates)
    T, B, H4 = xproj.shape
    H = H4 // 4
    _lstm_check(T, B, H)
    assert H4 == 4 * H and w_hh.shape == (4 * H, H)
    _f32_flat(xproj, T * B * 4 * H), _f32_flat(w_hh, 4 * H * H), _f32_flat(b_hh, 4 * H), _f32_flat(gates, T * B * 4 * H)
    _f32_flat(h0, B * H), _f32_flat(c0, B * H), _f32_flat(h_all, T * B * H), _f32_flat(c_all, T * B * H)
    _run("rg_lstm_forward", dict(T=T, B=B, H=H, save=gates is not None),
         lambda: L.lib().rg_lstm_forward(L.ptr(xproj), L.ptr(w_hh), L.ptr(b_hh), L.ptr(h0), L.ptr(c0), T, B, H, L.ptr(h_all),
                                         L.ptr(c_all), L.ptr(gates), L.stream_ptr()))


def lstm_backward(dh_all, gates, c_all, c0, w_hh, dgates, dh0=None, dc0=None):
    """the layer's backward (see rg_lstm_backward): dgates [T, B, 4H] = d loss / d pre-activation, dh0 / dc0 [B, H]"""
    _chk_dev(dh_all, gates, c_all, c0, w_hh, dgates, dh0, dc0)
    T, B, H = dh_all.shape
    _lstm_check(T, B, H)
    assert w_hh.shape == (4 * H, H)
    _f32_flat(dh_all, T * B * H), _f32_flat(c_all, T * B * H), _f32_flat(gates, T * B * 4 * H), _f32_flat(dgates, T * B * 4 * H)
    _f32_flat(w_hh, 4 * H * H), _f32_flat(c0, B * H), _f32_flat(dh0, B * H), _f32_flat(dc0, B * H)
    _run("rg_lstm_backward", dict(T=T, B=B, H=H),
         lambda: L.lib().rg_lstm_backward(L.ptr(dh_all), L.ptr(gates), L.ptr(c_all), L.ptr(c0), L.ptr(w_hh), T, B, H,
                                          L.ptr(dgates), L.ptr(dh0), L.ptr(dc0), L.stream_ptr()))


def _mdn_check(G, S):
    if G > L.MDN_MAX_GAUSSIANS:
        raise NotImplementedError(f"mixture-density head: {G} gaussians are not supported (1 .. {L.MDN_MAX_GAUSSIANS})")
    if S > L.MDN_MAX_STATE_DIM:
        raise NotImplementedError(f"mixture-density head: state_dim {S} is not supported (1 .. {L.MDN_MAX_STATE_DIM})")
    assert G >= 1 and S >= 1


def mdn_head_partials(n: int) -> int:
    return int(L.lib().rg_mdn_head_partials(n))


def mdn_head(z, next_state, reward, not_terminal, num_gaussians: int, weights, divide_by_state_dim: bool, first_row: int, dz,
             partials, losses, sigmas=None, logpi=None):
    """the mixture-density head over z [N, (2S + 1) G + 2] (see rg_mdn_head): weights = (next_state, not_terminal, reward)
    loss weights; losses [4] = gmm, bce, mse, loss; partials: float64 [3 * mdn_head_partials(N)]"""
    _chk_dev(z, next_state, reward, not_terminal, dz, partials, losses, sigmas, logpi)
    N, S = next_state.shape
    G = int(num_gaussians)
    _mdn_check(G, S)
    width = (2 * S + 1) * G + 2
    assert z.dtype == dz.dtype == F32 and z.shape == (N, width) == dz.shape and 0 <= first_row < N
    _f32_flat(next_state, N * S), _f32_flat(reward, N), _f32_flat(not_terminal, N), _f32_flat(losses, 4)
    _f32_flat(sigmas, N * G * S), _f32_flat(logpi, N * G)
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 3 * mdn_head_partials(N)
    w = [float(x) for x in weights]
    _run("rg_mdn_head", dict(N=N, G=G, S=S),
         lambda: L.lib().rg_mdn_head(L.ptr(z), _ld(z), L.ptr(next_state), L.ptr(reward), L.ptr(not_terminal), w[0], w[1], w[2],
                                     int(bool(divide_by_state_dim)), int(first_row), N, G, S, L.ptr(dz), _ld(dz),
                                     L.ptr(sigmas), L.ptr(logpi), L.ptr(partials), L.ptr(losses), L.stream_ptr()))


def mdn_outputs(z, num_gaussians: int, state_dim: int, sigmas, logpi):
    """sigmas [N, G, S] = exp(z's log sigmas), logpi [N, G] = log_softmax(z's mixture logits) (see rg_mdn_outputs)"""
    _chk_dev(z, sigmas, logpi)
    N, G, S = z.shape[0], int(num_gaussians), int(state_dim)
    _mdn_check(G, S)
    assert z.dtype == F32 and z.shape == (N, (2 * S + 1) * G + 2)
    _f32_flat(sigmas, N * G * S), _f32_flat(logpi, N * G)
    _run("rg_mdn_outputs", dict(N=N, G=G, S=S),
         lambda: L.lib().rg_mdn_outputs(L.ptr(z), _ld(z), N, G, S, L.ptr(sigmas), L.ptr(logpi), L.stream_ptr()))


def mdn_gmm_nll(batch, mus, sigmas, logpi, nll):
    """nll [N] = gmm_loss(batch [N, S], mus [N, G, S], sigmas [N, G, S], logpi [N, G], reduce=False)"""
    _chk_dev(batch, mus, sigmas, logpi, nll)
    N, G, S = mus.shape
    _mdn_check(G, S)
    _f32_flat(batch, N * S), _f32_flat(mus, N * G * S), _f32_flat(sigmas, N * G * S), _f32_flat(logpi, N * G), _f32_flat(nll, N)
    _run("rg_mdn_gmm_nll", dict(N=N, G=G, S=S),
         lambda: L.lib().rg_mdn_gmm_nll(L.ptr(batch), L.ptr(mus), L.ptr(sigmas), L.ptr(logpi), N, G, S, L.ptr(nll),
                                        L.stream_ptr()))


# ---- world model (Seq2Reward) -----------------------------------------------------------------------------------
def lstm_fanout_step(h_prev, c_prev, proj, from_table: bool, w_hh, b_hh, fanout: int, h, c):
    """one LSTM layer's single step over the parents * fanout children of a prefix-tree level (see rg_lstm_fanout_step): child
    r continues row r // fanout of h_prev / c_prev [parents, H] (c_prev None: zeros); its input projection is row r %
    proj.shape[0] of proj (from_table) or row r of proj [parents * fanout, 4H]"""
    _chk_dev(h_prev, c_prev, proj, w_hh, b_hh, h, c)
    parents, H = h_prev.shape
    n = parents * int(fanout)
    if H > L.LSTM_MAX_HIDDEN:
        raise NotImplementedError(f"LSTM kernels: hidden size {H} is not supported (1 .. {L.LSTM_MAX_HIDDEN})")
    if n >= 1 << 29:
        raise NotImplementedError(f"LSTM kernels: {n} child rows are not supported (below 2^29)")
    assert parents >= 1 and fanout >= 1 and H >= 1 and w_hh.shape == (4 * H, H) and proj.shape[1] == 4 * H
    assert from_table or proj.shape[0] == n
    _f32_flat(h_prev, parents * H), _f32_flat(c_prev, parents * H), _f32_flat(proj, proj.shape[0] * 4 * H)
    _f32_flat(w_hh, 4 * H * H), _f32_flat(b_hh, 4 * H), _f32_flat(h, n * H), _f32_flat(c, n * H)
    _run("rg_lstm_fanout_step", dict(N=n, H=H, fanout=int(fanout), table=bool(from_table)),
         lambda: L.lib().rg_lstm_fanout_step(L.ptr(h_prev), L.ptr(c_prev), L.ptr(proj), proj.shape[0] if from_table else 0,
                                             L.ptr(w_hh), L.ptr(b_hh), parents, int(fanout), H, L.ptr(h), L.ptr(c),
                                             L.stream_ptr()))


def seq2reward_plan_max(h, w, bias, group_size: int, q):
    """q [groups] = max over each group of group_size consecutive rows of h [groups * group_size, H] of h @ w + bias (see
    rg_seq2reward_plan_max); w [H] and bias [1] are lstm_linear's"""
    _chk_dev(h, w, bias, q)
    n, H = h.shape
    groups = n // int(group_size)
    if n >= 1 << 29:
        raise NotImplementedError(f"seq2reward_plan_max: {n} leaf rows are not supported (below 2^29)")
    assert groups >= 1 and groups * group_size == n
    _f32_flat(h, n * H), _f32_flat(w, H), _f32_flat(bias, 1), _f32_flat(q, groups)
    _run("rg_seq2reward_plan_max", dict(groups=groups, size=int(group_size), H=H),
         lambda: L.lib().rg_seq2reward_plan_max(L.ptr(h), L.ptr(w), L.ptr(bias), groups, int(group_size), H, L.ptr(q),
                                                L.stream_ptr()))


def seq2reward_head_partials(batch: int) -> int:
    return int(L.lib().rg_seq2reward_head_partials(batch))


def seq2reward_head(h_all, valid_step, reward, gamma_pow, w, bias, acc_reward, dh_all=None, dw=None, dbias=None, partials=None,
                    loss=None):
    """lstm_linear at each row's valid step, the discounted target, the mse loss and its gradients (see rg_seq2reward_head);
    valid_step [B] int64 is clamped into [1, T] by the kernel (None: the last step); dh_all=None: acc_reward alone"""
    _chk_dev(h_all, valid_step, reward, gamma_pow, w, bias, acc_reward, dh_all, dw, dbias, partials, loss)
    T, B, H = h_all.shape
    if T * B >= 1 << 29:
        raise NotImplementedError(f"seq2reward_head: seq_len * batch = {T * B} is not supported (below 2^29)")
    _f32_flat(h_all, T * B * H), _f32_flat(w, H), _f32_flat(bias, 1), _f32_flat(acc_reward, B)
    if valid_step is not None:
        assert valid_step.dtype == torch.int64 and valid_step.is_contiguous() and valid_step.numel() == B
    if dh_all is not None:
        assert reward is not None and gamma_pow is not None and dw is not None and dbias is not None and loss is not None
        _f32_flat(reward, T * B), _f32_flat(gamma_pow, T), _f32_flat(dh_all, T * B * H), _f32_flat(dw, H), _f32_flat(dbias, 1)
        _f32_flat(loss, 1)
        assert partials.dtype == torch.float64 and partials.is_contiguous()
        assert partials.numel() >= (H + 2) * seq2reward_head_partials(B)
    _run("rg_seq2reward_head", dict(T=T, B=B, H=H, train=dh_all is not None),
         lambda: L.lib().rg_seq2reward_head(L.ptr(h_all), L.ptr(valid_step), L.ptr(reward), L.ptr(gamma_pow), L.ptr(w),
                                            L.ptr(bias), T, B, H, L.ptr(acc_reward), L.ptr(dh_all), L.ptr(dw), L.ptr(dbias),
                                            L.ptr(partials), L.ptr(loss), L.stream_ptr()))


def step_ce_head_partials(batch: int) -> int:
    return int(L.lib().rg_step_ce_head_partials(batch))


def step_ce_head(logits, valid_step, dlogits=None, softmax=None, partials=None, loss=None):
    """mean cross-entropy of logits [B, K] against valid_step - 1 (clamped into [0, K - 1]), d loss / d logits and (optional)
    the softmax (see rg_step_ce_head); valid_step=None: the softmax alone"""
    _chk_dev(logits, valid_step, dlogits, softmax, partials, loss)
    B, K = logits.shape
    if K > L.STEP_CE_MAX_CLASSES:
        raise NotImplementedError(f"step_ce_head: {K} classes are not supported (1 .. {L.STEP_CE_MAX_CLASSES})")
    _f32_flat(logits, B * K), _f32_flat(dlogits, B * K), _f32_flat(softmax, B * K), _f32_flat(loss, 1)
    if valid_step is not None:
        assert valid_step.dtype == torch.int64 and valid_step.is_contiguous() and valid_step.numel() == B
        assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= step_ce_head_partials(B)
    _run("rg_step_ce_head", dict(B=B, K=K, train=valid_step is not None),
         lambda: L.lib().rg_step_ce_head(L.ptr(logits), L.ptr(valid_step), B, K, L.ptr(dlogits), L.ptr(softmax),
                                         L.ptr(partials), L.ptr(loss), L.stream_ptr()))


# ---- world model (the CEM planner) ---------------------------------------------------------------------------------
def _typed_flat(t, dtype, numel, what):
    assert t is None or (t.dtype == dtype and t.is_contiguous() and t.numel() == numel), f"{what}: expected {numel} contiguous {dtype}"


def _cem_count_check(n: int, horizon: int = 1):
    if n >= L.CEM_MAX_TRAJECTORIES:
        raise NotImplementedError(f"CEM kernels: {n} trajectories are not supported (population * ensemble below 2^20)")
    if horizon > L.CEM_MAX_HORIZON:
        raise NotImplementedError(f"CEM kernels: plan_horizon_length {horizon} is not supported (1 .. {L.CEM_MAX_HORIZON})")


def cem_fill_noise(seed: int, iteration: int, u_model, u_mix, eps, u_term):
    """the noise rg_cem_group and rg_cem_rollout would draw in place for (seed, iteration) (see rg_cem_fill_noise): u_model
    [N], u_mix [T, N], eps [T, N, S], u_term [T, N]"""
    _chk_dev(u_model, u_mix, eps, u_term)
    T, N, S = eps.shape
    _cem_count_check(N, T)
    _f32_flat(u_model, N), _f32_flat(u_mix, T * N), _f32_flat(eps, T * N * S), _f32_flat(u_term, T * N)
    _run("rg_cem_fill_noise", dict(N=N, T=T, S=S),
         lambda: L.lib().rg_cem_fill_noise(int(seed), int(iteration), N, T, S, L.ptr(u_model), L.ptr(u_mix), L.ptr(eps),
                                           L.ptr(u_term), L.stream_ptr()))


def cem_rollout_tiles(trajectories: int, models: int) -> int:
    return int(L.lib().rg_cem_rollout_tiles(int(trajectories), int(models)))


def cem_rollout_lds_bytes(state_dim: int, action_dim: int, hidden: int) -> int:
    return int(L.lib().rg_cem_rollout_lds_bytes(int(state_dim), int(action_dim), int(hidden)))


def cem_group(u_model, seed: int, iteration: int, trajectories: int, models: int, done, rowmap, tile_model):
    """the trajectories sorted by their world model into tiles of 32 (see rg_cem_group); u_model None: drawn in place"""
    _chk_dev(u_model, done, rowmap, tile_model)
    N, M = int(trajectories), int(models)
    _cem_count_check(N)
    if not 1 <= M <= L.CEM_MAX_MODELS:
        raise NotImplementedError(f"CEM kernels: {M} world models are not supported (1 .. {L.CEM_MAX_MODELS})")
    tiles = cem_rollout_tiles(N, M)
    _f32_flat(u_model, N)
    _typed_flat(rowmap, torch.int32, tiles * 32, "rowmap"), _typed_flat(tile_model, torch.int32, tiles, "tile_model")
    assert done is None or done.dtype == torch.float64
    _run("rg_cem_group", dict(N=N, M=M),
         lambda: L.lib().rg_cem_group(L.ptr(u_model), int(seed), int(iteration), N, M, L.ptr(done), L.ptr(rowmap),
                                      L.ptr(tile_model), L.stream_ptr()))


def cem_rollout(table, rowmap, tile_model, init_state, solutions, action_idx, gamma_pow, action_dim: int, num_gaussians: int,
                hidden: int, terminal_effective: bool, ensemble: int, out, *, traj=None, u_mix=None, eps=None, u_term=None, seed: int = 0,
                iteration: int = 0, done=None, trace=None):
    """accumulated rewards of every solution (see rg_cem_rollout).  table [M, 3 L + 2] int64 holds the members' parameter
    pointers; solutions [P, T, A] fp32 or action_idx [P, T] int32; trace: None or [T, N, S + W + 2] fp32 (per step and
    trajectory the entry state, the z row, the sampled index, not_terminal)"""
    _chk_dev(table, rowmap, tile_model, init_state, solutions, action_idx, gamma_pow, out, traj, u_mix, eps, u_term, done, trace)
    assert (solutions is None) != (action_idx is None), "one of solutions and action_idx"
    M, cols = table.shape
    layers = (cols - 2) // 3
    S = init_state.numel()
    if solutions is not None:
        P, T, A = solutions.shape
        assert A == int(action_dim), (solutions.shape, action_dim)
        _f32_flat(solutions, P * T * A)
    else:
        P, T = action_idx.shape
        A = int(action_dim)
        _typed_flat(action_idx, torch.int32, P * T, "action_idx")
    E = int(ensemble)
    N = P * E
    _cem_count_check(N, T)
    G, H = int(num_gaussians), int(hidden)
    W = (2 * S + 1) * G + 2
    if H > L.LSTM_MAX_HIDDEN or layers > L.LSTM_MAX_LAYERS or G > L.MDN_MAX_GAUSSIANS or S + A > L.CEM_MAX_INPUT:
        raise NotImplementedError(f"rg_cem_rollout: hidden {H}, layers {layers}, gaussians {G}, state_dim + action_dim {S + A} are not "
                       f"supported (at most {L.LSTM_MAX_HIDDEN}, {L.LSTM_MAX_LAYERS}, {L.MDN_MAX_GAUSSIANS}, {L.CEM_MAX_INPUT})")
    tiles = cem_rollout_tiles(N, M)
    assert table.dtype == torch.int64 and table.is_contiguous() and cols == 3 * layers + 2 and layers >= 1
    _typed_flat(rowmap, torch.int32, tiles * 32, "rowmap"), _typed_flat(tile_model, torch.int32, tiles, "tile_model")
    _f32_flat(init_state, S), _f32_flat(gamma_pow, T), _f32_flat(u_mix, T * N), _f32_flat(eps, T * N * S), _f32_flat(u_term, T * N)
    _typed_flat(out, torch.float64, P, "out"), _typed_flat(traj, torch.float64, N, "traj")
    assert E == 1 or traj is not None, "ensemble > 1 needs the per-trajectory workspace"
    assert done is None or done.dtype == torch.float64
    _f32_flat(trace, T * N * (S + W + 2))
    _run("rg_cem_rollout", dict(P=P, E=E, T=T, S=S, A=A, G=G, H=H, L=layers, M=M),
         lambda: L.lib().rg_cem_rollout(L.ptr(table), M, L.ptr(rowmap), L.ptr(tile_model), tiles, L.ptr(init_state),
                                        L.ptr(solutions), L.ptr(action_idx), L.ptr(gamma_pow), L.ptr(u_mix), L.ptr(eps),
                                        L.ptr(u_term), int(seed), int(iteration), L.ptr(done), P, E, T, S, A, G, H, layers,
                                        1 if terminal_effective else 0, L.ptr(traj), L.ptr(out), L.ptr(trace), L.stream_ptr()))


def cem_sample(planner_state, lower, upper, seed: int, iteration: int, solutions, solutions_f32, tn=None):
    """solutions [P, D] = tn * sqrt(constrained_variance(mean, var)) + mean and their fp32 copy (see rg_cem_sample);
    planner_state [2 D + 2] float64; tn [P, D] float64 replaces the truncated-normal draw"""
    _chk_dev(planner_state, lower, upper, solutions, solutions_f32, tn)
    P, D = solutions.shape
    _cem_count_check(P)
    f64 = torch.float64
    _typed_flat(planner_state, f64, 2 * D + 2, "planner_state"), _typed_flat(lower, f64, D, "lower"), _typed_flat(upper, f64, D, "upper")
    _typed_flat(solutions, f64, P * D, "solutions"), _f32_flat(solutions_f32, P * D), _typed_flat(tn, f64, P * D, "tn")
    _run("rg_cem_sample", dict(P=P, D=D),
         lambda: L.lib().rg_cem_sample(L.ptr(planner_state), L.ptr(lower), L.ptr(upper), L.ptr(tn), int(seed), int(iteration), P,
                                       D, L.ptr(solutions), L.ptr(solutions_f32), L.stream_ptr()))


def cem_sample_discrete(seed: int, iteration: int, action_dim: int, actions):
    """actions [P, T] int32 = floor(u * action_dim) (see rg_cem_sample_discrete)"""
    _chk_dev(actions)
    P, T = actions.shape
    _cem_count_check(P, T)
    _typed_flat(actions, torch.int32, P * T, "actions")
    _run("rg_cem_sample_discrete", dict(P=P, T=T, A=int(action_dim)),
         lambda: L.lib().rg_cem_sample_discrete(int(seed), int(iteration), P, T, int(action_dim), L.ptr(actions), L.stream_ptr()))


def cem_refit(rewards, solutions, num_elites: int, alpha: float, epsilon: float, planner_state, flags):
    """the elites' mean and variance folded into planner_state, the iteration count and the done flag (see rg_cem_refit)"""
    _chk_dev(rewards, solutions, planner_state, flags)
    P, D = solutions.shape
    _cem_count_check(P)
    if not 1 <= int(num_elites) <= P:
        raise ValueError(f"num_elites {num_elites} is outside [1, cem_population_size = {P}]")
    f64 = torch.float64
    _typed_flat(rewards, f64, P, "rewards"), _typed_flat(solutions, f64, P * D, "solutions")
    _typed_flat(planner_state, f64, 2 * D + 2, "planner_state"), _typed_flat(flags, torch.int32, P, "flags")
    _run("rg_cem_refit", dict(P=P, D=D, elites=int(num_elites)),
         lambda: L.lib().rg_cem_refit(L.ptr(rewards), L.ptr(solutions), P, D, int(num_elites), float(alpha), float(epsilon),
                                      L.ptr(planner_state), L.ptr(flags), L.stream_ptr()))


def cem_tally(actions, rewards, action_dim: int, out):
    """per first action the count, the reward sum and their quotient, then np.nanargmax (see rg_cem_tally): out [3 A + 1]"""
    _chk_dev(actions, rewards, out)
    P, T = actions.shape
    A = int(action_dim)
    _cem_count_check(P)
    _typed_flat(actions, torch.int32, P * T, "actions"), _typed_flat(rewards, torch.float64, P, "rewards")
    _typed_flat(out, torch.float64, 3 * A + 1, "out")
    _run("rg_cem_tally", dict(P=P, A=A),
         lambda: L.lib().rg_cem_tally(L.ptr(actions), T, L.ptr(rewards), P, A, L.ptr(out), L.stream_ptr()))


def linucb_workspace(batch: int, dim: int, device) -> torch.Tensor:
    """the byte workspace rg_linucb_accumulate asks for at (batch, dim)"""
    n = int(L.lib().rg_linucb_workspace_bytes(int(batch), int(dim)))
    if n == 0:
        raise L.ReagentHipError(f"rg_linucb_accumulate does not take batch={batch}, dim={dim} "
                                f"(1 <= dim <= {L.LINUCB_MAX_DIM}, batch >= 1)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def linucb_accumulate(x, y, weight, cur_avg_A, cur_avg_b, cur_sum_weight, cur_num_obs, workspace, action=None):
    """LinUCBTrainer.update_params on the device-resident state (see rg_linucb_accumulate), in place.  x [B, d], or
    x [B, A, d] with action (int64, B entries): the chosen arm's row is read where it lies.  y, weight: B entries each
    (weight None: ones).  Two launches, no synchronisation."""
    _chk_dev(x, y, weight, cur_avg_A, cur_avg_b, cur_sum_weight, cur_num_obs, workspace, action)
    assert x.dtype == F32 and x.is_contiguous() and x.dim() == (3 if action is not None else 2)
    B, d = x.shape[0], x.shape[-1]
    arms = x.shape[1] if action is not None else 1
    assert y.dtype == F32 and y.is_contiguous() and y.numel() == B
    assert weight is None or (weight.dtype == F32 and weight.is_contiguous() and weight.numel() == B)
    assert action is None or (action.dtype == torch.int64 and action.is_contiguous() and action.numel() == B)
    assert cur_avg_A.dtype == F32 and cur_avg_A.is_contiguous() and cur_avg_A.shape == (d, d)
    assert cur_avg_b.dtype == F32 and cur_avg_b.is_contiguous() and cur_avg_b.numel() == d
    assert cur_sum_weight.dtype == F32 and cur_sum_weight.numel() == 1
    assert cur_num_obs.dtype == torch.int64 and cur_num_obs.numel() == 1
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
    _run("rg_linucb_accumulate", dict(B=B, d=d, arms=arms),
         lambda: L.lib().rg_linucb_accumulate(L.ptr(x), L.ptr(action), arms, L.ptr(y), L.ptr(weight), B, d, L.ptr(cur_avg_A),
                                              L.ptr(cur_avg_b), L.ptr(cur_sum_weight), L.ptr(cur_num_obs), L.ptr(workspace),
                                              workspace.numel(), L.stream_ptr()))


def linucb_score_partials(n: int) -> int:
    return int(L.lib().rg_linucb_score_partials(int(n)))


def linucb_score(x, coefs, inv_avg_A, sum_weight, ucb_alpha: float, pred_label, pred_sigma, ucb, nan_partials, nan_count,
                 arms: int = 0, arm_presence=None, best_arm=None):
    """LinearRegressionUCB's scores over x [N, d] (see rg_linucb_score): pred_label, pred_sigma, ucb [N]; nan_count [1] int32
    = rows with a NaN sigma; with arms > 0 (N = B * arms) best_arm [B] int64 = the masked arg-max of ucb over each row's
    arms (arm_presence: N entries, uint8 or bool)"""
    m = _u8(arm_presence)
    _chk_dev(x, coefs, inv_avg_A, sum_weight, pred_label, pred_sigma, ucb, nan_partials, nan_count, m, best_arm)
    assert x.dtype == F32 and x.is_contiguous() and x.dim() == 2
    N, d = x.shape
    assert coefs.dtype == F32 and coefs.is_contiguous() and coefs.numel() == d
    assert inv_avg_A.dtype == F32 and inv_avg_A.is_contiguous() and inv_avg_A.shape == (d, d)
    assert sum_weight.dtype == F32 and sum_weight.numel() == 1
    for t in (pred_label, pred_sigma, ucb):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == N
    assert nan_partials.dtype == torch.int32 and nan_partials.numel() >= linucb_score_partials(N)
    assert nan_count.dtype == torch.int32 and nan_count.numel() == 1
    if arms > 0:
        assert N % arms == 0 and best_arm.dtype == torch.int64 and best_arm.is_contiguous() and best_arm.numel() == N // arms
        assert m is None or (m.is_contiguous() and m.numel() == N)
    _run("rg_linucb_score", dict(N=N, d=d, arms=arms),
         lambda: L.lib().rg_linucb_score(L.ptr(x), L.ptr(coefs), L.ptr(inv_avg_A), L.ptr(sum_weight), float(ucb_alpha), N, d,
                                         int(arms), L.ptr(m), L.ptr(pred_label), L.ptr(pred_sigma), L.ptr(ucb),
                                         L.ptr(nan_partials), L.ptr(nan_count), L.ptr(best_arm), L.stream_ptr()))


def linucb_solve(l2_reg_lambda: float, avg_A, avg_b, sum_weight, num_obs, cur_avg_A, cur_avg_b, cur_sum_weight, cur_num_obs,
                 inv_avg_A, coefs, coefs_valid_for_avg_A, status):
    """LinearRegressionUCB._calculate_coefs on the device-resident buffers (see rg_linucb_solve), in place: one launch, no
    synchronisation.  status [1] int32 is sticky: 1 after a pivot that was not positive or not finite"""
    _chk_dev(avg_A, avg_b, sum_weight, num_obs, cur_avg_A, cur_avg_b, cur_sum_weight, cur_num_obs, inv_avg_A, coefs,
             coefs_valid_for_avg_A, status)
    d = avg_A.shape[0]
    for t in (avg_A, cur_avg_A, inv_avg_A, coefs_valid_for_avg_A):
        assert t.dtype == F32 and t.is_contiguous() and t.shape == (d, d)
    for t in (avg_b, cur_avg_b, coefs):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == d
    for t in (sum_weight, cur_sum_weight):
        assert t.dtype == F32 and t.numel() == 1
    for t in (num_obs, cur_num_obs):
        assert t.dtype == torch.int64 and t.numel() == 1
    assert status.dtype == torch.int32 and status.numel() == 1
    _run("rg_linucb_solve", dict(d=d),
         lambda: L.lib().rg_linucb_solve(d, float(l2_reg_lambda), L.ptr(avg_A), L.ptr(avg_b), L.ptr(sum_weight), L.ptr(num_obs),
                                         L.ptr(cur_avg_A), L.ptr(cur_avg_b), L.ptr(cur_sum_weight), L.ptr(cur_num_obs),
                                         L.ptr(inv_avg_A), L.ptr(coefs), L.ptr(coefs_valid_for_avg_A), L.ptr(status),
                                         L.stream_ptr()))


def linucb_solve_blocked_workspace(dim: int, device) -> torch.Tensor:
    """the byte workspace rg_linucb_solve_blocked asks for at `dim`"""
    n = int(L.lib().rg_linucb_solve_blocked_workspace_bytes(int(dim)))
    if n == 0:
        raise L.ReagentHipError(f"rg_linucb_solve_blocked does not take dim={dim} (1 <= dim <= {L.LINUCB_MAX_DIM})")
    return torch.empty(n, dtype=torch.uint8, device=device)


def linucb_solve_blocked(l2_reg_lambda: float, avg_A, avg_b, sum_weight, num_obs, cur_avg_A, cur_avg_b, cur_sum_weight,
                         cur_num_obs, inv_avg_A, coefs, coefs_valid_for_avg_A, status, workspace):
    """linucb_solve's contract for every LinUCB width (see rg_linucb_solve_blocked), in place: a blocked Cholesky route in
    dim / 32 + 3 launches on `workspace` (linucb_solve_blocked_workspace), no synchronisation.  inv_avg_A leaves exactly
    symmetric; status [1] int32 is sticky: 1 after a pivot that was not positive or not finite"""
    _chk_dev(avg_A, avg_b, sum_weight, num_obs, cur_avg_A, cur_avg_b, cur_sum_weight, cur_num_obs, inv_avg_A, coefs,
             coefs_valid_for_avg_A, status, workspace)
    d = avg_A.shape[0]
    for t in (avg_A, cur_avg_A, inv_avg_A, coefs_valid_for_avg_A):
        assert t.dtype == F32 and t.is_contiguous() and t.shape == (d, d)
    for t in (avg_b, cur_avg_b, coefs):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == d
    for t in (sum_weight, cur_sum_weight):
        assert t.dtype == F32 and t.numel() == 1
    for t in (num_obs, cur_num_obs):
        assert t.dtype == torch.int64 and t.numel() == 1
    assert status.dtype == torch.int32 and status.numel() == 1
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
    _run("rg_linucb_solve_blocked", dict(d=d),
         lambda: L.lib().rg_linucb_solve_blocked(d, float(l2_reg_lambda), L.ptr(avg_A), L.ptr(avg_b), L.ptr(sum_weight),
                                                 L.ptr(num_obs), L.ptr(cur_avg_A), L.ptr(cur_avg_b), L.ptr(cur_sum_weight),
                                                 L.ptr(cur_num_obs), L.ptr(inv_avg_A), L.ptr(coefs),
                                                 L.ptr(coefs_valid_for_avg_A), L.ptr(status), L.ptr(workspace),
                                                 workspace.numel(), L.stream_ptr()))


def drlinucb_head_partials(batch: int, h: int) -> int:
    return int(L.lib().rg_drlinucb_head_partials(int(batch), int(h)))


def drlinucb_head(mlp_out, v, act: int, z, lin, pred_label, label=None, weight=None, loss_type: int = 0, row_loss=None,
                  dmlp_out=None, loss_partials=None, dv_partials=None, loss=None, dv=None):
    """the deep-represent LinUCB head over mlp_out [B, h] (see rg_drlinucb_head): z [B, h + 1] = [1, mlp_out], lin = z . v,
    pred_label = act(lin); with a label also row_loss [B], loss [1], dmlp_out [B, h] and (dv given) dv [h + 1].  label None
    is the forward-only mode"""
    _chk_dev(mlp_out, v, z, lin, pred_label, label, weight, row_loss, dmlp_out, loss_partials, dv_partials, loss, dv)
    B, h = mlp_out.shape
    assert mlp_out.dtype == F32 and v.dtype == F32 and v.is_contiguous() and v.numel() == h + 1
    assert z.dtype == F32 and z.is_contiguous() and z.shape == (B, h + 1)
    for t in (lin, pred_label, label, weight, row_loss):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.numel() == B)
    ldd = 0
    if label is not None:
        P = drlinucb_head_partials(B, h)
        assert dmlp_out.dtype == F32 and dmlp_out.shape == (B, h) and row_loss is not None
        ldd = _ld(dmlp_out)
        assert loss_partials.dtype == F32 and loss_partials.is_contiguous() and loss_partials.numel() >= P
        assert loss.dtype == F32 and loss.numel() == 1
        if dv is not None:
            assert dv.dtype == F32 and dv.is_contiguous() and dv.numel() == h + 1
            assert dv_partials.dtype == F32 and dv_partials.is_contiguous() and dv_partials.numel() >= P * (h + 1)
    _run("rg_drlinucb_head", dict(B=B, h=h, train=label is not None),
         lambda: L.lib().rg_drlinucb_head(L.ptr(mlp_out), _ld(mlp_out), L.ptr(v), L.ptr(label), L.ptr(weight), int(act),
                                          int(loss_type), B, h, L.ptr(z), L.ptr(lin), L.ptr(pred_label), L.ptr(row_loss),
                                          L.ptr(dmlp_out), ldd, L.ptr(loss_partials), L.ptr(dv_partials), L.ptr(loss),
                                          L.ptr(dv), L.stream_ptr()))


def drlinucb_activate(a, b, act: int):
    """a = act(a) and (b given) b = act(b) in place, one launch (see rg_drlinucb_activate)"""
    _chk_dev(a, b)
    n = a.numel()
    assert a.dtype == F32 and a.is_contiguous() and (b is None or (b.dtype == F32 and b.is_contiguous() and b.numel() == n))
    _run("rg_drlinucb_activate", dict(n=n),
         lambda: L.lib().rg_drlinucb_activate(L.ptr(a), L.ptr(b), n, int(act), L.stream_ptr()))


def cb_eval_partials(batch: int, device) -> torch.Tensor:
    """the per-workgroup partial sums rg_cb_eval_ingest leaves for its finishing launch at `batch` rows (float64)"""
    n = int(L.lib().rg_cb_eval_ingest_partials(int(batch)))
    if n == 0:
        raise L.ReagentHipError(f"rg_cb_eval_ingest does not take batch={batch} (batch >= 1)")
    return torch.empty(8 * n, dtype=torch.float64, device=device)


def cb_eval_ingest(action, model_action, reward, weight, action_log_probability, arm_presence, arms: int,
                   max_importance_weight, importance_weight, effective_weight, partials, sums, sum_weight_since_update):
    """BaseOfflineEval.ingest_batch on the device (see rg_cb_eval_ingest): importance_weight and effective_weight [B], and the
    batch's sums added to `sums` (the eight one-element fp32 buffers, in the header's order) and to sum_weight_since_update.
    weight, action_log_probability, arm_presence ([B, arms] uint8 or bool) and max_importance_weight may be None.  Two
    launches, no synchronisation."""
    m = _u8(arm_presence)
    _chk_dev(action, model_action, reward, weight, action_log_probability, m, importance_weight, effective_weight, partials,
             sum_weight_since_update, *sums)
    B = action.numel()
    for t in (action, model_action):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B
    for t in (reward, weight, action_log_probability, importance_weight, effective_weight):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.numel() == B)
    assert m is None or (m.is_contiguous() and m.numel() == B * int(arms))
    assert partials.dtype == torch.float64 and partials.is_contiguous()
    assert partials.numel() >= 8 * int(L.lib().rg_cb_eval_ingest_partials(B))
    assert len(sums) == 8
    for t in (*sums, sum_weight_since_update):
        assert t.dtype == F32 and t.numel() == 1
    clip = max_importance_weight is not None
    _run("rg_cb_eval_ingest", dict(B=B, arms=arms),
         lambda: L.lib().rg_cb_eval_ingest(L.ptr(action), L.ptr(model_action), L.ptr(reward), L.ptr(weight),
                                           L.ptr(action_log_probability), L.ptr(m), B, int(arms), int(clip),
                                           float(max_importance_weight) if clip else 0.0, L.ptr(importance_weight),
                                           L.ptr(effective_weight), L.ptr(partials), *[L.ptr(t) for t in sums],
                                           L.ptr(sum_weight_since_update), L.stream_ptr()))


def dlinucb_workspace(max_arm_rows: int, arms: int, dim: int, device) -> torch.Tensor:
    """the byte workspace rg_dlinucb_accumulate asks for at (max_arm_rows, arms, dim)"""
    n = int(L.lib().rg_dlinucb_workspace_bytes(int(max_arm_rows), int(arms), int(dim)))
    if n == 0:
        raise L.ReagentHipError(f"rg_dlinucb_accumulate does not take max_arm_rows={max_arm_rows}, arms={arms}, dim={dim} "
                                f"(1 <= dim <= {L.LINUCB_MAX_DIM}, 1 <= arms <= 65535, max_arm_rows >= 0)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def dlinucb_accumulate(x, y, weight, row_offsets, max_arm_rows: int, cur_A, cur_b, cur_num_obs, workspace):
    """DisjointLinUCBTrainer.cb_training_step on the device-resident state (see rg_dlinucb_accumulate), in place.  x [N, d],
    y and weight N entries each (weight None: ones): the arms' sub-batches back to back; row_offsets [arms + 1] int64 on the
    device; max_arm_rows: the longest sub-batch (a hint).  cur_A [arms, d, d], cur_b [arms, d], cur_num_obs [arms] int64.
    Two launches, no synchronisation."""
    _chk_dev(x, y, weight, row_offsets, cur_A, cur_b, cur_num_obs, workspace)
    assert x.dtype == F32 and x.is_contiguous() and x.dim() == 2
    N, d = x.shape
    assert row_offsets.dtype == torch.int64 and row_offsets.is_contiguous() and row_offsets.numel() >= 2
    arms = row_offsets.numel() - 1
    assert y.dtype == F32 and y.is_contiguous() and y.numel() == N
    assert weight is None or (weight.dtype == F32 and weight.is_contiguous() and weight.numel() == N)
    assert cur_A.dtype == F32 and cur_A.is_contiguous() and cur_A.shape == (arms, d, d)
    assert cur_b.dtype == F32 and cur_b.is_contiguous() and cur_b.shape == (arms, d)
    assert cur_num_obs.dtype == torch.int64 and cur_num_obs.is_contiguous() and cur_num_obs.numel() == arms
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
    _run("rg_dlinucb_accumulate", dict(N=N, d=d, arms=arms),
         lambda: L.lib().rg_dlinucb_accumulate(L.ptr(x), L.ptr(y), L.ptr(weight), L.ptr(row_offsets), N, arms,
                                               int(max_arm_rows), d, L.ptr(cur_A), L.ptr(cur_b), L.ptr(cur_num_obs),
                                               L.ptr(workspace), workspace.numel(), L.stream_ptr()))


def dlinucb_score(x, coefs, inv_A, ucb_alpha: float, ucb, mean=None, sigma=None, arm_presence=None, best_arm=None):
    """DisjointLinearRegressionUCB.forward over x [B, d] (see rg_dlinucb_score): ucb (and mean, sigma where given) [B, arms];
    best_arm [B] int64 = the arg-max of ucb over the arms arm_presence ([B, arms] uint8 or bool; None: all) marks present"""
    m = _u8(arm_presence)
    _chk_dev(x, coefs, inv_A, ucb, mean, sigma, m, best_arm)
    assert x.dtype == F32 and x.is_contiguous() and x.dim() == 2
    B, d = x.shape
    assert coefs.dtype == F32 and coefs.is_contiguous() and coefs.dim() == 2 and coefs.shape[1] == d
    arms = coefs.shape[0]
    assert inv_A.dtype == F32 and inv_A.is_contiguous() and inv_A.shape == (arms, d, d)
    for t in (ucb, mean, sigma):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.shape == (B, arms))
    assert ucb is not None
    assert best_arm is None or (best_arm.dtype == torch.int64 and best_arm.is_contiguous() and best_arm.numel() == B)
    assert m is None or (best_arm is not None and m.numel() == B * arms)
    _run("rg_dlinucb_score", dict(B=B, d=d, arms=arms),
         lambda: L.lib().rg_dlinucb_score(L.ptr(x), L.ptr(coefs), L.ptr(inv_A), float(ucb_alpha), B, d, arms, L.ptr(m),
                                          L.ptr(mean), L.ptr(sigma), L.ptr(ucb), L.ptr(best_arm), L.stream_ptr()))


def cpe_head(reward_est, q_cpe, q_cpe_tgt_next, next_scores, next_mask, action, reward, extra_metrics,
             not_terminal, gamma, gamma_exponent, temperature, num_metrics, loss_type, d_reward_est, d_q_cpe,
             reward_partials, cpe_partials, propensities_out=None):
    _chk_dev(reward_est, q_cpe, q_cpe_tgt_next, next_scores, next_mask, action, reward, extra_metrics,
             not_terminal, gamma_exponent, d_reward_est, d_q_cpe, reward_partials, cpe_partials, propensities_out)
    batch, A = action.shape
    M = num_metrics
    for t in (reward_est, q_cpe, q_cpe_tgt_next, d_reward_est, d_q_cpe):
        assert t.is_contiguous() and t.dtype == F32 and t.shape == (batch, M * A)
    for t in (next_scores, next_mask, action):
        assert t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A)
    assert extra_metrics is None or (extra_metrics.is_contiguous() and extra_metrics.shape == (batch, M - 1))
    for t in (reward_partials, cpe_partials):  # one partial per workgroup of 256 transitions
        assert t.is_contiguous() and t.dtype == F32 and t.numel() >= dqn_head_partials(batch)
    _run("rg_cpe_head", dict(B=batch, A=A, M=M),
         lambda: L.lib().rg_cpe_head(L.ptr(reward_est), L.ptr(q_cpe), L.ptr(q_cpe_tgt_next), L.ptr(next_scores),
                                     L.ptr(next_mask), L.ptr(action), L.ptr(reward), L.ptr(extra_metrics),
                                     L.ptr(not_terminal), float(gamma), L.ptr(gamma_exponent), float(temperature),
                                     batch, A, M, loss_type, L.ptr(d_reward_est), L.ptr(d_q_cpe),
                                     L.ptr(reward_partials), L.ptr(cpe_partials), L.ptr(propensities_out),
                                     L.stream_ptr()))


# ---- counterfactual policy evaluation on a device-resident EvaluationDataPage (cpe_eval.hip, ABI 21) --------------------
CPE_BOOTSTRAP_MAX_COLUMNS = 4  # RG_CPE_BOOTSTRAP_MAX_COLUMNS


def _f32_rows(t, rows, cols):
    """a [rows, cols] fp32 tensor or column view whose entries of a row are adjacent -> its row pitch in floats"""
    assert t.dtype == F32 and t.dim() == 2 and t.shape == (rows, cols) and (cols == 1 or t.stride(1) == 1)
    return int(t.stride(0)) if rows > 1 else max(int(t.stride(0)), cols)


def cpe_page_rows(q, q_cpe, reward_est, action, possible_actions_mask, reward, reward_boosts, temperature: float,
                  num_metrics: int):
    """The row arithmetic of EvaluationDataPage.create_from_tensors_dqn in one launch (see rg_cpe_page_rows) -> (logged_rewards
    [B, 1], model_propensities [B, A], eval_action_idxs [B, 1] int64, model_rewards_for_logged_action [B, 1],
    model_metrics_for_logged_action, model_metrics_values_for_logged_action [B, M - 1] or None where M == 1)."""
    _chk_dev(q, q_cpe, reward_est, action, possible_actions_mask, reward, reward_boosts)
    B, A = action.shape
    M = int(num_metrics)
    for t in (q, action, possible_actions_mask):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.shape == (B, A))
    for t in (q_cpe, reward_est):
        assert t is None or (t.dtype == F32 and t.is_contiguous() and t.shape == (B, M * A))
    assert reward.dtype == F32 and reward.is_contiguous() and reward.numel() == B
    assert reward_boosts is None or (reward_boosts.dtype == F32 and reward_boosts.is_contiguous() and reward_boosts.numel() == A)
    f32 = dict(dtype=F32, device=q.device)
    logged_rewards, mr_logged = torch.empty(B, 1, **f32), torch.empty(B, 1, **f32)
    propensities = torch.empty(B, A, **f32)
    idx = torch.empty(B, 1, dtype=torch.int64, device=q.device)
    mm = torch.empty(B, M - 1, **f32) if M > 1 else None
    mmv = torch.empty(B, M - 1, **f32) if M > 1 else None
    _run("rg_cpe_page_rows", dict(B=B, A=A, M=M),
         lambda: L.lib().rg_cpe_page_rows(L.ptr(q), L.ptr(q_cpe), L.ptr(reward_est), L.ptr(action),
                                          L.ptr(possible_actions_mask), L.ptr(reward), L.ptr(reward_boosts), float(temperature),
                                          B, A, M, L.ptr(logged_rewards), L.ptr(propensities), L.ptr(idx), L.ptr(mr_logged),
                                          L.ptr(mm), L.ptr(mmv), L.stream_ptr()))
    return logged_rewards, propensities, idx, mr_logged, mm, mmv


def cpe_episode_values(column, sequence_number, episode_offsets, gamma: float, out):
    """compute_values_for_mdps over one [N, 1] column (a view of a wider matrix is fine: its pitch is passed) of a sorted page
    into `out` (same shape, may be a column view too); sequence_number [N] int64, episode_offsets [E + 1] int32 on the device
    (see rg_cpe_episode_values)."""
    _chk_dev(column, sequence_number, episode_offsets, out)
    N = column.shape[0]
    ld, ldv = _f32_rows(column, N, 1), _f32_rows(out, N, 1)
    assert sequence_number.dtype == torch.int64 and sequence_number.is_contiguous() and sequence_number.numel() == N
    assert episode_offsets.dtype == torch.int32 and episode_offsets.is_contiguous() and episode_offsets.numel() >= 2
    E = episode_offsets.numel() - 1
    _run("rg_cpe_episode_values", dict(N=N, E=E),
         lambda: L.lib().rg_cpe_episode_values(L.ptr(column), ld, L.ptr(sequence_number), L.ptr(episode_offsets), E, N,
                                               float(gamma), L.ptr(out), ldv, L.stream_ptr()))
    return out


def cpe_dr_rows(model_propensities, action_mask, model_rewards, model_values, logged_propensities, logged_rewards,
                model_rewards_for_logged_action):
    """The row quantities of the one-step and sequential doubly-robust estimators and their five totals (see rg_cpe_dr_rows)
    -> dict(target_propensity, importance_weight, state_value, q_logged [N]; dm_ips_dr [3, N]; totals [5] float64: sum
    logged_rewards, dm, model_rewards_for_logged_action, ips, dr).  Two launches, nothing read back."""
    _chk_dev(model_propensities, action_mask, model_rewards, model_values, logged_propensities, logged_rewards,
             model_rewards_for_logged_action)
    N, A = model_propensities.shape
    for t in (model_propensities, action_mask):
        assert t.dtype == F32 and t.is_contiguous() and t.shape == (N, A)
    ld_mr, ld_mv = _f32_rows(model_rewards, N, A), _f32_rows(model_values, N, A)
    ld_r, ld_mrl = _f32_rows(logged_rewards, N, 1), _f32_rows(model_rewards_for_logged_action, N, 1)
    assert logged_propensities.dtype == F32 and logged_propensities.is_contiguous() and logged_propensities.numel() == N
    dev = model_propensities.device
    f32 = dict(dtype=F32, device=dev)
    out = dict(target_propensity=torch.empty(N, **f32), importance_weight=torch.empty(N, **f32),
               dm_ips_dr=torch.empty(3, N, **f32), state_value=torch.empty(N, **f32), q_logged=torch.empty(N, **f32),
               totals=torch.empty(5, dtype=torch.float64, device=dev))
    P = int(L.lib().rg_cpe_dr_partials(N))
    if P == 0:
        raise L.ReagentHipError(f"rg_cpe_dr_rows does not take rows={N} (rows >= 1)")
    partials = torch.empty(5 * P, dtype=torch.float64, device=dev)
    _run("rg_cpe_dr_rows", dict(N=N, A=A),
         lambda: L.lib().rg_cpe_dr_rows(L.ptr(model_propensities), L.ptr(action_mask), L.ptr(model_rewards), ld_mr,
                                        L.ptr(model_values), ld_mv, L.ptr(logged_propensities), L.ptr(logged_rewards), ld_r,
                                        L.ptr(model_rewards_for_logged_action), ld_mrl, N, A, L.ptr(out["target_propensity"]),
                                        L.ptr(out["importance_weight"]), L.ptr(out["dm_ips_dr"]), L.ptr(out["state_value"]),
                                        L.ptr(out["q_logged"]), L.ptr(partials), L.ptr(out["totals"]), L.stream_ptr()))
    return out


def cpe_sdr(state_value, importance_weight, logged_rewards, q_logged, episode_offsets, gamma: float):
    """The sequential doubly-robust recurrence, one lane per episode (see rg_cpe_sdr) -> (doubly_robust [E], episode_value [E])"""
    _chk_dev(state_value, importance_weight, logged_rewards, q_logged, episode_offsets)
    N = state_value.numel()
    for t in (state_value, importance_weight, q_logged):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == N
    ld_r = _f32_rows(logged_rewards, N, 1)
    assert episode_offsets.dtype == torch.int32 and episode_offsets.is_contiguous() and episode_offsets.numel() >= 2
    E = episode_offsets.numel() - 1
    dr = torch.empty(E, dtype=F32, device=state_value.device)
    ev = torch.empty(E, dtype=F32, device=state_value.device)
    _run("rg_cpe_sdr", dict(N=N, E=E),
         lambda: L.lib().rg_cpe_sdr(L.ptr(state_value), L.ptr(importance_weight), L.ptr(logged_rewards), ld_r, L.ptr(q_logged),
                                    L.ptr(episode_offsets), E, N, float(gamma), L.ptr(dr), L.ptr(ev), L.stream_ptr()))
    return dr, ev


def cpe_bootstrap(values, sample_size: int, num_samples: int, seed: int):
    """Bootstrap resampling of the C <= 4 rows of values [C, n] with one index stream (see rg_cpe_bootstrap, which states the
    draw recipe) -> (means [C, num_samples], std [C]), float64 on the device."""
    _chk_dev(values)
    assert values.dtype == F32 and values.dim() == 2 and values.stride(1) == 1
    C, n = values.shape
    ld = int(values.stride(0)) if C > 1 else max(int(values.stride(0)), n)
    means = torch.empty(C, int(num_samples), dtype=torch.float64, device=values.device)
    std = torch.empty(C, dtype=torch.float64, device=values.device)
    _run("rg_cpe_bootstrap", dict(C=C, n=n, S=int(sample_size), K=int(num_samples)),
         lambda: L.lib().rg_cpe_bootstrap(L.ptr(values), ld, C, n, int(sample_size), int(num_samples),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(means), L.ptr(std), L.stream_ptr()))
    return means, std


# ---- weighted sequential DR and MAGIC: row and episode arithmetic (cpe_wsdr.hip, ABI 22) ---------------------------------
CPE_WSDR_MAX_J_STEPS = 32  # RG_CPE_WSDR_MAX_J_STEPS
CPE_WSDR_MAX_SUBSETS = 32  # RG_CPE_WSDR_MAX_SUBSETS


def cpe_wsdr(model_propensities, action_mask, model_values, logged_propensities, logged_rewards, episode_offsets,
             longest: int, gamma: float, self_normalize: bool, j_steps, subset_offsets=None):
    """The device part of WeightedSequentialDoublyRobustEstimator.estimate on a sorted page (see rg_cpe_wsdr): j_steps (a
    sequence of J ints in -1 .. longest - 1) and subset_offsets (G + 1 ints, None where J == 1) are host values.
    -> (ret [J + 1, E] float64 on the device: the per-episode j-step returns and, last, the episode values;
        out float64 on the device: j_step_returns [J], infinite_step_returns [G], covariance [J, J], mean episode value [1]
        (J == 1: j_step_returns[0] and the mean episode value)).  The launches go on the current stream; nothing is read back."""
    _chk_dev(model_propensities, action_mask, model_values, logged_propensities, logged_rewards, episode_offsets)
    N, A = model_propensities.shape
    for t in (model_propensities, action_mask):
        assert t.dtype == F32 and t.is_contiguous() and t.shape == (N, A)
    ld_mv, ld_r = _f32_rows(model_values, N, A), _f32_rows(logged_rewards, N, 1)
    assert logged_propensities.dtype == F32 and logged_propensities.is_contiguous() and logged_propensities.numel() == N
    assert episode_offsets.dtype == torch.int32 and episode_offsets.is_contiguous() and episode_offsets.numel() >= 2
    E = episode_offsets.numel() - 1
    js = [int(j) for j in j_steps]
    J = len(js)
    so = [int(b) for b in subset_offsets] if subset_offsets is not None else []
    G = len(so) - 1 if J > 1 else 0
    dev = model_propensities.device
    nbytes = int(L.lib().rg_cpe_wsdr_workspace_bytes(N, E, int(longest), J, G))
    if nbytes == 0:
        raise L.ReagentHipError(f"rg_cpe_wsdr does not take rows={N} episodes={E} longest={longest} j_steps={J} subsets={G} "
                                f"(1 <= episodes <= rows, 1 <= longest <= rows, 1 <= j_steps <= {CPE_WSDR_MAX_J_STEPS}, "
                                f"1 <= subsets <= {CPE_WSDR_MAX_SUBSETS} where j_steps > 1)")
    workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    ret = torch.empty(J + 1, E, dtype=torch.float64, device=dev)
    out = torch.empty(J + G + J * J + 1 if J > 1 else 2, dtype=torch.float64, device=dev)
    c_js = (ctypes.c_int32 * J)(*js)
    c_so = (ctypes.c_int32 * len(so))(*so) if J > 1 else None
    _run("rg_cpe_wsdr", dict(N=N, A=A, E=E, T=int(longest), J=J, G=G),
         lambda: L.lib().rg_cpe_wsdr(L.ptr(model_propensities), L.ptr(action_mask), L.ptr(model_values), ld_mv,
                                     L.ptr(logged_propensities), L.ptr(logged_rewards), ld_r, L.ptr(episode_offsets), N, A, E,
                                     int(longest), float(gamma), int(bool(self_normalize)),
                                     ctypes.cast(c_js, ctypes.c_void_p), J,
                                     ctypes.cast(c_so, ctypes.c_void_p) if c_so is not None else None, G,
                                     L.ptr(workspace), nbytes, L.ptr(ret), L.ptr(out), L.stream_ptr()))
    return ret, out


def c51_head(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma,
             gamma_exponent, support, qmin, qmax, num_atoms, maxq, dq, loss_partials, all_q=None):
    _chk_dev(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma_exponent,
             support, dq, loss_partials, all_q)
    batch, A = action.shape
    for t in (q, qn_target, dq):
        assert t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A * num_atoms)
    _run("rg_c51_head", dict(B=batch, A=A, N=num_atoms),
         lambda: L.lib().rg_c51_head(L.ptr(q), L.ptr(qn_online), L.ptr(qn_target), L.ptr(action), L.ptr(next_mask),
                                     L.ptr(reward), L.ptr(reward_boosts), L.ptr(not_terminal), float(gamma),
                                     L.ptr(gamma_exponent), L.ptr(support), float(qmin), float(qmax), batch, A,
                                     num_atoms, int(maxq), L.ptr(dq), L.ptr(loss_partials), L.ptr(all_q),
                                     L.stream_ptr()))


def crr_partials(batch: int) -> int:
    return int(L.lib().rg_crr_partials(batch))


def crr_critic_head(q1, q2, q1_next_t, q2_next_t, next_logits, action, reward, reward_boosts, not_terminal, gamma,
                    target, dq1, dq2, partials1, partials2):
    _chk_dev(q1, q2, q1_next_t, q2_next_t, next_logits, action, reward, reward_boosts, not_terminal, target, dq1, dq2,
             partials1, partials2)
    batch, A = action.shape
    for t in (q1, q2, q1_next_t, q2_next_t, next_logits, action, dq1, dq2):
        assert t is None or (t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A))
    _run("rg_crr_critic_head", dict(B=batch, A=A),
         lambda: L.lib().rg_crr_critic_head(L.ptr(q1), L.ptr(q2), L.ptr(q1_next_t), L.ptr(q2_next_t),
                                            L.ptr(next_logits), L.ptr(action), L.ptr(reward), L.ptr(reward_boosts),
                                            L.ptr(not_terminal), float(gamma), batch, A, L.ptr(target), L.ptr(dq1),
                                            L.ptr(dq2), L.ptr(partials1), L.ptr(partials2), L.stream_ptr()))


def crr_actor_head(q, logits, action, logged_prob, beta, max_weight, entropy_coeff, clip_limit, dlogits,
                   plain_partials, entropy_partials):
    _chk_dev(q, logits, action, logged_prob, dlogits, plain_partials, entropy_partials)
    batch, A = action.shape
    for t in (q, logits, action, dlogits):
        assert t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A)
    _run("rg_crr_actor_head", dict(B=batch, A=A),
         lambda: L.lib().rg_crr_actor_head(L.ptr(q), L.ptr(logits), L.ptr(action), L.ptr(logged_prob), float(beta),
                                           float(max_weight), float(entropy_coeff), float(clip_limit), batch, A,
                                           L.ptr(dlogits), L.ptr(plain_partials), L.ptr(entropy_partials),
                                           L.stream_ptr()))


def qr_head(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma,
            gamma_exponent, quantiles, num_atoms, maxq, dq, loss_partials, all_q=None):
    _chk_dev(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma_exponent,
             quantiles, dq, loss_partials, all_q)
    batch, A = action.shape
    for t in (q, qn_online, qn_target, dq):
        assert t is None or (t.is_contiguous() and t.dtype == F32 and t.shape == (batch, A * num_atoms))
    _run("rg_qr_head", dict(B=batch, A=A, N=num_atoms),
         lambda: L.lib().rg_qr_head(L.ptr(q), L.ptr(qn_online), L.ptr(qn_target), L.ptr(action), L.ptr(next_mask),
                                    L.ptr(reward), L.ptr(reward_boosts), L.ptr(not_terminal), float(gamma),
                                    L.ptr(gamma_exponent), L.ptr(quantiles), batch, A, num_atoms, int(maxq),
                                    L.ptr(dq), L.ptr(loss_partials), L.ptr(all_q), L.stream_ptr()))


def reduce_sum_runs(inp, n: int, run: int, scale: float, out):
    """out = scale * sum of the n inputs, each run of `run` of them added in order first (the per-wave loss sums of
    FusedMLP.dqn_pair_forward with run = 16: the bits of dqn_head's partials through reduce_sum)"""
    _chk_dev(inp, out)
    _run("rg_reduce_sum_runs", dict(n=n, run=run),
         lambda: L.lib().rg_reduce_sum_runs(L.ptr(inp), n, run, scale, L.ptr(out), L.stream_ptr()))


def reduce_sum(inp, n: int, scale: float, out):
    _chk_dev(inp, out)
    _run("rg_reduce_sum", dict(n=n), lambda: L.lib().rg_reduce_sum(L.ptr(inp), n, scale, L.ptr(out), L.stream_ptr()))


# ---- optimizer --------------------------------------------------------------------------------
def adam_step(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt,
              grad_scale=1.0, offset=0):
    """Flat fp32 slabs; [offset, offset+n) is updated."""
    _chk_dev(param, grad, exp_avg, exp_avg_sq)
    o = offset * 4
    _run("rg_adam_step", dict(n=n),
         lambda: L.lib().rg_adam_step(param.data_ptr() + o, grad.data_ptr() + o, exp_avg.data_ptr() + o,
                                      exp_avg_sq.data_ptr() + o, n, lr, beta1, beta2, eps, weight_decay, bc1,
                                      bc2_sqrt, grad_scale, L.stream_ptr()))


def adam_step_sched(param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, weight_decay, sched, grad_scale=1.0,
                    offset=0):
    """rg_adam_step with lr and the bias corrections read from the device schedule `sched` (graph-safe)."""
    _chk_dev(param, grad, exp_avg, exp_avg_sq, sched)
    tick_fence(sched)
    o = offset * 4
    _run("rg_adam_step", dict(n=n),
         lambda: L.lib().rg_adam_step_sched(param.data_ptr() + o, grad.data_ptr() + o, exp_avg.data_ptr() + o,
                                            exp_avg_sq.data_ptr() + o, n, beta1, beta2, eps, weight_decay,
                                            grad_scale, sched.data_ptr(), L.stream_ptr()))


# ---- schedule ticks of a native step in ONE launch ---------------------------------------------------------
# A device-scheduled update is followed by the tick of ITS schedule (sched[0] += 1).  Nothing reads a schedule again before that
# optimizer's next step, so inside `deferred_ticks()` (the trainers' native steps, dqn_trainer.native_step) the ticks are collected
# and leave as one rg_sched_tick_many launch when the scope closes: SAC's four launch-bound ticks (15 us per step) become one.
# `tick_fence(sched)` — called by every launch that READS a schedule — flushes first if that schedule has a tick waiting.
MAX_TICKS = 8
_tick_scopes = []
_DEFER_TICKS = os.environ.get("RG_DEFER_TICKS", "1") != "0"  # 0: a tick launch per schedule, where it was (same-box A/B)


def _flush_ticks(pending):
    if not pending:
        return
    if len(pending) == 1:
        s = pending[0]
        _run("rg_sched_tick", {}, lambda: L.lib().rg_sched_tick(s.data_ptr(), L.stream_ptr()))
    else:
        arr = (ctypes.c_void_p * len(pending))(*[s.data_ptr() for s in pending])
        _run("rg_sched_tick", dict(n=len(pending)), lambda: L.lib().rg_sched_tick_many(arr, len(pending), L.stream_ptr()))
    del pending[:]


class deferred_ticks:
    def __enter__(self):
        _tick_scopes.append([])
        return self

    def __exit__(self, *exc):
        _flush_ticks(_tick_scopes.pop())
        return False


def tick_fence(sched):
    """before a launch that reads `sched`: its waiting tick (if any) must have been enqueued"""
    for pending in _tick_scopes:
        if any(s.data_ptr() == sched.data_ptr() for s in pending):
            _flush_ticks(pending)


def sched_tick(sched):
    _chk_dev(sched)
    if _tick_scopes and _DEFER_TICKS:
        pending = _tick_scopes[-1]
        if any(s.data_ptr() == sched.data_ptr() for s in pending) or len(pending) == MAX_TICKS:
            _flush_ticks(pending)
        pending.append(sched)
        return
    _run("rg_sched_tick", {}, lambda: L.lib().rg_sched_tick(sched.data_ptr(), L.stream_ptr()))


def soft_update(target, source, n, tau, t_off=0, s_off=0):
    _chk_dev(target, source)
    _run("rg_soft_update", dict(n=n),
         lambda: L.lib().rg_soft_update(target.data_ptr() + 4 * t_off, source.data_ptr() + 4 * s_off, n, tau,
                                        L.stream_ptr()))


# ---- SAC --------------------------------------------------------------------------------------
def gaussian_head_forward(loc_scale, noise, action, log_prob=None, squashed_mean=None):
    _chk_dev(loc_scale, noise, action, log_prob, squashed_mean)
    B, A = noise.shape
    assert noise.is_contiguous() and loc_scale.shape == (B, 2 * A)
    _run("rg_gaussian_head_forward", dict(B=B, A=A),
         lambda: L.lib().rg_gaussian_head_forward(L.ptr(loc_scale), _ld(loc_scale), L.ptr(noise), B, A,
                                                  L.ptr(action), _ld(action), L.ptr(log_prob),
                                                  L.ptr(squashed_mean), L.stream_ptr()))


def gaussian_log_prob(loc_scale, action, log_prob):
    _chk_dev(loc_scale, action, log_prob)
    B, A = action.shape
    _run("rg_gaussian_log_prob", dict(B=B, A=A),
         lambda: L.lib().rg_gaussian_log_prob(L.ptr(loc_scale), _ld(loc_scale), L.ptr(action), _ld(action), B, A,
                                              L.ptr(log_prob), L.stream_ptr()))


def gaussian_head_backward(loc_scale, noise, g_action, g_log_prob, d_loc_scale, kld_coef=None, kld_on_mean=False):
    _chk_dev(loc_scale, noise, g_action, g_log_prob, d_loc_scale, kld_coef)
    B, A = noise.shape
    _run("rg_gaussian_head_backward", dict(B=B, A=A),
         lambda: L.lib().rg_gaussian_head_backward_kld(L.ptr(loc_scale), _ld(loc_scale), L.ptr(noise),
                                                       L.ptr(g_action), _ld(g_action) if g_action is not None else 0,
                                                       L.ptr(g_log_prob), B, A, L.ptr(d_loc_scale),
                                                       _ld(d_loc_scale), L.ptr(kld_coef), int(kld_on_mean),
                                                       L.stream_ptr()))


def sac_kld(x, squash, emb_mean, emb_var, weight, coef, kld_terms, kld=None, loss_inout=None):
    """action-embedding KLD term (sac_trainer.py:282-306) over the columns of x [B, A]: gradient coefficients into
    coef [2A], the value into kld [1], weight * kld added to loss_inout [1]"""
    _chk_dev(x, emb_mean, emb_var, coef, kld_terms, kld, loss_inout)
    B, A = x.shape[0], emb_mean.numel()
    assert coef.numel() == 2 * A and kld_terms.numel() >= A and x.stride(1) == 1
    _run("rg_sac_kld", dict(B=B, A=A),
         lambda: L.lib().rg_sac_kld(L.ptr(x), x.stride(0), int(squash), B, A, L.ptr(emb_mean), L.ptr(emb_var), float(weight),
                                    L.ptr(coef), L.ptr(kld_terms), L.ptr(kld), L.ptr(loss_inout), L.stream_ptr()))


def sac_partials(batch: int) -> int:
    return int(L.lib().rg_sac_partials(batch))


def sac_critic_head(q1, q2, q1t, q2t, lp_next, reward, not_terminal, gamma, alpha, target, dq1, dq2, l1, l2):
    _chk_dev(q1, q2, q1t, q2t, lp_next, reward, not_terminal, alpha, target, dq1, dq2, l1, l2)
    B = q1.numel()
    _run("rg_sac_critic_head", dict(B=B),
         lambda: L.lib().rg_sac_critic_head(L.ptr(q1), L.ptr(q2), L.ptr(q1t), L.ptr(q2t), L.ptr(lp_next),
                                            L.ptr(reward), L.ptr(not_terminal), float(gamma), L.ptr(alpha), B,
                                            L.ptr(target), L.ptr(dq1), L.ptr(dq2), L.ptr(l1), L.ptr(l2),
                                            L.stream_ptr()))


def sac_actor_head(lp, q1a, q2a, alpha, target_entropy, g_lp, dq1a, dq2a, loss_part, ent_part, v_cur=None, crr_mode=0,
                   crr_p0=0.0, crr_clamp=0.0, backprop_log_prob=True):
    """crr_mode 0: alpha * clamp(log_prob) - min q; 1 / 2: -(clamp(log_prob) * CRR weight of (min q - v_cur)), indicator
    (threshold crr_p0) / exponent (beta crr_p0, clamp crr_clamp)"""
    _chk_dev(lp, q1a, q2a, alpha, g_lp, dq1a, dq2a, loss_part, ent_part, v_cur)
    B = lp.numel()
    _run("rg_sac_actor_head", dict(B=B),
         lambda: L.lib().rg_sac_actor_head(L.ptr(lp), L.ptr(q1a), L.ptr(q2a), L.ptr(alpha), float(target_entropy),
                                           B, L.ptr(v_cur), int(crr_mode), float(crr_p0), float(crr_clamp),
                                           int(bool(backprop_log_prob)), L.ptr(g_lp), L.ptr(dq1a), L.ptr(dq2a),
                                           L.ptr(loss_part), L.ptr(ent_part), L.stream_ptr()))


def sac_alpha_grad(ent_part, batch, log_alpha, grad, alpha_loss=None):
    _chk_dev(ent_part, log_alpha, grad, alpha_loss)
    _run("rg_sac_alpha_grad", dict(B=batch),
         lambda: L.lib().rg_sac_alpha_grad(L.ptr(ent_part), batch, L.ptr(log_alpha), L.ptr(grad),
                                           L.ptr(alpha_loss), L.stream_ptr()))


def adam_step_f64(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, bc1, bc2_sqrt, exp_out=None):
    _chk_dev(param, grad, exp_avg, exp_avg_sq, exp_out)
    _run("rg_adam_step_f64", dict(n=param.numel()),
         lambda: L.lib().rg_adam_step_f64(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq),
                                          param.numel(), lr, beta1, beta2, eps, bc1, bc2_sqrt, L.ptr(exp_out),
                                          L.stream_ptr()))


def adam_step_f64_sched(param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, sched, exp_out=None):
    _chk_dev(param, grad, exp_avg, exp_avg_sq, exp_out, sched)
    tick_fence(sched)
    _run("rg_adam_step_f64", dict(n=param.numel()),
         lambda: L.lib().rg_adam_step_f64_sched(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq),
                                                param.numel(), beta1, beta2, eps, sched.data_ptr(), L.ptr(exp_out),
                                                L.stream_ptr()))


def add_cols(a, b, out):
    _chk_dev(a, b, out)
    B, C = out.shape
    _run("rg_add_cols", dict(B=B, C=C),
         lambda: L.lib().rg_add_cols(L.ptr(a), _ld(a), L.ptr(b), _ld(b) if b is not None else 0, B, C, L.ptr(out),
                                     _ld(out), L.stream_ptr()))


# ---- QR-DQN with a grouped output layer (qr_grouped.hip) ------------------------------------------------------
def group_rows(key, n_groups, n_tiles, rowmap, tile_key, row_begin, workspace, dense: bool = True):
    _chk_dev(key, rowmap, tile_key, row_begin, workspace)
    assert key.dtype == torch.int32 and rowmap.numel() == n_tiles * 128 and tile_key.numel() == n_tiles
    _run("rg_group_rows", dict(B=key.numel(), G=n_groups),
         lambda: L.lib().rg_group_rows(key.data_ptr(), key.numel(), n_groups, n_tiles, int(dense), rowmap.data_ptr(),
                                       tile_key.data_ptr(), row_begin.data_ptr(), workspace.data_ptr(), workspace.numel() * 4,
                                       L.stream_ptr()))


def group_wfrag_elems(group_rows: int, in_features: int, transposed: bool) -> int:
    return int(L.lib().rg_group_wfrag_elems(group_rows, in_features, int(transposed)))


def group_weights_stage(w, n_groups, group_rows, wf, wb, x3: bool = False):
    """x3: split-bf16 — every group's fragment set is [hi plane | lo plane] (wf / wb hold 2 x the elements)"""
    _chk_dev(w, wf, wb)
    assert w.is_contiguous() and w.dtype == F32 and w.shape[0] == n_groups * group_rows
    _run("rg_group_weights_stage", dict(G=n_groups, Ng=group_rows, K=w.shape[1]),
         lambda: L.lib().rg_group_weights_stage(w.data_ptr(), n_groups, group_rows, w.shape[1], int(x3), L.ptr(wf), L.ptr(wb),
                                                L.stream_ptr()))


def wide_head_mean(w, b, n_groups, group_rows, wbar, bbar, wfrag_fwd=None, x3: bool = False):
    """wfrag_fwd: the (already staged once) forward fragments of the [n_groups, in] mean layer, rewritten in the same launch
    (x3: both planes)"""
    _chk_dev(w, b, wbar, bbar)
    assert w.is_contiguous() and wbar.is_contiguous() and wbar.shape == (n_groups, w.shape[1])
    if wfrag_fwd is None:
        _run("rg_wide_head_mean", dict(G=n_groups, Ng=group_rows, K=w.shape[1]),
             lambda: L.lib().rg_wide_head_mean(w.data_ptr(), L.ptr(b), n_groups, group_rows, w.shape[1], wbar.data_ptr(),
                                               bbar.data_ptr(), L.stream_ptr()))
    else:
        _chk_dev(wfrag_fwd)
        _run("rg_wide_head_mean", dict(G=n_groups, Ng=group_rows, K=w.shape[1]),
             lambda: L.lib().rg_wide_head_mean_staged(w.data_ptr(), L.ptr(b), n_groups, group_rows, w.shape[1],
                                                      wbar.data_ptr(), bbar.data_ptr(), wfrag_fwd.data_ptr(), int(x3),
                                                      L.stream_ptr()))


def qr_select_action(q, mask, maxq: bool, key):
    _chk_dev(q, mask, key)
    B, A = mask.shape
    assert mask.is_contiguous() and mask.dtype == F32 and key.dtype == torch.int32 and key.numel() == B
    _run("rg_qr_select_action", dict(B=B, A=A),
         lambda: L.lib().rg_qr_select_action(L.ptr(q), _ld(q) if q is not None else 0, mask.data_ptr(), B, A, int(maxq),
                                             key.data_ptr(), L.stream_ptr()))


def qr_select_group_rows(q, mask, maxq: bool, key, n_tiles, rowmap, tile_key, row_begin, workspace, dense: bool = True):
    """qr_select_action + group_rows (n_groups = number of actions) in two launches"""
    _chk_dev(q, mask, key, rowmap, tile_key, row_begin, workspace)
    B, A = mask.shape
    assert mask.is_contiguous() and mask.dtype == F32 and key.dtype == torch.int32 and key.numel() == B
    assert rowmap.numel() == n_tiles * 128 and tile_key.numel() == n_tiles
    _run("rg_group_rows", dict(B=B, G=A),
         lambda: L.lib().rg_qr_select_group_rows(L.ptr(q), _ld(q) if q is not None else 0, mask.data_ptr(), B, A, int(maxq),
                                                 key.data_ptr(), n_tiles, int(dense), rowmap.data_ptr(), tile_key.data_ptr(),
                                                 row_begin.data_ptr(), workspace.data_ptr(), workspace.numel() * 4,
                                                 L.stream_ptr()))


def qr_compact_head(z, zt, rowmap, row_key, reward, reward_boosts, not_terminal, gamma, gamma_exponent, quantiles,
                    batch, num_atoms, dz, loss_partials, tile_losses=None):
    """row_key [batch] int32: the group (logged action) of every batch row — read for the reward boost only"""
    _chk_dev(z, zt, rowmap, row_key, reward, reward_boosts, not_terminal, gamma_exponent, quantiles, dz, loss_partials,
             tile_losses)
    rows = rowmap.numel()
    assert z.shape[0] == rows and dz.shape[0] == rows and loss_partials.numel() == rows
    assert reward_boosts is None or (row_key is not None and row_key.numel() == batch)
    _run("rg_qr_compact_head", dict(rows=rows, N=num_atoms),
         lambda: L.lib().rg_qr_compact_head(z.data_ptr(), _ld(z), zt.data_ptr(), _ld(zt), rowmap.data_ptr(),
                                            L.ptr(row_key), rows, reward.data_ptr(), L.ptr(reward_boosts),
                                            not_terminal.data_ptr(), float(gamma), L.ptr(gamma_exponent),
                                            quantiles.data_ptr(), batch, num_atoms, dz.data_ptr(), _ld(dz),
                                            loss_partials.data_ptr(), L.ptr(tile_losses), L.stream_ptr()))


def grouped_dz_rows(rows: int, n_groups: int) -> int:
    """rows of the fragment matrix that holds a grouped layer's dZ (include/reagent_hip.h, rg_mlp_desc: group g's blocks g late)"""
    return rows + 32 * n_groups


def group_head_wgrad(dzw_frag, h_frag, row_begin, n_groups, group_rows, in_features, splits, dw, workspace, x3: bool = False,
                     rows: int = 0):
    """x3: split-bf16 operands ([hi plane | lo plane] over the `rows` rows of the grouped space)"""
    _chk_dev(dzw_frag, h_frag, row_begin, dw, workspace)
    assert dw.is_contiguous() and dw.shape == (n_groups * group_rows, in_features)
    _run("rg_group_head_wgrad", dict(G=n_groups, Ng=group_rows, K=in_features),
         lambda: L.lib().rg_group_head_wgrad(dzw_frag.data_ptr(), h_frag.data_ptr(), row_begin.data_ptr(), n_groups,
                                             group_rows, in_features, splits, int(x3), int(rows), dw.data_ptr(),
                                             workspace.data_ptr(), workspace.numel() * 4, L.stream_ptr()))


# ---- dueling aggregation -------------------------------------------------------------------------------------
def dueling_combine(value, adv, num_actions, num_atoms, q):
    _chk_dev(value, adv, q)
    B = q.shape[0]
    _run("rg_dueling_combine", dict(B=B, A=num_actions, N=num_atoms),
         lambda: L.lib().rg_dueling_combine(value.data_ptr(), _ld(value), adv.data_ptr(), _ld(adv), B, num_actions, num_atoms,
                                            q.data_ptr(), _ld(q), L.stream_ptr()))


def dueling_split(dq, num_actions, num_atoms, dadv, dvalue):
    _chk_dev(dq, dadv, dvalue)
    B = dq.shape[0]
    _run("rg_dueling_split", dict(B=B, A=num_actions, N=num_atoms),
         lambda: L.lib().rg_dueling_split(dq.data_ptr(), _ld(dq), B, num_actions, num_atoms, dadv.data_ptr(), _ld(dadv),
                                          dvalue.data_ptr(), _ld(dvalue), L.stream_ptr()))


# ---- synthetic reward --------------------------------------------------------------------------------------------------
def ngram_concat(state, action, context_size: int, out):
    """out [T, B, (S + A) * n] = ngram(cat(state, action), n) (see rg_ngram_concat): window slot i of step t holds step
    t + i - n // 2, zeros outside the sequence; n = 1 is the plain cat.  state [T, B, S], action [T, B, A] and out may have
    padded rows (a unit last stride and (t, b) rows a constant pitch apart)"""
    _chk_dev(state, action, out)
    T, B, S = state.shape
    A, n = action.shape[2], int(context_size)
    if n < 1 or n % 2 == 0:
        raise NotImplementedError(f"ngram_concat: context_size {n} is not supported (odd, at least 1)")
    if T * B >= 1 << 29:
        raise NotImplementedError(f"ngram_concat: seq_len * batch = {T * B} is not supported (below 2^29)")
    assert action.shape[:2] == (T, B) and out.shape == (T, B, (S + A) * n)
    for t in (state, action, out):
        assert t.dtype == F32 and t.stride(2) == 1 and (B == 1 or t.stride(0) == B * t.stride(1)), "rows a constant pitch apart"
    ld = lambda t: t.stride(1) if B > 1 or T == 1 else t.stride(0)  # noqa: E731
    _run("rg_ngram_concat", dict(T=T, B=B, S=S, A=A, n=n),
         lambda: L.lib().rg_ngram_concat(L.ptr(state), ld(state), L.ptr(action), ld(action), T, B, S, A, n, L.ptr(out), ld(out),
                                         L.stream_ptr()))


def step_reward_head_partials(batch: int) -> int:
    return int(L.lib().rg_step_reward_head_partials(batch))


def step_reward_head_workspace(seq_len: int, batch: int, width: int) -> int:
    """doubles of workspace rg_step_reward_head asks for"""
    return step_reward_head_partials(batch) * (width + 3) + (seq_len + 1) * batch


def step_reward_head(h, w, bias, act: int, valid_step, output, mask, predicted_reward, target=None, loss_type: int = 0,
                     threshold=None, apply_threshold: bool = False, loss=None, n_kept=None, dh=None, dw=None, dbias=None,
                     workspace=None):
    """the synthetic-reward head behind the trunk's output h [T, B, P] (see rg_step_reward_head): the last Linear(P, 1) and
    its activation, the valid-step mask and the masked sum; with target [B] the loss (threshold=None: no filter) and n_kept;
    with dh the gradients.  valid_step [B] int64 is clamped into [1, T] by the kernel"""
    _chk_dev(h, w, bias, valid_step, output, mask, predicted_reward, target, loss, n_kept, dh, dw, dbias, workspace)
    T, B, P = h.shape
    if T * B >= 1 << 29:
        raise NotImplementedError(f"step_reward_head: seq_len * batch = {T * B} is not supported (below 2^29)")
    _f32_flat(h, T * B * P), _f32_flat(w, P), _f32_flat(bias, 1), _f32_flat(output, B * T), _f32_flat(mask, B * T)
    _f32_flat(predicted_reward, B), _f32_flat(target, B), _f32_flat(loss, 1), _f32_flat(dh, T * B * P), _f32_flat(dw, P)
    _f32_flat(dbias, 1)
    assert valid_step.dtype == torch.int64 and valid_step.is_contiguous() and valid_step.numel() == B
    if target is not None:
        assert loss is not None and n_kept is not None and n_kept.dtype == torch.int32 and n_kept.numel() == 1
        assert workspace.dtype == torch.float64 and workspace.is_contiguous()
        assert workspace.numel() >= step_reward_head_workspace(T, B, P)
    if dh is not None:
        assert target is not None and dw is not None and dbias is not None
    _run("rg_step_reward_head", dict(T=T, B=B, P=P, train=dh is not None),
         lambda: L.lib().rg_step_reward_head(L.ptr(h), L.ptr(w), L.ptr(bias), int(act), L.ptr(valid_step), L.ptr(target),
                                             int(loss_type), int(threshold is not None),
                                             float(threshold) if threshold is not None else 0.0, int(bool(apply_threshold)), T, B,
                                             P, L.ptr(output), L.ptr(mask), L.ptr(predicted_reward), L.ptr(loss), L.ptr(n_kept),
                                             L.ptr(dh), L.ptr(dw), L.ptr(dbias), L.ptr(workspace), L.stream_ptr()))


# ---- counterfactual-evaluation reward models (bbb.hip) -----------------------------------------------------------------
def bbb_table(segments) -> "L.BbbTable":
    """the segment table of the Bayes-by-backprop kernels (see rg_bbb_sample) from dicts of flat fp32 tensors: mu, rho, w,
    eps and, for rg_bbb_grad, dw, dmu, drho.  The caller keeps the tensors alive while the table is in use."""
    if not 1 <= len(segments) <= L.BBB_MAX_SEGMENTS:
        raise NotImplementedError(f"bbb_table: {len(segments)} segments are not supported (1 to {L.BBB_MAX_SEGMENTS}: a layer's "
                                  "weights and its biases are a segment each)")
    t = L.BbbTable()
    t.n_segments = len(segments)
    for i, s in enumerate(segments):
        n = s["mu"].numel()
        for k in ("mu", "rho", "w", "eps", "dw", "dmu", "drho"):
            v = s.get(k)
            if v is not None:
                _chk_dev(v)
                assert v.dtype == F32 and v.is_contiguous() and v.numel() == n, (i, k, v.shape, v.dtype)
            setattr(t.seg[i], k, L.ptr(v))
        t.seg[i].n = n
    return t


def bbb_chunks(table) -> int:
    return int(L.lib().rg_bbb_chunks(ctypes.byref(table)))


def bbb_fill_noise(table, seed: int, sample: int = 0):
    """every segment's eps = what rg_bbb_sample would draw in place for (seed, sample)"""
    _run("rg_bbb_fill_noise", dict(chunks=bbb_chunks(table)),
         lambda: L.lib().rg_bbb_fill_noise(ctypes.byref(table), int(seed), int(sample), L.stream_ptr()))


def bbb_sample(table, prior_var: float, log_prior, log_post, terms, workspace, seed: Optional[int] = None, sample: int = 0):
    """w = mu + softplus(rho) * eps for every segment and the two log-densities (see rg_bbb_sample); seed None: eps is read
    (the explicit-noise path), else drawn and written.  terms: 2 doubles for bbb_elbo_head."""
    _chk_dev(log_prior, log_post, terms, workspace)
    chunks = bbb_chunks(table)
    assert terms.dtype == workspace.dtype == torch.float64 and terms.numel() >= 2 and workspace.numel() >= 2 * chunks
    assert log_prior.dtype == log_post.dtype == F32
    _run("rg_bbb_sample", dict(chunks=chunks, draw=seed is not None),
         lambda: L.lib().rg_bbb_sample(ctypes.byref(table), float(prior_var), int(seed is not None), int(seed or 0), int(sample),
                                       L.ptr(log_prior), L.ptr(log_post), L.ptr(terms), L.ptr(workspace), L.stream_ptr()))


def bbb_elbo_head_partials(batch: int) -> int:
    return int(L.lib().rg_bbb_elbo_head_partials(batch))


def bbb_elbo_head(out, target, noise_tol: float, terms, acc, result, workspace, dout=None, scale: float = 1.0,
                  accumulate: bool = False):
    """the ELBO's likelihood, the loss and d loss / d out for one sample (see rg_bbb_elbo_head): out [B, 1] or [B], target
    [B]; result [4] = the loss, log_prior, log_post, log_like (means over the samples so far)"""
    _chk_dev(out, target, terms, acc, result, workspace, dout)
    B = target.numel()
    ld = out.stride(0) if out.dim() == 2 else 1
    assert out.shape[0] == B and out.numel() == B and out.dtype == target.dtype == result.dtype == F32 and target.is_contiguous()
    assert acc.dtype == torch.float64 and acc.numel() >= 4 and result.numel() >= 4
    assert workspace.dtype == torch.float64 and workspace.numel() >= bbb_elbo_head_partials(B)
    assert dout is None or (dout.dtype == F32 and dout.is_contiguous() and dout.numel() == B)
    _run("rg_bbb_elbo_head", dict(B=B),
         lambda: L.lib().rg_bbb_elbo_head(L.ptr(out), ld, L.ptr(target), B, float(noise_tol), float(scale), int(accumulate),
                                          L.ptr(terms), L.ptr(acc), L.ptr(result), L.ptr(dout), L.ptr(workspace), L.stream_ptr()))


def bbb_grad(table, prior_var: float, scale: float = 1.0, accumulate: bool = False):
    """d loss / d mu and d loss / d rho of every segment from its dw = d (-log_like) / d w (see rg_bbb_grad)"""
    _run("rg_bbb_grad", dict(chunks=bbb_chunks(table)),
         lambda: L.lib().rg_bbb_grad(ctypes.byref(table), float(prior_var), float(scale), int(accumulate), L.stream_ptr()))


def bandit_reward_head_workspace(batch: int) -> int:
    """doubles of workspace rg_bandit_reward_head asks for"""
    return int(L.lib().rg_bandit_reward_head_workspace(batch))


def bandit_reward_head(q, action, reward, predicted_reward, loss, n_kept, workspace, action_prob=None, loss_type: int = 0,
                       threshold: Optional[float] = None, apply_threshold: bool = True, unweighted_loss=None, dq=None):
    """the bandit reward trainer behind its [B, A] forward (see rg_bandit_reward_head): the logged action's prediction, the
    loss over the kept rows (weighted by 1 / action_prob when given), the unweighted loss, n_kept and d loss / d q"""
    _chk_dev(q, action, reward, predicted_reward, loss, n_kept, workspace, action_prob, unweighted_loss, dq)
    B, A = q.shape
    if B * A >= 1 << 31:
        raise NotImplementedError(f"bandit_reward_head: batch * actions = {B * A} is not supported (below 2^31)")
    assert action.shape == (B, A) and q.dtype == action.dtype == reward.dtype == F32
    assert reward.numel() == B and reward.is_contiguous() and predicted_reward.numel() == B and predicted_reward.is_contiguous()
    assert action_prob is None or (action_prob.dtype == F32 and action_prob.numel() == B and action_prob.is_contiguous())
    assert n_kept.dtype == torch.int32 and workspace.dtype == torch.float64
    assert workspace.numel() >= bandit_reward_head_workspace(B)
    assert dq is None or (dq.shape == (B, A) and dq.dtype == F32)
    _run("rg_bandit_reward_head", dict(B=B, A=A, train=dq is not None),
         lambda: L.lib().rg_bandit_reward_head(L.ptr(q), _ld(q), L.ptr(action), _ld(action), L.ptr(reward), L.ptr(action_prob),
                                               int(loss_type), int(threshold is not None),
                                               float(threshold) if threshold is not None else 0.0, int(apply_threshold), B, A,
                                               L.ptr(predicted_reward), L.ptr(loss), L.ptr(unweighted_loss), L.ptr(n_kept),
                                               L.ptr(dq), _ld(dq) if dq is not None else 0, L.ptr(workspace), L.stream_ptr()))


# ---- multi-head self-attention and the transformer reward net's joins (attention.hip) ---------------------------------------
def _rows_f32(t, rows, cols, what):
    assert t.dtype == F32 and t.shape == (rows, cols) and t.stride(1) == 1, (what, t.dtype, t.shape, t.stride())
    return t.stride(0)


def _attn_check(T: int, B: int, E: int, nhead: int):
    if nhead < 1 or E % nhead != 0:
        raise NotImplementedError(f"attention: nhead {nhead} does not divide the embedding width {E}")
    if not 1 <= T <= L.ATTN_MAX_SEQ_LEN:
        raise NotImplementedError(f"attention: seq_len {T} is not supported (1 .. {L.ATTN_MAX_SEQ_LEN}: a lane per key)")
    if E > L.ATTN_MAX_EMBED or E // nhead > L.ATTN_MAX_HEAD_DIM:
        raise NotImplementedError(f"attention: width {E} with {nhead} heads is not supported (width up to {L.ATTN_MAX_EMBED}, "
                                  f"head width up to {L.ATTN_MAX_HEAD_DIM})")
    if T * B >= 1 << 29 or B * nhead >= 1 << 29:
        raise NotImplementedError(f"attention: seq_len * batch = {T * B} is not supported (below 2^29)")


def attn_forward(q, k, v, seq_len: int, batch: int, nhead: int, ctx, p=None):
    """ctx [T * B, E] = softmax(q k^T / sqrt(E / nhead)) v per (b, head), rows ordered (t, b) (see rg_attn_forward); q, k, v
    and ctx are fp32 [T * B, E] views with their own pitches; p (optional) [B, nhead, T, T] contiguous = the probabilities"""
    _chk_dev(q, k, v, ctx, p)
    T, B, E = int(seq_len), int(batch), q.shape[1]
    _attn_check(T, B, E, nhead)
    ld = [_rows_f32(t, T * B, E, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (ctx, "ctx"))]
    if p is not None:
        _f32_flat(p, B * nhead * T * T)
    _run("rg_attn_forward", dict(T=T, B=B, E=E, nhead=nhead),
         lambda: L.lib().rg_attn_forward(L.ptr(q), ld[0], L.ptr(k), ld[1], L.ptr(v), ld[2], T, B, E, int(nhead), L.ptr(ctx), ld[3],
                                         L.ptr(p), L.stream_ptr()))


def attn_backward(dctx, q, k, v, p, seq_len: int, batch: int, nhead: int, dq, dk, dv):
    """dq, dk, dv [T * B, E] (written entirely; their own pitches) from d loss / d ctx, the forward's operands and its
    probabilities p [B, nhead, T, T] (see rg_attn_backward)"""
    _chk_dev(dctx, q, k, v, p, dq, dk, dv)
    T, B, E = int(seq_len), int(batch), q.shape[1]
    _attn_check(T, B, E, nhead)
    ld = [_rows_f32(t, T * B, E, n) for t, n in ((dctx, "dctx"), (q, "q"), (k, "k"), (v, "v"), (dq, "dq"), (dk, "dk"), (dv, "dv"))]
    _f32_flat(p, B * nhead * T * T)
    _run("rg_attn_backward", dict(T=T, B=B, E=E, nhead=nhead),
         lambda: L.lib().rg_attn_backward(L.ptr(dctx), ld[0], L.ptr(q), ld[1], L.ptr(k), ld[2], L.ptr(v), ld[3], L.ptr(p), T, B, E,
                                          int(nhead), L.ptr(dq), ld[4], L.ptr(dk), ld[5], L.ptr(dv), ld[6], L.stream_ptr()))


def residual_join(a, out, seq_len: int, batch: int, b=None, pe=None, relu: bool = False):
    """out = act((a + b) + pe[row // batch]) on fp32 [T * B, E] views (see rg_residual_join): b and pe [>= T, E] optional, act
    relu or linear, each element fp32 adds in that order"""
    _chk_dev(a, out, b, pe)
    T, B, E = int(seq_len), int(batch), a.shape[1]
    if T * B >= 1 << 29:
        raise NotImplementedError(f"residual_join: seq_len * batch = {T * B} is not supported (below 2^29)")
    lda, ldo = _rows_f32(a, T * B, E, "a"), _rows_f32(out, T * B, E, "out")
    ldb = _rows_f32(b, T * B, E, "b") if b is not None else 0
    if pe is not None:
        assert pe.dtype == F32 and pe.dim() == 2 and pe.shape[0] >= T and pe.shape[1] == E and pe.stride(1) == 1, pe.shape
    _run("rg_residual_join", dict(N=T * B, E=E),
         lambda: L.lib().rg_residual_join(L.ptr(a), lda, L.ptr(b), ldb, L.ptr(pe), pe.stride(0) if pe is not None else 0, T, B, E,
                                          L.ACT["relu"] if relu else L.ACT["linear"], L.ptr(out), ldo, L.stream_ptr()))


def residual_join_backward(grads, dx, out=None):
    """dx = (((g0 + g1) + g2) + g3) over the one to four fp32 [N, E] gradient streams of grads, in their order, where the
    join's saved relu output out is positive (out=None: a linear join) (see rg_residual_join_backward)"""
    grads = list(grads)
    assert 1 <= len(grads) <= 4, len(grads)
    _chk_dev(dx, out, *grads)
    N, E = dx.shape
    if N >= 1 << 29:
        raise NotImplementedError(f"residual_join_backward: {N} rows are not supported (below 2^29)")
    ld_dx = _rows_f32(dx, N, E, "dx")
    ldo = _rows_f32(out, N, E, "out") if out is not None else 0
    gs = [(L.ptr(g), _rows_f32(g, N, E, "grad")) for g in grads] + [(None, 0)] * (4 - len(grads))
    _run("rg_residual_join_backward", dict(N=N, E=E, streams=len(grads)),
         lambda: L.lib().rg_residual_join_backward(L.ptr(out), ldo, gs[0][0], gs[0][1], gs[1][0], gs[1][1], gs[2][0], gs[2][1],
                                                   gs[3][0], gs[3][1], N, E, L.ptr(dx), ld_dx, L.stream_ptr()))


# ---- Seq2Slate behind its encoder: embedding join, Frechet-sort likelihood and ranking (seq2slate.hip) ----------------------
def _s2s_check(S: int, T: int, B: int, E: int):
    if not 1 <= S <= L.S2S_MAX_SEQ_LEN:
        raise NotImplementedError(f"seq2slate: src_seq_len {S} is not supported (1 .. {L.S2S_MAX_SEQ_LEN}: a lane per candidate)")
    if not 1 <= T <= S:
        raise NotImplementedError(f"seq2slate: tgt_seq_len {T} is not supported (1 .. src_seq_len = {S})")
    if not 1 <= E <= L.S2S_MAX_EMBED:
        raise NotImplementedError(f"seq2slate: dim_model {E} is not supported (1 .. {L.S2S_MAX_EMBED})")
    if B < 1 or S * B >= 1 << 29:
        raise NotImplementedError(f"seq2slate: src_seq_len * batch = {S * B} is not supported (1 .. below 2^29)")


def s2s_embed_join(state_embed, cand_embed, seq_len: int, batch: int, src_embed):
    """src_embed [S * B, Es + Ec] = (sqrt(Es) * state_embed[b] | sqrt(Ec) * cand_embed[(s, b)]), rows ordered (s, b) (see
    rg_s2s_embed_join); state_embed [B, Es], cand_embed [S * B, Ec], fp32 views with their own pitches"""
    _chk_dev(state_embed, cand_embed, src_embed)
    S, B, Es, Ec = int(seq_len), int(batch), state_embed.shape[1], cand_embed.shape[1]
    _s2s_check(S, 1, B, Es + Ec)
    ld = [_rows_f32(state_embed, B, Es, "state_embed"), _rows_f32(cand_embed, S * B, Ec, "cand_embed"),
          _rows_f32(src_embed, S * B, Es + Ec, "src_embed")]
    _run("rg_s2s_embed_join", dict(N=S * B, Es=Es, Ec=Ec),
         lambda: L.lib().rg_s2s_embed_join(L.ptr(state_embed), ld[0], L.ptr(cand_embed), ld[1], S, B, Es, Ec, L.ptr(src_embed),
                                           ld[2], L.stream_ptr()))


def s2s_embed_join_backward(d_src_embed, seq_len: int, batch: int, d_state_embed, d_cand_embed):
    """d_state_embed [B, Es] = sqrt(Es) * the sum over s (ascending) of d_src_embed's left Es columns, d_cand_embed [S * B, Ec]
    = sqrt(Ec) * its right Ec columns (see rg_s2s_embed_join_backward)"""
    _chk_dev(d_src_embed, d_state_embed, d_cand_embed)
    S, B, Es, Ec = int(seq_len), int(batch), d_state_embed.shape[1], d_cand_embed.shape[1]
    _s2s_check(S, 1, B, Es + Ec)
    ld = [_rows_f32(d_src_embed, S * B, Es + Ec, "d_src_embed"), _rows_f32(d_state_embed, B, Es, "d_state_embed"),
          _rows_f32(d_cand_embed, S * B, Ec, "d_cand_embed")]
    _run("rg_s2s_embed_join_backward", dict(N=S * B, Es=Es, Ec=Ec),
         lambda: L.lib().rg_s2s_embed_join_backward(L.ptr(d_src_embed), ld[0], S, B, Es, Ec, L.ptr(d_state_embed), ld[1],
                                                    L.ptr(d_cand_embed), ld[2], L.stream_ptr()))


def frechet_head_workspace(batch: int, embed: int) -> int:
    """doubles of workspace rg_frechet_head asks for"""
    return int(L.lib().rg_frechet_head_workspace(batch, embed))


def _s2s_scorer(w, bias, E):
    assert w.dtype == F32 and w.is_contiguous() and w.numel() == E, ("encoder_scorer.weight", w.dtype, w.shape)
    assert bias.dtype == F32 and bias.numel() == 1, ("encoder_scorer.bias", bias.dtype, bias.shape)


def frechet_head(mem, w, bias, tgt_out_idx, seq_len: int, batch: int, log_prob, p, workspace, logged=None, reward=None,
                 baseline=None, clamp_method: int = 0, clamp_max: float = 0.0, impt=None, clamped=None, sums=None, dscore=None,
                 dmem=None, dw=None, dbias=None):
    """the Frechet-sort sequence likelihood behind the encoder and Seq2SlateTrainer's loss (see rg_frechet_head): mem [S * B, E]
    rows (s, b), w [E] and bias [1] the encoder scorer, tgt_out_idx [B, T] int64 offset by 2; log_prob, p [B].  With logged and
    reward [B] (baseline [B] optional): impt, clamped [B] and sums [3] = the loss and the unclamped and clamped IPS means;
    with dscore [B, S], dmem [S * B, E], dw [E] and dbias [1] the loss's gradients"""
    _chk_dev(mem, w, bias, tgt_out_idx, log_prob, p, workspace, logged, reward, baseline, impt, clamped, sums, dscore, dmem, dw,
             dbias)
    S, B, E = int(seq_len), int(batch), mem.shape[1]
    assert tgt_out_idx.dtype == torch.int64 and tgt_out_idx.dim() == 2 and tgt_out_idx.shape[0] == B, tgt_out_idx.shape
    assert tgt_out_idx.stride(1) == 1
    T = tgt_out_idx.shape[1]
    _s2s_check(S, T, B, E)
    ld_mem = _rows_f32(mem, S * B, E, "mem")
    _s2s_scorer(w, bias, E)
    for t in (log_prob, p, logged, reward, baseline, impt, clamped):
        _f32_flat(t, B)
    _f32_flat(sums, 3)
    assert workspace.dtype == torch.float64 and workspace.is_contiguous() and workspace.numel() >= frechet_head_workspace(B, E)
    train = dscore is not None
    assert all((t is not None) == train for t in (dmem, dw, dbias)), "dscore, dmem, dw and dbias come together"
    assert (logged is None) == (reward is None) == (impt is None) == (clamped is None) == (sums is None)
    assert logged is not None or (baseline is None and not train), "the loss needs logged propensities and rewards"
    ld_ds = _rows_f32(dscore, B, S, "dscore") if train else 0
    ld_dm = _rows_f32(dmem, S * B, E, "dmem") if train else 0
    if train:
        _f32_flat(dw, E)
        _f32_flat(dbias, 1)
    _run("rg_frechet_head", dict(S=S, T=T, B=B, E=E, train=train),
         lambda: L.lib().rg_frechet_head(L.ptr(mem), ld_mem, L.ptr(w), L.ptr(bias), L.ptr(tgt_out_idx), tgt_out_idx.stride(0),
                                         L.ptr(logged), L.ptr(reward), L.ptr(baseline), int(clamp_method), float(clamp_max), S, T,
                                         B, E, L.ptr(log_prob), L.ptr(p), L.ptr(impt), L.ptr(clamped), L.ptr(sums), L.ptr(dscore),
                                         ld_ds, L.ptr(dmem), ld_dm, L.ptr(dw), L.ptr(dbias), L.ptr(workspace), L.stream_ptr()))


def frechet_rank(mode: int, seq_len: int, batch: int, ranked_tgt_out_idx, ranked_per_symbol_probs, ranked_per_seq_probs,
                 scores=None, mem=None, w=None, bias=None, seed: int = 0):
    """RANK_MODE in one launch (see rg_frechet_rank): from scores [B, S], or from mem [S * B, E], w [E] and bias [1]; mode
    L.FRECHET_RANK_ENCODER / _GREEDY (argsort, one-hot probabilities) or _SAMPLED (draws without replacement keyed by seed).
    ranked_tgt_out_idx [B, T] int64 (offset by 2), ranked_per_symbol_probs [B, T, S + 2], ranked_per_seq_probs [B]"""
    _chk_dev(ranked_tgt_out_idx, ranked_per_symbol_probs, ranked_per_seq_probs, scores, mem, w, bias)
    S, B = int(seq_len), int(batch)
    assert ranked_tgt_out_idx.dtype == torch.int64 and ranked_tgt_out_idx.dim() == 2 and ranked_tgt_out_idx.is_contiguous()
    assert ranked_tgt_out_idx.shape[0] == B, ranked_tgt_out_idx.shape
    T = ranked_tgt_out_idx.shape[1]
    assert (scores is None) != (mem is None), "scores, or mem with the scorer"
    E = mem.shape[1] if mem is not None else 1
    _s2s_check(S, T, B, E)
    if mode not in (L.FRECHET_RANK_ENCODER, L.FRECHET_RANK_GREEDY, L.FRECHET_RANK_SAMPLED):
        raise NotImplementedError(f"frechet_rank: mode {mode} is not one of the three ranking modes")
    ld_s = _rows_f32(scores, B, S, "scores") if scores is not None else 0
    ld_m = _rows_f32(mem, S * B, E, "mem") if mem is not None else 0
    if mem is not None:
        _s2s_scorer(w, bias, E)
    _f32_flat(ranked_per_symbol_probs, B * T * (S + 2))
    _f32_flat(ranked_per_seq_probs, B)
    _run("rg_frechet_rank", dict(S=S, T=T, B=B, E=E, mode=int(mode)),
         lambda: L.lib().rg_frechet_rank(L.ptr(scores), ld_s, L.ptr(mem), ld_m, L.ptr(w), L.ptr(bias), int(mode),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, S, T, B, E, L.ptr(ranked_tgt_out_idx),
                                         L.ptr(ranked_per_symbol_probs), L.ptr(ranked_per_seq_probs), L.stream_ptr()))
