"""The parametric DQN step's kernels: the tiled two-panel fused forward (rg_mlp_desc.x_tile), rg_tile_concat and
rg_pdqn_head.  The first two only move data — the tiled forward has the BITS of the existing two-panel forward on the
materialised tiled state, rg_tile_concat those of torch.cat — so no tolerance applies there.  The head is held against a
torch restatement of the reference's lines (dqn_trainer_base.py:33-77, parametric_dqn_trainer.py:112-171) with the
tolerances tests/test_sac_heads.py uses for the same kind of head: target 1e-6, dq 1e-8, loss 1e-5; the selected index and
next_q exact.

Fully masked rows that are NOT terminal carry the -1e9 penalty into the target: the reference's own loss is then of the
order 1e16 (mse) or 1e9 / B (huber), where neighbouring fp32 values are 1e9 and 64 apart, so an absolute 1e-5 cannot be
stated for the LOSS of those cases by any fp32 implementation, the reference against a re-ordered sum of itself included.
Those cases (B a power of two, so that 2 / B is exact in every evaluation order) hold target and dq to the same absolute
1e-6 / 1e-8 — i.e. to the bit at that magnitude — and the loss to 1e-5 of its own magnitude; every other case holds the
loss to the absolute 1e-5."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.engine import FusedMLP, make_stack


def _stack(S, A, H, n_hidden, prec, dev, seed=1):
    dims = [S + A] + [H] * n_hidden + [1]
    g = torch.Generator().manual_seed(seed)
    ws = [torch.nn.Parameter((torch.randn(o, i, generator=g) * (1.5 / i ** 0.5)).to(dev)) for i, o in zip(dims, dims[1:])]
    bs = [torch.nn.Parameter((torch.randn(o, generator=g) * 0.1).to(dev)) for o in dims[1:]]
    st = make_stack(ws, bs, [L.ACT["relu"]] * n_hidden + [L.ACT["linear"]], prec)
    assert isinstance(st, FusedMLP)
    st.stage_weights(need_transposed=False)
    return st


# (hidden width, precision, M, tiled rows R, state width, candidate width, state dtype): rows that are and are not
# multiples of the 128- / 64-row tiles, M not dividing the tile height (3, 130: a tile starts in the middle of a state's
# candidates, one state spans several tiles), a last state with fewer than M candidates (R % M != 0)
TILED = [
    (256, L.PREC_BF16, 1, 200, 32, 8, torch.float32),
    (256, L.PREC_BF16, 3, 384, 64, 8, torch.float32),
    (256, L.PREC_BF16, 8, 256, 32, 16, torch.bfloat16),
    (256, L.PREC_BF16, 130, 390, 64, 5, torch.float32),
    (512, L.PREC_BF16, 3, 301, 96, 32, torch.bfloat16),
    (512, L.PREC_BF16, 8, 640, 256, 32, torch.float32),
    (256, L.PREC_BF16X3, 1, 64, 32, 8, torch.float32),
    (256, L.PREC_BF16X3, 3, 200, 64, 8, torch.bfloat16),
    (256, L.PREC_BF16X3, 8, 192, 32, 16, torch.float32),
    (512, L.PREC_BF16X3, 130, 261, 64, 7, torch.float32),
    (512, L.PREC_BF16X3, 8, 128, 256, 32, torch.bfloat16),
    (512, L.PREC_BF16X3, 3, 100, 32, 9, torch.float32),
]


@pytest.mark.parametrize("H,prec,M,R,S,A,sdt", TILED)
def test_tiled_forward_has_the_bits_of_the_two_panel_forward(backend, H, prec, M, R, S, A, sdt):
    dev = backend.device
    st = _stack(S, A, H, 2, prec, dev)
    g = torch.Generator().manual_seed(7)
    n_states = (R + M - 1) // M
    state = torch.randn(n_states, S, generator=g).to(sdt).to(dev)
    cand = torch.randn(R, A, generator=g).to(dev)
    want = torch.zeros(R, 1, device=dev)
    st.forward(state.repeat_interleave(M, 0)[:R].contiguous(), want, save=False, x2=cand)
    got = torch.full((R, 1), float("nan"), device=dev)
    st.forward(state, got, save=False, x2=cand, x_tile=M)
    assert torch.equal(got.cpu().view(torch.int32), want.cpu().view(torch.int32))


def test_tiled_forward_refuses_what_it_does_not_serve(backend):
    dev = backend.device
    S, A, M, R = 32, 8, 4, 128
    lib = L.lib()
    for prec in (L.PREC_BF16, L.PREC_BF16X3):
        st = _stack(S, A, 256, 2, prec, dev)
        state, cand, out = torch.randn(R // M, S).to(dev), torch.randn(R, A).to(dev), torch.zeros(R, 1).to(dev)
        st._ensure_ws(R, dev, training=True)  # (the saving forms are refused for being tiled, not for lacking a workspace)
        d = st._fill_desc()

        def call(save=0, x2=True, rowmap=None, tile_key=None, row_begin=None, n_groups=0):
            d.x2, d.ldx2, d.x_split, d.x2_dtype = (cand.data_ptr(), cand.stride(0), S, L.DT_F32) if x2 else (None, 0, 0, 0)
            d.x_tile = M
            d.rowmap = rowmap.data_ptr() if rowmap is not None else None
            d.tile_key = tile_key.data_ptr() if tile_key is not None else None
            d.row_begin = row_begin.data_ptr() if row_begin is not None else None
            d.n_groups = n_groups
            rc = lib.rg_mlp_forward_fused(d, state.data_ptr(), L.DT_F32, state.stride(0), R, out.data_ptr(), out.stride(0), save,
                                          L.stream_ptr())
            d.x_tile, d.rowmap, d.tile_key, d.row_begin, d.n_groups = 0, None, None, None, 0
            return rc

        rowmap = torch.arange(R, dtype=torch.int32).to(dev)
        tile_key, row_begin = torch.zeros(1, dtype=torch.int32).to(dev), torch.tensor([0, R], dtype=torch.int32).to(dev)
        assert call() == 0
        assert call(x2=False) == -1                       # RG_EINVAL: x_tile > 1 without x2
        assert call(save=1) == L.EUNSUPPORTED and call(save=2) == L.EUNSUPPORTED
        assert call(rowmap=rowmap) == L.EUNSUPPORTED
        assert call(rowmap=rowmap, tile_key=tile_key, row_begin=row_begin, n_groups=1) == L.EUNSUPPORTED
    with pytest.raises(ValueError):
        st.forward(state, out, x_tile=M)
    # the paired DQN forward: a 16-wide bf16 stack whose descriptor asks for a tiled panel is refused
    dims = [S, 256, 256, 16]
    g = torch.Generator().manual_seed(3)
    ws = [torch.nn.Parameter(torch.randn(o, i, generator=g).to(dev) * 0.05) for i, o in zip(dims, dims[1:])]
    bs = [torch.nn.Parameter(torch.zeros(o).to(dev)) for o in dims[1:]]
    sp = make_stack(ws, bs, [L.ACT["relu"]] * 2 + [L.ACT["linear"]], L.PREC_BF16)
    sp.stage_weights(need_transposed=True)
    B = 128
    sp._ensure_ws(B, dev, training=True)
    d = sp._fill_desc()
    f = lambda *s: torch.zeros(*s).to(dev)  # noqa: E731
    x, q, qn, qt, act, mask, rew, nt, dq = f(B, S), f(B, 16), f(B, 16), f(B, 16), f(B, 16), f(B, 16), f(B), f(B), f(B, 16)
    ws_ = f(ops.dqn_pair_wave_sums(B))

    def pair():
        return lib.rg_dqn_online_pair_forward(d, x.data_ptr(), L.DT_F32, S, x.data_ptr(), L.DT_F32, S, B, q.data_ptr(),
                                              qn.data_ptr(), qt.data_ptr(), act.data_ptr(), mask.data_ptr(), rew.data_ptr(), None,
                                              nt.data_ptr(), 0.9, None, 1, 0, dq.data_ptr(), ws_.data_ptr(), None, None, None,
                                              L.stream_ptr())

    assert pair() == 0
    d.x_tile = 2
    assert pair() == L.EUNSUPPORTED
    d.x_tile = 0


# aligned and odd widths and pitches: (R, M, S, A, state pitch pad, candidate pitch pad, output pitch pad, base offset)
CONCAT = [
    (64, 1, 8, 4, 0, 0, 0, 0),       # every access 16 bytes
    (300, 8, 256, 32, 0, 0, 0, 0),
    (37, 5, 6, 3, 0, 0, 0, 0),       # odd widths: scalar
    (50, 3, 8, 6, 0, 2, 0, 0),       # state panel vector, candidate pitch 8 with a 2-element tail
    (50, 3, 7, 8, 1, 0, 1, 0),       # state width 7: the candidate panel lands on an odd column
    (41, 4, 12, 8, 4, 4, 4, 1),      # aligned pitches, bases off by 4 bytes
    (33, 130, 16, 5, 0, 3, 3, 0),    # M > rows of a block; odd output pitch
    (1, 1, 1, 1, 0, 0, 0, 0),
]


@pytest.mark.parametrize("R,M,S,A,ps,pa,po,off", CONCAT)
def test_tile_concat_is_torch_cat(backend, R, M, S, A, ps, pa, po, off):
    dev = backend.device
    g = torch.Generator().manual_seed(R + M)
    n = (R + M - 1) // M

    def view(rows, cols, pad):
        flat = torch.randn(rows * (cols + pad) + off, generator=g).to(dev)
        return flat[off:].view(rows, cols + pad)[:, :cols]

    x, x2, out = view(n, S, ps), view(R, A, pa), view(R, S + A, po)
    base = out._base
    before = base.clone()
    ops.tile_concat(x, x2, out, x_tile=M)
    want = torch.cat((x.repeat_interleave(M, 0)[:R], x2), 1)
    assert torch.equal(out.cpu().view(torch.int32), want.cpu().view(torch.int32))
    if po:  # the padding of every output row is what it was
        pad_now = base[off:].view(R, S + A + po)[:, S + A:]
        pad_was = before[off:].view(R, S + A + po)[:, S + A:]
        assert torch.equal(pad_now.cpu(), pad_was.cpu())


def _head_ref(q, qo, qt, mask, reward, nt, gamma, ge, double_q, loss):
    """parametric_dqn_trainer.py:112-171 + dqn_trainer_base.py:33-77 in torch fp32 (CPU)"""
    B = q.numel()
    reward, nt, q = reward.reshape(B, 1), nt.reshape(B, 1), q.reshape(B, 1)
    discount = torch.full_like(reward, gamma) if ge is None else torch.pow(gamma, ge.reshape(B, 1).float())
    if mask is not None:
        pen = -1e9 * (1 - mask)
        qo_, qt_ = qo.reshape(mask.shape) + pen, qt.reshape(mask.shape) + pen
        if double_q:
            _, idx = torch.max(qo_, dim=1, keepdim=True)
            next_q = torch.gather(qt_, 1, idx)
        else:
            next_q, idx = torch.max(qt_, dim=1, keepdim=True)
    else:
        next_q, idx = qt.reshape(B, 1), torch.zeros(B, 1, dtype=torch.int64)
    target = reward + nt * discount * next_q
    qg = q.clone().requires_grad_(True)
    fn = {"mse": F.mse_loss, "huber": F.smooth_l1_loss, "bce": F.binary_cross_entropy_with_logits}[loss]
    lv = fn(qg, target)
    lv.backward()
    return target, qg.grad, lv.detach(), next_q, idx


def _head_inputs(B, M, seed, scale=3.0, with_exp=False):
    """values of magnitude < 32 without ties among a row's unmasked values; rows 0..3 fully masked (0, 1 terminal; 2, 3
    not), row 4 with one candidate left"""
    g = torch.Generator().manual_seed(seed)
    perm = lambda: torch.stack([torch.randperm(M, generator=g) for _ in range(B)]).float()  # noqa: E731
    qo = ((perm() + torch.rand(B, M, generator=g) * 0.5) / M - 0.5) * 2 * scale
    qt = ((perm() + torch.rand(B, M, generator=g) * 0.5) / M - 0.5) * 2 * scale
    mask = (torch.rand(B, M, generator=g) > 0.4).float()
    mask[torch.arange(B), torch.randint(M, (B,), generator=g)] = 1.0
    nt = (torch.rand(B, generator=g) > 0.2).float()
    if B > 4:
        mask[:4] = 0.0
        nt[:2], nt[2:4] = 0.0, 1.0
        mask[4] = 0.0
        mask[4, M // 2] = 1.0
    ge = torch.randint(1, 5, (B,), generator=g).float() if with_exp else None
    if ge is not None and B > 4:
        ge[2:4] = 1.0  # the rows whose target is of magnitude 1e9: gamma ** 1 is gamma in every pow
    return dict(q=torch.randn(B, generator=g) * scale, qo=qo.reshape(-1), qt=qt.reshape(-1), mask=mask,
                reward=torch.rand(B, generator=g), nt=nt, ge=ge)


HEAD = [
    # (B, M, loss, double_q, exponent, maxq, rows 2 and 3 — fully masked — not terminal)
    (300, 5, "mse", True, False, True, False),
    (300, 5, "huber", False, False, True, False),
    (257, 8, "huber", True, True, True, False),     # time_diff / step exponent
    (513, 7, "mse", False, True, True, False),
    (256, 130, "mse", True, False, True, True),     # M beyond a wave
    (128, 6, "huber", False, True, True, True),
    (64, 3, "mse", False, True, True, True),
    (100, 1, "mse", True, False, True, False),      # M = 1
    (64, 1, "huber", False, True, True, True),
    (513, 3, "mse", True, True, False, False),      # SARSA
    (64, 4, "huber", True, False, False, False),
]


@pytest.mark.parametrize("B,M,loss,double_q,with_exp,maxq,live_masked", HEAD)
def test_pdqn_head_matches_the_restated_reference(backend, B, M, loss, double_q, with_exp, maxq, live_masked):
    dev = backend.device
    i = _head_inputs(B, M, seed=B + M, with_exp=with_exp)
    gamma = 0.9
    if not maxq:
        i["qt"], i["qo"], i["mask"] = i["qt"].reshape(B, M)[:, 0].contiguous(), None, None
    assert not live_masked or (maxq and B & (B - 1) == 0)
    if not live_masked:
        i["nt"][2:4] = 0.0  # (they stay fully masked)
    want = _head_ref(i["q"], i["qo"], i["qt"], i["mask"], i["reward"], i["nt"], gamma, i["ge"], double_q, loss)
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    f = lambda *s: torch.full(s, float("nan")).to(dev)  # noqa: E731
    target, dq, nq, parts, out = f(B), f(B), f(B), f(ops.pdqn_head_partials(B)), f(1)
    idx = torch.full((B,), -1, dtype=torch.int64).to(dev)
    ops.pdqn_head(t(i["q"]), t(i["qo"]), t(i["qt"]), t(i["mask"]), t(i["reward"]), t(i["nt"]), gamma, t(i["ge"]), double_q,
                  L.LOSS[loss], target, dq, parts, nq, idx)
    ops.reduce_sum(parts, parts.numel(), 1.0 / B, out)
    assert torch.equal(idx.cpu(), want[4].reshape(-1))
    assert torch.equal(nq.cpu(), want[3].reshape(-1))
    if maxq:
        assert (nq.cpu()[:4] == -1e9).all() and (idx.cpu()[:4] == 0).all()  # fully masked: index 0, exactly -1e9
    assert (target.cpu() - want[0].reshape(-1)).abs().max() <= 1e-6
    assert (dq.cpu() - want[1].reshape(-1)).abs().max() <= 1e-8
    assert abs(out.item() - want[2].item()) <= (1e-5 * abs(want[2].item()) if live_masked else 1e-5)


@pytest.mark.parametrize("B,M", [(200, 4), (64, 1)])
def test_pdqn_head_bce_with_logits(backend, B, M):
    """gamma = 0, rewards in [0, 1]: the target is the reward, the loss F.binary_cross_entropy_with_logits"""
    dev = backend.device
    i = _head_inputs(B, M, seed=11)
    i["q"] = i["q"] * 4  # logits out to +-30: the stable form's range
    want = _head_ref(i["q"], i["qo"], i["qt"], i["mask"], i["reward"], i["nt"], 0.0, None, True, "bce")
    t = lambda x: x.to(dev)  # noqa: E731
    f = lambda *s: torch.full(s, float("nan")).to(dev)  # noqa: E731
    target, dq, nq, parts, out = f(B), f(B), f(B), f(ops.pdqn_head_partials(B)), f(1)
    ops.pdqn_head(t(i["q"]), t(i["qo"]), t(i["qt"]), t(i["mask"]), t(i["reward"]), t(i["nt"]), 0.0, None, True,
                  L.LOSS_BCE_LOGITS, target, dq, parts, nq, None)
    ops.reduce_sum(parts, parts.numel(), 1.0 / B, out)
    assert torch.equal(target.cpu(), i["reward"])
    assert torch.equal(nq.cpu(), want[3].reshape(-1))
    assert (dq.cpu() - want[1].reshape(-1)).abs().max() <= 1e-8
    assert abs(out.item() - want[2].item()) <= 1e-5


def test_pdqn_head_rejects_bad_arguments(backend):
    dev = backend.device
    lib = L.lib()
    z = torch.zeros(8).to(dev)
    p = z.data_ptr()
    ok = lambda **k: lib.rg_pdqn_head(p, k.get("qo", p), p, k.get("mask", p), p, p, 0.9, None, k.get("B", 2), k.get("M", 2),  # noqa: E731
                                      k.get("maxq", 1), k.get("dq_", 1), k.get("loss", 0), p, p, p, p, None, L.stream_ptr())
    assert ok() == 0
    assert ok(loss=3) == -1 and ok(B=0) == -1 and ok(M=0) == -1 and ok(mask=None) == -1 and ok(qo=None) == -1
    assert ok(qo=None, dq_=0) == 0 and ok(maxq=0, qo=None, mask=None) == 0
    assert lib.rg_tile_concat(p, 2, p, 2, 2, 0, 2, 2, p, 4, L.stream_ptr()) == -1  # x_tile < 1
    assert lib.rg_tile_concat(p, 2, p, 2, 2, 1, 2, 2, p, 3, L.stream_ptr()) == -1  # output pitch < width
    assert ctypes.sizeof(L.MlpDesc) % 8 == 0 and L.MlpDesc.x_tile.offset == L.MlpDesc.sum_run.offset + 4
