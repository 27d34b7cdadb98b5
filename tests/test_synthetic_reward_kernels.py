"""The synthetic-reward kernels (reagent_amd/csrc/synthetic_reward.hip): rg_ngram_concat and rg_step_reward_head.

rg_ngram_concat is a copy and is held to bit equality with the torch statement of the reference's ngram()
(reagent_amd.models.synthetic_reward.ngram); where the window reaches past the sequence on both sides (n // 2 > T, where the
reference raises) it is held to "pad cat(state, action) with n // 2 zero steps on both sides and take windows".

rg_step_reward_head is held to the reference's lines (synthetic_reward.py:245-266 behind a Linear(P, 1) + activation,
reward_network_trainer.py:27-66) in float64 under autograd with the self-calibrating bound of tests/test_lstm_kernels.py:
the larger of 4 x torch's own fp32 error against float64 on those inputs and 4 ulp (fp32) of the quantity's largest magnitude;
and to exact statements on small-integer inputs, where every partial sum is an fp32 integer."""
import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.models.synthetic_reward import _gen_mask, ngram

from test_lstm_kernels import _bits, _close

ACT_MODULES = {"linear": torch.nn.Identity, "relu": torch.nn.ReLU, "leaky_relu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh,
               "sigmoid": torch.nn.Sigmoid, "softplus": torch.nn.Softplus}
LOSS_MODULES = {"MSE_Loss": torch.nn.MSELoss, "SmoothL1_Loss": torch.nn.SmoothL1Loss, "L1_Loss": torch.nn.L1Loss,
                "BCE_Loss": torch.nn.BCELoss}


# ---- rg_ngram_concat -------------------------------------------------------------------------------------------------------
def _padded_windows(state, action, n):
    """pad cat(state, action) with n // 2 zero steps on both sides and take windows: total in n"""
    x = torch.cat((state, action), dim=-1)
    T, B, F = x.shape
    z = torch.zeros(n // 2, B, F)
    padded = torch.cat((z, x, z), dim=0)
    return torch.cat([padded[i:i + T] for i in range(n)], dim=-1)


def _ngram_inputs(T, B, S, A, seed=0):
    g = torch.Generator().manual_seed(10000 * T + 100 * B + 10 * S + A + seed)
    return torch.randn(T, B, S, generator=g), torch.randn(T, B, A, generator=g)


def _run_ngram(dev, state, action, n, pad=0):
    T, B, S = state.shape
    A = action.shape[2]

    def place(t):  # rows a padded pitch apart, the padding NaN
        if not pad:
            return t.to(dev).contiguous()
        buf = torch.full((T, B, t.shape[2] + pad), float("nan"), device=dev)
        buf[:, :, :t.shape[2]] = t.to(dev)
        return buf[:, :, :t.shape[2]]

    W = (S + A) * n
    out = torch.full((T, B, W + pad), float("nan"), device=dev)[:, :, :W]
    ops.ngram_concat(place(state), place(action), n, out)
    return out.cpu()


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("S,A", [(1, 1), (4, 3), (33, 31)])
def test_ngram_concat_has_the_bits_of_the_torch_statement(backend, S, A, B):
    for T in (1, 2, 3, 7):
        state, action = _ngram_inputs(T, B, S, A)
        for n in (1, 3, 5, 7):
            got = _run_ngram(backend.device, state, action, n)
            assert not torch.isnan(got).any(), (T, n)  # every element is written
            want = _padded_windows(state, action, n)
            assert torch.equal(_bits(got), _bits(want)), (T, n)
            if n // 2 <= T:  # the reference's own statement runs there
                ref = ngram(torch.cat((state, action), dim=-1), n, torch.zeros(1, 1, S + A))
                assert torch.equal(_bits(got), _bits(ref)), (T, n)
            if n == 1:
                assert torch.equal(_bits(got), _bits(torch.cat((state, action), dim=-1)))


def test_ngram_concat_reads_and_writes_padded_pitches(backend):
    for T, B in ((3, 5), (1, 4), (4, 1)):
        state, action = _ngram_inputs(T, B, 4, 3, seed=1)
        state[0, 0, 0] = float("inf")
        got = _run_ngram(backend.device, state, action, 3, pad=5)
        assert torch.equal(_bits(got), _bits(_padded_windows(state, action, 3))), (T, B)


# ---- rg_step_reward_head -----------------------------------------------------------------------------------------------
def _head_statement(dtype, h, w, b, act, v, target, loss_type, threshold, apply_threshold):
    """synthetic_reward.py:245-266 behind Linear(P, 1) + activation, reward_network_trainer.py:43-64, in dtype
    -> (output, mask, pred, loss, n_kept, dh, dw, db)"""
    T, B, P = h.shape
    h_ = h.to(dtype).requires_grad_(True)
    w_, b_ = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    valid_step = v.clamp(1, T).view(B, 1)
    output = ACT_MODULES[act]()(torch.nn.functional.linear(h_, w_.view(1, P), b_)).squeeze(2).transpose(0, 1)
    mask = _gen_mask(valid_step, B, T).to(dtype)
    pred = (output * mask).sum(dim=1, keepdim=True)
    p, y = pred, target.to(dtype).view(B, 1)
    if loss_type == "BCE_Loss":
        p, y = p / valid_step, y / valid_step
    loss = LOSS_MODULES[loss_type](reduction="none")(p, y)
    if apply_threshold and threshold is not None:
        keep = target.view(B, 1) / valid_step <= threshold if loss_type == "BCE_Loss" else target.view(B, 1) <= threshold
        loss = loss[keep]
    n = loss.numel()
    loss = torch.mean(loss)
    if n:
        loss.backward()
        grads = (h_.grad, w_.grad, b_.grad)
    else:
        grads = (torch.zeros_like(h_), torch.zeros_like(w_), torch.zeros_like(b_))
    return (output.detach(), mask, pred.detach().view(B), loss.detach(), n) + grads


def _run_head(dev, h, w, b, act, v, target, loss_type, threshold=None, apply_threshold=False, grad=True):
    T, B, P = h.shape
    f = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f)  # noqa: E731
    output, mask, pred, loss = nan(B, T), nan(B, T), nan(B), nan(1)
    n_kept = torch.full((1,), -7, dtype=torch.int32, device=dev)
    dh, dw, db = (nan(T, B, P), nan(P), nan(1)) if grad else (None, None, None)
    ws = torch.empty(ops.step_reward_head_workspace(T, B, P), dtype=torch.float64, device=dev) if target is not None else None
    ops.step_reward_head(h.to(dev), w.to(dev), b.to(dev), L.ACT[act], v.to(dev), output, mask, pred,
                         target=None if target is None else target.to(dev), loss_type=L.SRW_LOSS[loss_type], threshold=threshold,
                         apply_threshold=apply_threshold, loss=loss if target is not None else None,
                         n_kept=n_kept if target is not None else None, dh=dh, dw=dw, dbias=db, workspace=ws)
    res = [output.cpu(), mask.cpu(), pred.cpu(), loss.cpu()[0], int(n_kept.cpu()[0])]
    return res + ([dh.cpu(), dw.cpu(), db.cpu()] if grad else [])


def _head_inputs(T, B, P, loss_type, act, steps="mixed", seed=0):
    g = torch.Generator().manual_seed(100000 * T + 1000 * B + 10 * P + seed)
    h = torch.tanh(torch.randn(T, B, P, generator=g))
    w, b = (torch.rand(P, generator=g) * 2 - 1) / P ** 0.5, torch.randn(1, generator=g) * 0.1
    if steps == "ones":
        v = torch.ones(B, dtype=torch.int64)
    elif steps == "full":
        v = torch.full((B,), T, dtype=torch.int64)
    elif steps == "outside":
        v = torch.tensor([0, -5, T + 1, T + 40, 2])[torch.arange(B) % 5]
    else:
        v = torch.randint(1, T + 1, (B,), generator=g)
        v[0], v[-1] = 1, T
    if loss_type == "BCE_Loss":
        # nn.BCELoss wants pred / v inside [0, 1]: z inside [0.03, 0.48], where every one of the six activations is inside
        # (0, 1) (softplus(0.48) = 0.96), and binary targets, as the reference's binary task
        h, w, b = h.abs(), torch.rand(P, generator=g) * (0.45 / P), torch.full((1,), 0.03)
        target = v.clamp(1, T).float() * torch.randint(0, 2, (B,), generator=g).float()
    else:
        target = torch.randn(B, generator=g) * 2
    return h, w, b, v.long(), target


def _same(xs, ys):
    """every pair the same: bits for tensors, equality for the count"""
    return all(x == y if isinstance(x, int) else torch.equal(_bits(x.view(-1)), _bits(y.view(-1))) for x, y in zip(xs, ys))


NAMES = ("output", "mask", "predicted_reward", "loss", "n_kept", "dh", "dw", "dbias")


def _check(backend, T, B, P, loss_type, act, steps="mixed", threshold=None, apply_threshold=False):
    h, w, b, v, target = _head_inputs(T, B, P, loss_type, act, steps)
    args = (h, w, b, act, v, target, loss_type, threshold, apply_threshold)
    r64, r32 = _head_statement(torch.float64, *args), _head_statement(torch.float32, *args)
    got = _run_head(backend.device, h, w, b, act, v, target, loss_type, threshold, apply_threshold)
    tag = f"T={T} B={B} P={P} {loss_type} {act} {steps} thr={threshold}/{apply_threshold}"
    assert got[4] == r64[4], tag
    assert torch.equal(got[1], r64[1].float()), tag
    for i in (0, 2, 3, 5, 6, 7):
        _close(got[i], r64[i], r32[i], f"{NAMES[i]} {tag}")
    # rows the mask drops are exactly zero
    off = r64[1].t() == 0
    assert not got[5][off].any(), tag
    return got, (h, w, b, v, target)


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("B", [1, 5, 33, 257])
def test_step_reward_head_against_float64_over_shapes(backend, T, B):
    for P in (1, 3, 64, 65, 130):
        _check(backend, T, B, P, "MSE_Loss", "leaky_relu")


@pytest.mark.parametrize("loss_type", ["MSE_Loss", "SmoothL1_Loss", "L1_Loss", "BCE_Loss"])
@pytest.mark.parametrize("act", ["linear", "relu", "leaky_relu", "tanh", "sigmoid", "softplus"])
def test_step_reward_head_losses_and_activations(backend, loss_type, act):
    _check(backend, 3, 33, 65, loss_type, act)


@pytest.mark.parametrize("loss_type", ["SmoothL1_Loss", "BCE_Loss"])
def test_step_reward_head_threshold(backend, loss_type):
    act = "sigmoid"
    h, w, b, v, target = _head_inputs(3, 33, 65, loss_type, act)
    shown = target / v.clamp(1, 3) if loss_type == "BCE_Loss" else target
    order = shown.sort().values
    all_rows, one_row = order[-1].item(), ((order[0] + order[order > order[0]][0]) / 2).item()
    if loss_type != "BCE_Loss":
        got, _ = _check(backend, 3, 33, 65, loss_type, act, threshold=one_row, apply_threshold=True)
        assert got[4] == 1
    got, _ = _check(backend, 3, 33, 65, loss_type, act, threshold=all_rows, apply_threshold=True)
    assert got[4] == 33
    mid = 0.5 if loss_type == "BCE_Loss" else order[16].item()  # (BCE's shown targets are 0 or 1)
    got, _ = _check(backend, 3, 33, 65, loss_type, act, threshold=mid, apply_threshold=True)
    assert 1 <= got[4] < 33
    off, _ = _check(backend, 3, 33, 65, loss_type, act, threshold=mid, apply_threshold=False)  # validation: no filter
    none, _ = _check(backend, 3, 33, 65, loss_type, act)
    assert off[4] == 33 and all(torch.equal(_bits(a), _bits(c)) for a, c in zip(off[5:], none[5:]))
    assert torch.equal(_bits(off[3]), _bits(none[3]))


@pytest.mark.parametrize("steps", ["ones", "full", "outside"])
def test_step_reward_head_valid_steps(backend, steps):
    got, (h, w, b, v, target) = _check(backend, 7, 33, 3, "L1_Loss", "tanh", steps)
    if steps == "outside":  # the clamp: the bits of the clamped steps
        again = _run_head(backend.device, h, w, b, "tanh", v.clamp(1, 7), target, "L1_Loss")
        assert _same(got, again)


def _integers(T, B, P, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(-3, 4, (T, B, P), generator=g).float()
    w, b = torch.randint(-2, 3, (P,), generator=g).float(), torch.randint(-2, 3, (1,), generator=g).float()
    v = torch.randint(1, T + 1, (B,), generator=g)
    target = torch.randint(-9, 10, (B,), generator=g).float()
    return h, w, b, v, target


@pytest.mark.parametrize("B,keep", [(8, 8), (33, 4), (257, 16)])
def test_exact_statements_on_small_integers(backend, B, keep):
    T, P = 5, 67
    h, w, b, v, target = _integers(T, B, P, seed=B)
    target[:keep] = -20.0  # a threshold of -15 keeps exactly these rows: a power of two
    got = _run_head(backend.device, h, w, b, "linear", v, target, "MSE_Loss", threshold=-15.0, apply_threshold=True)
    output = (torch.nn.functional.linear(h, w.view(1, P), b)).squeeze(2).transpose(0, 1)
    mask = _gen_mask(v.view(B, 1), B, T)
    pred = (output * mask).sum(dim=1)
    assert torch.equal(_bits(got[0]), _bits(output)) and torch.equal(_bits(got[1]), _bits(mask)) and torch.equal(_bits(got[2]), _bits(pred))
    assert got[4] == keep
    kept = (target <= -15.0).float()
    d = 2.0 * (pred - target) * kept  # integers
    coef = mask.t() * d.view(1, B)  # [T, B]
    dw = (coef.unsqueeze(2).double() * h.double()).sum((0, 1))
    assert dw.abs().max() < 2 ** 24
    assert torch.equal(_bits(got[6]), _bits((dw * (1.0 / keep)).float()))
    assert torch.equal(_bits(got[7]), _bits((coef.double().sum() * (1.0 / keep)).float().view(1)))
    want_dh = (coef.unsqueeze(2).double() * w.double() * (1.0 / keep)).float()
    assert torch.equal(got[5], want_dh)
    loss = ((pred - target).double() ** 2 * kept).sum() / keep
    assert got[3].item() == loss.float().item()


def test_no_row_kept(backend):
    h, w, b, v, target = _integers(3, 9, 5)
    got = _run_head(backend.device, h, w, b, "linear", v, target, "MSE_Loss", threshold=-100.0, apply_threshold=True)
    assert torch.isnan(got[3]) and got[4] == 0
    assert not got[5].any() and not torch.isnan(got[5]).any() and not got[6].any() and not got[7].any()


def test_l1_gradient_at_a_zero_residual_is_zero(backend):
    T, B, P = 2, 5, 3
    h, w, b, v, target = _integers(T, B, P, seed=3)
    got = _run_head(backend.device, h, w, b, "linear", v, target, "L1_Loss")
    target = got[2].clone()  # every residual zero
    target[1] += 1.0
    got = _run_head(backend.device, h, w, b, "linear", v, target, "L1_Loss")
    rows = [0, 2, 3, 4]
    assert not got[5][:, rows].any() and got[5][:, 1].any()
    assert got[3].item() == pytest.approx(1.0 / B)


def test_bce_clamps_its_logs_at_minus_100(backend):
    """a saturated sigmoid: pred / v is exactly 1 (or 0) against the opposite label; nn.BCELoss gives 100 for the row"""
    T, B, P = 2, 4, 1
    h = torch.tensor([800.0, 800.0, -800.0, -800.0]).view(1, B, 1).repeat(T, 1, 1)
    w, b = torch.ones(1), torch.zeros(1)
    v = torch.tensor([2, 1, 2, 1])
    target = torch.tensor([0.0, 1.0, 2.0, 0.0])  # rows 0 and 2 are wrong by everything, rows 1 and 3 are right
    got = _run_head(backend.device, h, w, b, "sigmoid", v, target, "BCE_Loss")
    r64 = _head_statement(torch.float64, h, w, b, "sigmoid", v, target, "BCE_Loss", None, False)
    assert r64[3].item() == 50.0 and got[3].item() == 50.0
    assert torch.isfinite(got[5]).all() and torch.isfinite(got[6]).all()
    # outside [0, 1] (a linear head): NaN for the row, where torch raises
    got = _run_head(backend.device, h, w, b, "linear", v, target, "BCE_Loss")
    assert torch.isnan(got[3])


def test_two_runs_give_the_same_bits_and_rows_are_independent(backend):
    T, B, P = 3, 33, 65
    h, w, b, v, target = _head_inputs(T, B, P, "SmoothL1_Loss", "softplus")
    a = _run_head(backend.device, h, w, b, "softplus", v, target, "SmoothL1_Loss")
    c = _run_head(backend.device, h, w, b, "softplus", v, target, "SmoothL1_Loss")
    assert _same(a, c)
    r = 17  # the row alone: the bits of its outputs in the batch
    alone = _run_head(backend.device, h[:, r:r + 1].contiguous(), w, b, "softplus", v[r:r + 1], target[r:r + 1], "SmoothL1_Loss")
    for i in (0, 1, 2):
        assert torch.equal(_bits(alone[i][0]), _bits(a[i][r])), NAMES[i]
    other = h.clone()
    other[:, r + 1] += 1.0  # another row changes: this row's outputs do not
    changed = _run_head(backend.device, other, w, b, "softplus", v, target, "SmoothL1_Loss")
    for i in (0, 1, 2):
        assert torch.equal(_bits(changed[i][r]), _bits(a[i][r])) and torch.equal(_bits(changed[i][:r]), _bits(a[i][:r]))
    assert not torch.equal(_bits(changed[0][r + 1]), _bits(a[0][r + 1]))
    # d loss / d h of a row: its own inputs and the count of kept rows alone
    assert torch.equal(_bits(changed[5][:, r]), _bits(a[5][:, r])) and not torch.equal(_bits(changed[5][:, r + 1]), _bits(a[5][:, r + 1]))


def test_the_forward_alone_has_the_bits_of_the_full_mode(backend):
    T, B, P = 7, 33, 130
    h, w, b, v, target = _head_inputs(T, B, P, "MSE_Loss", "tanh")
    full = _run_head(backend.device, h, w, b, "tanh", v, target, "MSE_Loss")
    no_grad = _run_head(backend.device, h, w, b, "tanh", v, target, "MSE_Loss", grad=False)
    alone = _run_head(backend.device, h, w, b, "tanh", v, None, "MSE_Loss", grad=False)
    for i in (0, 1, 2):
        assert torch.equal(_bits(full[i]), _bits(no_grad[i])) and torch.equal(_bits(full[i]), _bits(alone[i])), NAMES[i]
    assert torch.equal(_bits(full[3]), _bits(no_grad[3])) and full[4] == no_grad[4] == B
    assert torch.isnan(alone[3]) and alone[4] == -7  # not written without a target


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    i = torch.ones(8, dtype=torch.int64, device=dev)
    k = torch.zeros(2, dtype=torch.int32, device=dev)
    d = torch.zeros(256, dtype=torch.float64, device=dev)
    p, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()
    EINVAL = -1

    def ng(T=1, B=1, S=1, A=1, n=1, state=p, lds=None, action=p, lda=None, out=p, ldo=None):
        return lib.rg_ngram_concat(state, S if lds is None else lds, action, A if lda is None else lda, T, B, S, A, n, out,
                                   (S + A) * n if ldo is None else ldo, s)

    assert ng() == 0 and ng(n=3) == 0 and ng(T=2, n=7) == 0 and ng(lds=4, lda=4, ldo=8) == 0
    for bad in (0, -1, 2, 4):
        assert ng(n=bad) == EINVAL
    for key in ("T", "B", "S", "A"):
        assert ng(**{key: 0}) == EINVAL
    for key in ("state", "action", "out"):
        assert ng(**{key: None}) == EINVAL
    assert ng(S=2, lds=1) == EINVAL and ng(A=2, lda=1) == EINVAL and ng(n=3, ldo=5) == EINVAL
    assert ng(T=1 << 15, B=1 << 14) == L.EUNSUPPORTED and ng(T=1 << 20, B=1 << 20) == L.EUNSUPPORTED
    assert ng(S=1 << 30, A=1 << 30, n=3) == L.EUNSUPPORTED

    def head(T=1, B=1, P=1, h=p, w=p, b=p, act=0, v=i.data_ptr(), target=p, loss_type=0, out=p, mask=p, pred=p, loss=p,
             n=k.data_ptr(), dh=p, dw=p, db=p, ws=d.data_ptr()):
        return lib.rg_step_reward_head(h, w, b, act, v, target, loss_type, 0, 0.0, 0, T, B, P, out, mask, pred, loss, n, dh, dw,
                                       db, ws, s)

    assert head() == 0 and head(dh=None, dw=None, db=None) == 0
    assert head(target=None, loss=None, n=None, dh=None, dw=None, db=None, ws=None) == 0
    assert head(act=5, loss_type=3) == 0
    assert head(T=1 << 15, B=1 << 14) == L.EUNSUPPORTED
    for key in ("T", "B", "P"):
        assert head(**{key: 0}) == EINVAL
    assert head(act=-1) == EINVAL and head(act=6) == EINVAL and head(loss_type=-1) == EINVAL and head(loss_type=4) == EINVAL
    for key in ("h", "w", "b", "v", "out", "mask", "pred", "loss", "n", "dw", "db", "ws", "target"):
        assert head(**{key: None}) == EINVAL, key
    assert lib.rg_step_reward_head_partials(0) == 0 and lib.rg_step_reward_head_partials(257) == 65


def test_refusals_by_name(backend):
    dev = backend.device
    f = dict(dtype=torch.float32, device=dev)
    for n in (0, 2):
        with pytest.raises(NotImplementedError, match=f"context_size {n}"):
            ops.ngram_concat(torch.zeros(1, 1, 1, **f), torch.zeros(1, 1, 1, **f), n, torch.zeros(1, 1, 2 * max(n, 1), **f))
