"""rg_bandit_reward_head (reagent_amd/csrc/bbb.hip) against the float64 statement of BanditRewardNetTrainer's
_get_predicted_reward (cfeval/bandit_reward_network_trainer.py:57-61) and the loss wrapper of
reward_network_trainer.py:27-66 under autograd.  The bound is the self-calibrating one of tests/test_lstm_kernels.py: the
larger of 4 x torch's own fp32 error against float64 on the same inputs and 4 ulp of the largest magnitude."""
import numpy as np
import pytest
import torch

from reagent_amd import _lib as L
from reagent_amd import ops

F32, F64 = torch.float32, torch.float64
LOSSES = {"MSE_Loss": torch.nn.MSELoss, "SmoothL1_Loss": torch.nn.SmoothL1Loss, "L1_Loss": torch.nn.L1Loss}


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _close(got, ref64, torch32, what):
    ref64 = ref64.detach().double()
    own = (torch32.detach().double() - ref64).abs().max().item()
    bound = max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item()))
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (what, err, bound, own)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _statement(dtype, q, action, reward, prob, loss, threshold, training):
    """-> (predicted_reward, loss, unweighted loss, kept rows, d loss / d q)"""
    q = q.detach().clone().to(dtype).requires_grad_()
    idx = torch.argmax(action, dim=1, keepdim=True)
    pred = q.gather(1, idx)
    target = reward.to(dtype)
    elementwise = LOSSES[loss](reduction="none")(pred, target)
    weighted = elementwise * (1.0 / prob.to(dtype)) if prob is not None else elementwise
    keep = (reward <= threshold) if (training and threshold is not None) else torch.ones_like(reward, dtype=torch.bool)
    if keep.sum() == 0:
        return pred.detach(), None, None, 0, torch.zeros_like(q)
    total = weighted[keep].mean()
    total.backward()
    return pred.detach(), total.detach().view(1), elementwise[keep].mean().detach().view(1), int(keep.sum()), q.grad


def _run(dev, q, action, reward, prob, loss, threshold, training, pitch=0):
    """the kernel on row pitches A + pitch, the padding NaN"""
    B, A = q.shape

    def padded(t):
        wide = torch.full((B, A + pitch), float("nan"))
        wide[:, :A] = t
        return wide.to(dev)[:, :A]

    f = dict(dtype=F32, device=dev)
    out = dict(pred=torch.empty(B, 1, **f), loss=torch.empty(1, **f), unweighted=torch.empty(1, **f),
               n_kept=torch.empty(1, dtype=torch.int32, device=dev),
               dq=torch.full((B, A + pitch), float("nan"), **f)[:, :A] if training else None)
    ops.bandit_reward_head(padded(q), padded(action), reward.to(dev).view(B), out["pred"].view(B), out["loss"], out["n_kept"],
                           torch.empty(ops.bandit_reward_head_workspace(B), dtype=F64, device=dev),
                           action_prob=prob.to(dev).view(B) if prob is not None else None, loss_type=L.SRW_LOSS[loss],
                           threshold=threshold, apply_threshold=training, unweighted_loss=out["unweighted"], dq=out["dq"])
    return out


def _case(B, A, seed, weights):
    g = torch.Generator().manual_seed(seed)
    q, reward = torch.randn(B, A, generator=g), torch.randn(B, 1, generator=g)
    action = torch.nn.functional.one_hot(torch.randint(0, A, (B,), generator=g), A).float()
    prob = (1.0 - 0.9 * torch.rand(B, 1, generator=g)) if weights else None
    return q, action, reward, prob


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("A", [1, 2, 33])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_head_against_the_float64_statement(backend, B, A, loss):
    for weights, threshold, training in ((True, 0.3, True), (False, None, True), (True, 0.3, False)):
        q, action, reward, prob = _case(B, A, 1000 * B + A, weights)
        if threshold is not None:
            reward[0, 0] = -1.0  # (at least one row kept)
        pred64, loss64, un64, kept, dq64 = _statement(F64, q, action, reward, prob, loss, threshold, training)
        pred32, loss32, un32, _, dq32 = _statement(F32, q, action, reward, prob, loss, threshold, training)
        out = _run(backend.device, q, action, reward, prob, loss, threshold, training, pitch=3)
        assert torch.equal(_bits(out["pred"]), _bits(pred32))  # a gather: the bits
        assert out["n_kept"].item() == kept
        _close(out["loss"], loss64, loss32, "loss")
        _close(out["unweighted"], un64, un32, "unweighted loss")
        if training:
            _close(out["dq"], dq64, dq32, "d q")
            assert torch.equal(out["dq"].cpu() != 0, (dq64 != 0))
        if not training:  # validation does not filter
            assert kept == B


@pytest.mark.parametrize("loss", ["MSE_Loss", "L1_Loss"])
@pytest.mark.parametrize("B", [63, 257])
def test_small_integers_are_exact(backend, B, loss):
    """q and rewards small integers, B kept rows a power of two or not: every partial sum is an fp32 integer, so the loss sums,
    n_kept and dq's bits inside the logged column equal torch's"""
    A = 5
    g = torch.Generator().manual_seed(B)
    q = torch.randint(-4, 5, (B, A), generator=g).float()
    reward = torch.randint(-4, 5, (B, 1), generator=g).float()
    action = torch.nn.functional.one_hot(torch.randint(0, A, (B,), generator=g), A).float()
    threshold = 1.0
    out = _run(backend.device, q, action, reward, None, loss, threshold, True)
    pred32, loss32, _, kept, dq32 = _statement(F32, q, action, reward, None, loss, threshold, True)
    assert 0 < kept < B and out["n_kept"].item() == kept
    assert out["loss"].item() * kept == pytest.approx(loss32.item() * kept, abs=1e-4)
    total = LOSSES[loss](reduction="none")(pred32, reward)[reward <= threshold].sum().item()
    assert round(out["loss"].item() * kept) == total  # the sum: an integer
    idx = torch.argmax(action, 1, keepdim=True)
    dq = out["dq"].cpu()
    outside = torch.ones(B, A, dtype=torch.bool).scatter_(1, idx, False)
    assert torch.equal(_bits(dq[outside]), torch.zeros(int(outside.sum()), dtype=torch.int32))  # +0, not -0
    assert torch.equal(_bits(dq.gather(1, idx)), _bits(dq32.gather(1, idx)))
    assert (dq.gather(1, idx)[reward > threshold] == 0).all()
    tie = (pred32 == reward) & (reward <= threshold)
    assert tie.any() and (dq.gather(1, idx)[tie] == 0).all()  # L1's gradient at a tie is 0 (MSE's too)


def test_argmax_follows_torch(backend):
    """ties take the first maximum; a NaN ranks above everything, the first NaN first"""
    nan, inf = float("nan"), float("inf")
    action = torch.tensor([[0, 1, 1, 0], [2, 2, 2, 2], [0, nan, 5, nan], [nan, 1, 2, 3], [-inf, -inf, -inf, -inf], [1, inf, nan, inf],
                           [0.5, 0.25, 0.5, 0.1], [-1, -2, -0.0, 0.0]])
    B, A = action.shape
    q = torch.arange(B * A, dtype=F32).view(B, A)
    reward = torch.zeros(B, 1)
    out = _run(backend.device, q, action, reward, None, "MSE_Loss", None, True)
    want = q.gather(1, torch.argmax(action, dim=1, keepdim=True))
    assert torch.equal(out["pred"].cpu(), want)
    assert torch.equal((out["dq"].cpu() != 0).float().argmax(1), torch.argmax(action, dim=1))


def test_all_rows_dropped(backend):
    q, action, reward, prob = _case(65, 3, 5, True)
    out = _run(backend.device, q, action, reward, prob, "SmoothL1_Loss", -100.0, True)
    assert out["n_kept"].item() == 0 and torch.isnan(out["loss"]).all() and torch.isnan(out["unweighted"]).all()
    assert torch.equal(_bits(out["dq"]), torch.zeros(65, 3, dtype=torch.int32))
    val = _run(backend.device, q, action, reward, prob, "SmoothL1_Loss", -100.0, False)  # threshold off: every row
    assert val["n_kept"].item() == 65 and torch.isfinite(val["loss"]).all()


def test_refused_arguments(backend):
    q, action, reward, _ = _case(4, 3, 1, False)
    with pytest.raises(L.ReagentHipError, match="invalid"):
        _run(backend.device, q, action, reward, None, "BCE_Loss", None, True)
