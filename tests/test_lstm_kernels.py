"""The LSTM sequence kernels: rg_lstm_forward and rg_lstm_backward (reagent_amd/csrc/lstm.hip), one layer.

The yardstick is torch.nn.LSTM(...).double() under autograd on the same fp32 inputs.  The kernels take xproj = x W_ih^T +
b_ih, so the statement's layer has input_size = 4H, W_ih = the identity and b_ih = 0: its input IS xproj, exactly, in either
precision, and d loss / d input is d loss / d pre-activation (the kernel's dgates).  The loss is sum(h_all * G) for a fixed
random G, so dh_all = G.  Every bound is self-calibrating, as in tests/test_pg_kernels.py: the larger of 4 x the error of
torch's fp32 nn.LSTM against the float64 statement on those inputs and 4 ulp (fp32) of the quantity's largest magnitude."""
import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops

HS, BS, TS = [1, 31, 32, 33, 65, 256], [1, 32, 33, 65], [1, 2, 6]
SHAPES = [(H, B, T) for H in HS for B in BS for T in TS]


def _emu_cost(H, B, T):
    """MFMA steps a fiber of the interpreter runs in the forward, times the workgroups"""
    hp = (H + 31) // 32 * 32
    return T * ((hp // 32 + 3) // 4) * hp * ((B + 31) // 32)


SMALL = [s for s in SHAPES if _emu_cost(*s) <= 2000]  # the interpreter takes the large H with small B and T only
LARGE = [s for s in SHAPES if _emu_cost(*s) > 2000]
assert any(s[0] == 256 for s in SMALL) and all(s[0] == 256 for s in LARGE)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _close(got, ref64, torch32, what):
    ref64 = ref64.detach().double()
    own = (torch32.detach().double() - ref64).abs().max().item()
    bound = max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item()))
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (what, err, bound, own)


def _statement(H, dtype, w_hh, b_hh, xproj, h0, c0, G):
    """nn.LSTM with the identity as W_ih -> (h_all, c_n, d xproj, d h0, d c0)"""
    m = torch.nn.LSTM(input_size=4 * H, hidden_size=H, num_layers=1)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H))
        m.bias_ih_l0.zero_()
        m.weight_hh_l0.copy_(w_hh)
        m.bias_hh_l0.copy_(b_hh)
    m = m.to(dtype)
    x = xproj.to(dtype).requires_grad_(True)
    h = h0.to(dtype).unsqueeze(0).requires_grad_(True)
    c = c0.to(dtype).unsqueeze(0).requires_grad_(True)
    out, (_, cn) = m(x, (h, c))
    (out * G.to(dtype)).sum().backward()
    return out.detach(), cn.detach()[0], x.grad, h.grad[0], c.grad[0]


_CASES = {}


def _case(H, B, T, with_state=False):
    """inputs and both statements of one shape (computed once and left unchanged)"""
    key = (H, B, T, with_state)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * H + 10 * B + T)
        k = 1.0 / max(H, 1) ** 0.5
        w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) * k
        b_hh = (torch.rand(4 * H, generator=g) * 2 - 1) * k
        xproj = torch.randn(T, B, 4 * H, generator=g)
        G = torch.randn(T, B, H, generator=g)
        h0 = torch.randn(B, H, generator=g) * 0.5 if with_state else torch.zeros(B, H)
        c0 = torch.randn(B, H, generator=g) if with_state else torch.zeros(B, H)
        inp = dict(w_hh=w_hh, b_hh=b_hh, xproj=xproj, h0=h0, c0=c0, G=G)
        _CASES[key] = (inp, _statement(H, torch.float64, **inp), _statement(H, torch.float32, **inp))
    return _CASES[key]


def _run(dev, inp, with_state, save=True, backward=True):
    T, B, H4 = inp["xproj"].shape
    H = H4 // 4
    d = {k: v.to(dev).contiguous() for k, v in inp.items()}
    f = dict(dtype=torch.float32, device=dev)
    h_all, c_all = torch.full((T, B, H), float("nan"), **f), torch.full((T, B, H), float("nan"), **f)
    gates = torch.full((T, B, 4 * H), float("nan"), **f) if save else None
    h0, c0 = (d["h0"], d["c0"]) if with_state else (None, None)
    ops.lstm_forward(d["xproj"], d["w_hh"], d["b_hh"], h0, c0, h_all, c_all, gates)
    if not (save and backward):
        return h_all.cpu(), c_all.cpu(), None, None, None
    dgates = torch.full((T, B, 4 * H), float("nan"), **f)
    dh0, dc0 = torch.full((B, H), float("nan"), **f), torch.full((B, H), float("nan"), **f)
    ops.lstm_backward(d["G"], gates, c_all, c0, d["w_hh"], dgates, dh0, dc0)
    return h_all.cpu(), c_all.cpu(), dgates.cpu(), dh0.cpu(), dc0.cpu()


def _check(dev, H, B, T, with_state=False):
    inp, r64, r32 = _case(H, B, T, with_state)
    h_all, c_all, dgates, dh0, dc0 = _run(dev, inp, with_state)
    tag = f"H={H} B={B} T={T}"
    _close(h_all, r64[0], r32[0], f"h_all {tag}")
    _close(c_all[-1], r64[1], r32[1], f"c_n {tag}")
    _close(dgates, r64[2], r32[2], f"dgates {tag}")
    _close(dh0, r64[3], r32[3], f"dh0 {tag}")
    _close(dc0, r64[4], r32[4], f"dc0 {tag}")


@pytest.mark.parametrize("H,B,T", SMALL)
def test_forward_and_backward_against_float64(backend, H, B, T):
    _check(backend.device, H, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("H,B,T", LARGE)
def test_forward_and_backward_against_float64_wide(H, B, T):
    _check("cuda", H, B, T)


@pytest.mark.parametrize("H,B,T", [(33, 33, 2), (65, 1, 6), (256, 1, 1)])
def test_initial_state(backend, H, B, T):
    _check(backend.device, H, B, T, with_state=True)


def test_a_forward_that_saves_nothing_gives_the_same_bits(backend):
    inp, _, _ = _case(33, 33, 2, True)
    a = _run(backend.device, inp, True, save=True, backward=False)
    b = _run(backend.device, inp, True, save=False)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_a_row_depends_on_that_row_alone(backend):
    H, B, T, r = 33, 65, 6, 40
    inp, _, _ = _case(H, B, T, True)
    whole = _run(backend.device, inp, True)
    one = dict(inp, xproj=inp["xproj"][:, r:r + 1], G=inp["G"][:, r:r + 1], h0=inp["h0"][r:r + 1], c0=inp["c0"][r:r + 1])
    alone = _run(backend.device, one, True)
    assert torch.equal(_bits(whole[0][:, r]), _bits(alone[0][:, 0]))  # h_all
    assert torch.equal(_bits(whole[1][:, r]), _bits(alone[1][:, 0]))
    assert torch.equal(_bits(whole[2][:, r]), _bits(alone[2][:, 0]))  # dgates
    assert torch.equal(_bits(whole[3][r]), _bits(alone[3][0])) and torch.equal(_bits(whole[4][r]), _bits(alone[4][0]))


def test_two_runs_give_the_same_bits(backend):
    inp, _, _ = _case(65, 33, 6)
    a, b = _run(backend.device, inp, False), _run(backend.device, inp, False)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    p, s = t.data_ptr(), L.stream_ptr()
    lib = L.lib()
    EINVAL = -1

    def fwd(T=1, B=1, H=1, xproj=p, w=p, h_all=p, c_all=p):
        return lib.rg_lstm_forward(xproj, w, None, None, None, T, B, H, h_all, c_all, None, s)

    def bwd(T=1, B=1, H=1, dh=p, gates=p, c_all=p, w=p, dgates=p):
        return lib.rg_lstm_backward(dh, gates, c_all, None, w, T, B, H, dgates, None, None, s)

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        assert call(H=257) == L.EUNSUPPORTED and call(H=1024) == L.EUNSUPPORTED
        assert call(T=1 << 15, B=1 << 14) == L.EUNSUPPORTED
        assert call(T=0) == EINVAL and call(B=0) == EINVAL and call(H=0) == EINVAL
    for k in ("xproj", "w", "h_all", "c_all"):
        assert fwd(**{k: None}) == EINVAL
    for k in ("dh", "gates", "c_all", "w", "dgates"):
        assert bwd(**{k: None}) == EINVAL
    f = dict(dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="hidden size 257"):
        ops.lstm_forward(torch.zeros(1, 1, 4 * 257, **f), torch.zeros(4 * 257, 257, **f), None, None, None,
                         torch.zeros(1, 1, 257, **f), torch.zeros(1, 1, 257, **f))
    with pytest.raises(NotImplementedError, match="hidden size 300"):
        ops.lstm_backward(torch.zeros(1, 1, 300, **f), torch.zeros(1, 1, 1200, **f), torch.zeros(1, 1, 300, **f), None,
                          torch.zeros(1200, 300, **f), torch.zeros(1, 1, 1200, **f))
