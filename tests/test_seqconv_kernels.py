"""rg_seqconv_forward / _dgrad / _wgrad and rg_ngram_window / _window_backward (reagent_amd/csrc/seqconv.hip).

The float64 statement is the reference's own route: pad the sequence by context_size // 2 zero steps on either side, unfold the
windows, Conv2d -> relu per layer on [T * B, 1, n, S + A], flatten, autograd from dfeat.  A layer's activation at window t,
height h is the kernels' activation at position t + h; the gradient of a position is the sum over the windows holding it.
Bounds: tests/test_lstm_kernels.py's _close (4 x torch's own fp32 error on the same inputs, or 4 ulp of the largest entry),
for every intermediate of the chain forward tower -> window -> window backward -> dgrad / wgrad per layer.  Every operand has a
padded pitch with NaN in the padding and in every output before the call.

Exact statements: with small-integer inputs and weights every partial sum is an fp32 integer and the whole chain equals the
float64 statement bit for bit (one dropped tap or boundary row fails this and passes the bound); with kh = [1, 1] every
window slot that lies in the padding holds relu(b_1 + W_1 relu(b_0)); dgrad masking dy on load equals dgrad of the masked dz;
two runs give the same bits."""
import pytest
import torch
import torch.nn.functional as F

import reagent_amd._lib as L
from reagent_amd import ops
from test_attention_kernels import _padded
from test_lstm_kernels import _bits, _close

F32 = torch.float32
#        T,  B,   S,  A, conv_dims, n, kh
SMALL = [(1, 1, 1, 1, [3], 5, [3]), (2, 3, 4, 3, [3], 1, [1]), (5, 3, 4, 3, [33, 5], 3, [1, 1]), (2, 33, 20, 13, [33, 5], 5, [2, 2]),
         (5, 1, 4, 3, [3], 7, [7]), (2, 3, 1, 1, [33, 5], 5, [3, 3])]
# over about 2 s on the interpreter (a fibre per lane): on the device alone
LARGE = [(33, 130, 100, 60, [130, 33], 5, [2, 2]), (5, 130, 4, 3, [130, 33], 5, [3, 3]), (33, 33, 20, 13, [3], 7, [7]),
         (1, 130, 100, 60, [130, 33], 3, [1, 1])]
EXACT = [(5, 33, 20, 13, [33, 5], 5, [2, 2]), (2, 3, 4, 3, [3], 5, [3]), (2, 3, 4, 3, [33, 5], 3, [1, 1])]
_id = lambda cases: [f"T{T}-B{B}-F{S + A}-C{'x'.join(map(str, d))}-n{n}-kh{'x'.join(map(str, kh))}"  # noqa: E731
                     for T, B, S, A, d, n, kh in cases]
_cases = {}


def _heights(n, kh):
    hs = [n]
    for k in kh:
        hs.append(hs[-1] - k + 1)
    return hs


def _inputs(case, integer):
    T, B, S, A, dims, n, kh = case
    gen = torch.Generator().manual_seed(1000 * T + 10 * B + S + n + len(dims) + integer)
    draw = (lambda *s, lo=-2, hi=3: torch.randint(lo, hi, s, generator=gen).float()) if integer else \
        (lambda *s, **_: torch.randn(*s, generator=gen))
    cin, ws, bs = 1, [], []
    for i, (c, k) in enumerate(zip(dims, kh)):
        shape = (c, cin, k, S + A if i == 0 else 1)
        ws.append(draw(*shape, lo=-1, hi=2) if integer else draw(*shape) / (shape[1] * shape[2] * shape[3]) ** 0.5)
        bs.append(draw(c))
        cin = c
    return draw(T, B, S), draw(T, B, A), ws, bs, draw(T * B, dims[-1] * _heights(n, kh)[-1], lo=-1, hi=2)


def _statement(case, inp, dtype):
    """-> dict: g (per layer [P_i * B, C_i]), feat, dz (masked, per layer), dw, db — the reference's windows under autograd"""
    T, B, S, A, dims, n, kh = case
    state, action, ws, bs, dfeat = (x.to(dtype) if torch.is_tensor(x) else [y.detach().clone().to(dtype).requires_grad_() for y in x] for x in inp)
    x = F.pad(torch.cat((state, action), dim=-1), (0, 0, 0, 0, n // 2, n // 2))            # [T + n - 1, B, F]
    h = x.unfold(0, n, 1).permute(0, 1, 3, 2).reshape(T * B, 1, n, S + A)                  # the windows
    acts = []
    for w, b in zip(ws, bs):
        h = torch.relu(F.conv2d(h, w, b))
        h.retain_grad()
        acts.append(h)
    feat = h.flatten(1)
    feat.backward(dfeat)

    def positions(a):  # [T * B, C, H, 1] per window -> [P * B, C] per position: position p is height p - t of window t = min(p, T - 1)
        a = a.detach().view(T, B, a.shape[1], a.shape[2])
        return torch.cat([a[min(p, T - 1), :, :, p - min(p, T - 1)] for p in range(T + a.shape[3] - 1)])

    def summed(a):     # the gradient of position p: the sum over the windows t + h = p
        d = a.grad.view(T, B, a.shape[1], a.shape[2])
        out = torch.zeros(T + d.shape[3] - 1, B, d.shape[2], dtype=dtype)
        for t in range(T):
            out[t:t + d.shape[3]] += d[t].permute(2, 0, 1)
        return out.view(-1, d.shape[2])

    g = [positions(a) for a in acts]
    return dict(g=g, feat=feat.detach(), dz=[torch.where(gi > 0, summed(a), torch.zeros((), dtype=dtype)) for a, gi in zip(acts, g)], dw=[w.grad for w in ws],
                db=[b.grad for b in bs])


def _case(case, integer=False):
    key = (tuple(map(str, case)), integer)
    if key not in _cases:
        inp = _inputs(case, integer)
        _cases[key] = (inp, _statement(case, inp, torch.float64), _statement(case, inp, F32))
    return _cases[key]


def _chain(dev, case, inp):
    """the five entry points in the module's order -> the same dict as _statement"""
    T, B, S, A, dims, n, kh = case
    state, action, ws, bs, dfeat = inp
    hs, half = _heights(n, kh), n // 2
    nan = lambda r, c, pad: _padded(torch.full((r, c), float("nan")), dev, pad)  # noqa: E731
    cur, cur2, P, pad, g, bufs = _padded(state.view(T * B, S), dev, 1)[0], _padded(action.view(T * B, A), dev, 2)[0], T, half, [], []
    ws_d, bs_d = [w.to(dev) for w in ws], [b.to(dev) for b in bs]
    layers = []
    for w, b, k in zip(ws_d, bs_d, kh):
        p_out = P + 2 * pad - k + 1
        y, buf = nan(p_out * B, w.shape[0], 3)
        ops.seqconv_forward(cur, cur2, P, pad, B, w, b, y)
        layers.append((cur, cur2, P, pad))
        bufs.append((buf, w.shape[0]))
        g.append(y)
        cur, cur2, P, pad = y, None, p_out, 0
    C, H = dims[-1], hs[-1]
    feat, buf = nan(T * B, C * H, 1)
    ops.ngram_window(g[-1], T, B, H, feat)
    bufs.append((buf, C * H))
    dz, buf = nan(P * B, C, 2)
    ops.ngram_window_backward(_padded(dfeat, dev, 5)[0], T, B, H, dz, g=g[-1])
    bufs.append((buf, C))
    dzs, dws, dbs = [dz], [], []
    for i in range(len(dims) - 1, -1, -1):
        x, x2, p_in, pad = layers[i]
        dw, db = torch.full_like(ws_d[i], float("nan")), torch.full_like(bs_d[i], float("nan"))
        nbytes = ops.seqconv_wgrad_workspace_bytes(p_in + 2 * pad - kh[i] + 1, B, kh[i], ws[i].shape[1] * ws[i].shape[3], dims[i])
        ops.seqconv_wgrad(dzs[0], x, x2, p_in, pad, B, dw, db, torch.full((nbytes // 4,), float("nan"), device=dev))
        dws.insert(0, dw)
        dbs.insert(0, db)
        if i > 0:
            dx, buf = nan(p_in * B, dims[i - 1], 1)
            ops.seqconv_dgrad(dzs[0], p_in - kh[i] + 1, B, ws_d[i], dx, below=g[i - 1])
            bufs.append((buf, dims[i - 1]))
            dzs.insert(0, dx)
    for buf, cols in bufs:  # every element written, no padding touched
        assert not torch.isnan(buf[:, :cols]).any() and torch.isnan(buf[:, cols:]).all()
    return dict(g=g, feat=feat, dz=dzs, dw=dws, db=dbs)


def _pairs(got, *refs):
    for name in ("g", "feat", "dz", "dw", "db"):
        items = [r[name] if isinstance(r[name], list) else [r[name]] for r in (got,) + refs]
        for i, xs in enumerate(zip(*items)):
            yield f"{name}[{i}]", xs


def _check(dev, case):
    inp, r64, r32 = _case(case)
    for name, (g, a, b) in _pairs(_chain(dev, case, inp), r64, r32):
        assert not torch.isnan(g).any(), name
        _close(g.reshape(a.shape), a, b, f"{name} {case}")


@pytest.mark.parametrize("case", SMALL, ids=_id(SMALL))
def test_chain_against_float64(backend, case):
    _check(backend.device, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE, ids=_id(LARGE))
def test_chain_against_float64_large(case):
    _check("cuda", case)


@pytest.mark.parametrize("case", EXACT, ids=_id(EXACT))
def test_integer_chain_equals_float64_bit_for_bit(backend, case):
    T, B, S, A, dims, n, kh = case
    inp, r64, _ = _case(case, integer=True)
    got = _chain(backend.device, case, inp)
    for name, (g, a) in _pairs(got, r64):
        # (the gradients + 0.0: there a zero's sign is decided by autograd's own products, -1 * 0, and is no part of the
        # statement; the forward's g and feat are compared with their signs)
        zero = 0.0 if name[:2] in ("dz", "dw", "db") else None
        g, a = g.reshape(a.shape).cpu(), a.float()
        assert a.abs().max() < 2 ** 24 and torch.equal(_bits(g if zero is None else g + zero), _bits(a if zero is None else a + zero)), name
    assert any((d != 0).any() for d in r64["dw"]) and (r64["feat"] != 0).any()
    if len(dims) == 2:  # dy masked on load by its own layer's output = dgrad of the masked dz
        dev, dy = backend.device, torch.randint(-2, 3, got["g"][1].shape).float()
        a, b = (torch.full(got["g"][0].shape, float("nan"), device=dev) for _ in range(2))
        ops.seqconv_dgrad(dy.to(dev), got["g"][1].shape[0] // B, B, inp[2][1].to(dev), a, y=got["g"][1], below=got["g"][0])
        ops.seqconv_dgrad((dy * (got["g"][1].cpu() > 0)).to(dev), got["g"][1].shape[0] // B, B, inp[2][1].to(dev), b, below=got["g"][0])
        assert torch.equal(_bits(a), _bits(b)) and (dy * (got["g"][1].cpu() <= 0)).any()
    if all(k == 1 for k in kh):  # a window slot in the padding holds the bias-only chain
        (w0, w1), (b0, b1) = inp[2], inp[3]
        want = torch.relu(b1 + w1.view(dims[1], dims[0]) @ torch.relu(b0))
        feat, slots = got["feat"].cpu().view(T, B, dims[1], n), 0
        for t in range(T):
            for h in range(n):
                if not 0 <= t + h - n // 2 < T:
                    assert torch.equal(_bits(feat[t, :, :, h]), _bits(want.expand(B, -1)))
                    slots += 1
        assert slots == 2 * sum(range(1, n // 2 + 1))


def test_two_runs_give_the_same_bits(backend):
    inp, *_ = _case(SMALL[3])
    for (name, (x, y)) in _pairs(_chain(backend.device, SMALL[3], inp), _chain(backend.device, SMALL[3], inp)):
        assert torch.equal(_bits(x), _bits(y)), name


def test_limits_are_refused_at_one_past_and_accepted_at_the_limit(backend):
    dev = backend.device
    # inputs (x / dy / dz / dfeat, weights, bias) and outputs (y / dx / dw / feat, dbias, workspace) in buffers of their own
    bufs = [torch.zeros(1 << 19, device=dev) for _ in range(6)]
    p, pw, pb, o, ob, ow = (t.data_ptr() for t in bufs)
    s, lib = L.stream_ptr(), L.lib()

    def fwd(F_=4, C=4, kh=1, pad=0, P=16):
        return lib.rg_seqconv_forward(p, F_, None, 0, F_, 0, P, pad, 1, kh, pw, 1, F_, pb, C, o, C, s)

    def dgrad(Cin=4, C=4, kh=1):
        return lib.rg_seqconv_dgrad(p, C, None, 0, 2, 1, kh, pw, kh, 1, Cin, C, None, 0, o, Cin, s)

    def wgrad(F_=4, C=4, kh=1, pad=0, P=16):
        n = lib.rg_seqconv_wgrad_workspace_bytes(P + 2 * pad - kh + 1, 1, kh, F_, C)
        return lib.rg_seqconv_wgrad(p, C, pw, F_, None, 0, F_, 0, P, pad, 1, kh, C, 1, F_, o, ob, ow, n, s)

    def window(C=4, H=2, back=False):
        if back:
            return lib.rg_ngram_window_backward(p, C * H, None, 0, 2, 1, C, H, o, C, s)
        return lib.rg_ngram_window(p, C, 2, 1, C, H, o, C * H, s)

    for call in (fwd, wgrad):
        assert call() == 0 and call(F_=512) == 0 and call(F_=513) == L.EINVAL
        assert call(C=512) == 0 and call(C=513) == L.EINVAL
        assert call(kh=15) == 0 and call(kh=16) == L.EINVAL
        assert call(pad=7) == 0 and call(pad=8) == L.EINVAL        # context_size 15 / 17
        assert call(kh=15, P=14) == L.EINVAL                       # no output position
    assert dgrad() == 0 and dgrad(Cin=512) == 0 and dgrad(Cin=513) == L.EINVAL and dgrad(C=512) == 0 and dgrad(C=513) == L.EINVAL
    assert dgrad(kh=15) == 0 and dgrad(kh=16) == L.EINVAL
    for back in (False, True):
        assert window(back=back) == 0 and window(C=512, back=back) == 0 and window(C=513, back=back) == L.EINVAL
        assert window(H=15, back=back) == 0 and window(H=16, back=back) == L.EINVAL
    assert lib.rg_seqconv_wgrad(p, 4, pw, 4, None, 0, 4, 0, 16, 0, 1, 1, 4, 1, 4, o, ob, ow, 8, s) == L.EWORKSPACE
    f = dict(dtype=F32, device=dev)
    with pytest.raises(NotImplementedError, match="513 input"):
        ops.seqconv_forward(torch.zeros(2, 513, **f), None, 2, 0, 1, torch.zeros(4, 1, 1, 513, **f), torch.zeros(4, **f),
                            torch.zeros(2, 4, **f))
    with pytest.raises(NotImplementedError, match="height 16"):
        ops.ngram_window(torch.zeros(17, 4, **f), 2, 1, 16, torch.zeros(2, 64, **f))
