"""rg_attn_forward / rg_attn_backward and the residual joins (reagent_amd/csrc/attention.hip).

Bounds: tests/test_lstm_kernels.py's _close — the larger of 4 x torch's own fp32 error against float64 on the same inputs and
4 ulp of the reference's largest entry.  The float64 statement is softmax(q k^T / sqrt(hd)) v per (b, head) under autograd; the
kernels are also held to torch.nn.MultiheadAttention itself, in float64 with identity projections.  Every run here passes q | k
and dq | dk as the halves of one [N, 2E] buffer, v, ctx, dctx and dv with padded pitches, NaN in every padding and in every output
before the call: an element the kernel skips, or a read of the padding, shows as NaN.

Exact statements: (a) q = 0 and integer v: every p is 1 / T and ctx is the mean over the steps, bit for bit; (b) q_i = k_i =
256 e_i at hd = 64: p is the identity exactly, ctx has v's bits, dv has dctx's bits, dq = dk = 0; (c) two runs give the same
bits.  The joins are fp32 adds in a stated order and are held to torch's fp32 statement bit for bit."""
import itertools
import math

import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from test_lstm_kernels import _bits, _close

F32 = torch.float32
SEQ, BATCH, HEADS = [1, 2, 5, 33, 64], [1, 3, 33], [(1, 1), (2, 4), (3, 33), (1, 128), (4, 128)]
SHAPES = list(itertools.product(SEQ, BATCH, HEADS))
# the interpreter runs a fiber per lane: the ten shapes with B = 33 and T >= 33 take 2 to 11 s there and run on the device alone
LARGE = [s for s in SHAPES if s[1] == 33 and s[0] >= 33]
SMALL = [s for s in SHAPES if s not in LARGE]
_id = lambda shapes: [f"T{T}-B{B}-{nh}x{hd}" for T, B, (nh, hd) in shapes]  # noqa: E731
_cases = {}


def _heads(x, T, B, nh):
    """[T * B, E] rows (t, b) -> [B, nh, T, hd]"""
    return x.view(T, B, nh, -1).permute(1, 2, 0, 3)


def _statement(q, k, v, dctx, T, B, nh):
    """the formula under autograd in the operands' dtype -> (ctx [N, E], p [B, nh, T, T], dq, dk, dv)"""
    q, k, v = (x.detach().clone().requires_grad_() for x in (q, k, v))
    hd = q.shape[1] // nh
    p = torch.softmax(_heads(q, T, B, nh) @ _heads(k, T, B, nh).transpose(-1, -2) / math.sqrt(hd), dim=-1)
    ctx = (p @ _heads(v, T, B, nh)).permute(2, 0, 1, 3).reshape(T * B, -1)
    ctx.backward(dctx)
    return ctx.detach(), p.detach(), q.grad, k.grad, v.grad


def _torch_module(q, k, v, dctx, T, B, nh):
    """nn.MultiheadAttention in float64 with identity projections and zero biases -> the same five"""
    E = q.shape[1]
    mha = torch.nn.MultiheadAttention(E, nh, dropout=0.0, batch_first=False).double()
    eye = torch.eye(E, dtype=torch.float64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.cat((eye, eye, eye)))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(eye)
        mha.out_proj.bias.zero_()
    q, k, v = (x.detach().double().view(T, B, E).clone().requires_grad_() for x in (q, k, v))
    ctx, p = mha(q, k, v, need_weights=True, average_attn_weights=False)
    ctx.backward(dctx.double().view(T, B, E))
    return ctx.detach().view(T * B, E), p.detach(), q.grad.view(T * B, E), k.grad.view(T * B, E), v.grad.view(T * B, E)


def _case(T, B, nh, hd):
    """inputs and the three statements of one shape (computed once and left unchanged)"""
    key = (T, B, nh, hd)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * T + 10 * B + nh + hd)
        q, k, v, dctx = (torch.randn(T * B, nh * hd, generator=gen) for _ in range(4))
        inp = (q, k, v, dctx)
        _cases[key] = (inp, _statement(*(x.double() for x in inp), T, B, nh), _statement(*inp, T, B, nh),
                       _torch_module(*inp, T, B, nh))
    return _cases[key]


def _padded(x, dev, pad=3):
    """a view of x inside a buffer with a wider pitch, NaN in the padding"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=F32, device=dev)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]], buf


def _run(dev, inp, T, B, nh, backward=True):
    """-> (ctx, p, dq, dk, dv); asserts that every output element was written and no padding was"""
    q, k, v, dctx = inp
    N, E = q.shape
    qk = torch.cat((q, k), dim=1).to(dev)  # q | k: the halves of one buffer
    v_, _ = _padded(v, dev)
    ctx, ctx_buf = _padded(torch.full((N, E), float("nan")), dev)
    p = torch.full((B, nh, T, T), float("nan"), dtype=F32, device=dev)
    ops.attn_forward(qk[:, :E], qk[:, E:], v_, T, B, nh, ctx, p)
    assert not torch.isnan(ctx).any() and not torch.isnan(p).any() and torch.isnan(ctx_buf[:, E:]).all()
    if not backward:
        return ctx.cpu(), p.cpu()
    dctx_, _ = _padded(dctx, dev, pad=5)
    dqk = torch.full((N, 2 * E), float("nan"), dtype=F32, device=dev)
    dv, dv_buf = _padded(torch.full((N, E), float("nan")), dev, pad=1)
    ops.attn_backward(dctx_, qk[:, :E], qk[:, E:], v_, p, T, B, nh, dqk[:, :E], dqk[:, E:], dv)
    assert not torch.isnan(dqk).any() and not torch.isnan(dv).any() and torch.isnan(dv_buf[:, E:]).all()
    return ctx.cpu(), p.cpu(), dqk[:, :E].cpu(), dqk[:, E:].cpu(), dv.cpu()


def _check(dev, T, B, nh, hd):
    inp, r64, r32, module = _case(T, B, nh, hd)
    got = _run(dev, inp, T, B, nh)
    tag = f"T={T} B={B} nhead={nh} hd={hd}"
    for name, g, a, b, m in zip(("ctx", "p", "dq", "dk", "dv"), got, r64, r32, module):
        _close(g, a, b, f"{name} {tag}")
        _close(g, m, b, f"{name} {tag} against nn.MultiheadAttention")


@pytest.mark.parametrize("T,B,heads", SMALL, ids=_id(SMALL))
def test_forward_and_backward_against_float64(backend, T, B, heads):
    _check(backend.device, T, B, *heads)


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,heads", LARGE, ids=_id(LARGE))
def test_forward_and_backward_against_float64_large(T, B, heads):
    _check("cuda", T, B, *heads)


def test_without_p_the_context_has_the_same_bits(backend):
    T, B, nh, hd = 5, 3, 2, 4
    (q, k, v, _), *_ = _case(T, B, nh, hd)
    dev = backend.device
    ctx = torch.empty(T * B, nh * hd, device=dev)
    ops.attn_forward(q.to(dev), k.to(dev), v.to(dev), T, B, nh, ctx, None)
    assert torch.equal(_bits(ctx), _bits(_run(dev, (q, k, v, None), T, B, nh, backward=False)[0]))


@pytest.mark.parametrize("T", [2, 64])
def test_zero_queries_give_the_mean_exactly(backend, T):
    """(a) q = 0: every score is 0, every p is 1 / T and ctx is the mean of the integer v over the steps — one dropped key
    changes both"""
    B, nh, hd = 3, 2, 4
    gen = torch.Generator().manual_seed(T)
    v = torch.randint(-8, 9, (T * B, nh * hd), generator=gen).float()
    k, dctx = torch.randn(T * B, nh * hd, generator=gen), torch.randn(T * B, nh * hd, generator=gen)
    ctx, p = _run(backend.device, (torch.zeros(T * B, nh * hd), k, v, dctx), T, B, nh, backward=False)
    assert torch.equal(_bits(p), _bits(torch.full((B, nh, T, T), 1.0 / T)))
    mean = v.view(T, B, -1).sum(0) / T  # (integers: exact)
    assert torch.equal(_bits(ctx.view(T, B, -1)), _bits(mean.expand(T, B, -1)))


@pytest.mark.parametrize("T", [33, 64])
def test_orthogonal_keys_give_the_identity_exactly(backend, T):
    """(b) q_i = k_i = 256 e_i at hd = 64: the scores are 8192 on the diagonal and 0 off it, so p is the identity in fp32"""
    B, nh, hd = 2, 2, 64
    E = nh * hd
    gen = torch.Generator().manual_seed(T)
    qk = torch.zeros(T, B, nh, hd)
    for i in range(T):
        qk[i, :, :, i] = 256.0
    qk = qk.view(T * B, E)
    v, dctx = torch.randn(T * B, E, generator=gen), torch.randn(T * B, E, generator=gen)
    ctx, p, dq, dk, dv = _run(backend.device, (qk, qk.clone(), v, dctx), T, B, nh)
    assert torch.equal(_bits(p), _bits(torch.eye(T).expand(B, nh, T, T)))
    assert torch.equal(_bits(ctx), _bits(v)) and torch.equal(_bits(dv), _bits(dctx))
    assert (dq == 0).all() and (dk == 0).all()


def test_two_runs_give_the_same_bits(backend):
    T, B, nh, hd = 33, 3, 3, 33
    inp, *_ = _case(T, B, nh, hd)
    for x, y in zip(_run(backend.device, inp, T, B, nh), _run(backend.device, inp, T, B, nh)):
        assert torch.equal(_bits(x), _bits(y))


def test_a_pair_depends_on_that_pair_alone(backend):
    T, B, nh, hd, b = 5, 33, 2, 4, 17
    inp, *_ = _case(T, B, nh, hd)
    whole = _run(backend.device, inp, T, B, nh)
    one = tuple(x.view(T, B, -1)[:, b].contiguous() for x in inp)
    alone = _run(backend.device, one, T, 1, nh)
    assert torch.equal(_bits(whole[1][b]), _bits(alone[1][0]))
    for i in (0, 2, 3, 4):
        assert torch.equal(_bits(whole[i].view(T, B, -1)[:, b]), _bits(alone[i].view(T, -1)))


def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(1 << 16, device=dev)
    p, s = t.data_ptr(), L.stream_ptr()
    lib = L.lib()
    EINVAL = -1

    def fwd(T=2, B=1, E=4, nh=2, q=p, k=p, v=p, ctx=p, ld=None):
        ld = E if ld is None else ld
        return lib.rg_attn_forward(q, ld, k, ld, v, ld, T, B, E, nh, ctx, ld, p, s)

    def bwd(T=2, B=1, E=4, nh=2, dctx=p, q=p, k=p, v=p, pr=p, dq=p, dk=p, dv=p, ld=None):
        ld = E if ld is None else ld
        return lib.rg_attn_backward(dctx, ld, q, ld, k, ld, v, ld, pr, T, B, E, nh, dq, ld, dk, ld, dv, ld, s)

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        assert call(T=65) == L.EUNSUPPORTED                # a score row is one wavefront
        assert call(E=129, nh=1) == L.EUNSUPPORTED         # head width
        assert call(E=258, nh=2) == L.EUNSUPPORTED
        assert call(E=520, nh=8) == L.EUNSUPPORTED         # width
        assert call(E=6, nh=4) == EINVAL                   # nhead does not divide the width
        assert call(T=0) == EINVAL and call(B=0) == EINVAL and call(nh=0) == EINVAL
        assert call(ld=3) == EINVAL                        # a pitch below the width
        assert call(T=64, B=1 << 23) == L.EUNSUPPORTED
    for k_ in ("q", "k", "v", "ctx"):
        assert fwd(**{k_: None}) == EINVAL
    for k_ in ("dctx", "q", "k", "v", "pr", "dq", "dk", "dv"):
        assert bwd(**{k_: None}) == EINVAL
    assert lib.rg_residual_join(p, 4, None, 0, None, 0, 2, 1, 4, L.ACT["tanh"], p, 4, s) == EINVAL
    assert lib.rg_residual_join(p, 3, None, 0, None, 0, 2, 1, 4, L.ACT["relu"], p, 4, s) == EINVAL
    assert lib.rg_residual_join_backward(None, 0, None, 0, None, 0, None, 0, None, 0, 2, 4, p, 4, s) == EINVAL
    f = dict(dtype=F32, device=dev)
    with pytest.raises(NotImplementedError, match="seq_len 65"):
        ops.attn_forward(torch.zeros(65, 4, **f), torch.zeros(65, 4, **f), torch.zeros(65, 4, **f), 65, 1, 2, torch.zeros(65, 4, **f))
    with pytest.raises(NotImplementedError, match="nhead 4 does not divide"):
        ops.attn_forward(torch.zeros(2, 6, **f), torch.zeros(2, 6, **f), torch.zeros(2, 6, **f), 2, 1, 4, torch.zeros(2, 6, **f))


@pytest.mark.parametrize("B", [1, 33])
def test_residual_join_has_torchs_bits(backend, B):
    """out = act((a + b) + pe[t]): one or two fp32 adds per element in that order, pe broadcast over the batch"""
    T, E, dev = 5, 33, backend.device
    gen = torch.Generator().manual_seed(B)
    a, b = torch.randn(T * B, E, generator=gen), torch.randn(T * B, E, generator=gen)
    pe = torch.randn(7, 1, E, generator=gen)  # (more rows than steps, as max_len > seq_len)
    a_, _ = _padded(a, dev)
    b_, _ = _padded(b, dev, pad=1)
    pe_rows = pe.to(dev).view(7, E)

    def run(relu, b=None, pe=None):
        out, buf = _padded(torch.full((T * B, E), float("nan")), dev, pad=2)
        ops.residual_join(a_, out, T, B, b=b, pe=pe, relu=relu)
        assert torch.isnan(buf[:, E:]).all()
        return out.cpu()

    pe_t = pe[:T].expand(T, B, E).reshape(T * B, E)
    assert torch.equal(_bits(run(False, pe=pe_rows)), _bits(a + pe_t))                      # x + pe
    assert torch.equal(_bits(run(True, b=b_)), _bits(torch.relu(a + b)))                    # relu(x + block(x))
    assert torch.equal(_bits(run(False, b=b_)), _bits(a + b))                               # a pre-norm sum
    assert torch.equal(_bits(run(True, b=b_, pe=pe_rows)), _bits(torch.relu((a + b) + pe_t)))
    assert torch.equal(_bits(run(False)), _bits(a))


@pytest.mark.parametrize("B", [1, 33])
def test_residual_join_backward_has_torchs_bits(backend, B):
    """dx = (((g0 + g1) + g2) + g3) where the saved relu output is positive, 0 elsewhere: the relu's backward through its output
    applied to the ordered fp32 sum of the gradient streams"""
    T, E, dev = 5, 33, backend.device
    gen = torch.Generator().manual_seed(100 + B)
    g = [torch.randn(T * B, E, generator=gen) for _ in range(4)]
    out = torch.relu(torch.randn(T * B, E, generator=gen))
    assert (out == 0).any() and (out > 0).any()
    g_ = [_padded(x, dev, pad=i + 1)[0] for i, x in enumerate(g)]
    out_, _ = _padded(out, dev)

    def run(n, masked):
        dx, buf = _padded(torch.full((T * B, E), float("nan")), dev, pad=2)
        ops.residual_join_backward(g_[:n], dx, out=out_ if masked else None)
        assert torch.isnan(buf[:, E:]).all()
        return dx.cpu()

    sums = [g[0], g[0] + g[1], (g[0] + g[1]) + g[2], ((g[0] + g[1]) + g[2]) + g[3]]
    for n in (1, 2, 3, 4):
        assert torch.equal(_bits(run(n, False)), _bits(sums[n - 1]))
        want = torch.where(out > 0, sums[n - 1], torch.zeros(()))
        assert torch.equal(_bits(run(n, True)), _bits(want))
    # the same statement through autograd: relu's backward of the summed streams
    x = torch.randn(T * B, E, generator=gen).requires_grad_()
    y = torch.relu(x)
    y.backward(sums[3])
    out2, _ = _padded(y.detach(), dev)
    dx = torch.empty(T * B, E, device=dev)
    ops.residual_join_backward(g_, dx, out=out2)
    assert torch.equal(_bits(dx), _bits(x.grad))
