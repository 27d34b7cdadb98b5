"""rg_s2s_embed_join, rg_frechet_head and rg_frechet_rank (reagent_amd/csrc/seq2slate.hip).

Bounds: tests/test_lstm_kernels.py's _close — the larger of 4 x torch's own fp32 error against the float64 statement on the same
inputs and 4 ulp of the statement's largest entry.  The float64 statement is the formula written out in float64 under autograd:
the scorer's linear map, mask_logits_by_idx on float64 logits, softmax, per_symbol_to_per_seq_probs, log, exp, the importance
weight, helper.ips_clamp's three methods and the trainer's mean(-clamped * (reward - baseline)).  (It is not the reference
module cast to double: that module builds its logits with a dtype-less torch.zeros and runs the soft-max in float32.)

The gradient of the scores sums to zero in every row, so its entries cancel: _close holds them by the absolute error against
the row-wide maximum, and the row sums themselves are held to S half-ulps of the row's largest entry (each entry is the double
value rounded once, and the double values sum to zero up to T * S roundings of 2^-53).

Every run passes mem, dmem, dscore and tgt_out_idx with padded pitches, NaN (for the indices: a wild value) in every padding
and NaN in every output before the call: an element the kernel skips, or a read of the padding, shows.

Targets are Plackett-Luce samples of the scores themselves (Gumbel arg-sort), and at T = 64 the scores spread wider (a standard
deviation of 10, not 3), so that at S = 64 both kinds of row occur: at B = 33, 30 rows of 33 stay above the 1e-40 clamp at T = 32
and 2, 32 and 30 (E = 2, 8, 130) at T = 64 and carry a gradient, the others fall under it and carry none; the rows of B = 1 and
most of B = 3 at T = 64 fall under it."""
import itertools
import math

import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.model_utils.seq2slate_utils import mask_logits_by_idx, per_symbol_to_per_seq_probs
from test_lstm_kernels import _bits, _close, _ulp

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
NONE, UNIVERSAL, AGGRESSIVE = L.IPS_CLAMP_NONE, L.IPS_CLAMP_UNIVERSAL, L.IPS_CLAMP_AGGRESSIVE
SEQ, BATCH, EMBED = [1, 2, 5, 33, 64], [1, 3, 33], [2, 8, 130]
SHAPES = [(S, T, B, E) for S, B, E in itertools.product(SEQ, BATCH, EMBED) for T in sorted({1, max(S // 2, 1), S})]
# the interpreter runs a fiber per lane: B = 33 with S >= 33 runs on the device alone
LARGE = [s for s in SHAPES if s[2] == 33 and s[0] >= 33]
SMALL = [s for s in SHAPES if s not in LARGE]
VARIANTS = [(NONE, False), (NONE, True), (UNIVERSAL, False), (UNIVERSAL, True), (AGGRESSIVE, False), (AGGRESSIVE, True)]
_id = lambda shapes: [f"S{S}-T{T}-B{B}-E{E}" for S, T, B, E in shapes]  # noqa: E731
_cases = {}
NAMES = ("log_prob", "p", "impt", "clamped", "sums", "dscore", "dmem", "dw", "dbias")


def _clamp(impt, method, cmax):
    """helper.ips_clamp, written out"""
    if method == NONE:
        return impt.clone()
    if method == UNIVERSAL:
        return torch.clamp(impt, 0, cmax)
    return torch.where(impt > cmax, torch.zeros_like(impt), impt)


def _statement(inp, S, B, method, cmax, baseline, dtype):
    """the formula under autograd in dtype -> NAMES' tensors (and the scores)"""
    mem, w, bias, idx, logged, reward, base = inp
    mem, w, bias = (x.to(dtype).clone().requires_grad_() for x in (mem, w, bias))
    T = idx.shape[1]
    scores = ((mem.view(S, B, -1) @ w).t() + bias)  # [B, S]
    scores.retain_grad()
    logits = torch.cat((torch.zeros(B, T, 2, dtype=dtype), scores.unsqueeze(1).expand(B, T, S)), dim=2)
    tgt_in_idx = torch.cat((torch.ones(B, 1, dtype=torch.int64), idx[:, :-1]), dim=1)
    probs = torch.softmax(mask_logits_by_idx(logits, tgt_in_idx), dim=2)
    p = per_symbol_to_per_seq_probs(probs, idx)
    log_prob = torch.log(p)
    impt = torch.exp(log_prob) / logged.to(dtype).view(B, 1)
    clamped = _clamp(impt, method, cmax)
    r = reward.to(dtype).view(B, 1)
    b = base.to(dtype).view(B, 1) if baseline else torch.zeros_like(r)
    loss = torch.mean(-clamped * (r - b))
    loss.backward()
    sums = torch.stack((loss.detach(), torch.mean(-impt * r).detach(), torch.mean(-clamped * r).detach()))
    out = (log_prob.detach().view(B), p.detach().view(B), impt.detach().view(B), clamped.detach().view(B), sums, scores.grad,
           mem.grad, w.grad, bias.grad.view(1))
    return out, scores.detach()


def _inputs(S, T, B, E, seed=None):
    gen = torch.Generator().manual_seed(100000 * S + 1000 * T + 10 * B + E if seed is None else seed)
    mem = torch.randn(S * B, E, generator=gen)
    w = torch.randn(E, generator=gen) * ((10.0 if T == 64 else 3.0) / math.sqrt(E))
    bias = torch.randn(1, generator=gen)
    scores = (mem.double().view(S, B, E) @ w.double()).t()
    gumbel = -torch.log(-torch.log(torch.rand(B, S, generator=gen, dtype=F64)))
    idx = torch.argsort(scores + gumbel, dim=1, descending=True)[:, :T].contiguous() + 2
    logged = torch.rand(B, generator=gen) * 0.9 + 0.05
    reward = torch.randn(B, generator=gen)
    base = torch.randn(B, generator=gen)
    return mem, w, bias, idx, logged, reward, base


def _case(S, T, B, E):
    """inputs, the clamp threshold and, per variant, the float64 and fp32 statements (computed once and left unchanged)"""
    key = (S, T, B, E)
    if key not in _cases:
        inp = _inputs(S, T, B, E)
        (_, _, impt, *_), _ = _statement(inp, S, B, NONE, 0.0, False, F64)
        srt = torch.sort(impt).values
        # the threshold sits between the two middle importance weights (B = 1: below the only one, which then clamps)
        cmax = math.sqrt(srt[B // 2 - 1].item() * srt[B // 2].item()) if B > 1 else 0.5 * srt[0].item()
        n_clamped = int((impt > cmax).sum())
        if B >= 3:
            assert 1 <= n_clamped <= B - 1, (n_clamped, B)
        _cases[key] = (inp, cmax, {})
    return _cases[key]


def _statements(S, T, B, E, method, baseline):
    inp, cmax, memo = _case(S, T, B, E)
    if (method, baseline) not in memo:
        memo[(method, baseline)] = (_statement(inp, S, B, method, cmax, baseline, F64)[0],
                                    _statement(inp, S, B, method, cmax, baseline, F32)[0])
    return inp, cmax, memo[(method, baseline)]


def _padded(x, dev, pad=3, fill=NAN):
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]], buf


def _run(dev, inp, S, B, method=NONE, cmax=0.0, baseline=False, train=True, loss=True):
    """-> NAMES' tensors (those asked for); asserts that every output element was written and no padding was"""
    mem, w, bias, idx, logged, reward, base = inp
    E, T = mem.shape[1], idx.shape[1]
    mem_, _ = _padded(mem, dev)
    idx_, _ = _padded(idx, dev, pad=2, fill=-(1 << 62))
    nan = lambda *shape: torch.full(shape, NAN, dtype=F32, device=dev)  # noqa: E731
    log_prob, p = nan(B), nan(B)
    ws = torch.full((ops.frechet_head_workspace(B, E),), NAN, dtype=F64, device=dev)
    kw = {}
    if loss:
        kw = dict(logged=logged.to(dev), reward=reward.to(dev), baseline=base.to(dev) if baseline else None, clamp_method=method,
                  clamp_max=cmax, impt=nan(B), clamped=nan(B), sums=nan(3))
    if train:
        dscore, ds_buf = _padded(nan(B, S), dev, pad=1)
        dmem, dm_buf = _padded(nan(S * B, E), dev, pad=5)
        kw.update(dscore=dscore, dmem=dmem, dw=nan(E), dbias=nan(1))
    ops.frechet_head(mem_, w.to(dev), bias.to(dev), idx_, S, B, log_prob, p, ws, **kw)
    out = [log_prob, p]
    if loss:
        out += [kw["impt"], kw["clamped"], kw["sums"]]
    if train:
        assert torch.isnan(ds_buf[:, S:]).all() and torch.isnan(dm_buf[:, E:]).all()
        out += [kw["dscore"], kw["dmem"], kw["dw"], kw["dbias"]]
    for name, t in zip(NAMES, out):
        assert not torch.isnan(t).any(), name
    return tuple(t.cpu() for t in out)


def _row_sums_vanish(dscore, S, T, what):
    d = dscore.double()
    top = d.abs().max(dim=1).values
    bound = torch.tensor([S * 0.5 * _ulp(x) + S * T * 2.0 ** -50 * x for x in top.tolist()], dtype=F64)
    assert (d.sum(dim=1).abs() <= bound).all(), (what, d.sum(dim=1), bound)


def _check(dev, S, T, B, E, variants=VARIANTS):
    for method, baseline in variants:
        inp, cmax, (r64, r32) = _statements(S, T, B, E, method, baseline)
        got = _run(dev, inp, S, B, method, cmax, baseline)
        tag = f"S={S} T={T} B={B} E={E} clamp={method} baseline={baseline}"
        for name, g, a, b in zip(NAMES, got, r64, r32):
            if name == "dbias":
                # the sum of entries that cancel (every row's sum vanishes): its error scales with the sum of their
                # magnitudes, the sum's condition, not with the vanishing result — the same factor of 4 on that scale
                scale = r64[5].abs().sum().item()
                own, err = (b.double() - a).abs().item(), (g.double() - a).abs().item()
                bound = max(4.0 * own, 4.0 * _ulp(scale))
                print(f"dbias {tag}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}")
                assert err <= bound, (tag, err, bound)
                continue
            _close(g, a, b, f"{name} {tag}")
        _row_sums_vanish(got[5], S, T, tag)


@pytest.mark.parametrize("S,T,B,E", SMALL, ids=_id(SMALL))
def test_head_against_float64(backend, S, T, B, E):
    _check(backend.device, S, T, B, E)


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,B,E", LARGE, ids=_id(LARGE))
def test_head_against_float64_large(S, T, B, E):
    _check("cuda", S, T, B, E)


@pytest.mark.gpu
def test_head_beyond_the_workgroup_limit():
    """B = 2 051: past 4 x 512 rows a wave takes two consecutive rows, the last waves' second rows do not exist, and the second
    launch adds 512 rows of partials (513 workgroups' worth of fibers on the interpreter: the device alone)"""
    _check("cuda", 5, 2, 2051, 8, variants=[(UNIVERSAL, True)])


@pytest.mark.parametrize("method", [UNIVERSAL, AGGRESSIVE])
def test_the_real_clamps_clamp_some_rows_and_stop_their_gradient(backend, method):
    """between 1 and B - 1 rows clamp (asserted from the float64 statement); a clamped row's d score is zero, bit for bit"""
    S, T, B, E = 5, 2, 33, 8
    inp, cmax, (r64, _) = _statements(S, T, B, E, method, True)
    hit = r64[2] > cmax
    assert 1 <= int(hit.sum()) <= B - 1
    assert torch.equal(r64[3][hit], torch.full_like(r64[3][hit], cmax if method == UNIVERSAL else 0.0))
    got = _run(backend.device, inp, S, B, method, cmax, True)
    assert (got[5][hit] == 0).all() and (got[5][~hit] != 0).any(dim=1).all()
    want = torch.full((int(hit.sum()),), cmax if method == UNIVERSAL else 0.0, dtype=F64).float()
    assert torch.equal(_bits(got[3][hit]), _bits(want))


def test_a_wild_or_repeated_index_gives_the_clamp_value_and_no_gradient(backend):
    """the indices are compared in int64 and never form an address: 2^32 + 2 is not candidate 0, and neither it, a negative
    index nor a repeated one is a remaining candidate, so the product is 0, p is the clamp value and nothing flows; the row
    beside them is untouched"""
    S, T, B, E = 5, 2, 4, 8
    mem, w, bias, idx, logged, reward, base = _inputs(S, T, B, E)
    good = _run(backend.device, (mem, w, bias, idx, logged, reward, base), S, B)
    bad = idx.clone()
    bad[0, 1] = (1 << 32) + 2
    bad[1, 0] = -(1 << 40)
    bad[2, 1] = bad[2, 0]
    got = _run(backend.device, (mem, w, bias, bad, logged, reward, base), S, B)
    tiny = torch.full((3,), 1e-40, dtype=F64).float()
    assert torch.equal(_bits(got[1][:3]), _bits(tiny)) and (got[5][:3] == 0).all()
    assert torch.equal(_bits(got[1][3]), _bits(good[1][3])) and torch.equal(_bits(got[5][3]), _bits(good[5][3]))


def test_log_probs_alone_have_the_same_bits(backend):
    """without logged propensities the head writes log_prob and p only, the same bits as the training call's"""
    S, T, B, E = 5, 2, 3, 8
    inp, cmax, _ = _case(S, T, B, E)
    full = _run(backend.device, inp, S, B)
    alone = _run(backend.device, inp, S, B, train=False, loss=False)
    no_grad = _run(backend.device, inp, S, B, train=False)
    assert len(alone) == 2 and len(no_grad) == 5
    for i in range(2):
        assert torch.equal(_bits(full[i]), _bits(alone[i]))
    for i in range(5):
        assert torch.equal(_bits(full[i]), _bits(no_grad[i]))


def _equal_scores(S, T, B, E, gen):
    """mem whose rows are all orthogonal to w, so that every score is the bias exactly"""
    mem = torch.randint(-4, 5, (S * B, E), generator=gen).float()
    w = torch.zeros(E)
    idx = torch.stack([torch.randperm(S, generator=gen)[:T] for _ in range(B)]) + 2
    return mem, w, torch.tensor([0.75]), idx, torch.rand(B, generator=gen) * 0.9 + 0.05, torch.randn(B, generator=gen), \
        torch.randn(B, generator=gen)


@pytest.mark.parametrize("S", [2, 5, 33, 64])
def test_equal_scores_at_one_step_give_one_over_s(backend, S):
    """p = 1 / S rounded once and d score = g * p * (1[c = a] - 1 / S) with g = -(reward - baseline) / (B * logged)"""
    B, E = 3, 8
    inp = _equal_scores(S, 1, B, E, torch.Generator().manual_seed(S))
    _, _, _, idx, logged, reward, base = inp
    log_prob, p, impt, clamped, sums, dscore, dmem, dw, dbias = _run(backend.device, inp, S, B, baseline=True)
    assert torch.equal(_bits(p), _bits(torch.full((B,), 1.0 / S, dtype=F64).float()))
    assert torch.equal(_bits(log_prob), _bits(torch.full((B,), math.log(1.0 / S), dtype=F64).float()))
    g = -(reward.double() - base.double()) * (1.0 / B) / logged.double()
    onehot = torch.zeros(B, S, dtype=F64).scatter(1, idx - 2, 1.0)
    want = (g * (1.0 / S)).view(B, 1) * (onehot - 1.0 / S)
    assert (dscore.double() - want).abs().max().item() <= 4 * _ulp(want.abs().max().item())
    assert (dmem == 0).all()  # w = 0


def test_equal_scores_at_64_steps_fall_under_the_clamp(backend):
    """S = T = 64: 1 / 64! is far under 1e-40, so p is float32(1e-40) bit for bit (a subnormal, kept), log_prob is its log, and
    no gradient passes the clamp"""
    S, B, E = 64, 3, 8
    mem, w, bias, idx, logged, reward, base = _equal_scores(S, S, B, E, torch.Generator().manual_seed(64))
    w = torch.randn(E)  # a live scorer over equal rows: equal scores, and d mem = d score * w would show
    mem = mem[:1].expand(S * B, E).contiguous()
    log_prob, p, impt, clamped, sums, dscore, dmem, dw, dbias = _run(backend.device, (mem, w, bias, idx, logged, reward, base), S, B)
    tiny = np.float32(1e-40)
    assert tiny > 0 and torch.equal(_bits(p), _bits(torch.full((B,), float(tiny))))
    assert torch.equal(_bits(log_prob), _bits(torch.full((B,), math.log(1e-40), dtype=F64).float()))
    assert torch.equal(_bits(impt), _bits((torch.full((B,), 1e-40, dtype=F64) / logged.double()).float()))
    for t in (dscore, dmem, dw, dbias):
        assert (t == 0).all()


def test_a_dominant_first_candidate_has_probability_one(backend):
    """one score 200 above the rest, that candidate first, T = 1: p = 1 exactly and log_prob = 0"""
    S, B, E = 5, 3, 2
    mem = torch.zeros(S * B, E)
    first = torch.tensor([3, 0, 4])
    for b in range(B):
        mem[first[b] * B + b, 0] = 200.0
    w, bias = torch.tensor([1.0, 0.0]), torch.tensor([-7.0])
    inp = (mem, w, bias, (first + 2).view(B, 1), torch.full((B,), 0.5), torch.ones(B), torch.zeros(B))
    log_prob, p, impt, *_ = _run(backend.device, inp, S, B)
    assert torch.equal(_bits(p), _bits(torch.ones(B))) and (log_prob == 0).all()
    assert torch.equal(_bits(impt), _bits(torch.full((B,), 2.0)))


@pytest.mark.parametrize("S", [1, 2, 5, 33])
def test_the_last_step_of_a_full_slate_is_a_factor_of_one(backend, S):
    """T = S: the last step's soft-max has one candidate left; p has the bits of the slate cut at S - 1 steps"""
    if S == 1:
        inp = _inputs(1, 1, 3, 8)
        _, p, *_ = _run(backend.device, inp, 1, 3)
        assert torch.equal(_bits(p), _bits(torch.ones(3)))
        return
    B, E = 3, 8
    inp = _inputs(S, S, B, E)
    cut = inp[:3] + (inp[3][:, :S - 1].contiguous(),) + inp[4:]
    full, short = _run(backend.device, inp, S, B), _run(backend.device, cut, S, B)
    for x, y in zip(full, short):
        assert torch.equal(_bits(x), _bits(y))


def test_two_runs_give_the_same_bits(backend):
    S, T, B, E = 33, 16, 3, 130
    inp, cmax, _ = _case(S, T, B, E)
    for x, y in zip(_run(backend.device, inp, S, B, UNIVERSAL, cmax, True), _run(backend.device, inp, S, B, UNIVERSAL, cmax, True)):
        assert torch.equal(_bits(x), _bits(y))


def test_a_row_depends_on_that_row_alone(backend):
    """row b of a batch of 33 (nine workgroups) against the same row as a batch of one: the same per-row bits"""
    S, T, B, E, b = 5, 2, 33, 8, 17
    inp, cmax, _ = _case(S, T, B, E)
    mem, w, bias, idx, logged, reward, base = inp
    one = (mem.view(S, B, E)[:, b].contiguous(), w, bias, idx[b:b + 1], logged[b:b + 1], reward[b:b + 1], base[b:b + 1])
    whole, alone = _run(backend.device, inp, S, B), _run(backend.device, one, S, 1)
    for i in range(4):
        assert torch.equal(_bits(whole[i][b]), _bits(alone[i][0]))
    # the gradients carry the mean's 1 / B
    assert (whole[5][b].double() * B - alone[5][0].double()).abs().max().item() <= 2 * _ulp(alone[5].abs().max().item())


# ---- the embedding join ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Es,Ec", [(1, 1, 1, 1), (5, 3, 1, 1), (5, 3, 3, 4), (33, 33, 4, 5), (64, 3, 65, 65), (2, 33, 7, 2)])
def test_embed_join_has_torchs_bits(backend, S, B, Es, Ec):
    """Embedder's `linear(x) * math.sqrt(dim_out)` (the python double reaching the fp32 multiply rounded to fp32), repeat,
    reshape and cat, as encode builds src_embed; rows here are ordered (s, b)"""
    dev = backend.device
    gen = torch.Generator().manual_seed(S * 100 + B)
    state, cand = torch.randn(B, Es, generator=gen), torch.randn(S * B, Ec, generator=gen)
    state_, _ = _padded(state, dev)
    cand_, _ = _padded(cand, dev, pad=1)
    out, buf = _padded(torch.full((S * B, Es + Ec), NAN), dev, pad=2)
    ops.s2s_embed_join(state_, cand_, S, B, out)
    assert torch.isnan(buf[:, Es + Ec:]).all()
    se = (state * math.sqrt(Es)).repeat(1, S).reshape(B, S, Es)  # [B, S, Es] as the reference lays it out
    want = torch.cat((se, cand.view(S, B, Ec).transpose(0, 1) * math.sqrt(Ec)), dim=2).transpose(0, 1).reshape(S * B, Es + Ec)
    assert torch.equal(_bits(out), _bits(want))

    d = torch.randn(S * B, Es + Ec, generator=gen)
    d_, _ = _padded(d, dev, pad=4)
    ds, ds_buf = _padded(torch.full((B, Es), NAN), dev, pad=1)
    dc, dc_buf = _padded(torch.full((S * B, Ec), NAN), dev, pad=3)
    ops.s2s_embed_join_backward(d_, S, B, ds, dc)
    assert torch.isnan(ds_buf[:, Es:]).all() and torch.isnan(dc_buf[:, Ec:]).all()
    acc = d.view(S, B, -1)[0, :, :Es].clone()
    for s in range(1, S):  # ascending s, one fp32 add each
        acc = acc + d.view(S, B, -1)[s, :, :Es]
    assert torch.equal(_bits(ds), _bits(acc * math.sqrt(Es)))
    assert torch.equal(_bits(dc), _bits(d[:, Es:] * math.sqrt(Ec)))


# ---- ranking -----------------------------------------------------------------------------------------------------------------
def _rank(dev, mode, S, T, B, scores=None, mem=None, w=None, bias=None, seed=0):
    idx = torch.full((B, T), -1, dtype=torch.int64, device=dev)
    probs = torch.full((B, T, S + 2), NAN, dtype=F32, device=dev)
    per_seq = torch.full((B,), NAN, dtype=F32, device=dev)
    kw = {}
    if scores is not None:
        kw["scores"], _ = _padded(scores, dev)
    else:
        kw.update(mem=_padded(mem, dev)[0], w=w.to(dev), bias=bias.to(dev))
    ops.frechet_rank(mode, S, B, idx, probs, per_seq, seed=seed, **kw)
    assert not torch.isnan(probs).any() and not torch.isnan(per_seq).any()
    return idx.cpu(), probs.cpu(), per_seq.cpu()


def _tie_free_scores(S, B, gen):
    """a seeded permutation of well separated values per row"""
    base = torch.arange(S, dtype=F32) * 0.37 - 3.0
    return torch.stack([base[torch.randperm(S, generator=gen)] for _ in range(B)])


RANK_ALL = [(S, T, B) for S, B in itertools.product(SEQ, BATCH) for T in sorted({1, max(S // 2, 1), S})]
RANK_LARGE = [s for s in RANK_ALL if s[2] == 33 and s[0] >= 33]  # on the device alone, as the head's
RANK_SHAPES = [s for s in RANK_ALL if s not in RANK_LARGE]
MODES = [L.FRECHET_RANK_ENCODER, L.FRECHET_RANK_GREEDY]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,T,B", RANK_SHAPES)
def test_argsort_modes(backend, mode, S, T, B):
    _argsort_modes(backend.device, mode, S, T, B)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,T,B", RANK_LARGE)
def test_argsort_modes_large(mode, S, T, B):
    _argsort_modes("cuda", mode, S, T, B)


def _argsort_modes(dev, mode, S, T, B):
    scores = _tie_free_scores(S, B, torch.Generator().manual_seed(S + B))
    idx, probs, per_seq = _rank(dev, mode, S, T, B, scores=scores)
    want = torch.argsort(scores, dim=1, descending=True)[:, :T] + 2
    assert torch.equal(idx, want)
    assert torch.equal(probs, torch.zeros(B, T, S + 2).scatter(2, want.unsqueeze(2), 1.0))
    assert torch.equal(_bits(per_seq), _bits(torch.ones(B)))
    # through the scorer: mem . w + bias reproduces the scores' order
    E = 8
    mem = torch.zeros(S, B, E)
    mem[:, :, 3] = scores.t()
    idx2, probs2, _ = _rank(dev, mode, S, T, B, mem=mem.view(S * B, E), w=torch.eye(E)[3].contiguous(), bias=torch.tensor([0.5]))
    assert torch.equal(idx2, want) and torch.equal(probs2, probs)


def test_argsort_ties_go_to_the_lower_index(backend):
    scores = torch.tensor([[1.0, 2.0, 1.0, 2.0, 0.0]])
    for mode in (L.FRECHET_RANK_ENCODER, L.FRECHET_RANK_GREEDY):
        idx, _, _ = _rank(backend.device, mode, 5, 5, 1, scores=scores)
        assert idx.tolist() == [[3, 5, 2, 4, 6]]


def _sampled_statement(scores, idx):
    """the float64 pi_t rows at the returned indices [B, T, S + 2] and their clamped product [B]"""
    B, S = scores.shape
    T = idx.shape[1]
    logits = torch.cat((torch.zeros(B, T, 2, dtype=F64), scores.double().unsqueeze(1).expand(B, T, S)), dim=2)
    tgt_in_idx = torch.cat((torch.ones(B, 1, dtype=torch.int64), idx[:, :-1]), dim=1)
    probs = torch.softmax(mask_logits_by_idx(logits, tgt_in_idx), dim=2)
    return probs, per_symbol_to_per_seq_probs(probs, idx).view(B)


@pytest.mark.parametrize("S,T,B", RANK_SHAPES)
def test_sampled_mode(backend, S, T, B):
    _sampled_mode(backend.device, S, T, B)


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,B", RANK_LARGE)
def test_sampled_mode_large(S, T, B):
    _sampled_mode("cuda", S, T, B)


def _sampled_mode(dev, S, T, B):
    gen = torch.Generator().manual_seed(7 * S + B)
    scores = torch.randn(B, S, generator=gen) * 2
    idx, probs, per_seq = _rank(dev, L.FRECHET_RANK_SAMPLED, S, T, B, scores=scores, seed=1234)
    assert ((idx >= 2) & (idx < S + 2)).all()
    assert all(len(set(r)) == T for r in idx.tolist())
    want, want_seq = _sampled_statement(scores, idx)
    assert (probs[:, :, :2] == 0).all()
    for b in range(B):
        for t in range(1, T):
            assert (probs[b, t, idx[b, :t]] == 0).all()  # already chosen: exactly 0
    _close(probs, want, want.float(), f"sampled probabilities S={S} T={T} B={B}")
    _close(per_seq, want_seq, want_seq.float(), f"sampled per-sequence probability S={S} T={T} B={B}")
    again = _rank(dev, L.FRECHET_RANK_SAMPLED, S, T, B, scores=scores, seed=1234)
    for x, y in zip((idx, probs, per_seq), again):
        assert torch.equal(x, y) if x.dtype == torch.int64 else torch.equal(_bits(x), _bits(y))
    if S >= 5 and T * B >= 6:
        other, _, _ = _rank(dev, L.FRECHET_RANK_SAMPLED, S, T, B, scores=scores, seed=1235)
        assert not torch.equal(other, idx)


@pytest.mark.gpu
def test_sampled_mode_follows_the_plackett_luce_law():
    """S = T = 3, scores (0, 1, 2) in 6000 rows: each permutation's count within 5 binomial standard deviations of B times its
    exact probability prod_t e^{s_{a_t}} / sum over the remaining.  (1500 workgroups: half a minute on the interpreter, which
    runs the same statement over 400 rows below.)"""
    _plackett_luce_law("cuda", 6000)


def test_sampled_mode_follows_the_plackett_luce_law_over_400_rows(backend):
    """the same statement with the same 5 standard deviations at B = 400 (the rarest permutation is expected 12 times)"""
    _plackett_luce_law(backend.device, 400)


def _plackett_luce_law(dev, B):
    S = 3
    s = [0.0, 1.0, 2.0]
    scores = torch.tensor(s).expand(B, S).contiguous()
    idx, _, _ = _rank(dev, L.FRECHET_RANK_SAMPLED, S, S, B, scores=scores, seed=99)
    counts = {}
    for r in (idx - 2).tolist():
        counts[tuple(r)] = counts.get(tuple(r), 0) + 1
    total = 0.0
    for perm in itertools.permutations(range(S)):
        left, pr = list(range(S)), 1.0
        for a in perm:
            pr *= math.exp(s[a]) / sum(math.exp(s[c]) for c in left)
            left.remove(a)
        total += pr
        sd = math.sqrt(B * pr * (1 - pr))
        print(perm, counts.get(perm, 0), B * pr, sd)
        assert abs(counts.get(perm, 0) - B * pr) <= 5 * sd, (perm, counts.get(perm, 0), B * pr, sd)
    assert abs(total - 1.0) < 1e-12 and sum(counts.values()) == B


def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(1 << 16, device=dev)
    i = torch.full((64,), 2, dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 12, dtype=F64, device=dev)
    p, ip, wp, s = t.data_ptr(), i.data_ptr(), ws.data_ptr(), L.stream_ptr()
    lib = L.lib()
    EINVAL = -1

    def head(S=2, T=1, B=1, E=4, mem=p, w=p, bias=p, idx=ip, logged=p, clamp=NONE, log_prob=p, ld_mem=None, ld_idx=None, dw=p,
             sums=p):
        return lib.rg_frechet_head(mem, E if ld_mem is None else ld_mem, w, bias, idx, T if ld_idx is None else ld_idx, logged, p,
                                   None, clamp, 1.0, S, T, B, E, log_prob, p, p, p, sums, p, S, p, E, dw, p, wp, s)

    def rank(S=2, T=1, B=1, E=4, mode=L.FRECHET_RANK_ENCODER, scores=p, out=ip, ld=None):
        return lib.rg_frechet_rank(scores, S if ld is None else ld, None, 0, None, None, mode, 0, S, T, B, E, out, p, p, s)

    assert head() == 0 and rank() == 0
    assert head(S=65, T=1) == L.EUNSUPPORTED and rank(S=65) == L.EUNSUPPORTED  # a lane per candidate
    assert head(E=513) == L.EUNSUPPORTED
    assert head(S=64, B=1 << 23) == L.EUNSUPPORTED
    assert head(T=3) == EINVAL and rank(T=3) == EINVAL  # a slate longer than the candidates
    for bad in (dict(S=0), dict(T=0), dict(B=0), dict(E=0), dict(ld_mem=3), dict(ld_idx=0), dict(clamp=3), dict(dw=None),
                dict(sums=None), dict(logged=None), dict(mem=None), dict(w=None), dict(bias=None), dict(idx=None),
                dict(log_prob=None)):
        assert head(**bad) == EINVAL, bad
    for bad in (dict(S=0), dict(T=0), dict(B=0), dict(mode=3), dict(scores=None), dict(out=None), dict(ld=1)):
        assert rank(**bad) == EINVAL, bad
    assert lib.rg_s2s_embed_join(p, 1, p, 1, 2, 1, 2, 2, p, 4, s) == EINVAL  # a pitch below the width
    assert lib.rg_s2s_embed_join(p, 2, p, 2, 2, 1, 2, 2, p, 3, s) == EINVAL
    assert lib.rg_s2s_embed_join_backward(p, 3, 2, 1, 2, 2, p, 2, p, 2, s) == EINVAL
    assert lib.rg_s2s_embed_join_backward(p, 4, 2, 1, 2, 2, None, 2, p, 2, s) == EINVAL
    assert lib.rg_s2s_embed_join(p, 512, p, 512, 2, 1, 256, 257, p, 513, s) == L.EUNSUPPORTED  # wider than the encoder
    assert lib.rg_s2s_embed_join_backward(p, 513, 2, 1, 256, 257, p, 256, p, 257, s) == L.EUNSUPPORTED
    assert lib.rg_s2s_embed_join(p, 4, p, 4, 64, 1 << 23, 2, 2, p, 4, s) == L.EUNSUPPORTED
    assert lib.rg_frechet_head_workspace(33, 130) == 9 * 134 and lib.rg_frechet_head_workspace(1, 513) == 0
    f = dict(dtype=F32, device=dev)
    with pytest.raises(NotImplementedError, match="src_seq_len 65"):
        ops.frechet_rank(L.FRECHET_RANK_GREEDY, 65, 1, i[:1].view(1, 1), torch.zeros(67, **f), torch.zeros(1, **f),
                         scores=torch.zeros(1, 65, **f))
    with pytest.raises(NotImplementedError, match="tgt_seq_len 3"):
        ops.frechet_rank(L.FRECHET_RANK_GREEDY, 2, 1, i[:3].view(1, 3), torch.zeros(12, **f), torch.zeros(1, **f),
                         scores=torch.zeros(1, 2, **f))
    with pytest.raises(NotImplementedError, match="dim_model 513"):
        ops.frechet_head(torch.zeros(2, 513, **f), torch.zeros(513, **f), torch.zeros(1, **f), i[:1].view(1, 1), 2, 1,
                         torch.zeros(1, **f), torch.zeros(1, **f), ws)
