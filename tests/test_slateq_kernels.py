"""The SlateQ step's kernels: rg_slate_gather, rg_slate_topk and rg_slateq_head (reagent_amd/csrc/slateq.hip).

The gather only moves data (and multiplies a value by 0 or 1), so it is held to the BITS of torch's advanced indexing.
The top-k is held to a restated reference — the scores in torch fp32, then torch.sort(descending=True, stable=True) — with
exactly equal indices: the present candidates' scores are built from a permutation plus jitter (as `_head_inputs` of
tests/test_pdqn_kernels.py builds its values), the candidate's q being score / weight, so neighbouring scores are at least
0.5 / C of the range apart where a softmax or a product differs by 1e-7 of it; absent candidates score exactly +-0 and tie.
The head is held against the reference's lines (slate_q_trainer.py:204-259) restated in torch with autograd, with the
tolerances of test_pdqn_head_matches_the_restated_reference — target 1e-6, dq 1e-8, loss 1e-5 — for inputs of that test's
magnitude: q within +-3 * 3 sigma, rewards in [0, 1), and next-slate values of +-3 / K per item, so that |next_q| <= 3 and
|target| < 4 as there (1e-6 is four fp32 steps at that magnitude)."""
import pytest
import torch
import torch.nn.functional as F

import reagent_amd._lib as L
from reagent_amd import ops


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


# (B, C, K, D, output pitch pad, base offset in floats): D = 3 / 5 scalar; D = 8 / 12 / 16 in 16-byte pieces when pitch and base
# allow (pad 0 or 4, offset 0), scalar with an odd pitch (pad 1) or a base 4 bytes off; several blocks; K = C; K = 1
GATHER = [
    (5, 7, 3, 3, 0, 0),
    (300, 9, 4, 8, 0, 0),
    (300, 9, 4, 8, 1, 0),
    (64, 70, 70, 5, 3, 0),
    (33, 4, 1, 12, 4, 0),
    (33, 4, 1, 12, 0, 1),
    (257, 130, 6, 16, 0, 0),
    (257, 130, 6, 16, 2, 0),
]


@pytest.mark.parametrize("B,C,K,D,pad,off", GATHER)
def test_slate_gather_is_torch_indexing(backend, B, C, K, D, pad, off):
    dev = backend.device
    g = torch.Generator().manual_seed(B + C + K + D)
    features = torch.randn(B, C, D, generator=g)
    mask = torch.rand(B, C, generator=g) > 0.4
    value = torch.randn(B, C, generator=g)  # negative values: value * False is -0.0
    index = torch.randint(C, (B, K), generator=g)
    index[0, 0], index[B - 1, K - 1] = C - 1, 0
    nt = (torch.rand(B, generator=g) > 0.3).float()
    nt[0], nt[B - 1] = 0.0, 1.0
    rows = torch.arange(B).unsqueeze(1).expand(B, K)
    rmask = torch.rand(B, K, generator=g) > 0.5
    for not_terminal in (None, nt):
        idx = index if not_terminal is None else torch.where(not_terminal.bool().unsqueeze(1), index, torch.zeros_like(index))
        want_f, want_w = features[rows, idx].reshape(B * K, D), (value * mask)[rows, idx]
        assert torch.equal(want_w, value[rows, idx] * mask[rows, idx])
        flat = torch.full((B * K * (D + pad) + off,), float("nan")).to(dev)
        out = flat[off:].view(B * K, D + pad)[:, :D]
        weight = torch.full((B, K), float("nan")).to(dev)
        index_dev = index.to(dev)
        count = torch.full((1,), -1, dtype=torch.int32).to(dev)
        ops.slate_gather(features.to(dev), mask.to(dev), value.to(dev), index_dev, out, weight,
                         not_terminal=None if not_terminal is None else not_terminal.to(dev),
                         count_mask=rmask.to(dev), count_out=count)
        assert torch.equal(_bits(out), _bits(want_f))
        assert torch.equal(_bits(weight), _bits(want_w))
        assert torch.equal(index_dev.cpu(), index)  # the caller's indices are not zeroed in place
        assert count.item() == int(rmask.sum())
        if pad:  # the padding of every output row is untouched
            assert torch.isnan(flat[off:].view(B * K, D + pad)[:, D:]).all()


def test_slate_gather_clamps_indices_and_counts_alone(backend):
    """an index outside [0, C) is the caller's error; the kernel reads the nearest document instead of outside the arrays"""
    dev = backend.device
    B, C, K, D = 6, 5, 3, 4
    g = torch.Generator().manual_seed(2)
    features, value = torch.randn(B, C, D, generator=g), torch.rand(B, C, generator=g)
    mask = torch.ones(B, C, dtype=torch.bool)
    index = torch.randint(C, (B, K), generator=g)
    index[0, 0], index[1, 1], index[5, 2] = -3, C, 2 ** 40
    out, weight = torch.zeros(B * K, D).to(dev), torch.zeros(B, K).to(dev)
    ops.slate_gather(features.to(dev), mask.to(dev), value.to(dev), index.to(dev), out, weight)
    rows = torch.arange(B).unsqueeze(1).expand(B, K)
    idx = index.clamp(0, C - 1)
    assert torch.equal(_bits(out), _bits(features[rows, idx].reshape(B * K, D)))
    assert torch.equal(_bits(weight), _bits(value[rows, idx]))
    alone = torch.full((B, K), float("nan")).to(dev)
    ops.slate_gather(features.to(dev), mask.to(dev), value.to(dev), index.to(dev), None, alone)  # the weights alone
    assert torch.equal(_bits(alone), _bits(weight))


def _topk_inputs(B, C, single, seed, p_present=0.7, scale=3.0):
    """scores of the present candidates: a permutation of C levels plus jitter of half a level, spread over +-scale; the
    candidate's q is score / weight (weight = value * mask in (0.25, 1], or its softmax over the row).  Absent candidates
    score q * 0 = +-0 without single selection and q * softmax weight with it (then part of the permutation as well)."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(C, generator=g) for _ in range(B)]).float()
    score = ((perm + torch.rand(B, C, generator=g) * 0.5) / C - 0.5) * 2 * scale
    mask = torch.rand(B, C, generator=g) < p_present
    mask[torch.arange(B), torch.randint(C, (B,), generator=g)] = True
    value = 0.25 + 0.75 * torch.rand(B, C, generator=g)
    w = value * mask
    if single:
        w = F.softmax(w, dim=1)
    q = torch.where(w != 0, score / torch.where(w != 0, w, torch.ones_like(w)), score)
    return q, value, mask


def _topk_ref(q, value, mask, single, K):
    """_get_maxq_topk (slate_q_trainer.py:145-160) with the order of equal scores fixed: the lower index first"""
    w = value * mask
    if single:
        w = F.softmax(w, dim=1)
    order = torch.sort(q * w, dim=1, descending=True, stable=True).indices
    return order[:, :K]


def _run_topk(dev, q, value, mask, single, K):
    B = q.shape[0]
    idx = torch.full((B, K), -1, dtype=torch.int64).to(dev)
    q_sel = torch.full((B, K), float("nan")).to(dev)
    ops.slate_topk(q.to(dev), value.to(dev), mask.to(dev), single, idx, q_sel)
    return idx.cpu(), q_sel.cpu()


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("B,C,K", [(300, 7, 3), (64, 1, 1), (100, 64, 64), (65, 65, 5), (40, 130, 8), (16, 1024, 32)])
def test_slate_topk_is_a_stable_descending_sort(backend, B, C, K, single):
    q, value, mask = _topk_inputs(B, C, single, seed=B + C + K)
    want = _topk_ref(q, value, mask, single, K)
    idx, q_sel = _run_topk(backend.device, q, value, mask, single, K)
    assert torch.equal(idx, want)
    assert torch.equal(_bits(q_sel), _bits(torch.gather(q, 1, want)))


def test_slate_topk_lower_index_wins_among_exact_zeros(backend):
    """mostly padded rows without single selection: fewer positive scores than K, so the slate is filled with candidates
    whose score is exactly +0 or -0 — taken in index order, ahead of every negative score"""
    B, C, K = 50, 20, 8
    q, value, mask = _topk_inputs(B, C, False, seed=5, p_present=0.15)
    score = q * (value * mask)
    zeros_taken = (score > 0).sum(1) < K
    assert zeros_taken.sum() >= B // 2 and ((score == 0).sum(1) >= 2).all()
    assert (torch.signbit(score) & (score == 0)).any() and (~torch.signbit(score) & (score == 0)).any()
    want = _topk_ref(q, value, mask, False, K)
    idx, q_sel = _run_topk(backend.device, q, value, mask, False, K)
    assert torch.equal(idx, want)
    assert torch.equal(_bits(q_sel), _bits(torch.gather(q, 1, want)))
    for b in torch.nonzero(zeros_taken).reshape(-1).tolist():
        n_pos = int((score[b] > 0).sum())
        tail = idx[b, n_pos:]
        zero_idx = torch.nonzero(score[b] == 0).reshape(-1)
        assert torch.equal(tail[:zero_idx.numel()], zero_idx[:K - n_pos])


def _head_inputs(B, K, C, slate_size, seed, with_td):
    """rows 0, 1 terminal; rows 2, 3 with one present candidate in the normalising mask (a divisor of 1 < K when K > 1);
    row 4 with every reward_mask entry false; row 5 with all of them true; padded items (wn = 0) throughout"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, K, generator=g) * 3.0
    qn = (torch.rand(B, K, generator=g) - 0.5) * 2 * 3.0 / K
    wn = torch.rand(B, K, generator=g) * (torch.rand(B, K, generator=g) > 0.3)
    reward = torch.rand(B, K, generator=g)
    reward_mask = torch.rand(B, K, generator=g) > 0.5
    reward_mask[4], reward_mask[5] = False, True
    nt = (torch.rand(B, generator=g) > 0.2).float()
    nt[:2], nt[2:6] = 0.0, 1.0
    norm_mask = torch.rand(B, C, generator=g) > 0.5
    norm_mask[torch.arange(B), torch.randint(C, (B,), generator=g)] = True
    norm_mask[2:4] = False
    norm_mask[2, C - 1], norm_mask[3, 0] = True, True
    td = torch.randint(1, 5, (B,), generator=g).float() if with_td else None
    return dict(q=q, qn=qn, wn=wn, reward=reward, reward_mask=reward_mask, nt=nt, norm_mask=norm_mask, td=td)


def _head_ref(i, gamma, single, slate_size, scale):
    """slate_q_trainer.py:204-259 after the forwards, in torch fp32 (CPU)"""
    B, K = i["reward"].shape
    reward, nt = i["reward"], i["nt"].reshape(B, 1)
    discount = torch.full_like(reward, gamma)
    if scale and i["td"] is not None:
        discount = discount ** (i["td"].reshape(B, 1) / scale)
    value = F.softmax(i["wn"], dim=1) if single else i["wn"]
    next_q = torch.sum(i["qn"] * value, dim=1, keepdim=True)
    if not single:
        next_q = next_q / torch.minimum(i["norm_mask"].sum(1, keepdim=True), torch.tensor([slate_size]))
    next_q = next_q * nt
    target = reward + discount * next_q
    qg = i["q"].clone().requires_grad_(True)
    if single:
        loss = F.mse_loss(qg[i["reward_mask"]], target[i["reward_mask"]])
    else:
        loss = F.mse_loss(qg, target)
    loss.backward()
    return target, qg.grad, loss.detach(), next_q.reshape(-1)


# the two norm methods differ in which state's mask is handed over: "current" and "next" are two independent masks here
@pytest.mark.parametrize("with_td", [False, True])
@pytest.mark.parametrize("mode", ["single", "norm_current", "norm_next"])
@pytest.mark.parametrize("B,K", [(300, 3), (257, 8), (64, 1), (513, 5)])
def test_slateq_head_matches_the_restated_reference(backend, B, K, mode, with_td):
    dev = backend.device
    single = mode == "single"
    C, slate_size, gamma, scale = K + 4, K, 0.9, 2.0
    i = _head_inputs(B, K, C, slate_size, seed=B + K + (7 if mode == "norm_next" else 0), with_td=with_td)
    if not single:
        sizes = torch.minimum(i["norm_mask"].sum(1), torch.tensor(slate_size))
        assert (sizes[2:4] == 1).all() and (sizes >= 1).all() and (K == 1 or (sizes < K).sum() >= 2)
    want = _head_ref(i, gamma, single, slate_size, scale)
    assert want[0].abs().max() < 4.0
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    f = lambda *s: torch.full(s, float("nan")).to(dev)  # noqa: E731
    target, dq, nq, parts, out = f(B, K), f(B, K), f(B), f(ops.slateq_head_partials(B)), f(1)
    n = torch.tensor([int(i["reward_mask"].sum())], dtype=torch.int32).to(dev)
    ops.slateq_head(t(i["q"]), t(i["qn"]), t(i["wn"]), t(i["reward"]), t(i["reward_mask"]), t(i["nt"]), gamma, t(i["td"]), scale,
                    single, None if single else t(i["norm_mask"]), slate_size, n if single else None, target, dq, parts, nq)
    ops.reduce_sum(parts, parts.numel(), 1.0, out)
    assert (nq.cpu()[:2] == 0).all()  # terminal rows
    assert (nq.cpu() - want[3]).abs().max() <= 1e-6
    assert (target.cpu() - want[0]).abs().max() <= 1e-6
    assert (dq.cpu() - want[1]).abs().max() <= 1e-8
    assert abs(out.item() - want[2].item()) <= 1e-5
    if single:
        off = ~i["reward_mask"]
        assert off[4].all() and (_bits(dq)[off] == 0).all()  # exactly +0 where no reward was observed
        assert (dq.cpu()[i["reward_mask"]] != 0).any()
    else:
        assert (dq.cpu() != 0).all()  # reward_mask is ignored


def test_slateq_kernels_reject_bad_arguments(backend):
    dev = backend.device
    lib = L.lib()
    z = torch.zeros(64).to(dev)
    zi = torch.zeros(16, dtype=torch.int64).to(dev)
    p, pi, s = z.data_ptr(), zi.data_ptr(), L.stream_ptr()

    def gather(**k):
        return lib.rg_slate_gather(k.get("f", p), k.get("m", p), k.get("v", p), k.get("i", pi), k.get("nt", None), k.get("B", 2),
                                   k.get("C", 3), k.get("K", 2), k.get("D", 2), k.get("o", p), k.get("ldo", 2), k.get("w", p),
                                   k.get("cm", None), k.get("cn", 0), k.get("co", None), s)

    assert gather() == 0 and gather(nt=p) == 0 and gather(cm=p, cn=4, co=p) == 0 and gather(o=None, ldo=0) == 0
    for bad in (dict(f=None), dict(m=None), dict(v=None), dict(i=None), dict(w=None), dict(B=0), dict(B=-1),
                dict(K=0), dict(C=0), dict(D=0), dict(ldo=1), dict(cm=p, cn=4), dict(co=p), dict(cm=p, cn=0, co=p)):
        assert gather(**bad) == -1, bad

    def topk(**k):
        return lib.rg_slate_topk(k.get("q", p), k.get("v", p), k.get("m", p), k.get("B", 2), k.get("C", 4), k.get("K", 2), 0,
                                 k.get("i", pi), k.get("s", p), s)

    assert topk() == 0 and topk(K=4) == 0
    for bad in (dict(q=None), dict(v=None), dict(m=None), dict(i=None), dict(s=None), dict(B=0), dict(K=0), dict(K=5),
                dict(C=L.SLATE_MAX_CANDIDATES + 1, K=2)):
        assert topk(**bad) == -1, bad
    assert L.SLATE_MAX_CANDIDATES >= 1024

    def head(**k):
        return lib.rg_slateq_head(k.get("q", p), k.get("qn", p), p, k.get("r", p), k.get("rm", p), k.get("nt", p), 0.9,
                                  k.get("td", None), k.get("scale", 0.0), k.get("single", 1), k.get("nm", None), k.get("C", 0),
                                  k.get("ss", 0), k.get("n", pi), k.get("B", 2), k.get("K", 2), k.get("t", p), k.get("dq", p),
                                  k.get("lp", p), k.get("nq", p), s)

    zi.fill_(1)
    assert head() == 0 and head(single=0, nm=p, C=3, ss=2, rm=None, n=None) == 0 and head(td=p, scale=2.0) == 0
    for bad in (dict(q=None), dict(qn=None), dict(r=None), dict(nt=None), dict(t=None), dict(dq=None), dict(lp=None),
                dict(nq=None), dict(B=0), dict(K=0), dict(rm=None), dict(n=None), dict(td=p, scale=0.0),
                dict(single=0), dict(single=0, nm=p, C=0, ss=2), dict(single=0, nm=p, C=3, ss=0)):
        assert head(**bad) == -1, bad
