"""rg_dlinucb_accumulate and rg_dlinucb_score against the float64 statement of the reference's formulas
(reagent/training/cb/disjoint_linucb_trainer.py:66-76, reagent/models/disjoint_linucb_predictor.py:17-31 and :165-174), on
the interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24 throughout.

The bounds are those of fp32 arithmetic in ANY summation order, per arm and entry:
    |cur_A - (cur_A0 + S64)| <= (n_a + 2) u sum |w x_i x_j| + 2 u |cur_A0 + S64|      (likewise cur_b with |w y x_i|)
    |mean - x . c| <= (d + 2) u sum_i |x_i c_i|
    |sigma^2 - q64| <= (2 d + 8) u sum_ij |x_i M_ij x_j|
torch's own fp32 `x.t() @ (x * w)` is held to the first term in the same test, so the bound is fair to the reference."""
import os

import pytest
import torch

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
SIZES = [0, 1, 63, 64, 65, 257]
EINVAL = -1


def _subs(sizes, d, weighted, seed):
    """one (x [n, d], y [n], w [n] or None) per arm, on the host"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        x, y = torch.randn(n, d, generator=g), torch.randn(n, generator=g)
        out.append((x, y, (0.5 + torch.rand(n, generator=g)) if weighted else None))
    return out


def _fresh(arms, d, dev):
    return [torch.zeros(arms, d, d, device=dev), torch.zeros(arms, d, device=dev),
            torch.zeros(arms, dtype=torch.int64, device=dev)]


def _pack(subs, dev):
    x = torch.cat([s[0] for s in subs]).to(dev)
    y = torch.cat([s[1] for s in subs]).to(dev)
    w = None if subs[0][2] is None else torch.cat([s[2] for s in subs]).to(dev)
    offsets = [0]
    for s in subs:
        offsets.append(offsets[-1] + s[0].shape[0])
    return x, y, w, torch.tensor(offsets, dtype=torch.int64).to(dev)


def _accumulate(state, subs, dev, hint=None):
    from reagent_amd import ops

    x, y, w, offsets = _pack(subs, dev)
    longest = max(s[0].shape[0] for s in subs) if hint is None else hint
    ws = ops.dlinucb_workspace(longest, len(subs), x.shape[1], dev)
    ops.dlinucb_accumulate(x, y, w, offsets, longest, state[0], state[1], state[2], ws)


def _sums(sub):
    """-> (S, S_b) in float64 and their absolute sums (the bounds' right-hand sides) for one arm"""
    x, y = sub[0].double(), sub[1].double()
    w = torch.ones_like(y) if sub[2] is None else sub[2].double()
    return ((x.t() @ (x * w[:, None]), x.t() @ (w * y)),
            (x.abs().t() @ (x.abs() * w[:, None]), x.abs().t() @ (w * y).abs()))


def _check(state, before, subs, what):
    """every arm of `state` against `before` plus the float64 sums of `subs`, within the module's bound"""
    for a, sub in enumerate(subs):
        n = sub[0].shape[0]
        (S, Sb), (absS, absSb) = _sums(sub)
        for name, got, old, s64, asum in (("cur_A", state[0][a], before[0][a], S, absS),
                                          ("cur_b", state[1][a], before[1][a], Sb, absSb)):
            want = old.cpu().double() + s64
            bound = (n + 2) * U * asum + 2 * U * want.abs()
            err = (got.cpu().double() - want).abs()
            assert (err <= bound).all(), (what, a, name, (err / bound.clamp_min(1e-300)).max().item())
        assert torch.equal(state[0][a], state[0][a].t()), (what, a)
        assert state[2][a].item() == before[2][a].item() + n, (what, a)


@pytest.mark.parametrize("d", [1, 3, 32, 33, 130])
def test_accumulate_against_float64(backend, d):
    """six arms of 0, 1, 63, 64, 65 and 257 rows in ONE call, weights absent and given, from a zero state and from the state
    an earlier call left.  Per arm and entry: the bound; torch's own fp32 matmul inside its first term; cur_A[a] bitwise
    symmetric; cur_num_obs exact; the empty arm untouched; a second run bit-identical."""
    dev = backend.device
    for weighted in (False, True):
        subs = _subs(SIZES, d, weighted, 100 + d)
        for x, y, w in subs:  # the bound is fair to the reference: its fp32 matmul meets it
            n = x.shape[0]
            wc = torch.ones(n) if w is None else w
            (S, Sb), (absS, absSb) = _sums((x, y, w))
            ref_S = (x.t() @ (x * wc[:, None])).double()
            ref_Sb = (x.t() @ (y * wc)[:, None]).squeeze(1).double()
            assert ((ref_S - S).abs() <= (n + 2) * U * absS).all() and ((ref_Sb - Sb).abs() <= (n + 2) * U * absSb).all()
        for kind in ("zero", "used"):
            state = _fresh(len(SIZES), d, dev)
            if kind == "used":
                _accumulate(state, _subs([40, 3, 0, 5, 7, 9], d, weighted, 7 + d), dev)
            before = [t.clone() for t in state]
            twin = [t.clone() for t in state]
            _accumulate(state, subs, dev)
            what = (d, weighted, kind)
            _check(state, before, subs, what)
            assert torch.equal(state[0][0], before[0][0]) and torch.equal(state[1][0], before[1][0]), what  # the empty arm
            _accumulate(twin, subs, dev)
            assert all(torch.equal(a, b) for a, b in zip(state, twin)), what


@pytest.mark.parametrize("d", [3, 33])
def test_the_hint_never_drops_a_row(backend, d):
    """max_arm_rows = 1 (one slice an arm, far too short): every row still counts"""
    dev = backend.device
    subs = _subs(SIZES, d, True, 11 + d)
    state = _fresh(len(SIZES), d, dev)
    before = [t.clone() for t in state]
    _accumulate(state, subs, dev, hint=1)
    _check(state, before, subs, ("hint", d))
    zero = _fresh(len(SIZES), d, dev)
    _accumulate(zero, subs, dev, hint=0)
    _check(zero, before, subs, ("hint 0", d))


@pytest.mark.parametrize("d", [3, 33])
def test_an_arm_depends_on_its_own_rows_alone(backend, d):
    """two arms given identical rows at different positions of the packed batch (and next to different neighbours) end with
    bit-identical cur_A, cur_b; a longer neighbour (another hint, more slices in the grid) changes nothing either"""
    dev = backend.device
    other = _subs([5, 64, 300], d, True, 3 + d)
    same = _subs([257], d, True, 4 + d)[0]
    state = _fresh(5, d, dev)
    _accumulate(state, [other[0], same, other[1], same, other[2]], dev)
    assert torch.equal(state[0][1], state[0][3]) and torch.equal(state[1][1], state[1][3])
    assert state[0][1].abs().max() > 0
    longer = _subs([1100], d, True, 5 + d)[0]
    again = _fresh(2, d, dev)
    _accumulate(again, [longer, same], dev)
    assert torch.equal(again[0][1], state[0][1]) and torch.equal(again[1][1], state[1][1])


def _trainer(arms, d, dev):
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
    from reagent_amd.training import DisjointLinUCBTrainer

    scorer = DisjointLinearRegressionUCB(arms, d).to(dev)
    return DisjointLinUCBTrainer(Policy(scorer=scorer, sampler=None)), scorer


@pytest.mark.parametrize("weighted", [False, True])
def test_update_params_is_the_packed_call_on_one_arm(backend, weighted):
    """update_params(arm_idx, x, y, weight) on arm k: the bits of that arm in a packed call, the other arms untouched"""
    dev, d = backend.device, 33
    sizes = [65, 0, 257, 3]
    subs = _subs(sizes, d, weighted, 21)
    state = _fresh(len(sizes), d, dev)
    _accumulate(state, subs, dev)
    tr, scorer = _trainer(len(sizes), d, dev)
    for k in (2, 0):
        x, y, w = (None if t is None else t.to(dev) for t in subs[k])
        tr.update_params(k, x, y.reshape(-1, 1), None if w is None else w.reshape(-1, 1))
        assert torch.equal(scorer.cur_A[k], state[0][k]) and torch.equal(scorer.cur_b[k], state[1][k])
        assert scorer.cur_num_obs[k].item() == sizes[k]
    for k in (1, 3):
        assert not scorer.cur_A[k].any() and not scorer.cur_b[k].any() and scorer.cur_num_obs[k].item() == 0


@pytest.mark.gpu
def test_accumulate_d512_on_the_device():
    """the largest dimension (16 x 16 tiles, 136 of them computed per arm), two arms of 300 and 7 rows: the MI355X only"""
    import reagent_amd._lib as L

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    L.lib()
    subs = _subs([300, 7], 512, True, 5)
    state = _fresh(2, 512, "cuda")
    before = [t.clone() for t in state]
    _accumulate(state, subs, "cuda")
    _check(state, before, subs, "d512")


def _score(x, coefs, M, alpha, presence=None, want_best=False):
    from reagent_amd import ops

    B, arms, dev = x.shape[0], coefs.shape[0], x.device
    out = torch.full((3, B, arms), -7.0, device=dev)
    best = torch.full((B,), -7, dtype=torch.int64, device=dev) if want_best or presence is not None else None
    ops.dlinucb_score(x, coefs, M, alpha, out[2], mean=out[0], sigma=out[1], arm_presence=presence, best_arm=best)
    return out, best


def _score_inputs(B, d, arms, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * B + 10 * d + arms + seed)
    x, c = torch.randn(B, d, generator=g), torch.randn(arms, d, generator=g)
    G = torch.randn(arms, d, d, generator=g)
    M = G @ G.transpose(1, 2) / d + torch.eye(d) * (1.0 + torch.arange(arms).view(arms, 1, 1))
    M = ((M + M.transpose(1, 2)) / 2).contiguous()  # symmetric positive definite, another one per arm
    return x.to(dev), c.to(dev), M.to(dev)


def _check_score_against_float64(dev, B, d, arms, alpha):
    """the module's score bounds at one shape; prints the worst error / bound of the mean and of sigma^2"""
    x, c, M = _score_inputs(B, d, arms, dev)
    if alpha == 0.0:
        M = torch.full_like(M, float("nan"))  # never read
    out, _ = _score(x, c, M, alpha)
    x64, c64, M64 = x.cpu().double(), c.cpu().double(), M.cpu().double()
    mean, sigma, ucb = (t.cpu() for t in out)
    mean_err, mean_bound = (mean.double() - x64 @ c64.t()).abs(), (d + 2) * U * (x64.abs() @ c64.abs().t())
    ratios = [(mean_err / mean_bound.clamp_min(1e-300)).max().item(), 0.0]
    assert (mean_err <= mean_bound).all()
    if alpha == 0.0:
        assert torch.isfinite(out).all()
        assert torch.equal(sigma, torch.zeros(B, arms)) and torch.equal(ucb.view(torch.int32), mean.view(torch.int32))
    else:
        q64 = torch.einsum("ijk,jk->ji", torch.matmul(x64, M64), x64)
        qabs = torch.einsum("ijk,jk->ji", torch.matmul(x64.abs(), M64.abs()), x64.abs())
        err = (sigma.double() ** 2 - q64).abs()
        ratios[1] = (err / ((2 * d + 8) * U * qabs)).max().item()
        assert (err <= (2 * d + 8) * U * qabs).all(), (err / qabs).max().item() / U
        assert torch.equal(ucb, mean + torch.tensor(alpha) * sigma)  # one multiply and one add in fp32
    again, _ = _score(x, c, M, alpha)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # the optional outputs may be absent: ucb alone has the same bits
    from reagent_amd import ops

    alone = torch.empty(B, arms, device=x.device)
    ops.dlinucb_score(x, c, M, alpha, alone)
    assert torch.equal(alone, out[2])
    print(f"dlinucb_score B={B} d={d} arms={arms} alpha={alpha}: mean {ratios[0]:.4f} of its bound, sigma^2 {ratios[1]:.4f}")


@pytest.mark.parametrize("alpha", [0.0, 1.5])
@pytest.mark.parametrize("arms", [1, 5])
@pytest.mark.parametrize("d", [1, 33, 130])
@pytest.mark.parametrize("B", [1, 33, 65])
def test_score_against_float64(backend, B, d, arms, alpha):
    _check_score_against_float64(backend.device, B, d, arms, alpha)


@pytest.mark.parametrize("d", [256, 257, 385, 512])
@pytest.mark.parametrize("B", [33, 65])
def test_score_over_the_whole_legal_width(backend, B, d):
    """the widths the two-row-tile kernel exists for (d > 256: four tiles of x do not fit in LDS) and the largest dynamic
    LDS requests: R = 4 at (B, d) = (65, 256), about 137 KB, R = 2 everywhere else, about 134 KB at d = 512.  Two arms with
    different matrices; B = 33 and 65 leave one live row in the last row tile.  The bounds are
    test_score_against_float64's."""
    _check_score_against_float64(backend.device, B, d, 2, 1.5)


@pytest.mark.parametrize("d", [33, 200, 257, 512])
def test_score_of_integer_inputs_is_exact(backend, d):
    """Small integer inputs (x, coefs in [-3, 3]; M = G + G^T + round(8 sqrt(d)) I, G in [-2, 2]; another M and coefs per
    arm): every product and every partial sum, in any order, is an integer below 2^24, so the mean is bit-equal to x @ c and
    round(sigma^2) == q exactly.  One dropped, doubled or misplaced (i, j) term fails at any d, where the any-order bound
    (which grows with d) would let it pass.  q < 2^20: a sigma 2 ulp off moves sigma^2 by less than q 2^-21 < 1/2."""
    dev, N, arms = backend.device, 40, 2
    g = torch.Generator().manual_seed(29 + d)
    x = torch.randint(-3, 4, (N, d), generator=g).float()
    c = torch.randint(-3, 4, (arms, d), generator=g).float()
    G = torch.randint(-2, 3, (arms, d, d), generator=g).float()
    M = (G + G.transpose(1, 2) + round(8 * d ** 0.5) * torch.eye(d)).contiguous()
    x64, M64 = x.double(), M.double()
    q64 = torch.einsum("ijk,jk->ji", torch.matmul(x64, M64), x64)
    qabs = torch.einsum("ijk,jk->ji", torch.matmul(x64.abs(), M64.abs()), x64.abs())
    assert qabs.max().item() < 2.0 ** 24 and (x64.abs() @ c.double().abs().t()).max().item() < 2.0 ** 24  # the sums are exact
    assert q64.min().item() > 0 and q64.max().item() < 2.0 ** 20
    out, _ = _score(x.to(dev), c.to(dev), M.to(dev), 1.5)
    mean, sigma, ucb = (t.cpu() for t in out)
    assert torch.equal(mean.double(), x64 @ c.double().t())
    got_q = torch.round(sigma.double() ** 2)
    assert torch.equal(got_q, q64), (got_q - q64).abs().max().item()
    assert torch.equal(ucb, mean + torch.tensor(1.5) * sigma)
    ulps = (sigma.view(torch.int32).long() - q64.sqrt().float().view(torch.int32).long()).abs().max().item()
    print(f"dlinucb_score exact d={d}: max qabs {qabs.max().item():.3e}, q in [{q64.min().item():.0f}, "
          f"{q64.max().item():.0f}], sigma within {ulps} ulp of sqrt(q)")


@pytest.mark.parametrize("B,d", [(65, 33), (300, 257), (600, 33)])
def test_accumulate_of_integer_inputs_is_exact(backend, B, d):
    """x, y integers in [-3, 3], w in {1, 2, 4}: every partial sum is an integer far below 2^24, so from a zero state
    cur_A[a] == S and cur_b[a] == S_b EXACTLY, per arm (one of B rows, one of 5; (600, 33) is three slices)"""
    dev = backend.device
    g = torch.Generator().manual_seed(5 * B + d)
    subs = []
    for n in (B, 5):
        x, y = torch.randint(-3, 4, (n, d), generator=g).float(), torch.randint(-3, 4, (n,), generator=g).float()
        subs.append((x, y, torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (n,), generator=g)]))
    state = _fresh(2, d, dev)
    _accumulate(state, subs, dev)
    for a, sub in enumerate(subs):
        (S, Sb), _ = _sums(sub)
        assert torch.equal(state[0][a].cpu().double(), S) and torch.equal(state[1][a].cpu().double(), Sb), a
        assert S.abs().max().item() > 0 and state[2][a].item() == sub[0].shape[0]


def test_accumulate_with_slices_longer_than_one_unit(backend):
    """d = 130: 15 tiles, so dcb_plan cuts an arm into slices of 3 x 256 = 768 rows; arms of 800, 0 and 769 rows take two
    slices each (the second of 32 rows and of one).  The module's bound per arm, and the arm of 800 rows in a call of its
    own gives the same bits."""
    dev, d = backend.device, 130
    subs = _subs([800, 0, 769], d, True, 41)
    state = _fresh(3, d, dev)
    before = [t.clone() for t in state]
    _accumulate(state, subs, dev)
    _check(state, before, subs, "long slices")
    for a, sub in enumerate(subs):
        if sub[0].shape[0]:
            (S, _), (absS, _) = _sums(sub)
            n = sub[0].shape[0]
            ratio = ((state[0][a].cpu().double() - S).abs() / ((n + 2) * U * absS + 2 * U * S.abs())).max().item()
            print(f"dlinucb_accumulate d={d} arm of {n} rows: cur_A {ratio:.4f} of its bound")
    assert not state[0][1].any() and not state[1][1].any() and state[2].tolist() == [800, 0, 769]
    alone = _fresh(1, d, dev)
    _accumulate(alone, subs[:1], dev)
    assert torch.equal(alone[0][0], state[0][0]) and torch.equal(alone[1][0], state[1][0])


@pytest.mark.parametrize("arms", [3, 5])
def test_best_arm_on_non_finite_scores_is_the_references(backend, arms):
    """tests/golden/cb/argmax_nonfinite.npz: the unmodified reference's get_model_actions on rows with NaN and +-inf among
    present and absent arms.  At d = 1, x = 1 and ucb_alpha = 0 the ucb of arm a is coefs[a] itself, so a row of the
    fixture is planted through coefs; every row with the same scores goes into one call, one batch row per mask.  The
    first present NaN wins, a present -inf is worth what an absent arm is, arm 0 where nothing beats -inf."""
    import numpy as np

    from golden_util import GOLDEN

    dev = backend.device
    with np.load(os.path.join(GOLDEN, "cb", "argmax_nonfinite.npz")) as z:
        scores, mask, masked, plain = (torch.from_numpy(z[f"a{arms}_{k}"])
                                       for k in ("scores", "mask", "actions_masked", "actions_plain"))
    groups = {}
    for r in range(scores.shape[0]):
        groups.setdefault(tuple(scores[r].view(torch.int32).tolist()), []).append(r)
    assert len(groups) >= 4
    for rows in groups.values():
        B = len(rows)
        c = scores[rows[0]].view(arms, 1).to(dev)
        out, best = _score(torch.ones(B, 1, device=dev), c, torch.ones(arms, 1, 1, device=dev), 0.0,
                           presence=mask[rows].to(dev))
        assert torch.equal(out[2].cpu().view(torch.int32), scores[rows].view(torch.int32))  # the scores, bit for bit
        assert torch.equal(best.cpu(), masked[rows].reshape(-1)), (scores[rows[0]], mask[rows], best)
        _, best = _score(torch.ones(1, 1, device=dev), c, torch.ones(arms, 1, 1, device=dev), 0.0, want_best=True)
        assert best.item() == plain[rows[0]].item(), scores[rows[0]]


def test_a_negative_definite_arm_is_nan_in_its_own_column_only(backend):
    dev, B, d, arms = backend.device, 65, 33, 5
    x, c, M = _score_inputs(B, d, arms, dev)
    M[3] = -torch.eye(d, device=dev)
    out, _ = _score(x, c, M, 1.5)
    nan = torch.isnan(out[2])
    assert nan[:, 3].all() and not nan[:, [0, 1, 2, 4]].any() and torch.isnan(out[1][:, 3]).all()
    assert torch.isfinite(out[0]).all()
    from reagent_amd.models.disjoint_linucb_predictor import batch_quadratic_form_multi_arms

    q = batch_quadratic_form_multi_arms(x, M[:3])
    x64, M64 = x.cpu().double(), M[:3].cpu().double()
    q64 = torch.einsum("ijk,jk->ji", torch.matmul(x64, M64), x64)
    qabs = torch.einsum("ijk,jk->ji", torch.matmul(x64.abs(), M64.abs()), x64.abs())
    assert q.shape == (B, 3) and ((q.cpu().double() - q64).abs() <= (2 * d + 8) * U * qabs).all()


@pytest.mark.parametrize("B,arms", [(1, 1), (37, 5), (70, 5)])
@pytest.mark.parametrize("masked", [False, True])
def test_best_arm_is_the_masked_argmax_of_the_kernels_ucb(backend, B, arms, masked):
    """best_arm equals torch.argmax of the kernel's own ucb under the mask.  Arms 1 and 3 share coefs and inv_A: an exact
    tie in every row, the maximum in rows 0 and 2 by construction (the lower index wins); with a mask, row 2 has the tie's
    lower arm absent and row 1 no arm present at all (arm 0)."""
    dev, d = backend.device, 33
    x, c, M = _score_inputs(B, d, arms, dev, seed=3)
    if arms > 2:
        c[3], M[3] = c[1], M[1]
        for b in (0, 2):
            x[b] = 4.0 * c[1] / c[1].norm()
    presence = None
    if masked:
        g = torch.Generator().manual_seed(B)
        presence = (torch.rand(B, arms, generator=g) < 0.6).to(dev)
        if arms > 2:
            presence[0, 1] = presence[0, 3] = True
            presence[2, 1] = False  # the tie's lower arm is absent: the higher one is the answer
            presence[2, 3] = True
            presence[1] = False
    out, best = _score(x, c, M, 1.5, presence=presence, want_best=True)
    ucb = out[2]
    if arms > 2:
        assert torch.equal(ucb[:, 1], ucb[:, 3]) and ucb[0, 1] == ucb[0].max() and ucb[2, 1] == ucb[2].max()
    want = (ucb if presence is None else torch.where(presence, ucb, torch.full_like(ucb, float("-inf")))).argmax(1)
    assert torch.equal(best, want)
    if arms > 2:
        assert best[0].item() == 1 and best[2].item() == (3 if masked else 1)
        if masked:
            assert best[1].item() == 0
    mean_only, best0 = _score(x, c, M, 0.0, presence=presence, want_best=True)
    m = mean_only[2]
    assert torch.equal(best0, (m if presence is None else torch.where(presence, m, torch.full_like(m, float("-inf")))).argmax(1))


def test_bad_arguments_are_refused(backend):
    import reagent_amd._lib as L

    lib, dev = L.lib(), backend.device
    d, arms = 4, 2
    subs = _subs([5, 3], d, False, 0)
    x, y, _, off = _pack(subs, dev)
    st = _fresh(arms, d, dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    p = L.ptr

    def acc(x_=p(x), y_=p(y), off_=p(off), n=8, arms_=arms, hint=5, d_=d, A_=p(st[0]), b_=p(st[1]), obs_=p(st[2]),
            ws_=p(ws), nbytes=ws.numel()):
        return lib.rg_dlinucb_accumulate(x_, y_, None, off_, n, arms_, hint, d_, A_, b_, obs_, ws_, nbytes, None)

    assert acc(d_=0) == EINVAL and acc(d_=513) == EINVAL and acc(arms_=0) == EINVAL and acc(n=-1) == EINVAL
    assert acc(hint=-1) == EINVAL and acc(nbytes=16) == EINVAL
    for name in ("x_", "y_", "off_", "A_", "b_", "obs_", "ws_"):
        assert acc(**{name: None}) == EINVAL, name
    assert lib.rg_dlinucb_workspace_bytes(5, arms, 0) == 0 and lib.rg_dlinucb_workspace_bytes(5, arms, 513) == 0
    assert lib.rg_dlinucb_workspace_bytes(5, 0, d) == 0 and lib.rg_dlinucb_workspace_bytes(-1, arms, d) == 0
    assert lib.rg_dlinucb_workspace_bytes(0, arms, d) > 0 and lib.rg_dlinucb_workspace_bytes(5, arms, 512) > 0
    assert not st[0].any() and not st[1].any() and not st[2].any()  # nothing ran
    assert acc(n=0, x_=None, y_=None) == 0  # no row at all is legal ...
    assert not st[0].any() and not st[1].any() and not st[2].any()  # ... and changes nothing
    assert acc() == 0 and st[2].tolist() == [5, 3]
    B = 8
    out = torch.zeros(3, B, arms, device=dev)
    c, M = torch.zeros(arms, d, device=dev), torch.eye(d, device=dev).repeat(arms, 1, 1)
    best = torch.zeros(B, dtype=torch.int64, device=dev)
    mask = torch.ones(B, arms, dtype=torch.uint8, device=dev)

    def score(x_=p(x), c_=p(c), M_=p(M), B_=B, d_=d, arms_=arms, mask_=None, ucb_=p(out[2]), best_=None):
        return lib.rg_dlinucb_score(x_, c_, M_, 1.0, B_, d_, arms_, mask_, p(out[0]), p(out[1]), ucb_, best_, None)

    assert score(B_=0) == EINVAL and score(arms_=0) == EINVAL and score(d_=0) == EINVAL and score(d_=513) == EINVAL
    assert score(x_=None) == EINVAL and score(c_=None) == EINVAL and score(M_=None) == EINVAL and score(ucb_=None) == EINVAL
    assert score(mask_=p(mask)) == EINVAL
    assert not out.any()
    assert score(mask_=p(mask), best_=p(best)) == 0 and score() == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cb_disjoint_kernels_have_no_scratch(tmp_path):
    """cb_disjoint.hip compiled for gfx950 with the resource remarks on: its kernels, no scratch, no spilled register"""
    kernels = kernel_resources("cb_disjoint.hip", tmp_path)
    for want, count in (("dlinucb_gram_kernel", 1), ("dlinucb_finish_kernel", 1), ("dlinucb_score_kernel", 2)):
        assert sum(want in k for k in kernels) == count, (want, list(kernels))
    assert len(kernels) == 4
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
