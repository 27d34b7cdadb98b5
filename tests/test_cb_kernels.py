"""rg_linucb_accumulate and rg_linucb_score against the float64 statement of the reference's formulas
(reagent/training/cb/linucb_trainer.py:64-75, reagent/models/linear_regression.py:213-234), on the interpreter and, under
`-m gpu`, on the MI355X.  u = 2^-24 throughout.

The bounds are those of fp32 arithmetic in ANY summation order, per entry:
    |S - S64| <= (B + 2) u sum_b |w x_i x_j|                      (and likewise S_b with |w y x_i|, s_w with |w|)
    updated average: that bound / cur_sum_weight + 8 u |value|
    |label - label64| <= (d + 2) u sum_i |x_i c_i|
    |sigma^2 W - q64| <= (2 d + 8) u sum_ij |x_i M_ij x_j|
torch's own fp32 `x.t() @ (x * w)` is held to the first one in the same test, so the bound is fair to the reference."""
import os

import pytest
import torch

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64


def _batch(B, d, weighted, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d, generator=g)
    y = torch.randn(B, generator=g)
    w = (0.5 + torch.rand(B, generator=g)) if weighted else None
    return x.to(dev), y.to(dev), None if w is None else w.to(dev)


def _fresh(d, dev, sum_weight=1e-5):
    return [torch.zeros(d, d, device=dev), torch.zeros(d, device=dev), torch.full((1,), sum_weight, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev)]


def _accumulate(state, x, y, w, action=None):
    from reagent_amd import ops

    ws = ops.linucb_workspace(x.shape[0], x.shape[-1], x.device)
    ops.linucb_accumulate(x, y, w, state[0], state[1], state[2], state[3], ws, action=action)


def _statement(state, x, y, w):
    """-> the float64 update of (cur_avg_A, cur_avg_b, cur_sum_weight) from the fp32 state and inputs, the batch sums
    (S, S_b, s_w) and their absolute sums (the bounds' right-hand sides)"""
    A0, b0, sw0 = (t.detach().cpu().double() for t in state[:3])
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    w = torch.ones_like(y) if w is None else w.detach().cpu().double()
    S, Sb, s_w = x.t() @ (x * w[:, None]), x.t() @ (w * y), w.sum()
    absS, absSb, absw = x.abs().t() @ (x.abs() * w.abs()[:, None]), x.abs().t() @ (w * y).abs(), w.abs().sum()
    sw1 = sw0 + s_w
    keep = 1.0 - s_w / sw1
    return (A0 * keep + S / sw1, b0 * keep + Sb / sw1, sw1), (S, Sb, s_w), (absS, absSb, absw)


def _check_update(state_after, want, abs_sums, B, what):
    (A1, b1, sw1), (absS, absSb, absw) = want, abs_sums
    got_A, got_b, got_sw = (t.detach().cpu().double() for t in state_after[:3])
    for name, got, ref, asum in (("cur_avg_A", got_A, A1, absS), ("cur_avg_b", got_b, b1, absSb)):
        bound = (B + 2) * U * asum / sw1 + 8 * U * ref.abs()
        over = ((got - ref).abs() - bound).max().item()
        assert over <= 0, (what, name, over, ((got - ref).abs() / bound.clamp_min(1e-300)).max().item())
    assert abs(got_sw.item() - sw1.item()) <= (B + 2) * U * absw.item() + 8 * U * abs(sw1.item()), (what, got_sw, sw1)


@pytest.mark.parametrize("d", [1, 3, 32, 33, 130])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_accumulate_against_float64(backend, B, d):
    """weights absent and given x an empty state (cur_sum_weight = 1e-5 as constructed, exactly 0 as after an epoch end) and a
    state an earlier batch left.  Held per entry: the batch sums of torch's own fp32 matmul, the updated averages and the
    sum of weights; cur_avg_A bitwise symmetric; cur_num_obs exact; a second run bit-identical."""
    dev = backend.device
    for weighted in (False, True):
        x, y, w = _batch(B, d, weighted, 100 * B + d, dev)
        # the bound is fair to the reference: its fp32 matmul meets it
        _, (S, Sb, _), (absS, absSb, _) = _statement(_fresh(d, "cpu"), x, y, w)
        xc, yc = x.cpu(), y.cpu()
        wc = torch.ones(B) if w is None else w.cpu()
        ref_S = (xc.t() @ (xc * wc[:, None])).double()
        ref_Sb = (xc.t() @ (yc * wc)[:, None]).squeeze(1).double()
        assert ((ref_S - S).abs() <= (B + 2) * U * absS).all() and ((ref_Sb - Sb).abs() <= (B + 2) * U * absSb).all()
        for kind in ("fresh", "zero", "used"):
            state = _fresh(d, dev, 0.0 if kind == "zero" else 1e-5)
            n0 = 0
            if kind == "used":
                x0, y0, w0 = _batch(40, d, weighted, 7 + d, dev)
                _accumulate(state, x0, y0, w0)
                n0 = 40
            twin = [t.clone() for t in state]
            want, sums, abs_sums = _statement(state, x, y, w)
            _accumulate(state, x, y, w)
            what = (B, d, weighted, kind)
            _check_update(state, want, abs_sums, B, what)
            if kind == "fresh":  # the batch sums themselves: cur_avg * cur_sum_weight from an empty state
                got_S = state[0].cpu().double() * state[2].cpu().double()
                assert ((got_S - sums[0]).abs() <= (B + 2) * U * abs_sums[0] + 8 * U * sums[0].abs()).all(), what
            assert torch.equal(state[0], state[0].t()), what
            assert state[3].item() == n0 + B, what
            _accumulate(twin, x, y, w)
            assert all(torch.equal(a, b) for a, b in zip(state, twin)), what


@pytest.mark.gpu
def test_accumulate_d512_on_the_device():
    """the largest dimension (16 x 16 tiles, 136 of them computed), B = 300 (two slices): the MI355X only"""
    import reagent_amd._lib as L

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    L.lib()
    B, d = 300, 512
    x, y, w = _batch(B, d, True, 5, "cuda")
    state = _fresh(d, "cuda")
    want, _, abs_sums = _statement(state, x, y, w)
    _accumulate(state, x, y, w)
    _check_update(state, want, abs_sums, B, (B, d))
    assert torch.equal(state[0], state[0].t()) and state[3].item() == B


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", [3, 33, 130])
@pytest.mark.parametrize("B", [1, 65, 256])
def test_the_joint_and_disjoint_accumulate_paths_are_one_arithmetic(backend, B, d, weighted):
    """From a state of exact zeros (cur_sum_weight included) the running average of one batch is S / s_w, and the disjoint
    kernels' one arm over the same rows holds S itself: cur_avg_A == cur_A[0] / cur_sum_weight and cur_avg_b == cur_b[0] /
    cur_sum_weight bit for bit (one fp32 division each), both counters B.  This holds the two Gram kernels to one walk over
    the rows, one merge of the waves and one order over the slices.  B stays at or below 256: above it the two plans cut
    the rows into different slices (cb_plan by (B, d), dcb_plan by d alone) and the bits legitimately differ."""
    from reagent_amd import ops

    dev = backend.device
    x, y, w = _batch(B, d, weighted, 31 * B + d, dev)
    joint = _fresh(d, dev, 0.0)
    _accumulate(joint, x, y, w)
    cur_A, cur_b = torch.zeros(1, d, d, device=dev), torch.zeros(1, d, device=dev)
    obs = torch.zeros(1, dtype=torch.int64, device=dev)
    offsets = torch.tensor([0, B], dtype=torch.int64).to(dev)
    ops.dlinucb_accumulate(x, y, w, offsets, B, cur_A, cur_b, obs, ops.dlinucb_workspace(B, 1, d, dev))
    assert joint[2].item() > 0
    assert torch.equal(joint[0], cur_A[0] / joint[2]) and torch.equal(joint[1], cur_b[0] / joint[2])
    assert joint[3].item() == B and obs.item() == B


@pytest.mark.parametrize("A", [1, 5])
def test_accumulate_reads_the_chosen_arm_in_place(backend, A):
    """[B, A, d] + action is bit-identical to the pre-gathered [B, d] form; an index outside [0, A) is clamped into it"""
    dev = backend.device
    B, d = 65, 33
    g = torch.Generator().manual_seed(A)
    x3 = torch.randn(B, A, d, generator=g).to(dev)
    action = torch.randint(0, A, (B,), generator=g).to(dev)
    y, w = torch.randn(B, generator=g).to(dev), (0.5 + torch.rand(B, generator=g)).to(dev)
    gathered = torch.gather(x3, 1, action.view(B, 1, 1).expand(-1, 1, d)).squeeze(1).contiguous()
    a, b = _fresh(d, dev), _fresh(d, dev)
    _accumulate(a, gathered, y, w)
    _accumulate(b, x3, y, w, action=action)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    wild = action.clone()
    wild[0], wild[1] = -3, A + 7
    clamped = wild.clamp(0, A - 1)
    c, e = _fresh(d, dev), _fresh(d, dev)
    _accumulate(c, x3, y, w, action=wild)
    _accumulate(e, x3, y, w, action=clamped)
    assert all(torch.equal(s, t) for s, t in zip(c, e))


def test_bad_arguments_are_refused(backend):
    import reagent_amd._lib as L

    lib, dev = L.lib(), backend.device
    d, B = 4, 8
    x, y, _ = _batch(B, d, False, 0, dev)
    st = _fresh(d, dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    act = torch.zeros(B, dtype=torch.int64, device=dev)
    p = L.ptr

    def acc(x_=p(x), action=None, arms=1, y_=p(y), B_=B, d_=d, A_=p(st[0]), ws_=p(ws), nbytes=ws.numel()):
        return lib.rg_linucb_accumulate(x_, action, arms, y_, None, B_, d_, A_, p(st[1]), p(st[2]), p(st[3]), ws_, nbytes, None)

    EINVAL = -1
    assert acc(d_=0) == EINVAL and acc(d_=513) == EINVAL and acc(B_=0) == EINVAL
    assert acc(x_=None) == EINVAL and acc(y_=None) == EINVAL and acc(A_=None) == EINVAL and acc(ws_=None) == EINVAL
    assert acc(action=p(act), arms=0) == EINVAL and acc(nbytes=16) == EINVAL
    assert lib.rg_linucb_workspace_bytes(B, 0) == 0 and lib.rg_linucb_workspace_bytes(B, 513) == 0
    assert lib.rg_linucb_workspace_bytes(0, d) == 0 and lib.rg_linucb_workspace_bytes(B, 512) > 0
    assert torch.equal(st[0], torch.zeros_like(st[0])) and st[3].item() == 0  # nothing ran
    out = torch.empty(3, B, device=dev)
    nan = torch.zeros(2, dtype=torch.int32, device=dev)
    c, M, sw = torch.zeros(d, device=dev), torch.eye(d, device=dev), torch.ones(1, device=dev)
    best = torch.zeros(B, dtype=torch.int64, device=dev)

    def score(n=B, d_=d, arms=0, x_=p(x), best_=None, nan_=p(nan[:1])):
        return lib.rg_linucb_score(x_, p(c), p(M), p(sw), 1.0, n, d_, arms, None, p(out[0]), p(out[1]), p(out[2]),
                                   p(nan[1:]), nan_, best_, None)

    assert score(n=0) == EINVAL and score(d_=0) == EINVAL and score(d_=513) == EINVAL and score(arms=-1) == EINVAL
    assert score(x_=None) == EINVAL and score(nan_=None) == EINVAL
    assert score(arms=2, best_=None) == EINVAL and score(arms=3, best_=p(best)) == EINVAL  # 8 rows are no multiple of 3
    assert score(arms=2, best_=p(best)) == 0


def _score(x, coefs, M, sw, alpha, arms=0, presence=None):
    from reagent_amd import ops

    N, dev = x.shape[0], x.device
    out = torch.empty(3, N, device=dev)
    nan = torch.full((ops.linucb_score_partials(N) + 1,), -7, dtype=torch.int32, device=dev)
    best = torch.full((N // arms,), -7, dtype=torch.int64, device=dev) if arms else None
    ops.linucb_score(x, coefs, M, sw, alpha, out[0], out[1], out[2], nan[1:], nan[:1], arms=arms, arm_presence=presence,
                     best_arm=best)
    return out, int(nan[0].item()), best


def _score_inputs(N, d, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * N + d + seed)
    x, c = torch.randn(N, d, generator=g), torch.randn(d, generator=g)
    G = torch.randn(d, d, generator=g)
    M = G @ G.t() / d + torch.eye(d)
    M = ((M + M.t()) / 2).contiguous()  # symmetric positive definite
    return x.to(dev), c.to(dev), M.to(dev), torch.full((1,), 37.5, device=dev)


def _check_score_against_float64(dev, N, d, alpha):
    """the module's score bounds at one shape; prints and returns the worst error / bound of the mean and of sigma^2"""
    x, c, M, sw = _score_inputs(N, d, dev)
    out, nan_count, _ = _score(x, c, M, sw, alpha)
    x64, c64, M64 = x.cpu().double(), c.cpu().double(), M.cpu().double()
    label, sigma, ucb = (t.cpu() for t in out)
    mean_err, mean_bound = (label.double() - x64 @ c64).abs(), (d + 2) * U * (x64.abs() @ c64.abs())
    ratios = [(mean_err / mean_bound.clamp_min(1e-300)).max().item(), 0.0]
    assert (mean_err <= mean_bound).all()
    assert nan_count == 0
    if alpha == 0.0:
        assert torch.equal(sigma, torch.zeros(N)) and torch.equal(ucb, label)  # exactly 0, not a small number
    else:
        q64 = ((x64 @ M64) * x64).sum(-1)
        qabs = ((x64.abs() @ M64.abs()) * x64.abs()).sum(-1)
        q_err, q_bound = (sigma.double() ** 2 * sw.cpu().double() - q64).abs(), (2 * d + 8) * U * qabs
        ratios[1] = (q_err / q_bound).max().item()
        assert (q_err <= q_bound).all()
        assert torch.equal(ucb, label + torch.tensor(alpha) * sigma)  # one multiply and one add in fp32
    again, _, _ = _score(x, c, M, sw, alpha)
    assert torch.equal(out, again)
    print(f"linucb_score N={N} d={d} alpha={alpha}: mean {ratios[0]:.4f} of its bound, sigma^2 {ratios[1]:.4f}")
    return ratios


@pytest.mark.parametrize("alpha", [0.0, 1.5])
@pytest.mark.parametrize("d", [1, 33, 130])
@pytest.mark.parametrize("N", [1, 65, 5 * 37])
def test_score_against_float64(backend, N, d, alpha):
    _check_score_against_float64(backend.device, N, d, alpha)


@pytest.mark.parametrize("d", [128, 129, 256, 257, 385, 512])
def test_score_over_the_whole_legal_width(backend, d):
    """the K loop's chunk boundaries (one, two, three and four staged chunks of 128 columns, each full and with one column
    in the last) and every count of column tiles a wave can own, score_chunk<1> .. <4>; N = 33: two workgroups, the second
    with one live row.  The bounds are test_score_against_float64's."""
    _check_score_against_float64(backend.device, 33, d, 1.5)


def _integer_score_inputs(N, d, arms, seed):
    """x [N, d] and coefs [arms, d] integers in [-3, 3]; M [arms, d, d] = G + G^T + round(8 sqrt(d)) I with G integer in
    [-2, 2]: symmetric, positive definite by its diagonal, and small enough that every product and every partial sum of
    x . c and of x^T M x, in ANY order, is an integer below 2^24 -- an fp32 result equals the float64 one exactly.
    -> x, coefs, M as float32 on the host; q64 [N, arms] and the largest sum of absolute terms"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, d), generator=g).float()
    c = torch.randint(-3, 4, (arms, d), generator=g).float()
    G = torch.randint(-2, 3, (arms, d, d), generator=g).float()
    M = (G + G.transpose(1, 2) + round(8 * d ** 0.5) * torch.eye(d)).contiguous()
    x64, M64 = x.double(), M.double()
    q64 = torch.einsum("ijk,jk->ji", torch.matmul(x64, M64), x64)
    qabs = torch.einsum("ijk,jk->ji", torch.matmul(x64.abs(), M64.abs()), x64.abs())
    # from the float64 statement alone: the sums are exact in fp32, and q is small enough that a sigma a few ulp off (sqrtf
    # and the division are the device's own) moves sigma^2 W by less than q 2^-21 < 1/2, so rounding recovers q
    assert qabs.max().item() < 2.0 ** 24 and (x64.abs() @ c.double().abs().t()).max().item() < 2.0 ** 24
    assert q64.min().item() > 0 and q64.max().item() < 2.0 ** 20
    return x, c, M, q64, qabs.max().item()


def _sigma_ulps(sigma, q_over_w):
    """the largest distance, in units of fp32 spacing, of sigma from the correctly rounded sqrt(q / W)"""
    want = q_over_w.sqrt().float()
    return (sigma.view(torch.int32).long() - want.view(torch.int32).long()).abs().max().item()


@pytest.mark.parametrize("d", [33, 200, 257, 512])
def test_score_of_integer_inputs_is_exact(backend, d):
    """Small integer inputs (_integer_score_inputs): the mean is bit-equal to x @ c and round(sigma^2 W) == q exactly, at
    any d.  One dropped, doubled or misplaced (i, j) term moves q by an integer and fails, where the any-order bound of
    test_score_against_float64 (which grows with d) would let it pass."""
    dev, N, W = backend.device, 40, 4.0
    x, c, M, q64, qabs = _integer_score_inputs(N, d, 1, 17 + d)
    out, nan_count, _ = _score(x.to(dev), c[0].to(dev), M[0].to(dev), torch.full((1,), W, device=dev), 1.5)
    label, sigma, ucb = (t.cpu() for t in out)
    assert nan_count == 0
    assert torch.equal(label.double(), x.double() @ c[0].double())
    got_q = torch.round(sigma.double() ** 2 * W)
    assert torch.equal(got_q, q64[:, 0]), (got_q - q64[:, 0]).abs().max().item()
    assert torch.equal(ucb, label + torch.tensor(1.5) * sigma)
    print(f"linucb_score exact d={d}: max qabs {qabs:.3e}, q in [{q64.min().item():.0f}, {q64.max().item():.0f}], "
          f"sigma within {_sigma_ulps(sigma, q64[:, 0] / W)} ulp of sqrt(q / W)")


@pytest.mark.parametrize("B,arms", [(1, 1), (13, 5), (37, 5)])
@pytest.mark.parametrize("masked", [False, True])
def test_best_arm_is_the_masked_argmax_of_the_kernels_ucb(backend, B, arms, masked):
    """N = 1, 65 and 5 * 37 rows as B rows of `arms` arms: best_arm equals torch.argmax of the kernel's own ucb under the
    mask.  Rows 0 and 2 carry a planted exact tie at their maximum (two arms with the same large features: the lower index
    wins); with a mask, row 1 has no arm present and gets arm 0."""
    dev, d = backend.device, 33
    x, c, M, sw = _score_inputs(B * arms, d, dev, seed=3)
    x = x.view(B, arms, d)
    if arms > 2:
        for b in (0, 2):
            x[b, 3] = x[b, 1] = 4.0 * c / c.norm()
    presence = None
    if masked:
        g = torch.Generator().manual_seed(B)
        presence = (torch.rand(B, arms, generator=g) < 0.6).to(dev)
        if arms > 2:
            presence[0, 1] = presence[0, 3] = True
            presence[2, 1] = False  # the tie's lower arm is absent: the higher one is the answer
            presence[2, 3] = True
            presence[1] = False
    out, _, best = _score(x.reshape(B * arms, d).contiguous(), c, M, sw, 1.5, arms=arms,
                          presence=None if presence is None else presence.reshape(-1))
    ucb = out[2].view(B, arms)
    if arms > 2:
        assert ucb[0, 1] == ucb[0, 3] and ucb[0, 1] == ucb[0].max()
    want = (ucb if presence is None else torch.where(presence, ucb, torch.full_like(ucb, float("-inf")))).argmax(1)
    assert torch.equal(best, want)
    if arms > 2:
        assert best[0].item() == 1 and best[2].item() == (3 if masked else 1)
        if masked:
            assert best[1].item() == 0
    from reagent_amd.training.cb import get_model_actions

    assert torch.equal(get_model_actions(ucb, presence), want.view(-1, 1))


def _integer_batch(B, d, seed):
    """x [B, d], y [B] integers in [-3, 3], w [B] in {1, 2, 4}: every product and partial sum of the Gram sums is an integer
    far below 2^24 (at most 36 B), so the fp32 sums are exact in any order"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, d), generator=g).float()
    y = torch.randint(-3, 4, (B,), generator=g).float()
    w = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (B,), generator=g)]
    assert 36 * B < 2 ** 24
    return x, y, w


@pytest.mark.parametrize("B,d", [(65, 33), (300, 257), (600, 33)])
def test_accumulate_of_integer_inputs_is_exact(backend, B, d):
    """From an all-zero state (cur_sum_weight included) cur_avg_A is fp32(S) / fp32(s_w), ONE division, bit for bit, where S
    and s_w are the float64 sums (exact integers): the rule the joint / disjoint twin test relies on, held against the
    statement itself.  (600, 33) is three slices.  At (65, 33) the rows also come as [B, A, d] + action."""
    dev = backend.device
    x, y, w = _integer_batch(B, d, 3 * B + d)
    x64, y64, w64 = x.double(), y.double(), w.double()
    S, Sb, s_w = x64.t() @ (x64 * w64[:, None]), x64.t() @ (w64 * y64), w64.sum()
    want_A, want_b = S.float() / s_w.float(), Sb.float() / s_w.float()
    assert torch.equal(S.float().double(), S) and S.abs().max().item() > 0
    state = _fresh(d, dev, 0.0)
    _accumulate(state, x.to(dev), y.to(dev), w.to(dev))
    assert torch.equal(state[0].cpu(), want_A) and torch.equal(state[1].cpu(), want_b)
    assert state[2].item() == s_w.item() and state[3].item() == B
    if B == 65:
        A = 3
        g = torch.Generator().manual_seed(B)
        x3 = torch.randint(-3, 4, (B, A, d), generator=g).float()
        action = torch.randint(0, A, (B,), generator=g)
        x3[torch.arange(B), action] = x
        arms = _fresh(d, dev, 0.0)
        _accumulate(arms, x3.to(dev), y.to(dev), w.to(dev), action=action.to(dev))
        assert torch.equal(arms[0].cpu(), want_A) and torch.equal(arms[1].cpu(), want_b) and arms[3].item() == B


def test_accumulate_at_the_cap_on_slices(backend):
    """(B, d) = (1800, 512): 136 tiles, so cb_plan's cap is 1024 / 136 = 7 slices where the rows alone would ask for 8 (the
    workspace size says which plan ran: it is a function of the slice count), and the largest dimension.  Held to
    test_accumulate_against_float64's bound, bitwise symmetry, the counters and a bit-identical rerun."""
    import reagent_amd._lib as L

    dev = backend.device
    B, d = 1800, 512
    tiles_1d, tiles, slices = 16, 136, 7
    assert L.lib().rg_linucb_workspace_bytes(B, d) == 4 * (slices * tiles * 1024 + slices * tiles_1d * 32 + slices + 1)
    x, y, w = _batch(B, d, True, 5, dev)
    state = _fresh(d, dev)
    twin = [t.clone() for t in state]
    want, _, abs_sums = _statement(state, x, y, w)
    _accumulate(state, x, y, w)
    _check_update(state, want, abs_sums, B, (B, d))
    got, ref = state[0].cpu().double(), want[0]
    bound = (B + 2) * U * abs_sums[0] / want[2] + 8 * U * ref.abs()
    print(f"linucb_accumulate B={B} d={d}: cur_avg_A {((got - ref).abs() / bound).max().item():.4f} of its bound")
    assert torch.equal(state[0], state[0].t()) and state[3].item() == B
    _accumulate(twin, x, y, w)
    assert all(torch.equal(a, b) for a, b in zip(state, twin))


def test_select_kernel_beyond_one_workgroup_and_one_pass_of_the_count(backend):
    """d = 2, two arms, N = 16 600 rows: 519 per-workgroup NaN counts (more than the 256 threads that add them: a second
    pass of the count loop) and 8300 batch rows (33 workgroups of the select kernel).  With -I as the matrix every row
    counts and best_arm is torch.argmax of the kernel's own (all-NaN) ucb; with a positive-definite matrix and a random
    presence mask it is the masked arg-max."""
    from reagent_amd import ops

    dev, d, arms, N = backend.device, 2, 2, 16600
    B = N // arms
    assert ops.linucb_score_partials(N) == 519
    x, c, M, sw = _score_inputs(N, d, dev)
    out, nan_count, best = _score(x, c, -torch.eye(d, device=dev), sw, 1.5, arms=arms)
    assert nan_count == N and torch.isnan(out[2]).all()
    assert torch.equal(best, out[2].view(B, arms).argmax(1))
    presence = (torch.rand(B, arms, generator=torch.Generator().manual_seed(1)) < 0.6).to(dev)
    out, nan_count, best = _score(x, c, M, sw, 1.5, arms=arms, presence=presence.reshape(-1))
    ucb = out[2].view(B, arms)
    assert nan_count == 0
    want = torch.where(presence, ucb, torch.full_like(ucb, float("-inf"))).argmax(1)
    assert torch.equal(best, want)
    assert 0 < want.sum().item() < B and (want[32 * 256:] == 1).any()  # both arms win, in the last workgroup's rows too


def _argmax_fixture(arms):
    """tests/golden/cb/argmax_nonfinite.npz (tests/golden_gen/make_cb_argmax_golden.py): the unmodified reference's
    get_model_actions on rows with NaN and +-inf among present and absent arms -> scores, mask, its answers under the mask
    and without one"""
    import numpy as np

    from golden_util import GOLDEN

    with np.load(os.path.join(GOLDEN, "cb", "argmax_nonfinite.npz")) as z:
        return tuple(torch.from_numpy(z[f"a{arms}_{k}"]) for k in ("scores", "mask", "actions_masked", "actions_plain"))


@pytest.mark.parametrize("arms", [3, 5])
def test_get_model_actions_on_non_finite_scores_is_the_references(backend, arms):
    """every row of the fixture, in one call and (the named rows) alone: the first present NaN wins, a present -inf is
    worth what an absent arm is, arm 0 where nothing beats -inf"""
    from reagent_amd.training.cb import get_model_actions

    dev = backend.device
    scores, mask, masked, plain = _argmax_fixture(arms)
    assert scores.shape[0] >= 9 and torch.isnan(scores).any() and torch.isinf(scores).any()
    assert torch.equal(get_model_actions(scores.to(dev), mask.to(dev)).cpu(), masked)
    assert torch.equal(get_model_actions(scores.to(dev)).cpu(), plain)
    for r in range(9):
        assert torch.equal(get_model_actions(scores[r:r + 1].to(dev), mask[r:r + 1].to(dev)).cpu(), masked[r:r + 1]), r
    if arms == 3:  # the rows that set the rule: all present arms -inf -> arm 0, not the first present arm
        assert scores[0].tolist() == [float("-inf")] * 3 and mask[0].tolist() == [False, True, True] and masked[0].item() == 0


def test_policy_evaluator_accepts_by_the_references_arm_on_non_finite_scores(backend):
    """the evaluator compares the model's arm with the logged one.  The fixture's row 0 (every score -inf, mask [0, 1, 1]) has
    the reference's arm 0, so a logged arm 1 is REJECTED there (the first present arm is not the answer); row 18 (finite
    scores, all arms present, arm 1) with the same logged arm is accepted."""
    from reagent_amd.core.types import CBInput
    from reagent_amd.evaluation.cb.policy_evaluator import PolicyEvaluator
    from reagent_amd.training.cb import get_model_actions

    dev = backend.device
    scores, mask, masked, _ = _argmax_fixture(3)
    rows = [0, 18]
    assert masked[rows].reshape(-1).tolist() == [0, 1] and mask[0].tolist() == [False, True, True] and mask[18].all()
    assert torch.isinf(scores[0]).all() and torch.isfinite(scores[18]).all()
    scores, mask = scores[rows].to(dev), mask[rows].to(dev)
    batch = CBInput(context_arm_features=torch.zeros(2, 3, 2, device=dev), action=torch.tensor([[1], [1]], device=dev),
                    reward=torch.tensor([[5.0], [7.0]], device=dev), arm_presence=mask)
    ev = PolicyEvaluator(torch.nn.Linear(1, 1)).to(dev)
    new = ev.ingest_batch(batch, get_model_actions(scores, mask))
    assert new.importance_weight.cpu().reshape(-1).tolist() == [0.0, 3.0]  # rejected; three arms present: 1 / (1 / 3)
    assert ev.sum_weight_accepted_local.item() == 1.0 and ev.sum_reward_weighted_accepted_local.item() == 7.0
    assert ev.sum_weight_all_data_local.item() == 2.0 and ev.sum_reward_weighted_all_data_local.item() == 12.0


def test_negative_definite_matrix_counts_every_row_and_forward_raises(backend):
    dev, N, d = backend.device, 65, 33
    x, c, _, sw = _score_inputs(N, d, dev)
    out, nan_count, _ = _score(x, c, -torch.eye(d, device=dev), sw, 1.5)
    assert nan_count == N and torch.isnan(out[1]).all()
    from reagent_amd.models.linear_regression import LinearRegressionUCB

    m = LinearRegressionUCB(d).to(dev)
    m.inv_avg_A.copy_(-torch.eye(d))
    m.sum_weight.fill_(1.0)
    m._coefs_dirty = False
    with pytest.raises(Exception, match="pred_sigma has nan values"):
        m(x)
    with pytest.raises(Exception, match="pred_sigma has nan values"):
        m.forward_inference(x)
    assert set(m(x, ucb_alpha=0.0)) == {"pred_label", "pred_sigma", "ucb"}  # the mean alone never reads the matrix


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cb_kernels_have_no_scratch(tmp_path):
    """cb.hip compiled for gfx950 with the resource remarks on: its four kernels, no scratch, no spilled register"""
    kernels = kernel_resources("cb.hip", tmp_path)
    for want in ("linucb_gram_kernel", "linucb_finish_kernel", "linucb_score_kernel", "linucb_select_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, list(kernels))
    assert len(kernels) == 4
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
