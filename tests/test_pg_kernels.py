"""The policy-gradient step's kernels: rg_pg_returns and rg_pg_head (reagent_amd/csrc/pg.hip).

The reward-to-go without whitening is held to the BITS of the reference's discounted_returns (training/utils.py:42-54,
restated below with the same 0-dim torch operations) on clamp(reward, max = reward_clip): alone, packed, in two orders and
around an empty trajectory.  Whitening and mean subtraction are held to the reference's lines (utils.py:32-39,
reinforce_trainer.py:113-116) evaluated in float64 on the same fp32 returns; the head to the reference's lines
(discrete_sampler.py:45-79, reinforce_trainer.py:105-132, ppo_trainer.py:127-152) restated in float64 under autograd.
Every such bound is self-calibrating: the larger of 4 x the error of the SAME lines in torch fp32 against the float64
statement on those inputs (4: another, equally valid, order of reduction), and 4 ulp (fp32) of the quantity's largest
magnitude.  Inputs keep 1e-3 away from the clip boundaries, as the trainer fixtures do."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reagent_amd._lib as L
from reagent_amd import ops

EPS = float(np.finfo(float).eps)
LENGTHS = [1, 2, 63, 64, 65, 130, 257]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bound(ref64, torch32):
    """4 x the fp32 torch restatement's own largest error, floored at 4 ulp of the largest magnitude"""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    own = (torch.as_tensor(torch32).double() - ref64).abs().max().item()
    return max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item())), own


def _close(got, ref64, torch32, what):
    bound, own = _bound(ref64, torch32)
    err = (torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(ref64, dtype=torch.float64)).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound, own)


# ---- rg_pg_returns --------------------------------------------------------------------------------------------
def _discounted_returns(rewards, gamma):
    """training/utils.py:42-54 with its own operations: one 0-dim fp32 multiply and add per step, from the end"""
    if gamma == 0:
        return rewards.float()
    out = torch.empty_like(rewards, dtype=torch.float)
    run = torch.zeros((), dtype=torch.float)
    for t in range(rewards.shape[0] - 1, -1, -1):
        run = rewards[t].float() + gamma * run
        out[t] = run
    return out


def _trajectories(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in LENGTHS]


_REF = {}


def _reference_returns(gamma, clip):
    """the reference's returns of the seven trajectories (computed once per (gamma, clip) and left unchanged)"""
    key = (gamma, clip)
    if key not in _REF:
        rewards = _trajectories(11)
        _REF[key] = (rewards, [_discounted_returns(torch.clamp(r, max=clip).clone(), gamma) for r in rewards])
    return _REF[key]


def _run_returns(dev, trajs, gamma, clip, normalize=False, subtract_mean=False, clamp_min=False, extra=0, pad=0):
    """-> (out [N + extra + pad] on the host, offsets list); `extra` reward rows after offsets[T], `pad` NaNs after the output"""
    lens = [len(t) for t in trajs]
    offsets = [0] + list(itertools.accumulate(lens))
    reward = torch.cat(list(trajs) + [torch.full((extra,), 7.0)])
    out = torch.full((reward.numel() + pad,), float("nan")).to(dev)
    ops.pg_returns(reward.to(dev), torch.tensor(offsets, dtype=torch.int32).to(dev), gamma, clip, normalize, subtract_mean,
                   clamp_min, out)
    return out.cpu(), offsets


@pytest.mark.parametrize("clip", [1e6, 0.8])
@pytest.mark.parametrize("gamma", [0.0, 0.37, 0.9, 1.0])
def test_returns_have_the_reference_bits(backend, gamma, clip):
    dev = backend.device
    rewards, want = _reference_returns(gamma, clip)
    assert clip > 1 or all((r > clip).any() for r in rewards[2:])
    for r, w in zip(rewards, want):  # alone
        out, _ = _run_returns(dev, [r], gamma, clip)
        assert torch.equal(_bits(out), _bits(w)), len(r)
    empty = torch.empty(0)
    orders = [list(range(7)), [6, 0, 4, 2, 5, 1, 3]]
    for order in orders:  # packed, then around an empty trajectory, with rows after offsets[T] and a pad after the output
        for with_empty in (False, True):
            trajs = [rewards[i] for i in order]
            refs = [want[i] for i in order]
            if with_empty:
                trajs, refs = trajs[:3] + [empty] + trajs[3:], refs[:3] + [empty] + refs[3:]
            out, offsets = _run_returns(dev, trajs, gamma, clip, extra=5, pad=9)
            assert torch.equal(_bits(out[:offsets[-1]]), _bits(torch.cat(refs)))
            assert torch.isnan(out[offsets[-1]:]).all() and out.numel() == offsets[-1] + 14


def _whiten_lines(x, normalize, subtract_mean, clamp_min):
    """utils.py:32-39, reinforce_trainer.py:109-116 in x's dtype"""
    if normalize:
        std = x.std(unbiased=False)
        numer = x - x.mean() if subtract_mean else x
        x = numer / (std + EPS)
    elif subtract_mean:
        x = x - x.mean()
    if clamp_min:
        x = x.clamp(min=0)
    return x


@pytest.mark.parametrize("clamp_min", [False, True])
@pytest.mark.parametrize("normalize,subtract_mean", [(True, True), (True, False), (False, True)])
def test_whitening_and_mean_subtraction_against_float64(backend, normalize, subtract_mean, clamp_min):
    gamma, clip = 0.9, 1e6
    rewards, returns = _reference_returns(gamma, clip)
    order = [6, 1, 4, 2, 5, 3]  # lengths 257, 2, 65, 63, 130, 64: every whitened trajectory has length >= 2
    out, offsets = _run_returns(backend.device, [rewards[i] for i in order], gamma, clip, normalize, subtract_mean, clamp_min,
                                pad=3)
    assert torch.isnan(out[offsets[-1]:]).all()
    got = out[:offsets[-1]]
    ref64 = torch.cat([_whiten_lines(returns[i].double(), normalize, subtract_mean, clamp_min) for i in order])
    ref32 = torch.cat([_whiten_lines(returns[i].clone(), normalize, subtract_mean, clamp_min) for i in order])
    assert 1.0 < ref64.abs().max() < 16.0
    _close(got, ref64, ref32, f"returns normalize={normalize} subtract_mean={subtract_mean} clamp_min={clamp_min}")
    if clamp_min:
        assert (got >= 0).all() and (got == 0).any() and (got > 0).any()
    else:
        assert (got < 0).any()


@pytest.mark.parametrize("normalize", [False, True])
def test_single_step_and_constant_trajectories_centre_to_exact_zero(backend, normalize):
    trajs = [torch.tensor([0.731]), torch.full((70,), 0.3), torch.tensor([-2.5]), torch.full((2,), -1.7)]
    for clamp_min in (False, True):
        out, offsets = _run_returns(backend.device, trajs, 0.0, 1e6, normalize, True, clamp_min)
        assert offsets[-1] == 74 and (out == 0).all()
    # discounted: a constant RETURN needs gamma = 0; with gamma = 0.5 the single steps still centre to exactly 0
    out, offsets = _run_returns(backend.device, trajs, 0.5, 1e6, normalize, True, False)
    assert out[0] == 0 and out[71] == 0 and (out[1:71] != 0).any()


def test_returns_are_deterministic_and_reject_bad_arguments(backend):
    dev = backend.device
    rewards, _ = _reference_returns(0.9, 1e6)
    a, _ = _run_returns(dev, rewards, 0.9, 0.8, True, True, False)
    b, _ = _run_returns(dev, rewards, 0.9, 0.8, True, True, False)
    assert torch.equal(_bits(a), _bits(b))
    lib = L.lib()
    r, o = torch.ones(8).to(dev), torch.full((8,), float("nan")).to(dev)
    off = torch.tensor([0, 8], dtype=torch.int32).to(dev)
    s = L.stream_ptr()
    call = lambda T=1, n=8, offsets=off, reward=r, out=o: lib.rg_pg_returns(  # noqa: E731
        L.ptr(reward), L.ptr(offsets), T, n, 0.9, 1e6, 0, 0, 0, L.ptr(out), s)
    for bad in (dict(T=0), dict(T=-1), dict(n=-1), dict(offsets=None), dict(reward=None), dict(out=None)):
        assert call(**bad) == -1, bad
    assert torch.isnan(o.cpu()).all()  # nothing was launched
    assert call(n=0) == 0 and torch.isnan(o.cpu()).all()
    assert call() == 0 and not torch.isnan(o.cpu()).any()


# ---- rg_pg_head -----------------------------------------------------------------------------------------------
MODES = [L.PG_REINFORCE, L.PG_REINFORCE_OFF_POLICY, L.PG_PPO]
CLIP = {L.PG_REINFORCE: 1e6, L.PG_REINFORCE_OFF_POLICY: 2.0, L.PG_PPO: 0.2}
NS, AS = [1, 5, 67, 300], [2, 3, 4, 5, 16, 17, 64, 65, 200, 256]
GRID = list(itertools.product(NS, AS))


def _options(k):
    """the k-th combination of the head's options (k counts (N, A, mode) triples)"""
    return dict(values=k % 2 == 0, entropy=0.01 if (k // 2) % 2 else 0.0, temperature=[0.5, 1.0, 2.0][(k // 4) % 3],
                int64=(k // 3) % 2 == 1, masked=(k // 5) % 2 == 0, layout=["dense", "pitch", "base"][(k // 7) % 3])


_ALL = [dict(_options(3 * i + m), mode=m) for i in range(len(GRID)) for m in range(3)]
for _m in range(3):  # every option value occurs with every mode
    _mine = [o for o in _ALL if o["mode"] == _m]
    assert {o["values"] for o in _mine} == {False, True} and {o["entropy"] for o in _mine} == {0.0, 0.01}
    assert {o["temperature"] for o in _mine} == {0.5, 1.0, 2.0} and {o["int64"] for o in _mine} == {False, True}
    assert {o["masked"] for o in _mine} == {False, True} and {o["layout"] for o in _mine} == {"dense", "pitch", "base"}


def _keep_away(d, boundaries, margin=0.02, jump=0.05):
    for b in boundaries:
        d = torch.where((d - b).abs() < margin, torch.full_like(d, b + jump), d)
    return d


def _head_inputs(N, A, mode, seed, masked, int64, temperature):
    """scores with the mask's -1e10 already added (never on the logged action, at least two allowed actions per row); row 0
    of the one-hot has a second 1 at a HIGHER index; the logged log-probability is placed by the float64 log-probability so
    that d = l - old spreads over both sides of the clip and keeps 0.02 away from its boundaries"""
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(N, A, generator=g) * 2.0
    a = torch.randint(A, (N,), generator=g)
    a[0] = min(a[0].item(), A - 2)
    rows = torch.arange(N)
    if masked:
        allowed = torch.rand(N, A, generator=g) > 0.4
        allowed[rows, a], allowed[rows, (a + 1) % A] = True, True
        allowed[0, A - 1] = True
        scores = scores + (1 - allowed.float()) * -1e10
    onehot = F.one_hot(a, A)
    onehot[0, A - 1] = 1  # two-hot: argmax takes the first
    assert int(onehot[0].argmax()) == a[0] and onehot[0].sum() == 2
    returns = torch.randn(N, generator=g) * 2.0
    values = torch.randn(N, generator=g)
    l64 = torch.log_softmax(scores.double() / temperature, dim=1)[rows, a]
    clip = CLIP[mode]
    if mode == L.PG_REINFORCE_OFF_POLICY:
        d = _keep_away((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * 1.5, [math.log(clip)])
    else:
        d = _keep_away((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * 0.5, [math.log(1 - 0.2), math.log(1 + 0.2)])
    old = (l64 - d).float()
    d = l64 - old.double()
    if mode == L.PG_REINFORCE_OFF_POLICY:
        assert ((d - math.log(clip)).abs() >= 1e-3).all()
    if mode == L.PG_PPO:
        rho = torch.exp(d)
        assert ((rho - (1 - clip)).abs() >= 1e-3).all() and ((rho - (1 + clip)).abs() >= 1e-3).all()
    return dict(scores=scores, action=onehot if int64 else onehot.float(), a=a, returns=returns, values=values, old=old)


def _head_lines(i, mode, temperature, clip, w, value_scale, with_values, dtype):
    """the reference's lines in `dtype` under autograd -> log_prob, ratio, advantage, dscores, dvalues, the two loss sums"""
    s = i["scores"].to(dtype).clone().requires_grad_(True)
    m = torch.distributions.Categorical(logits=s / temperature)
    l = m.log_prob(i["action"].argmax(dim=1))
    ret, old = i["returns"].to(dtype), i["old"].to(dtype)
    v = i["values"].to(dtype).clone().requires_grad_(True)
    adv = (ret - v).detach() if with_values else ret
    ratio = torch.ones_like(l)
    if mode == L.PG_REINFORCE:
        rows = -(adv * l)
    elif mode == L.PG_REINFORCE_OFF_POLICY:
        ratio = torch.exp(torch.clamp(l - old, max=math.log(float(clip))))
        rows = -(adv * ratio)
    else:
        ratio = torch.exp(l - old)
        rows = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip))
    loss = rows.sum()
    if w != 0:
        loss = loss - w * (m.entropy().mean() * s.shape[0])
    loss.backward()
    out = dict(log_prob=l.detach(), ratio=ratio.detach(), advantage=adv.detach(), dscores=s.grad, policy_loss=loss.detach())
    if with_values:
        vloss = value_scale * ((v - ret) ** 2).sum()
        vloss.backward()
        out.update(dvalues=v.grad, value_loss=vloss.detach())
    return out


def _strided(dev, N, A, layout, fill=None):
    """an [N, A] device view: dense, with an odd row pitch, or with a base 4 bytes off (both force the scalar path)"""
    pad, off = (1 if A % 2 == 0 else 2, 0) if layout == "pitch" else ((0, 1) if layout == "base" else (0, 0))
    flat = torch.full((N * (A + pad) + off,), float("nan"))
    view = flat[off:].view(N, A + pad)
    if fill is not None:
        view[:, :A] = fill
    flat = flat.to(dev)
    return flat, flat[off:].view(N, A + pad)[:, :A], (flat[off:].view(N, A + pad)[:, A:] if pad else None)


def _run_head(dev, i, mode, temperature, clip, w, value_scale, with_values, layout="dense", mask=None, scores=None):
    N, A = i["scores"].shape
    f = lambda *s: torch.full(s, float("nan")).to(dev)  # noqa: E731
    _, sc, _ = _strided(dev, N, A, layout, i["scores"] if scores is None else scores)
    _, dsc, dpad = _strided(dev, N, A, layout)
    P = ops.pg_head_partials(N, A)
    assert P == -(-N // (256 // (1 if A <= 4 else 4 if A <= 16 else 16 if A <= 64 else 64)))
    o = dict(dvalues=f(N), log_prob=f(N), ratio=f(N), advantage=f(N), pp=f(P), vp=f(P), policy_loss=f(1), value_loss=f(1))
    ops.pg_head(sc, i["action"].to(dev), i["returns"].to(dev), i["values"].to(dev) if with_values else None,
                None if mode == L.PG_REINFORCE else i["old"].to(dev), temperature, mode, clip, w, value_scale, dsc,
                o["dvalues"] if with_values else None, o["log_prob"], o["ratio"], o["advantage"], o["pp"],
                o["vp"] if with_values else None, possible_actions_mask=None if mask is None else mask.to(dev))
    ops.reduce_sum(o["pp"], P, 1.0, o["policy_loss"])
    if with_values:
        ops.reduce_sum(o["vp"], P, 1.0, o["value_loss"])
    if dpad is not None:
        assert torch.isnan(dpad.cpu()).all()  # the padding of every output row is untouched
    out = {k: v.cpu() for k, v in o.items()}
    out["dscores"] = dsc.cpu().contiguous()
    if not with_values:
        assert torch.isnan(out["dvalues"]).all() and torch.isnan(out["vp"]).all()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,A", GRID)
def test_head_against_the_float64_statement(backend, N, A, mode):
    k = 3 * GRID.index((N, A)) + mode
    o = _options(k)
    temp, w, with_values, clip = o["temperature"], o["entropy"], o["values"], CLIP[mode]
    value_scale = 1.0 if mode == L.PG_PPO else 1.0 / N
    i = _head_inputs(N, A, mode, 100 + k, o["masked"], o["int64"], temp)
    ref64 = _head_lines(i, mode, temp, clip, w, value_scale, with_values, torch.float64)
    ref32 = _head_lines(i, mode, temp, clip, w, value_scale, with_values, torch.float32)
    got = _run_head(backend.device, i, mode, temp, clip, w, value_scale, with_values, o["layout"])
    for key in ref64:
        _close(got[key], ref64[key], ref32[key], f"N={N} A={A} mode={mode} {o} {key}")
    if o["masked"] and w == 0:
        off = i["scores"] <= -1e9
        assert off.any() or A == 2 or N * A < 64  # (two actions: both stay allowed)
        assert (got["dscores"][off] == 0).all()  # exactly 0 on masked actions


def test_head_takes_the_first_maximum_of_a_two_hot_row(backend):
    """the logged action of a row with two 1s is the LOWER index, in fp32 and int64 and across the lanes of a group"""
    N, A = 6, 70
    i = _head_inputs(N, A, L.PG_REINFORCE, 3, False, False, 1.0)
    hot = torch.zeros(N, A)
    pairs = [(0, 69), (3, 4), (5, 64), (63, 64), (17, 18), (68, 69)]
    for r, (lo, hi) in enumerate(pairs):
        hot[r, lo], hot[r, hi] = 1.0, 1.0
    want = torch.log_softmax(i["scores"].double(), dim=1)[torch.arange(N), torch.tensor([p[0] for p in pairs])]
    for action in (hot, hot.long()):
        i["action"] = action
        got = _run_head(backend.device, i, L.PG_REINFORCE, 1.0, 1e6, 0.0, 1.0, False)
        assert (got["log_prob"].double() - want).abs().max() <= 4 * _ulp(want.abs().max())


def test_head_adds_the_possible_actions_mask_as_the_scorer_does(backend):
    """possible_actions_mask handed to the kernel gives the bits of scores that already carry (1 - mask) * -1e10"""
    N, A = 67, 17
    g = torch.Generator().manual_seed(5)
    i = _head_inputs(N, A, L.PG_PPO, 9, False, False, 0.7)
    allowed = torch.rand(N, A, generator=g) > 0.4
    allowed[torch.arange(N), i["a"]] = True
    allowed[torch.arange(N), (i["a"] + 1) % A] = True
    allowed[0, A - 1] = True
    raw = i["scores"]
    pre = raw + (1 - allowed.float()) * -1e10
    a = _run_head(backend.device, i, L.PG_PPO, 0.7, 0.2, 0.01, 1.0, True, scores=pre)
    b = _run_head(backend.device, i, L.PG_PPO, 0.7, 0.2, 0.01, 1.0, True, scores=raw, mask=allowed.float())
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_head_is_deterministic(backend):
    i = _head_inputs(300, 65, L.PG_PPO, 1, True, False, 0.5)
    a = _run_head(backend.device, i, L.PG_PPO, 0.5, 0.2, 0.01, 1.0, True)
    b = _run_head(backend.device, i, L.PG_PPO, 0.5, 0.2, 0.01, 1.0, True)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_head_rejects_bad_arguments(backend):
    dev = backend.device
    lib = L.lib()
    z = torch.zeros(64).to(dev)
    out = torch.full((64,), float("nan")).to(dev)
    p, q, s = z.data_ptr(), out.data_ptr(), L.stream_ptr()

    def head(**k):
        A = k.get("A", 4)
        return lib.rg_pg_head(k.get("scores", p), k.get("lds", A), None, k.get("action", p), 0, k.get("lda", A),
                              k.get("returns", p), k.get("values", None), k.get("old", p), k.get("temp", 1.0),
                              k.get("mode", L.PG_PPO), k.get("clip", 0.2), 0.0, 1.0, k.get("n", 2), A, k.get("dscores", q),
                              k.get("ldd", A), k.get("dvalues", None), None, None, None, k.get("pp", q), k.get("vp", None), s)

    for bad in (dict(scores=None), dict(action=None), dict(returns=None), dict(dscores=None), dict(pp=None), dict(n=0),
                dict(n=-3), dict(A=0), dict(A=L.PG_MAX_ACTIONS + 1, n=1), dict(mode=3), dict(mode=-1), dict(old=None),
                dict(old=None, mode=L.PG_REINFORCE_OFF_POLICY, clip=2.0), dict(temp=0.0), dict(temp=-1.0), dict(lds=3),
                dict(lda=3), dict(ldd=3), dict(mode=L.PG_REINFORCE_OFF_POLICY, clip=0.0), dict(clip=1.5),
                dict(values=p), dict(values=p, dvalues=q)):
        assert head(**bad) == -1, bad
    assert torch.isnan(out.cpu()).all()  # nothing was launched
    assert L.PG_MAX_ACTIONS == 256 and ops.pg_head_partials(1, 257) == 0
    assert head() == 0 and head(old=None, mode=L.PG_REINFORCE) == 0 and head(values=p, dvalues=q, vp=q) == 0
    assert not torch.isnan(out.cpu()[:8]).any()
