"""The Bayes-by-backprop kernels (reagent_amd/csrc/bbb.hip: rg_bbb_sample, rg_bbb_fill_noise, rg_bbb_elbo_head, rg_bbb_grad)
against the reference's lines (reagent/models/probabilistic_fully_connected_network.py:87-105, :190-213) restated in float64
under autograd, with the same fp32 w on both sides.  The bound is the self-calibrating one of tests/test_lstm_kernels.py: the
larger of 4 x torch's own fp32 error against float64 on the same inputs and 4 ulp of the largest magnitude."""
import numpy as np
import pytest
import torch
from torch.distributions import Normal

from reagent_amd import ops

F32, F64 = torch.float32, torch.float64
SETS = {"3-1": [3, 1], "33-65-34-1": [2145, 65, 2210, 34, 34, 1], "70001": [70001]}


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _bound(ref64, torch32):
    ref64 = ref64.detach().double()
    own = (torch32.detach().double() - ref64).abs().max().item()
    return max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item())), own


def _close(got, ref64, torch32, what):
    bound, own = _bound(ref64, torch32)
    err = (got.detach().cpu().double() - ref64.detach().double()).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (what, err, bound, own)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(sizes, seed, rho_shift=0.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda n, s=1.0: s * torch.randn(n, generator=g)  # noqa: E731
    return dict(mu=[r(n, 0.5) for n in sizes], rho=[r(n) + rho_shift for n in sizes], eps=[r(n) for n in sizes],
                dw=[r(n, 0.3) for n in sizes])


class _Run:
    """one segment table on the device and its buffers"""

    def __init__(self, d, dev, grads=True):
        self.dev = dev
        t = lambda xs: [x.clone().to(dev) for x in xs]  # noqa: E731
        self.mu, self.rho, self.eps, self.dw = t(d["mu"]), t(d["rho"]), t(d["eps"]), t(d["dw"])
        self.w = [torch.full_like(x, float("nan")) for x in self.mu]
        self.dmu = [torch.full_like(x, float("nan")) for x in self.mu]
        self.drho = [torch.full_like(x, float("nan")) for x in self.mu]
        segs = [dict(mu=self.mu[i], rho=self.rho[i], w=self.w[i], eps=self.eps[i], dw=self.dw[i], dmu=self.dmu[i], drho=self.drho[i])
                for i in range(len(self.mu))]
        self.table = ops.bbb_table(segs)
        f = dict(dtype=F32, device=dev)
        self.log_prior, self.log_post = torch.empty(1, **f), torch.empty(1, **f)
        self.terms = torch.empty(2, dtype=F64, device=dev)
        self.ws = torch.full((2 * ops.bbb_chunks(self.table),), float("nan"), dtype=F64, device=dev)

    def sample(self, prior_var, seed=None, sample=0):
        ops.bbb_sample(self.table, prior_var, self.log_prior, self.log_post, self.terms, self.ws, seed=seed, sample=sample)


def _statement(dtype, d, w32, prior_var, detach=True, scale=1.0):
    """:87-105 on every segment -> (w, log_prior, log_post, d mu, d rho) of loss = log_post - log_prior + sum(dw * w): dw
    stands for the network's d (-log_like) / d w.  w32: the fp32 draw both sides agree on (None: the statement's own)"""
    mu = [m.detach().clone().to(dtype).requires_grad_() for m in d["mu"]]
    rho = [r.detach().clone().to(dtype).requires_grad_() for r in d["rho"]]
    ws, prior, post, extra = [], 0, 0, 0
    for i in range(len(mu)):
        sigma = torch.log(1 + torch.exp(rho[i]))
        w = mu[i] + sigma * d["eps"][i].to(dtype)
        ws.append(w.detach().clone())
        if w32 is not None:
            w = w + (w32[i].cpu().to(dtype) - w).detach()
        prior = prior + Normal(torch.zeros((), dtype=dtype), torch.tensor(prior_var, dtype=dtype)).log_prob(w).sum()
        post = post + Normal(mu[i].data if detach else mu[i], sigma).log_prob(w).sum()
        extra = extra + (d["dw"][i].to(dtype) * w).sum()
    (scale * (post - prior) + extra).backward()
    return ws, prior.detach(), post.detach(), [m.grad for m in mu], [r.grad for r in rho]


@pytest.mark.parametrize("name", list(SETS))
def test_sample_and_grad_against_the_float64_statement(backend, name):
    sizes, prior_var = SETS[name], 0.7
    d = _inputs(sizes, seed=len(sizes))
    run = _Run(d, backend.device)
    run.sample(prior_var)
    ops.bbb_grad(run.table, prior_var)
    w64, _, _, _, _ = _statement(F64, d, None, prior_var)
    w32t, _, _, _, _ = _statement(F32, d, None, prior_var)
    for i in range(len(sizes)):
        _close(run.w[i], w64[i], w32t[i], f"w[{i}]")
        assert torch.equal(_bits(run.eps[i]), _bits(d["eps"][i]))  # a given eps is read, not written
    _, prior64, post64, dmu64, drho64 = _statement(F64, d, run.w, prior_var)
    _, prior32, post32, dmu32, drho32 = _statement(F32, d, run.w, prior_var)
    _close(run.log_prior, prior64.view(1), prior32.view(1), "log_prior")
    _close(run.log_post, post64.view(1), post32.view(1), "log_post")
    assert run.terms[0].item() == pytest.approx(prior64.item(), rel=1e-10) and run.terms[1].item() == pytest.approx(post64.item(), rel=1e-10)
    for i in range(len(sizes)):
        _close(run.dmu[i], dmu64[i], dmu32[i], f"d mu[{i}]")
        _close(run.drho[i], drho64[i], drho32[i], f"d rho[{i}]")


def test_the_posterior_mean_is_detached(backend):
    """the .data quirk (:101-102): a restatement that does NOT detach the mean gives another d mu; the kernel matches the
    detached one, and the two differ by more than the bound, so the test cannot pass both"""
    sizes, prior_var = SETS["33-65-34-1"], 1.0
    d = _inputs(sizes, seed=3)
    run = _Run(d, backend.device)
    run.sample(prior_var)
    ops.bbb_grad(run.table, prior_var)
    _, _, _, kept64, _ = _statement(F64, d, run.w, prior_var, detach=True)
    _, _, _, kept32, _ = _statement(F32, d, run.w, prior_var, detach=True)
    _, _, _, free64, _ = _statement(F64, d, run.w, prior_var, detach=False)
    for i in range(len(sizes)):
        bound, _ = _bound(kept64[i], kept32[i])
        assert (free64[i] - kept64[i]).abs().max().item() > 100 * bound
        _close(run.dmu[i], kept64[i], kept32[i], f"d mu[{i}]")


def test_zero_noise_is_exact(backend):
    sizes, prior_var = SETS["33-65-34-1"], 1.0
    d = _inputs(sizes, seed=4)
    d["eps"] = [torch.zeros(n) for n in sizes]
    d["dw"] = [torch.zeros(n) for n in sizes]
    run = _Run(d, backend.device)
    run.sample(prior_var)
    ops.bbb_grad(run.table, prior_var)
    for i in range(len(sizes)):
        assert torch.equal(_bits(run.w[i]), _bits(d["mu"][i]))
        rho = d["rho"][i].double()
        want = -torch.sigmoid(rho) / torch.log1p(torch.exp(rho))
        rho32 = d["rho"][i]
        _close(run.drho[i], want, -torch.sigmoid(rho32) / torch.log(1 + torch.exp(rho32)), f"d rho[{i}]")
        # d mu = w / prior_var^2 alone: the posterior term vanishes at w = mu
        _close(run.dmu[i], d["mu"][i].double(), d["mu"][i], f"d mu[{i}]")


@pytest.mark.parametrize("name", ["33-65-34-1", "70001"])
def test_drawn_noise_equals_filled_noise_and_a_seed_is_a_run(backend, name):
    sizes, prior_var = SETS[name], 1.0
    d = _inputs(sizes, seed=5)
    drawn, again, other, filled = (_Run(d, backend.device) for _ in range(4))
    drawn.sample(prior_var, seed=1234, sample=2)
    again.sample(prior_var, seed=1234, sample=2)
    other.sample(prior_var, seed=1235, sample=2)
    ops.bbb_fill_noise(filled.table, 1234, 2)
    filled.sample(prior_var)  # the explicit-noise path on what the kernel would have drawn
    for i in range(len(sizes)):
        assert not torch.equal(_bits(drawn.eps[i]), _bits(d["eps"][i]))
        for r in (again, filled):
            assert torch.equal(_bits(drawn.eps[i]), _bits(r.eps[i])) and torch.equal(_bits(drawn.w[i]), _bits(r.w[i]))
    assert not torch.equal(_bits(drawn.eps[0]), _bits(other.eps[0]))
    for r in (again, filled):
        assert torch.equal(_bits(drawn.log_prior), _bits(r.log_prior)) and torch.equal(_bits(drawn.log_post), _bits(r.log_post))
    assert not torch.equal(_bits(drawn.log_post), _bits(other.log_post))
    next_sample = _Run(d, backend.device)
    ops.bbb_fill_noise(next_sample.table, 1234, 3)
    assert not torch.equal(_bits(drawn.eps[0]), _bits(next_sample.eps[0]))
    if len(sizes) > 4:  # two segments of one size draw different noise: the segment is part of the counter
        assert sizes[3] == sizes[4] and not torch.equal(_bits(drawn.eps[3]), _bits(drawn.eps[4]))


def test_drawn_noise_is_standard_normal(backend):
    """2^16 draws at a fixed seed: the bounds are what a correct Box-Muller meets at this seed (computed once on the
    interpreter: mean -0.000002, variance 0.99274, largest |value| 4.6684) with a margin; the draw is deterministic"""
    n = 1 << 16
    d = _inputs([n], seed=6)
    run = _Run(d, backend.device)
    ops.bbb_fill_noise(run.table, 20261020, 0)
    e = run.eps[0].cpu().double()
    mean, var, top = e.mean().item(), e.var().item(), e.abs().max().item()
    print(f"mean {mean:.5f} variance {var:.5f} largest {top:.4f}")
    assert abs(mean) < 0.012 and abs(var - 1.0) < 0.02 and 4.2 < top < 5.1
    assert abs((e ** 3).mean().item()) < 0.05 and abs((e ** 4).mean().item() - 3.0) < 0.15
    assert torch.isfinite(e).all()


def test_extreme_rho_stays_finite(backend):
    """the stated departure: rho = 100 and rho = -40 give a finite w, log_post and gradients (the reference's fp32 softplus
    is inf and 0 there)"""
    sizes, prior_var = [65, 3], 1.0
    d = _inputs(sizes, seed=7)
    d["rho"][0][:32], d["rho"][0][32:] = 100.0, -40.0
    d["eps"][0][40] = 0.0
    run = _Run(d, backend.device)
    run.sample(prior_var)
    ops.bbb_grad(run.table, prior_var)
    for t in run.w + run.dmu + run.drho + [run.log_prior, run.log_post]:
        assert torch.isfinite(t).all()
    w64 = d["mu"][0].double() + torch.cat([torch.full((32,), 100.0, dtype=F64), torch.full((33,), float(np.exp(-40.0)), dtype=F64)]) * d["eps"][0].double()
    assert (run.w[0].cpu().double() - w64).abs().max().item() <= 4 * _ulp(w64.abs().max().item())


@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_elbo_head_against_the_float64_statement(backend, B):
    dev, tol = backend.device, 0.3
    g = torch.Generator().manual_seed(B)
    out, target = torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
    terms = torch.tensor([-123.456789, -98.7654321], dtype=F64)
    wide = torch.full((B, 3), float("nan"))  # the output as a column of a wider buffer: the pitch
    wide[:, :1] = out
    res = {}
    for dtype in (F64, F32):
        o = out.detach().clone().to(dtype).requires_grad_()
        like = Normal(o.reshape(-1), tol).log_prob(target.to(dtype).reshape(-1)).sum()
        loss = terms[1].to(dtype) - terms[0].to(dtype) - like
        loss.backward()
        res[dtype] = (loss.detach().view(1), like.detach().view(1), o.grad)
    acc, result = torch.full((4,), float("nan"), dtype=F64, device=dev), torch.empty(4, device=dev)
    dout = torch.empty(B, 1, device=dev)
    ws = torch.empty(ops.bbb_elbo_head_partials(B), dtype=F64, device=dev)
    ops.bbb_elbo_head(wide.to(dev)[:, :1], target.to(dev).view(B), tol, terms.to(dev), acc, result, ws, dout=dout)
    _close(result[0:1], res[F64][0], res[F32][0], "loss")
    _close(result[3:4], res[F64][1], res[F32][1], "log_like")
    _close(dout, res[F64][2], res[F32][2], "d out")
    assert result[1].item() == np.float32(terms[0].item()) and result[2].item() == np.float32(terms[1].item())
    assert acc[0].item() == pytest.approx(res[F64][0].item(), rel=1e-10)
    again = torch.empty(4, device=dev)
    ops.bbb_elbo_head(out.to(dev), target.to(dev).view(B), tol, terms.to(dev), acc, again, ws)  # no dout, the pitch 1
    assert torch.equal(_bits(again), _bits(result))


def test_three_samples_against_the_float64_loop(backend):
    """sample_elbo's loop (:190-213) at num_samples = 3 with recorded draws on a [3, 1] linear net: the kernels with scale 1 / 3
    and accumulate against the float64 loop under autograd; the network's own d (-log_like) / d w is handed in"""
    dev, S, B, tol, pv = backend.device, 3, 5, 0.5, 0.8
    sizes = [3, 1]
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(B, 3, generator=g), torch.randn(B, generator=g)
    d = _inputs(sizes, seed=12)
    draws = [[torch.randn(n, generator=g) for n in sizes] for _ in range(S)]
    run = _Run(d, dev)
    acc, result = torch.empty(4, dtype=F64, device=dev), torch.empty(4, device=dev)
    ws, dout = torch.empty(ops.bbb_elbo_head_partials(B), dtype=F64, device=dev), torch.empty(B, device=dev)
    w32 = []
    for i in range(S):
        for e, new in zip(run.eps, draws[i]):
            e.copy_(new)
        run.sample(pv, sample=i)
        w32.append([w.cpu().clone() for w in run.w])
        out = (x.double() @ w32[i][0].double().view(3, 1) + w32[i][1].double()).float().to(dev)  # the FC GEMM's stand-in
        ops.bbb_elbo_head(out, y.to(dev), tol, run.terms, acc, result, ws, dout=dout, scale=1.0 / S, accumulate=i > 0)
        run.dw[0].copy_((dout.cpu().double() @ x.double()).float())
        run.dw[1].copy_(dout.cpu().double().sum().float().view(1))
        ops.bbb_grad(run.table, pv, scale=1.0 / S, accumulate=i > 0)
    res = {}
    for dtype in (F64, F32):
        mu = [m.detach().clone().to(dtype).requires_grad_() for m in d["mu"]]
        rho = [r.detach().clone().to(dtype).requires_grad_() for r in d["rho"]]
        priors, posts, likes = [], [], []
        for i in range(S):
            prior = post = 0
            ws_ = []
            for k in range(2):
                sigma = torch.log(1 + torch.exp(rho[k]))
                w = mu[k] + sigma * draws[i][k].to(dtype)
                w = w + (w32[i][k].to(dtype) - w).detach()
                prior = prior + Normal(torch.zeros((), dtype=dtype), torch.tensor(pv, dtype=dtype)).log_prob(w).sum()
                post = post + Normal(mu[k].data, sigma).log_prob(w).sum()
                ws_.append(w)
            o = x.to(dtype) @ ws_[0].view(3, 1) + ws_[1]
            priors.append(prior), posts.append(post)
            likes.append(Normal(o.reshape(-1), tol).log_prob(y.to(dtype)).sum())
        loss = torch.stack(posts).mean() - torch.stack(priors).mean() - torch.stack(likes).mean()
        loss.backward()
        res[dtype] = (loss.detach().view(1), [m.grad for m in mu], [r.grad for r in rho])
    _close(result[0:1], res[F64][0], res[F32][0], "loss of three samples")
    for k in range(2):
        _close(run.dmu[k], res[F64][1][k], res[F32][1][k], f"d mu[{k}]")
        _close(run.drho[k], res[F64][2][k], res[F32][2][k], f"d rho[{k}]")


def test_refused_tables(backend):
    d = _inputs([4] * 17, seed=1)
    with pytest.raises(NotImplementedError, match="17 segments"):
        _Run(d, backend.device)
    run = _Run(_inputs([4], seed=1), backend.device)
    with pytest.raises(Exception, match="invalid"):
        run.sample(0.0)
