"""The mixture-density head: rg_mdn_head and rg_mdn_gmm_nll (reagent_amd/csrc/mdn.hip).

The losses, d loss / d z, sigmas and logpi are held to the reference's lines (mdn_rnn.py:75-92, gmm_loss :188-233,
mdnrnn_trainer.py:164-177) restated in tests/mdnrnn_statement.py with the same torch operations, evaluated in float64 under autograd on the same
fp32 inputs.  Every bound is self-calibrating, as in tests/test_pg_kernels.py: the larger of 4 x the error of the same lines
in torch fp32 against the float64 statement and 4 ulp (fp32) of the quantity's largest magnitude."""
import pytest
import torch
import torch.nn.functional as F

import reagent_amd._lib as L
from reagent_amd import ops
from mdnrnn_statement import close as _close, gmm_lines as _gmm_lines, head_lines
from reagent_amd.models.mdn_rnn import gmm_loss

WEIGHTS = (0.5, 2.0, 0.25)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _lines(z, next_state, reward, not_terminal, G, dtype, weights=WEIGHTS, divide=True, first_row=0):
    return head_lines(z, next_state, reward, not_terminal, G, dtype, weights, divide, first_row)


def _inputs(N, G, S, seed=0):
    g = torch.Generator().manual_seed(seed + 7919 * N + 31 * G + S)
    z = torch.randn(N, (2 * S + 1) * G + 2, generator=g)
    z[:, G * S:2 * G * S] *= 0.5  # log sigma
    return z, torch.randn(N, S, generator=g), torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.7).float()


def _head(dev, z, next_state, reward, not_terminal, G, weights=WEIGHTS, divide=True, first_row=0, outputs=True, pad=0):
    N, S = next_state.shape
    f = dict(dtype=torch.float32, device=dev)
    dz = torch.full((N, z.shape[1] + pad), float("nan"), **f)
    sig = torch.full((N, G, S), float("nan"), **f) if outputs else None
    lpi = torch.full((N, G), float("nan"), **f) if outputs else None
    losses = torch.full((4,), float("nan"), **f)
    partials = torch.empty(3 * ops.mdn_head_partials(N), dtype=torch.float64, device=dev)
    ops.mdn_head(z.to(dev), next_state.to(dev), reward.to(dev), not_terminal.to(dev), G, weights, divide, first_row,
                 dz[:, :z.shape[1]], partials, losses, sig, lpi)
    if pad:
        assert torch.isnan(dz[:, z.shape[1]:]).all()
    return losses.cpu(), dz[:, :z.shape[1]].cpu(), None if sig is None else sig.cpu(), None if lpi is None else lpi.cpu()


def _check(dev, inp, G, what, **kw):
    r64, r32 = _lines(*inp, G, torch.float64, **kw), _lines(*inp, G, torch.float32, **kw)
    got = _head(dev, *inp, G, **kw)
    for name, g, a, b in zip(("losses", "dz", "sigmas", "logpi"), got, r64, r32):
        _close(g, a, b, f"{name} {what}")
    return got


_REF = {}


@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("S", [1, 6, 33])
@pytest.mark.parametrize("G", [1, 2, 5, 32])
def test_head_against_float64(backend, G, S, N):
    key = (G, S, N)
    if key not in _REF:  # the statements of a shape: computed once, left unchanged
        inp = _inputs(N, G, S)
        _REF[key] = (inp, _lines(*inp, G, torch.float64), _lines(*inp, G, torch.float32))
    inp, r64, r32 = _REF[key]
    got = _head(backend.device, *inp, G, pad=3)
    for name, g, a, b in zip(("losses", "dz", "sigmas", "logpi"), got, r64, r32):
        _close(g, a, b, f"{name} G={G} S={S} N={N}")


@pytest.mark.parametrize("divide", [True, False])
def test_first_row_leaves_exact_zero_rows_in_front(backend, divide):
    N, G, S, first = 65, 5, 6, 52  # (T - 1) * B of T = 5, B = 13
    inp = _inputs(N, G, S, seed=3)
    _, dz, sig, lpi = _check(backend.device, inp, G, f"first_row divide={divide}", first_row=first, divide=divide)
    assert (dz[:first] == 0).all() and (dz[first:] != 0).any(dim=1).all()
    assert torch.isfinite(sig).all() and torch.isfinite(lpi).all()  # the outputs cover every row
    without = _head(backend.device, *inp, G, first_row=first, divide=divide, outputs=False)
    assert torch.equal(_bits(without[1]), _bits(dz))


def test_a_component_200_nats_ahead(backend):
    N, G, S = 5, 5, 6
    z, ns, r, nt = _inputs(N, G, S, seed=5)
    z[:, G * S:2 * G * S] = 0.0  # sigma = 1
    mus = z[:, :G * S].view(N, G, S)
    mus[:] = ns.unsqueeze(1) + (400.0 / S) ** 0.5  # every component 200 nats below the density's peak ...
    for i in range(N):
        mus[i, i % G] = ns[i] + 0.01 * torch.randn(S)  # ... but one
    z[:, 2 * G * S:2 * G * S + G] = 0.0
    losses, dz, _, _ = _check(backend.device, (z, ns, r, nt), G, "200 nats")
    assert torch.isfinite(losses).all() and torch.isfinite(dz).all()
    far = torch.ones(N, G, dtype=torch.bool)
    far[torch.arange(N), torch.arange(N) % G] = False
    assert (dz[:, :G * S].view(N, G, S)[far] == 0).all()  # responsibilities of e^-200: exactly 0 in fp32


@pytest.mark.parametrize("log_sigma", [30.0, -30.0])
def test_log_sigmas_at_30(backend, log_sigma):
    N, G, S = 9, 2, 6
    z, ns, r, nt = _inputs(N, G, S, seed=9)
    z[:, G * S:2 * G * S] = log_sigma
    losses, dz, sig, _ = _check(backend.device, (z, ns, r, nt), G, f"log sigma {log_sigma}")
    assert torch.isfinite(losses).all() and torch.isfinite(dz).all() and torch.isfinite(sig).all()


def test_two_runs_give_the_same_bits(backend):
    inp = _inputs(300, 5, 33, seed=2)
    a, b = _head(backend.device, *inp, 5), _head(backend.device, *inp, 5)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("shape", [(7, 3), (65,), (2, 3, 4)])
def test_gmm_loss_function(backend, shape):
    """reagent_amd.models.mdn_rnn.gmm_loss with the reference's signature, reduce=False included"""
    G, S = 5, 6
    g = torch.Generator().manual_seed(len(shape))
    batch, mus = torch.randn(*shape, S, generator=g), torch.randn(*shape, G, S, generator=g)
    sigmas = torch.exp(0.5 * torch.randn(*shape, G, S, generator=g))
    logpi = F.log_softmax(torch.randn(*shape, G, generator=g), dim=-1)
    dev = backend.device
    for reduce in (False, True):
        got = gmm_loss(batch.to(dev), mus.to(dev), sigmas.to(dev), logpi.to(dev), reduce=reduce)
        r64 = _gmm_lines(batch.double(), mus.double(), sigmas.double(), logpi.double(), reduce)
        r32 = _gmm_lines(batch, mus, sigmas, logpi, reduce)
        assert got.shape == r32.shape and got.dtype == torch.float32
        _close(got, r64, r32, f"gmm_loss reduce={reduce} {shape}")


def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    p, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()
    EINVAL = -1

    def head(n=1, G=1, S=1, ldz=5, lddz=5, first=0, z=p, ns=p, dz=p, partials=d.data_ptr(), losses=p):
        return lib.rg_mdn_head(z, ldz, ns, p, p, 1.0, 1.0, 1.0, 1, first, n, G, S, dz, lddz, None, None, partials, losses, s)

    def nll(n=1, G=1, S=1, mus=p, out=p):
        return lib.rg_mdn_gmm_nll(p, mus, p, p, n, G, S, out, s)

    t[1] = 1.0  # (a sigma of 1 for the stand-alone nll)
    assert head() == 0 and nll() == 0
    for call in (head, nll):
        assert call(G=33) == L.EUNSUPPORTED and call(S=513) == L.EUNSUPPORTED
        assert call(n=0) == EINVAL and call(G=0) == EINVAL and call(S=0) == EINVAL
    assert head(ldz=4) == EINVAL and head(lddz=4) == EINVAL and head(first=1) == EINVAL and head(first=-1) == EINVAL
    for k in ("z", "ns", "dz", "partials", "losses"):
        assert head(**{k: None}) == EINVAL
    assert nll(mus=None) == EINVAL and nll(out=None) == EINVAL
    assert lib.rg_mdn_head_partials(0) == 0 and lib.rg_mdn_head_partials(5) == 2
    f = dict(dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="33 gaussians"):
        ops.mdn_gmm_nll(torch.zeros(1, 1, **f), torch.zeros(1, 33, 1, **f), torch.ones(1, 33, 1, **f), torch.zeros(1, 33, **f),
                        torch.zeros(1, **f))
