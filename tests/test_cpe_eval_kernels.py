"""The five entry points of reagent_amd/csrc/cpe_eval.hip against the statements of include/reagent_hip.h (ABI 21), on the
interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24.

Page rows.  logged_rewards, eval_action_idxs and the three *_for_logged_action outputs are BIT-EQUAL to the torch fp32
statement (one-hot actions: one non-zero term in every sum, so the order cannot matter; planted ties and a masked-out maximum
are in the arg-max rows).  model_propensities is held to the bound rg_cpe_head's propensities are held to in
tests/test_head_kernels.py: 4 u (max |q / T| + 4) against the float64 masked softmax.  A fully masked row is all zeros.

DR rows.  A sum of A fp32 products added in any order differs from the float64 sum of the same products by at most
(A + 1) u sum|terms| (A - 1 additions and one rounding per product, first order; the + 1 covers second order at these A);
torch's own fp32 rows are held to the same bound in the same test.  importance_weight, ips and dr are bit-equal to the fp32
statement evaluated from the kernel's own target_propensity and dm.  The five totals (double sums of fp32 terms) are within
(N + 2) u sum|terms| of the float64 sums of the kernel's own rows.

Episode values and sequential DR.  Bit-equal to a numpy fp32 restatement of the two recurrences, from the kernel's own row
quantities; on small-integer inputs with gamma = 0.5 and gaps in {1, 2} every intermediate is exact in fp32, so the result
equals the float64 recurrence exactly and one dropped step fails.

Bootstrap.  `means` against a numpy restatement of the header's draw recipe (Philox4x32-10, index = (word * n) >> 32): a
double sum of sample_size terms in any order, (sample_size + 2) 2^-53 sum|terms|; std against numpy's over those means to
1e-12 relative; the same seed gives the same bits, another seed other means; statistically, at K = 1000 on 4 096 normal and
4 096 Pareto(3) values, std is within 6 / sqrt(2 (K - 1)) = 13.4 % of sqrt(var64 / sample_size): six standard deviations of
a sample standard deviation (the reference's own function stayed within 4.4 % on five seeds of both inputs).
"""
import math
import os

import numpy as np
import pytest
import torch

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
EINVAL = -1
F32, F64 = torch.float32, torch.float64


# ---- rg_cpe_page_rows -------------------------------------------------------------------------------------------------------
def _page_inputs(B, A, M, seed, masked=True, boosts=True):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, A, generator=g)
    logged = torch.randint(A, (B,), generator=g)
    action = torch.nn.functional.one_hot(logged, A).float()
    mask = None
    if masked:
        mask = (torch.rand(B, A, generator=g) < 0.7).float()
        mask[torch.arange(B), logged] = 1.0
    if A >= 3 and B >= 3:
        q[0, 0] = q[0, 2] = q[0].max() + 1.0     # a planted tie: the first index wins
        if mask is not None:
            mask[0, 0] = mask[0, 2] = 1.0
            q[1, 1] = q[1].max() + 5.0           # the maximum is masked out
            mask[1, 1] = 0.0
            mask[1, 0] = 1.0
            action[1] = torch.nn.functional.one_hot(torch.tensor(0), A).float()
            mask[2] = 0.0                        # a fully masked row
    return dict(q=q, q_cpe=torch.randn(B, M * A, generator=g), reward_est=torch.randn(B, M * A, generator=g), action=action,
                mask=mask, reward=torch.randn(B, generator=g), boosts=torch.randn(A, generator=g) if boosts else None)


def _page_statement(d, T, M, dtype):
    """create_from_tensors_dqn's row arithmetic as the reference writes it (dqn_trainer_base.py:33-77, 216-241;
    core/torch_utils.py:62-73; evaluation_data_page.py:376-433) in `dtype`"""
    B, A = d["action"].shape
    c = lambda t: t.to(dtype)
    mask = c(d["mask"]) if d["mask"] is not None else torch.ones(B, A, dtype=dtype)
    act = c(d["action"])
    boost = (act * c(d["boosts"]).reshape(1, A)).sum(1, keepdim=True) if d["boosts"] is not None else torch.zeros(B, 1, dtype=dtype)
    out = dict(logged_rewards=c(d["reward"]).reshape(B, 1) + boost)
    out["idx"] = torch.max(c(d["q"]) + -1e9 * (1 - mask), dim=1, keepdim=True)[1]
    logits = c(d["q"]) / T - (1.0 - mask) * 1e20
    w = (logits - logits.max(dim=1, keepdim=True).values).exp() * mask
    p = w / w.sum(dim=1, keepdim=True)
    out["prop"] = torch.where(torch.isnan(p), torch.zeros_like(p), p)
    re, qc = c(d["reward_est"]), c(d["q_cpe"])
    out["mr"] = (re[:, :A] * act).sum(1, keepdim=True)
    if M > 1:
        out["mm"] = torch.cat([(re[:, i * A:(i + 1) * A] * act).sum(1, keepdim=True) for i in range(1, M)], 1)
        out["mmv"] = torch.cat([(qc[:, i * A:(i + 1) * A] * act).sum(1, keepdim=True) for i in range(1, M)], 1)
    return out


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("A", [1, 3, 5, 16])
@pytest.mark.parametrize("B", [1, 37, 257])
def test_page_rows(backend, B, A, M):
    from reagent_amd import ops

    dev, T = backend.device, 0.5
    for masked, boosts in ((True, True), (False, False)):
        d = _page_inputs(B, A, M, 1000 * B + 10 * A + M, masked, boosts)
        t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}

        def run():
            return ops.cpe_page_rows(t["q"], t["q_cpe"] if M > 1 else None, t["reward_est"], t["action"], t["mask"], t["reward"],
                                     t["boosts"], T, M)

        got, again = run(), run()
        for a, b in zip(got, again):
            assert (a is None and b is None) or torch.equal(a, b)
        lr, prop, idx, mr, mm, mmv = [None if x is None else x.cpu() for x in got]
        want, w64 = _page_statement(d, T, M, F32), _page_statement(d, T, M, F64)
        assert torch.equal(lr, want["logged_rewards"]) and lr.shape == (B, 1)
        assert torch.equal(idx, want["idx"]) and idx.dtype == torch.int64 and idx.shape == (B, 1)
        assert torch.equal(mr, want["mr"])
        if M > 1:
            assert torch.equal(mm, want["mm"]) and torch.equal(mmv, want["mmv"]) and mm.shape == (B, M - 1)
        else:
            assert mm is None and mmv is None
        bound = 4 * U * ((d["q"] / T).abs().max().item() + 4)
        err = (prop.double() - w64["prop"]).abs().max().item()
        print(f"CPEERR page propensities B={B} A={A} M={M} err={err:.3e} bound={bound:.3e}")
        assert err <= bound
        assert (want["prop"].double() - w64["prop"]).abs().max().item() <= bound  # torch's own fp32 rows, same bound
        if masked:
            assert torch.equal(prop * (1 - d["mask"]), torch.zeros(B, A))
            if A >= 3 and B >= 3:
                assert idx[0, 0] == 0 and idx[1, 0] != 1 and not prop[2].any()


# ---- rg_cpe_dr_rows ------------------------------------------------------------------------------------------------------------
def _dr_inputs(N, A, seed):
    g = torch.Generator().manual_seed(seed)
    prop = torch.softmax(torch.randn(N, A, generator=g), 1)
    mask = torch.nn.functional.one_hot(torch.randint(A, (N,), generator=g), A).float()
    wide_r, wide_v = torch.randn(N, 2 * A, generator=g), torch.randn(N, 2 * A, generator=g)  # a metric's columns, read in place
    cols = torch.randn(N, 3, generator=g)
    return dict(prop=prop, mask=mask, mr=wide_r[:, A:], mv=wide_v[:, A:], lp=0.2 + 0.8 * torch.rand(N, generator=g),
                r=cols[:, 1:2], mrl=cols[:, 2:3])


@pytest.mark.parametrize("A", [1, 3, 5, 16])
@pytest.mark.parametrize("N", [1, 37, 257])
def test_dr_rows(backend, N, A):
    from reagent_amd import ops

    d = _dr_inputs(N, A, 77 * N + A)
    t = {k: v.to(backend.device) for k, v in d.items()}
    run = lambda: ops.cpe_dr_rows(t["prop"], t["mask"], t["mr"], t["mv"], t["lp"], t["r"], t["mrl"])
    got, again = run(), run()
    for k in got:
        assert torch.equal(got[k], again[k]), k
    o = {k: v.cpu() for k, v in got.items()}
    p64, m64, mr64, mv64 = (d[k].double() for k in ("prop", "mask", "mr", "mv"))
    sums = dict(target_propensity=(p64 * m64, d["prop"] * d["mask"]), state_value=(p64 * mv64, d["prop"] * d["mv"]),
                q_logged=(mv64 * m64, d["mv"] * d["mask"]), dm=(p64 * mr64, d["prop"] * d["mr"]))
    for name, (terms, terms32) in sums.items():
        mine = o["dm_ips_dr"][0] if name == "dm" else o[name]
        bound = (A + 1) * U * terms.abs().sum(1)
        assert ((mine.double() - terms.sum(1)).abs() <= bound).all(), name
        assert ((terms32.sum(1).double() - terms.sum(1)).abs() <= bound).all(), name  # torch's own fp32 rows
    tp, dm = o["target_propensity"], o["dm_ips_dr"][0]
    iw = tp / d["lp"]
    r, mrl = d["r"].reshape(-1), d["mrl"].reshape(-1)
    assert torch.equal(o["importance_weight"], iw)
    assert torch.equal(o["dm_ips_dr"][1], iw * r)
    assert torch.equal(o["dm_ips_dr"][2], iw * (r - mrl) + dm)
    rows = [r, dm, mrl, o["dm_ips_dr"][1], o["dm_ips_dr"][2]]
    for k, x in enumerate(rows):
        s64 = x.double().sum().item()
        assert abs(o["totals"][k].item() - s64) <= (N + 2) * U * x.double().abs().sum().item(), k
    assert o["totals"].dtype == F64 and o["dm_ips_dr"].shape == (3, N)


# ---- episodes: rg_cpe_episode_values, rg_cpe_sdr ---------------------------------------------------------------------------------
def _episodes(kind, N, g):
    if kind == "ones":
        lengths = [1] * N
    elif kind == "single":
        lengths = [N]
    else:
        lengths = []
        while sum(lengths) < N:
            lengths.append(min(int(torch.randint(1, 41, (1,), generator=g)), N - sum(lengths)))
    return lengths


def _np_values(c, seq, lengths, gamma):
    """compute_values_for_mdps, the header's fp32 statement: v[x] = c[x] + v[x + 1] * fp32(pow(gamma, double(gap)))"""
    v = c.astype(np.float32).copy()
    b = 0
    for n in lengths:
        for x in range(b + n - 2, b - 1, -1):
            f = np.float32(math.pow(gamma, float(seq[x + 1] - seq[x])))
            v[x] = np.float32(c[x] + np.float32(v[x + 1] * f))
        b += n
    return v


def _np_sdr(sv, iw, r, q, lengths, gamma, dtype):
    g = dtype(np.float32(gamma))
    dr, ev, b = [], [], 0
    for n in lengths:
        d = e = dtype(0)
        for j in range(b + n - 1, b - 1, -1):
            d = dtype(sv[j] + dtype(iw[j] * dtype(dtype(r[j] + dtype(g * d)) - q[j])))
            e = dtype(dtype(e * g) + r[j])
        dr.append(d)
        ev.append(e)
        b += n
    return np.array(dr, dtype=dtype), np.array(ev, dtype=dtype)


EPISODE_CASES = [("ones", 37), ("ones", 300), ("ragged", 257), ("ragged", 1), ("single", 257), ("single", 1), ("ragged", 6000)]


@pytest.mark.parametrize("kind,N", EPISODE_CASES, ids=lambda v: str(v))
def test_episode_values_and_sdr(backend, kind, N):
    from reagent_amd import ops
    from reagent_amd.evaluation.evaluation_data_page import episode_offsets

    dev = backend.device
    g = torch.Generator().manual_seed(31 * N + len(kind))
    lengths = _episodes(kind, N, g)
    E = len(lengths)
    if (kind == "ones" and N == 300) or N == 6000:
        assert E > 256  # more episodes than one workgroup has lanes
    mdp = torch.repeat_interleave(torch.arange(E) * 3 + 5, torch.tensor(lengths))
    for exact in (False, True):
        gamma = 0.5 if exact else 0.93
        gaps = torch.randint(1, 3 if exact else 4, (N,), generator=g)
        seq = torch.cumsum(gaps, 0)  # (the gap across an episode border is never read)
        if exact:  # small integers and gamma = 0.5 (exactness itself is test_recurrences_exact_on_small_integers' subject)
            draw = lambda *s: torch.randint(-3, 4, s, generator=g).float()
        else:
            draw = lambda *s: torch.randn(*s, generator=g)
        wide = draw(N, 3)
        offsets = episode_offsets(mdp.to(dev))
        assert offsets.dtype == torch.int32 and offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
        out = torch.full((N, 3), 7.0, device=dev)
        src = wide.to(dev)
        ops.cpe_episode_values(src[:, 1:2], seq.to(dev), offsets, gamma, out[:, 1:2])
        got = out.cpu()
        assert (got[:, 0] == 7.0).all() and (got[:, 2] == 7.0).all()  # the pitch is honoured: the neighbours are untouched
        c = wide[:, 1].numpy()
        assert np.array_equal(got[:, 1].numpy(), _np_values(c, seq.numpy(), lengths, gamma))
        sv, q, r = draw(N), draw(N), wide[:, 1:2]
        iw = torch.randint(0, 3, (N,), generator=g).float() if exact else torch.rand(N, generator=g) * 2
        dr, ev = ops.cpe_sdr(sv.to(dev), iw.to(dev), src[:, 1:2], q.to(dev), offsets, gamma)
        want_dr, want_ev = _np_sdr(sv.numpy(), iw.numpy(), c, q.numpy(), lengths, gamma, np.float32)
        assert np.array_equal(dr.cpu().numpy(), want_dr) and np.array_equal(ev.cpu().numpy(), want_ev)
        assert dr.shape == (E,) and ev.shape == (E,)


def test_recurrences_exact_on_small_integers(backend):
    """gamma = 0.5, gaps in {1, 2}, integer inputs in [-3, 3], importance weights in {0, 1, 2}, episodes of at most 6 rows:
    every intermediate is a multiple of 2^-12 below 2^11, exact in fp32, so the kernels equal the float64 recurrences
    exactly -- a dropped or doubled step changes the value"""
    from reagent_amd import ops
    from reagent_amd.evaluation.evaluation_data_page import episode_offsets

    dev = backend.device
    g = torch.Generator().manual_seed(5)
    lengths = [1, 6, 2, 5, 6, 3, 1, 4] * 40
    N, E = sum(lengths), len(lengths)
    assert E > 256
    mdp = torch.repeat_interleave(torch.arange(E), torch.tensor(lengths))
    seq = torch.cumsum(torch.randint(1, 3, (N,), generator=g), 0)
    draw = lambda: torch.randint(-3, 4, (N,), generator=g).float()
    c, sv, q = draw(), draw(), draw()
    iw = torch.randint(0, 3, (N,), generator=g).float()
    offsets = episode_offsets(mdp.to(dev))
    out = torch.empty(N, 1, device=dev)
    ops.cpe_episode_values(c.reshape(N, 1).to(dev), seq.to(dev), offsets, 0.5, out)
    v64 = c.double().numpy().copy()
    b = 0
    for n in lengths:
        for x in range(b + n - 2, b - 1, -1):
            v64[x] = v64[x] + v64[x + 1] * 0.5 ** float(seq[x + 1] - seq[x])
        b += n
    assert np.array_equal(out.cpu().reshape(-1).double().numpy(), v64)
    dr, ev = ops.cpe_sdr(sv.to(dev), iw.to(dev), c.reshape(N, 1).to(dev), q.to(dev), offsets, 0.5)
    d64, e64 = _np_sdr(sv.double().numpy(), iw.double().numpy(), c.double().numpy(), q.double().numpy(), lengths, 0.5, np.float64)
    assert np.array_equal(dr.cpu().double().numpy(), d64) and np.array_equal(ev.cpu().double().numpy(), e64)
    assert np.abs(d64).max() > 3  # the recurrence did accumulate


def test_offsets_from_device_memory_are_clamped(backend):
    """offsets outside the page (a corrupted table) are clamped to it: nothing is read or written out of bounds"""
    from reagent_amd import ops

    dev = backend.device
    N = 9
    c = torch.arange(N, dtype=F32, device=dev).reshape(N, 1)
    seq = torch.arange(N, device=dev)
    offsets = torch.tensor([-5, 4, 3, 100], dtype=torch.int32, device=dev)
    out = torch.full((N + 4, 1), -1.0, device=dev)
    ops.cpe_episode_values(c, seq, offsets, 1.0, out[:N])
    assert (out[N:] == -1.0).all()
    dr, ev = ops.cpe_sdr(c.reshape(-1), torch.ones(N, device=dev), c, torch.zeros(N, device=dev), offsets, 1.0)
    assert ev.tolist() == [0 + 1 + 2 + 3, 0.0, 3 + 4 + 5 + 6 + 7 + 8]  # [0, 4), [4, 4), [3, 9)


# ---- rg_cpe_bootstrap ----------------------------------------------------------------------------------------------------------
def _philox4x32_10(seed, c0, c2):
    """the header's recipe on numpy uint64 arrays: key (lo32(seed), hi32(seed)), counter (c0, 0, c2, 0) -> four uint32 words"""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(c0, dtype=np.uint64) & mask, np.zeros_like(c0, dtype=np.uint64), np.asarray(c2, dtype=np.uint64) & mask,
         np.zeros_like(c0, dtype=np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c


def _indices(seed, n, sample_size, K):
    """[K, sample_size] int64: draw j of resample k = word j % 4 of the block with counter (j / 4, 0, k, 0); (word * n) >> 32"""
    j = np.arange(sample_size, dtype=np.uint64)
    jj, kk = np.meshgrid(j, np.arange(K, dtype=np.uint64))
    words = _philox4x32_10(seed, jj // np.uint64(4), kk)
    word = np.choose((jj % np.uint64(4)).astype(np.int64), words)
    return ((word * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


BOOT_CASES = [(3, 0, 8, 1), (4, 1, 8, 1), (1000, 250, 64, 3), (5000, 1030, 16, 2)]


@pytest.mark.parametrize("n,S,K,C", BOOT_CASES)
def test_bootstrap_against_the_documented_recipe(backend, n, S, K, C):
    from reagent_amd import ops

    dev = backend.device
    seed = 0x1234_5678_9ABC_DEF0 + n
    g = torch.Generator().manual_seed(n)
    wide = torch.randn(C, n + 5, generator=g)
    vals = wide.to(dev)[:, :n]  # a pitch of n + 5
    means, std = ops.cpe_bootstrap(vals, S, K, seed)
    means2, std2 = ops.cpe_bootstrap(vals, S, K, seed)
    assert torch.equal(means, means2) or (S == 0 and means.isnan().all() and means2.isnan().all())
    assert means.shape == (C, K) and std.shape == (C,) and means.dtype == F64 and std.dtype == F64
    if S == 0:
        assert means.isnan().all() and std.isnan().all()  # np.mean of nothing
        return
    assert torch.equal(std, std2)
    idx = _indices(seed, n, S, K)
    assert idx.min() >= 0 and idx.max() < n
    v = wide[:, :n].double().numpy()
    for c in range(C):
        terms = v[c][idx]  # [K, S]
        want = terms.sum(1) / S
        bound = (S + 2) * 2.0 ** -53 * np.abs(terms).sum(1) / S
        assert (np.abs(means[c].cpu().numpy() - want) <= bound).all(), c
        mine = means[c].cpu().numpy()
        assert abs(std[c].item() - np.std(mine)) <= 1e-12 * np.std(mine)
    other, _ = ops.cpe_bootstrap(vals, S, K, seed + 1)
    assert not torch.equal(other, means)


def test_bootstrap_indices_in_range_at_n_1(backend):
    from reagent_amd import ops

    v = torch.tensor([[2.5]], device=backend.device)
    means, std = ops.cpe_bootstrap(v, 1030, 8, 99)
    assert (means == 2.5).all() and std.item() == 0.0


@pytest.mark.parametrize("dist", ["normal", "pareto"])
def test_bootstrap_standard_error_statistically(backend, dist):
    from reagent_amd.evaluation.cpe import bootstrapped_std_error_of_mean

    rng = np.random.RandomState(7)
    x = rng.standard_normal(4096) if dist == "normal" else rng.pareto(3.0, 4096)
    x = x.astype(np.float32)
    K, S = 1000, 1024
    want = math.sqrt(x.astype(np.float64).var() / S)
    tol = 6.0 / math.sqrt(2.0 * (K - 1))
    assert abs(tol - 0.134) < 1e-3
    t = torch.from_numpy(x).to(backend.device)
    got = bootstrapped_std_error_of_mean(t, sample_percent=0.25, num_samples=K, seed=4242)
    print(f"CPEERR bootstrap {dist} std={got:.6e} want={want:.6e} rel={abs(got - want) / want:.4f} tol={tol:.4f}")
    assert abs(got - want) <= tol * want
    torch.manual_seed(11)  # seed=None: one draw from torch's default generator
    a = bootstrapped_std_error_of_mean(t, num_samples=50)
    torch.manual_seed(11)
    assert bootstrapped_std_error_of_mean(t, num_samples=50) == a


# ---- refusals and resources -----------------------------------------------------------------------------------------------------
def test_einval(backend):
    import reagent_amd._lib as L

    lib, dev, p = L.lib(), backend.device, L.ptr
    B, A, M = 8, 3, 2
    f = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
    i64 = torch.zeros(B, dtype=torch.int64, device=dev)
    off = torch.tensor([0, B], dtype=torch.int32, device=dev)
    d64 = torch.zeros(64, dtype=F64, device=dev)
    wide, sq, row = f(B, M * A), f(B, A), f(B)
    o = [f(3, B) for _ in range(6)]  # outputs (kept alive over the calls); o[k][0] is a [B] row, o[k] at most [B, A] or [3, B]

    def page(B_=B, A_=A, M_=M, null=()):
        a = [p(sq), p(wide), p(wide), p(sq), None, p(row), None, 1.0, B_, A_, M_, p(o[0]), p(o[1]), p(i64), p(o[2]),
             p(o[3]), p(o[4]), None]
        for k in null:
            a[k] = None
        return lib.rg_cpe_page_rows(*a)

    assert page() == 0 and page(B_=0) == EINVAL and page(A_=0) == EINVAL and page(M_=0) == EINVAL
    for k in (0, 2, 3, 5, 11, 12, 13, 14, 1, 15, 16):
        assert page(null=(k,)) == EINVAL, k
    assert page(M_=1, null=(1, 15, 16)) == 0  # q_cpe and the metric outputs are unused at M == 1

    def values(E=1, N=B, ld=1, ldv=1, null=()):
        a = [p(row), ld, p(i64), p(off), E, N, 0.9, p(o[0]), ldv, None]
        for k in null:
            a[k] = None
        return lib.rg_cpe_episode_values(*a)

    assert values() == 0 and values(E=0) == EINVAL and values(N=0) == EINVAL and values(E=B + 1) == EINVAL
    assert values(ld=0) == EINVAL and values(ldv=0) == EINVAL
    for k in (0, 2, 3, 7):
        assert values(null=(k,)) == EINVAL, k

    def dr(N=B, A_=A, ld=A, ld1=1, null=()):
        a = [p(sq), p(sq), p(sq), ld, p(sq), ld, p(row), p(row), ld1, p(row), ld1, N, A_, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
             p(o[4]), p(d64), p(d64[32:]), None]
        for k in null:
            a[k] = None
        return lib.rg_cpe_dr_rows(*a)

    assert dr() == 0 and dr(N=0) == EINVAL and dr(A_=0) == EINVAL and dr(ld=A - 1) == EINVAL and dr(ld1=0) == EINVAL
    for k in (0, 1, 2, 4, 6, 7, 9, 13, 14, 15, 16, 17, 18, 19):
        assert dr(null=(k,)) == EINVAL, k
    assert lib.rg_cpe_dr_partials(0) == 0 and lib.rg_cpe_dr_partials(256) == 1 and lib.rg_cpe_dr_partials(257) == 2

    def sdr(E=1, N=B, ld=1, null=()):
        a = [p(row), p(row), p(row), ld, p(row), p(off), E, N, 0.9, p(o[0]), p(o[1]), None]
        for k in null:
            a[k] = None
        return lib.rg_cpe_sdr(*a)

    assert sdr() == 0 and sdr(E=0) == EINVAL and sdr(N=0) == EINVAL and sdr(E=B + 1) == EINVAL and sdr(ld=0) == EINVAL
    for k in (0, 1, 2, 4, 5, 9, 10):
        assert sdr(null=(k,)) == EINVAL, k

    def boot(C=1, n=B, S=2, K=4, ld=B, null=()):
        a = [p(row), ld, C, n, S, K, 5, p(d64), p(d64[32:]), None]
        for k in null:
            a[k] = None
        return lib.rg_cpe_bootstrap(*a)

    assert boot() == 0 and boot(C=0) == EINVAL and boot(C=5) == EINVAL and boot(n=0) == EINVAL and boot(S=-1) == EINVAL
    assert boot(K=0) == EINVAL and boot(ld=B - 1) == EINVAL
    for k in (0, 7, 8):
        assert boot(null=(k,)) == EINVAL, k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cpe_eval_kernels_have_no_scratch(tmp_path):
    """cpe_eval.hip compiled for gfx950 with the resource remarks on: seven kernels, no scratch, no spilled register"""
    kernels = kernel_resources("cpe_eval.hip", tmp_path)
    names = ("cpe_page_rows_kernel", "cpe_episode_values_kernel", "cpe_dr_rows_kernel", "cpe_dr_finish_kernel",
             "cpe_sdr_kernel", "cpe_bootstrap_kernel", "cpe_bootstrap_finish_kernel")
    for want in names:
        found = [k for k in kernels if want in k]
        assert len(found) == (2 if want == "cpe_bootstrap_kernel" else 1), (want, found)
        for k in found:
            v = kernels[k]
            assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
            assert v["VGPRs"] <= 128, (k, v)
    assert len(kernels) == len(names) + 1, list(kernels)  # (the resampler has a one-wave and a four-wave shape)
