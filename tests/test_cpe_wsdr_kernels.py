"""rg_cpe_wsdr (reagent_amd/csrc/cpe_wsdr.hip, ABI 22) against a float64 numpy restatement of the reference's DENSE
computation (tests/cpe_wsdr_statement.py: padded cubes, np.cumprod, np.cov), on the interpreter and, under `-m gpu`, on the
MI355X.  u = 2^-53.

THE ANY-ORDER BOUND.  Every number compared is a sum of terms disc[s] * weight * value.  First order, per term:
  ratio = (sum of A exact products of non-negative numbers) / logged_p            (A + 1) u relative
  w_raw[s], a product of s + 1 ratios                                             (s + 1)(A + 2) u
  S[s], a sum of at most E non-negative w_raw in any order                        + E u
  wn = w_raw / S (or / n)                                                         2 (s + 1)(A + 2) u + (E + 1) u
  disc[s] = pow(gamma, s), each library within an ulp                             2 u
  value: r exact; sv, ql sums of A products in any order                          (A + 1) u of the sum of |products|
  the two or three multiplications and the at most 3 T + 2 additions of a return  (3 T + 5) u
so with K = T (2 A + 7) + E + A + 9 each side is within K u of the sum of the |terms| (sv and ql counted by their |products|),
and the kernel and the float64 statement differ by at most (2 K + 2) u sum|terms| (the + 2 covers second order at these
sizes: K u < 1e-11).  A sum over episodes adds E additions: 2 (K + E) + 2.  A covariance entry is a sum of products of two
centred returns, each centred return within (K + E + 2) u of (sum|terms| + mean sum|terms|) on each side: 4 (K + E + 2) u of
sum_e big_j big_k / (E - 1), big = sum|terms| + its mean.

Cases: E in 1, 5, 67, 257 with ragged lengths (lanes and workgroups crossed; 67 / 25 is not an integer); every episode of
length 1; one episode of 300 steps among short ones (the 256-thread chunk of the column sums); j-steps with duplicates, -1,
T - 1 and values beyond most episodes; both values of the self-normalize flag; a zero column with episodes alive; the first
E <= 2 000 with int(G * (E / G)) < E (E = 57: the reference's float interval leaves the last episode out of every subset),
and subsets given by hand that leave episodes out at both ends.

THE EXACT CASE.  Ratios in 1/2, 1, 2, gamma in 1, 1/2, E = 16, at most 3 steps, not self-normalized, integer rewards and
values in -3 .. 3 and propensities that are powers of two: every intermediate is a multiple of 2^-13 below 2^9 (returns:
multiples of 2^-9; their means and centred values: of 2^-13), a product of two centred values has 44 bits and a sum of 16 of
them 48, so ret, the sums and the covariance numerators are exact in double and the kernel equals the restatement bit for bit
(the covariance: the one rounded division by E - 1 of the same exact numerator).  profiles/NOTES_r20.md records that a copy
of the kernel without the j + 1 direct-method term or without the wprev shift fails this test.  It does not read the column
sums (not self-normalized), so a second exact case is self-normalized with weights that depend on the step alone (its
docstring); a copy with one episode dropped from a column sum fails that one.
"""
import ctypes

import numpy as np
import pytest
import torch

from cpe_wsdr_statement import dense_statement
from kernel_remarks import kernel_resources

U = 2.0 ** -53
EINVAL = -1
INF = float("inf")


def _K(T, E, A):
    return T * (2 * A + 7) + E + A + 9


def _subsets(E, most=25):
    """weighted_sequential_doubly_robust_estimator.py:112-119 of the reference, as written there"""
    num_subsets = int(min(E / 2, most))
    interval = E / num_subsets
    return [int(i * interval) for i in range(num_subsets)] + [int(num_subsets * interval)]


def _page(lengths, A, seed, zero_step=None, wide=False):
    g = torch.Generator().manual_seed(seed)
    N = int(sum(lengths))
    prop = torch.softmax(1.5 * torch.randn(N, A, generator=g), 1)
    logged = torch.randint(A, (N,), generator=g)
    mask = torch.nn.functional.one_hot(logged, A).float()
    if zero_step is not None:
        start = 0
        for n in lengths:
            if n > zero_step:
                prop[start + zero_step, logged[start + zero_step]] = 0.0
            start += n
    values = torch.randn(N, 2 * A, generator=g)[:, A:] if wide else torch.randn(N, A, generator=g)
    cols = torch.randn(N, 3, generator=g)
    return dict(prop=prop, mask=mask, values=values, lp=0.2 + 0.8 * torch.rand(N, generator=g),
                r=cols[:, 1:2] if wide else cols[:, :1].contiguous(), lengths=list(lengths),
                offsets=torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32))


def _ragged(E, top, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, top + 1, E)
    lengths[rng.integers(E)] = 1
    return lengths.tolist()


def _run(backend, d, gamma, flag, j_steps, subsets, T=None):
    from reagent_amd import ops

    dev = backend.device
    T = T or max(d["lengths"])
    js = [int(min(j, T - 1)) for j in j_steps]
    ret, out = ops.cpe_wsdr(d["prop"].to(dev), d["mask"].to(dev), d["values"].to(dev), d["lp"].to(dev), d["r"].to(dev),
                            d["offsets"].to(dev), T, gamma, flag, js, subsets)
    return ret.cpu().numpy(), out.cpu().numpy()


def _statement(d, gamma, flag, j_steps, subsets):
    return dense_statement(d["lengths"], d["mask"].numpy(), d["r"].numpy(), d["lp"].numpy(), d["prop"].numpy(),
                           d["values"].numpy(), gamma, flag, j_steps, subsets)


def _hold(label, got, want, mag, factor):
    err = np.abs(np.asarray(got) - np.asarray(want))
    bound = factor * U * np.asarray(mag)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"WSDRERR {label} max err={float(err.max()) if err.size else 0.0:.3e} worst err/bound={worst:.3f}")
    assert (err <= bound).all(), (label, float(err.max()), worst)


def _check(backend, label, d, gamma, flag, j_steps, subsets):
    J, A, E = len(j_steps), d["prop"].shape[1], len(d["lengths"])
    ret, out = _run(backend, d, gamma, flag, j_steps, subsets)
    want = _statement(d, gamma, flag, j_steps, subsets if J > 1 else None)
    K = _K(want["T"], E, A)
    assert ret.shape == (J + 1, E)
    _hold(label + " ret", ret, want["ret"], want["ret_mag"], 2 * K + 2)
    _hold(label + " j_step_returns", out[:J], want["j_step_returns"], want["j_step_returns_mag"], 2 * (K + E) + 2)
    _hold(label + " logged_policy_score", out[-1], want["logged_policy_score"], want["logged_policy_score_mag"],
          2 * (K + E) + 2)
    if J == 1:
        assert out.shape == (2,)
        return ret, out, want
    G = len(subsets) - 1
    assert out.shape == (J + G + J * J + 1,)
    _hold(label + " infinite_step_returns", out[J:J + G], want["infinite_step_returns"], want["infinite_step_returns_mag"],
          2 * (K + E) + 2)
    C = out[J + G:J + G + J * J].reshape(J, J)
    if E > 1:
        _hold(label + " covariance", C, want["covariance"], want["covariance_mag"], 4 * (K + E + 2))
        assert np.array_equal(C, C.T)  # exactly symmetric
    return ret, out, want


def _magic_j_steps(T, J=25):
    interval = T // (J - 1)
    return [INF, -1] + [i * interval for i in range(1, J - 1)]


def _first_left_out():
    for E in range(4, 2001):
        s = _subsets(E)
        if s[-1] < E:
            return E
    return None


@pytest.mark.parametrize("flag", [True, False])
@pytest.mark.parametrize("E", [1, 5, 67, 257])
def test_ragged_pages(backend, E, flag):
    d = _page(_ragged(E, 30, 11 * E), 3, 1000 + E, wide=E == 67)
    T = max(d["lengths"])
    _check(backend, f"E={E} sn={flag} J=1", d, 0.9, flag, [INF], None)
    if E >= 4:
        _check(backend, f"E={E} sn={flag} J=25", d, 0.9, flag, _magic_j_steps(T), _subsets(E))
    else:  # the kernel itself takes any E >= 1 with the subsets given (the estimator refuses MAGIC below four episodes)
        js = [INF, -1, 0, 0, T - 1, 2 * T]
        ret, out, _ = _check(backend, f"E={E} sn={flag} J=6", d, 0.9, flag, js, [0, E])
        if E == 1:
            assert np.isnan(out[6 + 1:6 + 1 + 36]).all()  # np.cov of one observation: 0 / 0


def test_every_episode_of_length_one(backend):
    d = _page([1] * 37, 4, 5)
    for flag in (True, False):
        _check(backend, f"T=1 sn={flag}", d, 0.8, flag, [INF, -1, 0, 0], _subsets(37))


def test_one_long_episode_among_short_ones(backend):
    lengths = _ragged(12, 6, 3)
    lengths[7] = 300
    d = _page(lengths, 2, 9)
    js = [INF, -1, 0, 0, 3, 5, 255, 256, 257, 299, 12]  # duplicates, -1, T - 1, beyond most episodes' lengths
    for flag in (True, False):
        _check(backend, f"T=300 sn={flag}", d, 0.99, flag, js, _subsets(12))


def test_zero_column_with_episodes_alive(backend):
    lengths = [1, 9, 4, 7, 2, 8, 3, 9, 6, 5]
    d = _page(lengths, 3, 21, zero_step=3)
    want = _statement(d, 0.9, True, [INF], None)
    assert sum(n > 3 for n in lengths) >= 2
    for flag in (True, False):
        _check(backend, f"zero column sn={flag}", d, 0.9, flag, [INF, -1, 1, 2, 3, 4, 8], _subsets(10))
    # quirk 5 is what the statement holds: with the flag set the steps from 3 on carry weight 1 / n, so the returns differ
    # from the ones without normalisation by more than the bound
    a, b = _run(backend, d, 0.9, True, [INF], None)[0], _run(backend, d, 0.9, False, [INF], None)[0]
    assert np.abs(a[0] - b[0]).max() > 1e-3 and want["T"] == 9


def test_episodes_outside_every_subset(backend):
    E = _first_left_out()
    assert E == 57  # int(25 * (57 / 25)) = 56: the reference's float interval leaves the last episode out
    d = _page(_ragged(E, 14, 57), 3, 57)
    s = _subsets(E)
    assert s[-1] == E - 1
    ret, out, want = _check(backend, "E=57 left out", d, 0.9, True, _magic_j_steps(max(d["lengths"])), s)
    # it counts in the whole set: without it the whole-set returns move
    short = {k: (v[:int(d["offsets"][-2])] if torch.is_tensor(v) and k != "offsets" else v) for k, v in d.items()}
    short["lengths"], short["offsets"] = d["lengths"][:-1], d["offsets"][:-1].clone()
    other = _run(backend, short, 0.9, True, [INF], None)[1]
    assert abs(other[0] - out[0]) > 1e-6
    # subsets given by hand that leave episodes out at both ends
    _check(backend, "E=57 by hand", d, 0.9, True, [INF, -1, 2], [3, 10, 10, 31, 50])


def _exact_page(seed, E=16):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, 4, (E,), generator=g).tolist()
    lengths[0], lengths[1] = 1, 3
    N, A = sum(lengths), 3
    prop = 2.0 ** torch.randint(-2, 1, (N, A), generator=g).float()
    logged = torch.randint(A, (N,), generator=g)
    mask = torch.nn.functional.one_hot(logged, A).float()
    ratio = 2.0 ** torch.randint(-1, 2, (N,), generator=g).float()
    lp = prop[torch.arange(N), logged] / ratio
    return dict(prop=prop, mask=mask, values=torch.randint(-3, 4, (N, A), generator=g).float(), lp=lp,
                r=torch.randint(-3, 4, (N, 1), generator=g).float(), lengths=lengths,
                offsets=torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32))


@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_exact_case_is_bit_equal(backend, gamma):
    d = _exact_page(77)
    js, s = [INF, -1, 0, 1, 0, 2], _subsets(16)
    ret, out = _run(backend, d, gamma, False, js, s)
    want = _statement(d, gamma, False, js, s)
    J, G = 6, len(s) - 1
    assert np.array_equal(ret, want["ret"])
    assert np.array_equal(out[:J], want["j_step_returns"])
    assert np.array_equal(out[J:J + G], want["infinite_step_returns"])
    assert np.array_equal(out[J + G:J + G + J * J].reshape(J, J), want["cov_numerators"] / 15.0)
    assert out[-1] == want["logged_policy_score"]
    assert np.abs(want["cov_numerators"]).max() > 0 and len(set(want["j_step_returns"].tolist())) >= 4
    ret1, out1 = _run(backend, d, gamma, False, [INF], None)
    assert np.array_equal(ret1[0], want["ret"][0]) and out1[0] == want["j_step_returns"][0]


@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_exact_case_self_normalized_is_bit_equal(backend, gamma):
    """The column sums in an exact case: the ratio of a row depends on its step alone (1/2, 2, 1/2), so every live episode has
    the same raw weight and wn = 1 / (episodes alive), and 8, 4 and 4 episodes of 1, 2 and 3 steps leave 16, 8 and 4 alive (1 or
    2 of a subset's two): all powers of two.  One episode dropped from a column sum makes 1 / 15 of it."""
    g = torch.Generator().manual_seed(78)
    lengths = [1] * 8 + [2] * 4 + [3] * 4
    lengths = [lengths[i] for i in torch.randperm(16, generator=g).tolist()]
    N, A = sum(lengths), 3
    step = torch.cat([torch.arange(n) for n in lengths])
    prop = 2.0 ** torch.randint(-2, 1, (N, A), generator=g).float()
    logged = torch.randint(A, (N,), generator=g)
    lp = prop[torch.arange(N), logged] / torch.tensor([0.5, 2.0, 0.5])[step]
    d = dict(prop=prop, mask=torch.nn.functional.one_hot(logged, A).float(),
             values=torch.randint(-3, 4, (N, A), generator=g).float(), lp=lp, r=torch.randint(-3, 4, (N, 1), generator=g).float(),
             lengths=lengths, offsets=torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32))
    js, s = [INF, -1, 0, 1, 0, 2], _subsets(16)
    ret, out = _run(backend, d, gamma, True, js, s)
    want = _statement(d, gamma, True, js, s)
    assert np.array_equal(ret, want["ret"])
    assert np.array_equal(out[:6], want["j_step_returns"]) and np.array_equal(out[6:14], want["infinite_step_returns"])
    assert np.array_equal(out[14:50].reshape(6, 6), want["cov_numerators"] / 15.0)
    ret1, out1 = _run(backend, d, gamma, True, [INF], None)  # the even runs of the J = 1 column sums
    assert np.array_equal(ret1[0], want["ret"][0]) and out1[0] == want["j_step_returns"][0]


def test_offsets_out_of_range_are_clamped(backend):
    d = _page([3, 8], 3, 31)
    N = 11
    clamped = dict(d, offsets=torch.tensor([-5, 3, 3, N + 10], dtype=torch.int32))  # [0, 3), an empty episode, [3, N)
    ret, out = _run(backend, clamped, 0.9, True, [INF, -1, 1], [0, 3], T=8)
    # the same page with the empty episode in the middle, stated densely: an episode of no rows is all padding
    assert ret.shape == (4, 3) and (ret[:, 1] == 0.0).all()
    dense = dense_statement_with_empty(d, 0.9, True, [INF, -1, 1])
    K = _K(8, 3, 3)
    _hold("clamped ret", ret[:3][:, [0, 2]], dense["ret"][:, [0, 2]], dense["ret_mag"][:, [0, 2]], 2 * K + 2)
    # an episode longer than `longest` is cut to it: nothing past the column sums is read
    ret_cut, _ = _run(backend, d, 0.9, True, [INF], None, T=5)
    cut = _page([3, 8], 3, 31)
    keep = [0, 1, 2, 3, 4, 5, 6, 7]
    short = dict(cut, lengths=[3, 5], **{k: cut[k][keep] for k in ("prop", "mask", "values", "lp", "r")})
    want_cut = _statement(short, 0.9, True, [INF], None)
    _hold("cut ret", ret_cut, want_cut["ret"], want_cut["ret_mag"], 2 * _K(5, 2, 3) + 2)
    assert want_cut["T"] == 5


def dense_statement_with_empty(d, gamma, flag, j_steps):
    """three episodes of 3, 0 and 8 rows: the dense cube of the two real ones with an all-padding row between them"""
    import cpe_wsdr_statement as S

    actions, r, lp, tp, qv = S.to_dense([3, 8], d["mask"].numpy(), d["r"].numpy(), d["lp"].numpy(), d["prop"].numpy(),
                                        d["values"].numpy())
    ins = lambda x, fill: np.insert(x, 1, fill, axis=0)
    actions, r, lp, tp, qv = ins(actions, 0.0), ins(r, 0.0), ins(lp, 1.0), ins(tp, 0.0), ins(qv, 0.0)
    ql, sv = np.sum(qv * actions, axis=2), np.sum(tp * qv, axis=2)
    ql_abs, sv_abs = np.sum(np.abs(qv * actions), axis=2), np.sum(np.abs(tp * qv), axis=2)
    ratio = np.sum(tp * actions, axis=2) / lp
    disc = np.power(gamma, np.arange(8, dtype=np.float64))
    ret, mag = S._returns(ratio, r, sv, ql, disc, flag, j_steps, sv_abs, ql_abs)
    return dict(ret=ret, ret_mag=mag)


def test_two_runs_give_the_same_bits(backend):
    d = _page(_ragged(300, 20, 8), 5, 8)
    js, s = _magic_j_steps(max(d["lengths"])), _subsets(300)
    a, b = _run(backend, d, 0.95, True, js, s), _run(backend, d, 0.95, True, js, s)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    C = a[1][25 + 25:25 + 25 + 625].reshape(25, 25)
    assert np.array_equal(C, C.T)


def test_invalid_arguments(backend):
    import reagent_amd._lib as L

    lib = L.lib()
    dev = backend.device
    d = _page([2, 3, 4, 1], 3, 2)
    N, A, E, T = 10, 3, 4, 4
    t = {k: d[k].to(dev) for k in ("prop", "mask", "values", "lp", "r", "offsets")}
    good = dict(prop=L.ptr(t["prop"]), mask=L.ptr(t["mask"]), values=L.ptr(t["values"]), ld_mv=A, lp=L.ptr(t["lp"]),
                r=L.ptr(t["r"]), ld_r=1, offsets=L.ptr(t["offsets"]), N=N, A=A, E=E, T=T, js=[3, -1, 1], so=[0, 2, 4])

    def call(**kw):
        a = dict(good, **kw)
        js, so = a["js"], a["so"]
        J = a.get("J", len(js) if js is not None else 3)
        G = a.get("G", len(so) - 1 if so is not None else 2)
        nbytes = int(lib.rg_cpe_wsdr_workspace_bytes(N, E, T, 3, 2))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        ret = torch.empty(4, E, dtype=torch.float64, device=dev)
        out = torch.empty(3 + 2 + 9 + 1, dtype=torch.float64, device=dev)
        c_js = (ctypes.c_int32 * len(js))(*js) if js is not None else None
        c_so = (ctypes.c_int32 * len(so))(*so) if so is not None else None
        p = lambda c: ctypes.cast(c, ctypes.c_void_p) if c is not None else None
        return lib.rg_cpe_wsdr(a["prop"], a["mask"], a["values"], a["ld_mv"], a["lp"], a["r"], a["ld_r"], a["offsets"], a["N"],
                               a["A"], a["E"], a["T"], 0.9, 1, p(c_js), J, p(c_so), G,
                               None if a.get("no_ws") else L.ptr(ws), a.get("ws_bytes", nbytes),
                               None if a.get("no_ret") else L.ptr(ret), None if a.get("no_out") else L.ptr(out), L.stream_ptr())

    assert call() == 0
    for k in ("prop", "mask", "values", "lp", "r", "offsets"):
        assert call(**{k: None}) == EINVAL, k
    for kw in (dict(js=None), dict(so=None), dict(no_ws=True), dict(no_ret=True), dict(no_out=True),
               dict(J=0), dict(J=33), dict(G=0), dict(G=33), dict(E=0), dict(N=0), dict(E=N + 1), dict(T=0), dict(T=N + 1),
               dict(A=0), dict(js=[3, -2, 1]), dict(js=[4, -1, 1]), dict(so=[0, 3, 2]), dict(so=[-1, 2, 4]), dict(so=[0, 2, 5]),
               dict(ld_mv=A - 1), dict(ld_r=0), dict(ws_bytes=8)):
        assert call(**kw) == EINVAL, kw
    assert lib.rg_cpe_wsdr_workspace_bytes(0, 1, 1, 1, 0) == 0 and lib.rg_cpe_wsdr_workspace_bytes(N, E, T, 33, 2) == 0
    assert lib.rg_cpe_wsdr_workspace_bytes(N, E, T, 2, 0) == 0 and lib.rg_cpe_wsdr_workspace_bytes(N, E, T, 1, 0) > 0
    from reagent_amd import ops

    with pytest.raises(L.ReagentHipError, match="rg_cpe_wsdr does not take"):
        ops.cpe_wsdr(t["prop"], t["mask"], t["values"], t["lp"], t["r"], t["offsets"], T, 0.9, True, list(range(-1, 32)), [0, 4])
    with pytest.raises(L.ReagentHipError, match="rg_cpe_wsdr failed"):
        ops.cpe_wsdr(t["prop"], t["mask"], t["values"], t["lp"], t["r"], t["offsets"], T, 0.9, True, [T], None)


def test_abi_22_is_bound():
    import reagent_amd._lib as L

    assert L.ABI_VERSION == 22
    assert "rg_cpe_wsdr" in L.SIGNATURES and "rg_cpe_wsdr_workspace_bytes" in L.SIGNATURES


def test_cpe_wsdr_kernels_have_no_scratch(tmp_path):
    """cpe_wsdr.hip compiled for gfx950 with the resource remarks on: seven kernels, no scratch, no spilled register"""
    kernels = kernel_resources("cpe_wsdr.hip", tmp_path)
    names = ("wsdr_rows_kernel", "wsdr_cumprod_kernel", "wsdr_column_sums_kernel", "wsdr_column_totals_kernel",
             "wsdr_returns_kernel", "wsdr_sums_kernel", "wsdr_cov_kernel")
    for want in names:
        found = [k for k in kernels if want in k]
        assert len(found) == 1, (want, found)
        v = kernels[found[0]]
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 128, (want, v)
    assert len(kernels) == len(names), list(kernels)
