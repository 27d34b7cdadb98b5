"""rg_linucb_solve_blocked (reagent_amd/csrc/cb_solve.hip): the ridge solve of LinearRegressionUCB by a blocked Cholesky
route for every LinUCB width, against the statements tests/test_cb_deep_kernels.py holds rg_linucb_solve to (restated
here), on the interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24 throughout.

Float64 bound.  The fold is held BIT FOR BIT to the reference's fp32 operations on the CPU.  The inverse is held, relative
to the largest entry of the float64 inverse of the same fp32 A_extended, to max(4 e_ref, max(d, 8) 2^-23) where e_ref is
the error of torch's own CPU fp32 linalg.inv on that matrix.  coefs is held per entry to (d + 2) u sum_j |inv_ij b_j| of the
float64 product of the kernel's OWN inverse.  A twin run gives the same bits, and inv_avg_A is exactly symmetric.

Exact statement.  A = L L^T with L = D (I + E): D diagonal in {0.5, 1, 2, 4}, E integer in [-2, 2] and non-zero only in
rows >= s and columns < s (E^2 = 0), s off every block edge.  Then L is A's Cholesky factor, W = L^-1 = (I - E) D^-1 and
A^-1 = W^T W, every pivot is the square of a power of two, and every product the route forms is a multiple of 2^-5 whose
sums of absolute values stay below 2^19: every partial sum is exact in fp32 IN ANY ORDER, so the kernel's inverse and
coefficients equal the float64 ones bit for bit.  The preconditions are asserted from float64 alone.

What the exact statement sees that the bound may not (broken copies compiled for the interpreter, not committed; d = 129,
257 at s = 100): see profiles/NOTES_r18.md.
"""
import os

import pytest
import torch

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
F64 = torch.float64
EINVAL = -1
STATE = ("avg_A", "avg_b", "sum_weight", "num_obs", "cur_avg_A", "cur_avg_b", "cur_sum_weight", "cur_num_obs", "inv_avg_A",
         "coefs", "valid", "status")


def _state(d, dev):
    """LinearRegressionUCB's buffers as constructed, plus the status flag"""
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    return dict(avg_A=z(d, d), avg_b=z(d), sum_weight=torch.full((1,), 1e-5, device=dev),
                num_obs=torch.zeros(1, dtype=torch.int64, device=dev), cur_avg_A=z(d, d), cur_avg_b=z(d),
                cur_sum_weight=torch.full((1,), 1e-5, device=dev), cur_num_obs=torch.zeros(1, dtype=torch.int64, device=dev),
                inv_avg_A=z(d, d), coefs=z(d), valid=-torch.ones(d, d, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev))


_WORKSPACES = {}


def _workspace(d, dev):
    """one workspace per (d, device), filled with NaNs before every call: the route may rely on nothing left in it"""
    from reagent_amd import ops

    key = (d, str(dev))
    if key not in _WORKSPACES:
        _WORKSPACES[key] = ops.linucb_solve_blocked_workspace(d, dev)
    ws = _WORKSPACES[key]
    ws.view(torch.float32).fill_(float("nan"))
    return ws


def _solve(st, lam):
    from reagent_amd import ops

    d = st["avg_A"].shape[0]
    ops.linucb_solve_blocked(lam, *[st[k] for k in STATE], _workspace(d, st["avg_A"].device))


def _accumulate_rows(st, x, y, w):
    from reagent_amd import ops

    dev = st["avg_A"].device
    B, d = x.shape
    ops.linucb_accumulate(x.to(dev), y.to(dev), w.to(dev), st["cur_avg_A"], st["cur_avg_b"], st["cur_sum_weight"],
                          st["cur_num_obs"], ops.linucb_workspace(B, d, dev))


def _accumulate(st, B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d, generator=g)
    x[:, 0] = 1.0  # the ones column of mlp_out_with_ones
    y, w = torch.randn(B, generator=g), 0.5 + torch.rand(B, generator=g)
    _accumulate_rows(st, x, y, w)


def _fold_statement(st, lam):
    """linear_regression.py:157-199 in torch fp32 on the CPU -> the folded buffers and A_extended"""
    c = {k: v.detach().cpu().clone() for k, v in st.items()}
    total = c["cur_sum_weight"].clone() + c["sum_weight"]
    avg_A = (c["avg_A"] * c["sum_weight"] + c["cur_avg_A"] * c["cur_sum_weight"]) / total
    avg_b = (c["avg_b"] * c["sum_weight"] + c["cur_avg_b"] * c["cur_sum_weight"]) / total
    sum_weight = c["sum_weight"] + c["cur_sum_weight"]
    ext = avg_A + lam * torch.eye(avg_A.shape[0]) / sum_weight
    want = dict(avg_A=avg_A, avg_b=avg_b, sum_weight=sum_weight, num_obs=c["num_obs"] + c["cur_num_obs"], valid=avg_A,
                cur_avg_A=torch.zeros_like(avg_A), cur_avg_b=torch.zeros_like(avg_b), cur_sum_weight=torch.zeros(1),
                cur_num_obs=torch.zeros(1, dtype=torch.int64))
    return want, ext


def _check_solve(st, lam, what):
    d = st["avg_A"].shape[0]
    twin = {k: v.clone() for k, v in st.items()}
    want, ext = _fold_statement(st, lam)
    _solve(st, lam)
    for k, v in want.items():
        assert torch.equal(st[k].cpu(), v), (what, k)
    assert st["status"].item() == 0, what
    inv64 = torch.linalg.inv(ext.double())
    scale = inv64.abs().max()
    e_ref = ((torch.linalg.inv(ext).double() - inv64).abs().max() / scale).item()
    tol = max(4 * e_ref, max(d, 8) * 2.0 ** -23)
    got32 = st["inv_avg_A"].cpu()
    got = got32.double()
    err = ((got - inv64).abs().max() / scale).item()
    print(what, f"inverse {err:.3e} of {tol:.3e}: ratio {err / tol:.3f} (torch fp32 {e_ref:.3e}, "
                f"cond {torch.linalg.cond(ext.double()).item():.1f})")
    assert err <= tol, (what, err, tol)
    assert torch.equal(got32, got32.T), what
    b64 = want["avg_b"].double()
    bound = (d + 2) * U * (got.abs() @ b64.abs())
    assert ((st["coefs"].cpu().double() - got @ b64).abs() <= bound).all(), what
    _solve(twin, lam)
    assert all(torch.equal(st[k], twin[k]) for k in st), what


def _device():
    """the product path alone, for the d = 512 cases the interpreter would take a minute over: they run under `-m gpu`"""
    import reagent_amd._lib as L

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    L.lib()
    return "cuda"


def _three_states(dev, d):
    """the state as constructed; as an accumulate on B = 4 d + 37 rows (with a ones column) left it; and the same again on
    top of the averages the first solve folded (avg_A, avg_b, sum_weight no longer trivial)"""
    lam = 0.5 if d in (33, 160) else 1.0
    st = _state(d, dev)
    _check_solve(st, lam, (d, lam, "constructed"))
    st = _state(d, dev)
    _accumulate(st, 4 * d + 37, d, 10 * d)
    _check_solve(st, lam, (d, lam, "one batch"))
    assert st["num_obs"].item() == 4 * d + 37
    _accumulate(st, 4 * d + 37, d, 10 * d + 1)
    _check_solve(st, lam, (d, lam, "second batch"))
    assert st["num_obs"].item() == 2 * (4 * d + 37)


# one block below, at and above each block edge the route has (32 k), a last block of a single row (33, 65, 129, 257, 385),
# rg_linucb_solve's own limit and the first width past it
@pytest.mark.parametrize("d", [1, 31, 32, 33, 65, 128, 129, 160, 257, 385])
def test_fold_is_exact_and_the_inverse_within_the_references_error(backend, d):
    _three_states(backend.device, d)


@pytest.mark.gpu
def test_fold_is_exact_and_the_inverse_within_the_references_error_at_512():
    _three_states(_device(), 512)


def _hard_features(kind, B, d, seed):
    """[B, d] features with a ones column, of the kinds a trained MLP's last layer hands the solve: `dead` every third
    column exactly zero behind a ReLU; `correlated` every column a common base plus 3 % noise; `scaled` the columns scaled
    over four decades"""
    g = torch.Generator().manual_seed(seed)
    if kind == "dead":
        x = torch.relu(torch.randn(B, d, generator=g))
        x[:, 2::3] = 0.0
    elif kind == "correlated":
        x = torch.randn(B, 1, generator=g) + 0.03 * torch.randn(B, d, generator=g)
    else:
        x = torch.randn(B, d, generator=g) * torch.logspace(-2, 2, d)
    x[:, 0] = 1.0
    return x, torch.randn(B, generator=g)


def _hard_case(dev, d, kind):
    """B = 4 d + 37 rows of weight 50, l2_reg_lambda = 1: ill-conditioned A_extended.  _check_solve as it stands."""
    B = 4 * d + 37
    x, y = _hard_features(kind, B, d, 100 * d + len(kind))
    st = _state(d, dev)
    _accumulate_rows(st, x, y, torch.full((B,), 50.0))
    if kind == "dead":
        assert not st["cur_avg_A"][2].any() and not st["cur_avg_A"][:, 2].any()
    _check_solve(st, 1.0, (d, kind))
    assert st["num_obs"].item() == B


@pytest.mark.parametrize("kind", ["dead", "correlated", "scaled"])
@pytest.mark.parametrize("d", [129, 257, 385])
def test_dead_correlated_and_badly_scaled_columns(backend, d, kind):
    _hard_case(backend.device, d, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dead", "correlated", "scaled"])
def test_dead_correlated_and_badly_scaled_columns_at_512(kind):
    _hard_case(_device(), 512, kind)


def _exact_case(d, s, seed):
    """-> A, b (fp32) and the float64 L, W, W^T W, W^T W b of the module docstring, with the preconditions asserted"""
    g = torch.Generator().manual_seed(seed)
    D = torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=F64)[torch.randint(0, 4, (d,), generator=g)]
    E = torch.zeros(d, d, dtype=F64)
    E[s:, :s] = torch.randint(-2, 3, (d - s, s), generator=g).double()
    eye = torch.eye(d, dtype=F64)
    Lf = D[:, None] * (eye + E)
    W = (eye - E) / D[None, :]
    A, inv = Lf @ Lf.T, W.T @ W
    b = torch.randint(-1, 2, (d,), generator=g).double()
    assert torch.equal(Lf @ W, eye) and torch.equal(torch.linalg.cholesky(A), Lf)
    grid = lambda t: bool(((t * 16) == (t * 16).round()).all()) and t.abs().max().item() < 2.0 ** 20  # noqa: E731
    assert grid(Lf) and grid(W) and grid(inv) and grid(A) and grid(inv.abs() @ b.abs())
    # every product of two factors is a multiple of 2^-5 (L of 2^-1, W of 2^-2 at the least), and no sum of absolute
    # values the route can form reaches 2^19: partial sums of at most 24 significant bits, exact in any order
    assert bool(((Lf * 2) == (Lf * 2).round()).all()) and bool(((W * 4) == (W * 4).round()).all())
    for prod in (Lf.abs() @ Lf.abs().T, Lf.abs() @ W.abs(), W.abs() @ (Lf.abs() @ W.abs()), W.abs().T @ W.abs()):
        assert prod.max().item() < 2.0 ** 19
    assert A.abs().max().item() + (Lf.abs() @ Lf.abs().T).max().item() < 2.0 ** 19
    return A.float(), b.float(), inv, inv @ b


@pytest.mark.parametrize("d,s", [(129, 100), (257, 100), (512, 200)])
def test_exact_statement_on_a_matrix_whose_cholesky_route_is_exact_in_fp32(backend, d, s):
    dev = backend.device
    A, b, inv64, coefs64 = _exact_case(d, s, 7 * d)
    assert s % 32 != 0 and torch.equal(A.double() @ inv64, torch.eye(d, dtype=F64))
    st = _state(d, dev)
    st["sum_weight"].zero_()
    st["cur_sum_weight"].fill_(1.0)
    st["cur_avg_A"].copy_(A)
    st["cur_avg_b"].copy_(b)
    _solve(st, 0.0)
    assert torch.equal(st["avg_A"].cpu(), A) and torch.equal(st["avg_b"].cpu(), b) and st["status"].item() == 0
    assert torch.equal(st["inv_avg_A"].cpu().double(), inv64)
    assert torch.equal(st["coefs"].cpu().double(), coefs64)


@pytest.mark.parametrize("d", [129, 257])
def test_a_pivot_that_is_not_positive_is_flagged_and_the_call_returns(backend, d):
    """l2_reg_lambda = 0 and a rank-one avg_A: a legal input.  The fold is still exact, the flag is set and stays set
    through a later clean solve (sticky), which never writes it"""
    dev = backend.device
    st = _state(d, dev)
    v = torch.randn(d, generator=torch.Generator().manual_seed(d))
    st["cur_avg_A"].copy_(torch.outer(v, v))
    st["cur_sum_weight"].fill_(20.0)
    want, _ = _fold_statement(st, 0.0)
    _solve(st, 0.0)
    assert st["status"].item() == 1
    for k, val in want.items():
        assert torch.equal(st[k].cpu(), val), k
    _accumulate(st, 4 * d + 37, d, d)
    want, _ = _fold_statement(st, 1.0)
    _solve(st, 1.0)  # a good solve on the same state: the flag stays
    assert st["status"].item() == 1 and torch.isfinite(st["inv_avg_A"]).all()
    for k, val in want.items():
        assert torch.equal(st[k].cpu(), val), k
    neg = _state(d, dev)
    neg["cur_avg_A"].copy_(-torch.eye(d))
    neg["cur_sum_weight"].fill_(20.0)
    _solve(neg, 0.0)
    assert neg["status"].item() == 1


def test_bad_arguments_are_refused(backend):
    import reagent_amd._lib as L

    lib, dev, p = L.lib(), backend.device, L.ptr
    d = 40
    st = _state(d, dev)
    need = lib.rg_linucb_solve_blocked_workspace_bytes(d)
    assert need == 3 * 64 * 64 * 4 and lib.rg_linucb_solve_blocked_workspace_bytes(512) == 3 * 512 * 512 * 4
    assert lib.rg_linucb_solve_blocked_workspace_bytes(1) == 3 * 32 * 32 * 4
    for dim in (0, -3, 513):
        assert lib.rg_linucb_solve_blocked_workspace_bytes(dim) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    before = {k: v.clone() for k, v in st.items()}

    def solve(dim=d, nbytes=need, workspace=True, **null):
        return lib.rg_linucb_solve_blocked(dim, 1.0, *[None if k in null else p(st[k]) for k in STATE],
                                           p(ws) if workspace else None, nbytes, None)

    assert solve(dim=0) == EINVAL and solve(dim=-3) == EINVAL and solve(dim=513) == EINVAL
    for k in STATE:
        assert solve(**{k: True}) == EINVAL, k
    assert solve(workspace=False) == EINVAL and solve(nbytes=need - 1) == EINVAL and solve(nbytes=0) == EINVAL
    assert all(torch.equal(st[k], before[k]) for k in st) and not ws.any()  # nothing ran
    assert solve() == 0 and st["status"].item() == 0 and st["cur_sum_weight"].item() == 0.0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cb_solve_kernels_have_no_scratch(tmp_path):
    """cb_solve.hip compiled for gfx950 with the resource remarks on: no scratch, no spilled register (the substitution
    keeps its column of W_kk in registers under compile-time indices), and the LDS the file declares"""
    kernels = kernel_resources("cb_solve.hip", tmp_path)
    for want in ("linucb_blocked_fold_kernel", "linucb_blocked_column_kernel", "linucb_blocked_inverse_kernel",
                 "linucb_blocked_finish_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, list(kernels))
    assert len(kernels) == 4
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        lds = {"column": (4 * 32 * 32 + 4 * 32 * 33) * 4, "inverse": 4 * 32 * 32 * 4}
        assert v["LDS Size [bytes/block]"] == next((n for key, n in lds.items() if key in k), 0), (k, v)
