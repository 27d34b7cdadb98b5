"""rg_linucb_solve and rg_drlinucb_head (reagent_amd/csrc/cb_deep.hip) against torch statements of the reference's formulas
(reagent/models/linear_regression.py:157-199, reagent/models/deep_represent_linucb.py:136-165,
reagent/training/cb/deep_represent_linucb_trainer.py:81-89), on the interpreter and, under `-m gpu`, on the MI355X.
u = 2^-24 throughout.

Solve.  The fold is held BIT FOR BIT to the reference's fp32 operations on the CPU.  The inverse is held, relative to the
largest entry of the float64 inverse of the same fp32 A_extended, to max(4 e_ref, max(d, 8) 2^-23) where e_ref is the error
of torch's own CPU fp32 linalg.inv on that matrix (4: the elimination order differs).  coefs is held per entry to
(d + 2) u sum_j |inv_ij b_j| of the float64 product of the kernel's OWN inverse.

Head.  The float64 statement under autograd; fp32 bounds for ANY summation order, per row r:
    e_lin = (h + 3) u sum_j |z_j v_j|
    e_p   = e_lin * max|act'| + 4 u |p|                                   (max|act'| = 1 linear, 1/4 sigmoid)
    e_row = w (|d loss_r / d p| e_p + e_p^2) + 16 u |row_loss|           (mse: 2 |p - y|, mae: 1, bce: |p - y| / (p (1 - p)))
    e_dlin = (w / B) c e_p + 16 u |dlin|          (c = 2 mse; 0 mae, whose sign is exact for |p - y| > e_p; 1 bce + sigmoid,
                                                   where g * act' = p - y)
    loss: sum_r e_row / B + (B + 2) u sum_r |row_loss| / B;   dmlp_out[r, j]: e_dlin |v_j| + 2 u |dmlp_out|
    dv[c]: sum_r e_dlin |z_rc| + (B + 2) u sum_r |dlin_r z_rc|
"""
import os

import pytest
import torch
import torch.nn.functional as Fn

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
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


def _solve(st, lam):
    from reagent_amd import ops

    ops.linucb_solve(lam, *[st[k] for k in STATE])


def _accumulate(st, B, d, seed):
    from reagent_amd import ops

    dev = st["avg_A"].device
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d, generator=g)
    x[:, 0] = 1.0  # the ones column of mlp_out_with_ones
    y, w = torch.randn(B, generator=g), 0.5 + torch.rand(B, generator=g)
    ops.linucb_accumulate(x.to(dev), y.to(dev), w.to(dev), st["cur_avg_A"], st["cur_avg_b"], st["cur_sum_weight"],
                          st["cur_num_obs"], ops.linucb_workspace(B, d, dev))


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
    got = st["inv_avg_A"].cpu().double()
    err = ((got - inv64).abs().max() / scale).item()
    print(what, f"inverse {err:.3e} of {tol:.3e} (torch fp32 {e_ref:.3e}, cond {torch.linalg.cond(ext.double()).item():.1f})")
    assert err <= tol, (what, err, tol)
    b64 = want["avg_b"].double()
    bound = (d + 2) * U * (got.abs() @ b64.abs())
    assert ((st["coefs"].cpu().double() - got @ b64).abs() <= bound).all(), what
    _solve(twin, lam)
    assert all(torch.equal(st[k], twin[k]) for k in st), what


@pytest.mark.parametrize("d", [1, 2, 6, 31, 32, 33, 64, 65, 128])
def test_solve_fold_is_exact_and_the_inverse_within_the_references_error(backend, d):
    """the state as constructed; as an accumulate on B = 4 d + 37 rows (with a ones column) left it; and the same again on
    top of the averages the first solve folded (avg_A, avg_b, sum_weight no longer trivial)"""
    dev = backend.device
    for lam in (1.0, 0.5):
        st = _state(d, dev)
        _check_solve(st, lam, (d, lam, "constructed"))
        st = _state(d, dev)
        _accumulate(st, 4 * d + 37, d, 10 * d)
        _check_solve(st, lam, (d, lam, "one batch"))
        assert st["num_obs"].item() == 4 * d + 37
        _accumulate(st, 4 * d + 37, d, 10 * d + 1)
        _check_solve(st, lam, (d, lam, "second batch"))
        assert st["num_obs"].item() == 2 * (4 * d + 37)


def _hard_features(kind, B, d, seed):
    """[B, d] features with a ones column, of the kinds a trained MLP's last layer hands the solve (an elimination without
    pivoting): `dead` every third column exactly zero behind a ReLU; `correlated` every column a common base plus 3 %
    noise; `scaled` the columns scaled over four decades"""
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


@pytest.mark.parametrize("kind", ["dead", "correlated", "scaled"])
@pytest.mark.parametrize("d", [6, 33, 65, 128])
def test_solve_on_dead_correlated_and_badly_scaled_columns(backend, d, kind):
    """B = 4 d + 37 rows of weight 50, l2_reg_lambda = 1: ill-conditioned A_extended (cond up to 10^8).  _check_solve as it
    stands: the fold bit-exact, status 0, the inverse within max(4 e_ref, max(d, 8) 2^-23) of torch's own fp32 inverse."""
    from reagent_amd import ops

    dev = backend.device
    B = 4 * d + 37
    x, y = _hard_features(kind, B, d, 100 * d + len(kind))
    st = _state(d, dev)
    ops.linucb_accumulate(x.to(dev), y.to(dev), torch.full((B,), 50.0, device=dev), st["cur_avg_A"], st["cur_avg_b"],
                          st["cur_sum_weight"], st["cur_num_obs"], ops.linucb_workspace(B, d, dev))
    if kind == "dead":
        assert not st["cur_avg_A"][2].any() and not st["cur_avg_A"][:, 2].any()
    _check_solve(st, 1.0, (d, kind))
    assert st["num_obs"].item() == B


@pytest.mark.parametrize("d", [6, 33])
def test_solve_flags_a_pivot_that_is_not_positive_and_returns(backend, d):
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
    clean = _state(d, dev)
    clean["status"].fill_(1)
    _solve(clean, 1.0)
    assert clean["status"].item() == 1 and torch.isfinite(clean["inv_avg_A"]).all()
    neg = _state(d, dev)
    neg["cur_avg_A"].copy_(-torch.eye(d))
    neg["cur_sum_weight"].fill_(20.0)
    _solve(neg, 0.0)
    assert neg["status"].item() == 1


ACT_OF = {"mse": "linear", "mae": "linear", "cross_entropy": "sigmoid"}


def _head_inputs(B, h, loss, weighted, dev, seed):
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(B, h + 3, generator=g)
    v = torch.randn(h + 1, generator=g) / (h + 1) ** 0.5
    mlp = wide[:, :h]
    lin = v[0] + mlp @ v[1:]
    p = torch.sigmoid(lin) if loss == "cross_entropy" else lin
    if loss == "cross_entropy":
        y = torch.rand(B, generator=g)
    else:  # no residual within 0.01 of mae's kink
        y = p + (0.01 + torch.rand(B, generator=g)) * torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    w = (0.5 + torch.rand(B, generator=g)) if weighted else None
    wide = wide.to(dev)
    return wide[:, :h], v.to(dev), y.to(dev), None if w is None else w.to(dev)


def _run_head(mlp, v, y, w, loss, with_dv=True):
    import reagent_amd._lib as L
    from reagent_amd import ops

    B, h = mlp.shape
    dev = mlp.device
    P = ops.drlinucb_head_partials(B, h)
    o = dict(z=torch.full((B, h + 1), -7.0, device=dev), lin=torch.full((B,), -7.0, device=dev),
             pred=torch.full((B,), -7.0, device=dev), row_loss=torch.full((B,), -7.0, device=dev),
             dmlp=torch.full((B, h + 2), -7.0, device=dev), loss=torch.full((1,), -7.0, device=dev),
             dv=torch.full((h + 1,), -7.0, device=dev), lp=torch.full((P,), -7.0, device=dev),
             dvp=torch.full((P * (h + 1),), -7.0, device=dev))
    ops.drlinucb_head(mlp, v, L.ACT[ACT_OF[loss]], o["z"], o["lin"], o["pred"], label=y, weight=w, loss_type=L.CB_LOSS[loss],
                      row_loss=o["row_loss"], dmlp_out=o["dmlp"][:, :h], loss_partials=o["lp"],
                      dv_partials=o["dvp"] if with_dv else None, loss=o["loss"], dv=o["dv"] if with_dv else None)
    return o


def _head_statement(mlp, v, y, w, loss):
    m = mlp.detach().cpu().double().requires_grad_()
    v64 = v.detach().cpu().double().requires_grad_()
    y64 = y.cpu().double()
    B = m.shape[0]
    w64 = torch.ones(B, dtype=F64) if w is None else w.cpu().double()
    z = torch.cat([torch.ones(B, 1, dtype=F64), m], 1)
    lin = z @ v64
    p = torch.sigmoid(lin) if loss == "cross_entropy" else lin
    fn = {"mse": Fn.mse_loss, "mae": Fn.l1_loss, "cross_entropy": Fn.binary_cross_entropy}[loss]
    rows = fn(p, y64, reduction="none") * w64
    total = rows.sum() / B
    total.backward()
    return dict(z=z.detach(), lin=lin.detach(), p=p.detach(), rows=rows.detach(), loss=total.detach(), dm=m.grad, dv=v64.grad,
                w=w64, y=y64, v=v64.detach())


@pytest.mark.parametrize("h", [1, 5, 31, 32, 64, 129])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_head_against_float64_autograd(backend, B, h):
    dev = backend.device
    for loss in ("mse", "mae", "cross_entropy"):
        for weighted in (False, True):
            what = (B, h, loss, weighted)
            mlp, v, y, w = _head_inputs(B, h, loss, weighted, dev, 1000 * B + 10 * h + weighted)
            assert mlp.stride(0) == h + 3  # (a leading dimension that is not the width)
            o = _run_head(mlp, v, y, w, loss)
            s = _head_statement(mlp, v, y, w, loss)
            z, p64, diff = s["z"], s["p"], s["p"] - s["y"]
            assert torch.equal(o["z"].cpu(), torch.cat([torch.ones(B, 1), mlp.cpu()], 1)), what
            e_lin = (h + 3) * U * (z.abs() @ s["v"].abs())
            assert ((o["lin"].cpu().double() - s["lin"]).abs() <= e_lin).all(), what
            slope = 0.25 if loss == "cross_entropy" else 1.0
            e_p = e_lin * slope + 4 * U * p64.abs()
            assert ((o["pred"].cpu().double() - p64).abs() <= e_p).all(), what
            if loss == "mse":
                dl_dp, c = 2 * diff.abs(), 2.0
            elif loss == "mae":
                dl_dp, c = torch.ones(B, dtype=F64), 0.0
                assert (diff.abs() > e_p).all()
            else:
                dl_dp, c = diff.abs() / (p64 * (1 - p64)), 1.0
            e_row = s["w"] * (dl_dp * e_p + e_p ** 2) + 16 * U * s["rows"].abs()
            assert ((o["row_loss"].cpu().double() - s["rows"]).abs() <= e_row).all(), what
            e_loss = e_row.sum() / B + (B + 2) * U * s["rows"].abs().sum() / B
            assert abs(o["loss"].item() - s["loss"].item()) <= e_loss.item() + 2 * U * abs(s["loss"].item()), what
            # d loss / d lin of the statement: d loss / d mlp_out = dlin v[1:], so dlin = dv[0] taken per row
            dlin64 = {"mse": 2 * diff, "mae": torch.sign(diff), "cross_entropy": diff}[loss] * s["w"] / B
            e_dlin = s["w"] / B * c * e_p + 16 * U * dlin64.abs()
            dm = o["dmlp"][:, :h].cpu().double()
            assert ((dm - s["dm"]).abs() <= e_dlin[:, None] * s["v"][1:].abs()[None] + 2 * U * s["dm"].abs()).all(), what
            assert torch.equal(o["dmlp"][:, h:].cpu(), torch.full((B, 2), -7.0)), what  # nothing past the width
            e_dv = e_dlin @ z.abs() + (B + 2) * U * (dlin64.abs() @ z.abs())
            assert ((o["dv"].cpu().double() - s["dv"]).abs() <= e_dv).all(), what
            again = _run_head(mlp, v, y, w, loss)
            assert all(torch.equal(o[k], again[k]) for k in o), what
            if h in (5, 129) and weighted:  # dv not asked for: dv and its partials stay untouched, the rest the same bits
                lean = _run_head(mlp, v, y, w, loss, with_dv=False)
                assert torch.equal(lean["dv"], torch.full_like(lean["dv"], -7.0)) and (lean["dvp"] == -7.0).all()
                assert all(torch.equal(o[k], lean[k]) for k in ("z", "lin", "pred", "row_loss", "dmlp", "loss")), what


SATURATED_LIN = (-120, -100, -90, -40, -20, -17, -1, 0, 1, 16, 17, 18, 20, 40, 90, 120)


def _bce_statement(p, y, w):
    """F.binary_cross_entropy's row loss in float64 at a given prediction: both logs clamped at -100"""
    p, y, w = p.double(), y.double(), w.double()
    return -w * (y * torch.log(p).clamp_min(-100.0) + (1 - y) * torch.log1p(-p).clamp_min(-100.0))


def test_head_cross_entropy_where_the_sigmoid_saturates(backend):
    """h = 5 with one live column (v = e_1), so lin is the planted value exactly: SATURATED_LIN x y in {0, 1, 0.3}, weights
    on.  The clamps of both logs at -100 and of the backward's denominator at 1e-12 are reached (p = 0 and p = 1 in fp32).
    row_loss is held to 8 u |row_loss| + 2^-100 (the floor: a denormal product may be flushed) against the float64
    statement at the kernel's OWN fp32 pred_label, which keeps the error of lin and of the sigmoid out of the bound;
    torch's own fp32 F.binary_cross_entropy at that prediction is held to the same bound first.  In the tail this tells
    log1p(-p) from log(1 - p): at y = 0, lin = -20 the row loss is 2.06e-9 w, not 0.  dmlp_out is held to 8 u |value|
    against the fp32 backward of F.binary_cross_entropy on the CPU, taken at the same prediction."""
    dev, h = backend.device, 5
    lin = torch.tensor([float(v) for v in SATURATED_LIN for _ in range(3)])
    B = lin.shape[0]
    y = torch.tensor([0.0, 1.0, 0.3]).repeat(len(SATURATED_LIN))
    g = torch.Generator().manual_seed(3)
    w = 0.5 + torch.rand(B, generator=g)
    mlp = torch.randn(B, h, generator=g)
    mlp[:, 0] = lin
    v = torch.zeros(h + 1)
    v[1] = 1.0
    o = _run_head(mlp.to(dev), v.to(dev), y.to(dev), w.to(dev), "cross_entropy")
    assert torch.equal(o["lin"].cpu(), lin)
    p = o["pred"].cpu()
    assert (p == 0).any() and (p == 1).any() and ((p > 0) & (p < 2.0 ** -24)).any()  # both clamps, and the tail
    assert ((p.double() - torch.sigmoid(lin.double())).abs() <= 4 * U * torch.sigmoid(lin.double()) + 2.0 ** -126).all()
    want = _bce_statement(p, y, w)
    bound = 8 * U * want.abs() + 2.0 ** -100
    ref32 = (Fn.binary_cross_entropy(p, y, reduction="none") * w).double()
    assert ((ref32 - want).abs() <= bound).all()  # the bound is fair to the reference
    assert want.max().item() > 99.0 * 0.5  # a clamped log
    err = (o["row_loss"].cpu().double() - want).abs()
    print(f"drlinucb_head saturated bce: row_loss {(err / bound).max().item():.4f} of its bound")
    assert (err <= bound).all(), [(lin[i].item(), y[i].item(), o["row_loss"][i].item(), want[i].item())
                                  for i in torch.nonzero(err > bound).reshape(-1).tolist()]
    # the backward: d loss / d p in fp32 as torch takes it at the same p, through the sigmoid's p (1 - p) and v[1] = 1
    leaf = p.clone().requires_grad_()
    ((Fn.binary_cross_entropy(leaf, y, reduction="none") * w).sum() / B).backward()
    want_dm = leaf.grad * (p * (1 - p))
    dm = o["dmlp"][:, :h].cpu()
    gerr, gbound = (dm[:, 0].double() - want_dm.double()).abs(), 8 * U * want_dm.double().abs()
    print(f"drlinucb_head saturated bce: dmlp_out {(gerr / gbound.clamp_min(1e-300)).max().item():.4f} of its bound")
    assert (gerr <= gbound).all()
    assert torch.equal(dm[:, 1:], torch.zeros(B, h - 1)) and torch.isfinite(o["loss"]).all() and torch.isfinite(o["dv"]).all()
    assert (want_dm != 0).sum().item() >= 12  # (|lin| <= 17 at the least: the gradients held are not all zeros)


def test_head_mae_gradient_is_zero_where_the_residual_is(backend):
    """p - y exactly 0 on one row (row 1: lin = 2 through one live column, y = 2): its loss and its gradient are exactly 0,
    the neighbours' gradients are -+ w / B"""
    dev, h, B = backend.device, 5, 3
    mlp = torch.randn(B, h, generator=torch.Generator().manual_seed(7))
    mlp[:, 0] = 2.0
    v = torch.zeros(h + 1)
    v[1] = 1.0
    y, w = torch.tensor([2.5, 2.0, 1.5]), torch.tensor([0.75, 1.5, 1.25])
    o = _run_head(mlp.to(dev), v.to(dev), y.to(dev), w.to(dev), "mae")
    assert o["pred"].cpu().tolist() == [2.0, 2.0, 2.0]
    assert o["row_loss"].cpu().tolist() == [0.375, 0.0, 0.625]
    dm = o["dmlp"][:, :h].cpu()
    assert torch.equal(dm[1], torch.zeros(h)) and torch.equal(dm[:, 1:], torch.zeros(B, h - 1))
    assert torch.equal(dm[:, 0], torch.tensor([-1.0, 0.0, 1.0]) * (w * torch.tensor(1.0 / B)))


@pytest.mark.parametrize("B,h", [(1, 1), (65, 5), (257, 129)])
def test_head_without_a_label_writes_z_lin_and_pred_label_only(backend, B, h):
    import reagent_amd._lib as L

    dev = backend.device
    lib, p = L.lib(), L.ptr
    mlp, v, y, w = _head_inputs(B, h, "cross_entropy", True, dev, 5)
    full = _run_head(mlp, v, y, w, "cross_entropy")
    o = {k: torch.full_like(t, -7.0) for k, t in full.items()}
    rc = lib.rg_drlinucb_head(p(mlp), mlp.stride(0), p(v), None, p(w), L.ACT["sigmoid"], L.CB_LOSS["cross_entropy"], B, h,
                              p(o["z"]), p(o["lin"]), p(o["pred"]), p(o["row_loss"]), p(o["dmlp"]), h + 2, p(o["lp"]),
                              p(o["dvp"]), p(o["loss"]), p(o["dv"]), None)
    assert rc == 0
    for k in ("z", "lin", "pred"):
        assert torch.equal(o[k], full[k]), k
    for k in ("row_loss", "dmlp", "loss", "dv", "lp", "dvp"):
        assert (o[k] == -7.0).all(), k


@pytest.mark.parametrize("act", ["linear", "relu", "leaky_relu", "tanh", "sigmoid", "softplus"])
def test_every_output_activation_of_the_reference(backend, act):
    """all six names of ACTIVATION_MAP: pred_label and the gradient through the activation (mse), and the elementwise
    launch the scorer applies after rg_linucb_score"""
    import reagent_amd._lib as L
    from reagent_amd import ops

    dev = backend.device
    B, h = 65, 5
    mlp, v, y, w = _head_inputs(B, h, "mse", True, dev, 9)
    P = ops.drlinucb_head_partials(B, h)
    e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    z, lin, pred, rows, dm, loss, dv = e(B, h + 1), e(B), e(B), e(B), e(B, h), e(1), e(h + 1)
    ops.drlinucb_head(mlp, v, L.ACT[act], z, lin, pred, label=y, weight=w, loss_type=L.CB_LOSS["mse"], row_loss=rows,
                      dmlp_out=dm, loss_partials=e(P), dv_partials=e(P * (h + 1)), loss=loss, dv=dv)
    fn = {"linear": lambda t: t, "relu": torch.relu, "leaky_relu": Fn.leaky_relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
          "softplus": Fn.softplus}[act]
    m = mlp.cpu().double().requires_grad_()
    v64 = v.cpu().double().requires_grad_()
    p64 = fn(torch.cat([torch.ones(B, 1, dtype=F64), m], 1) @ v64)
    total = (((p64 - y.cpu().double()) ** 2) * w.cpu().double()).sum() / B
    total.backward()
    tol = 64 * U  # values of order 1, a handful of fp32 operations and one transcendental each
    assert (pred.cpu().double() - p64.detach()).abs().max() <= tol
    assert abs(loss.item() - total.item()) <= tol * max(1.0, abs(total.item()))
    assert (dm.cpu().double() - m.grad).abs().max() <= tol and (dv.cpu().double() - v64.grad).abs().max() <= tol
    a, b = lin.clone(), (lin + 1.0).contiguous()
    ops.drlinucb_activate(a, b, L.ACT[act])
    assert torch.equal(a, pred)
    assert (b.cpu().double() - fn((lin + 1.0).cpu().double())).abs().max() <= tol
    only = lin.clone()
    ops.drlinucb_activate(only, None, L.ACT[act])
    assert torch.equal(only, pred)


def test_bad_arguments_are_refused(backend):
    import reagent_amd._lib as L

    lib, dev, p = L.lib(), backend.device, L.ptr
    d = 4
    st = _state(d, dev)
    before = {k: v.clone() for k, v in st.items()}

    def solve(dim=d, **null):
        return lib.rg_linucb_solve(dim, 1.0, *[None if k in null else p(st[k]) for k in STATE], None)

    assert solve(dim=0) == EINVAL and solve(dim=129) == EINVAL and solve(dim=-3) == EINVAL
    for k in STATE:
        assert solve(**{k: True}) == EINVAL, k
    assert all(torch.equal(st[k], before[k]) for k in st)  # nothing ran
    B, h = 8, 3
    mlp, v, y, w = _head_inputs(B, h, "mse", True, dev, 1)
    o = _run_head(mlp, v, y, w, "mse")
    names = ("mlp", "v", "label", "weight", "z", "lin", "pred", "row_loss", "dmlp", "lp", "dvp", "loss", "dv")
    t = dict(o, mlp=mlp, v=v, label=y, weight=w)

    def head(B_=B, h_=h, ld=mlp.stride(0), ldd=h + 2, act=0, loss_code=0, **null):
        a = {k: (None if k in null else p(t[k])) for k in names}
        return lib.rg_drlinucb_head(a["mlp"], ld, a["v"], a["label"], a["weight"], act, loss_code, B_, h_, a["z"], a["lin"], a["pred"],
                                    a["row_loss"], a["dmlp"], ldd, a["lp"], a["dvp"], a["loss"], a["dv"], None)

    assert head() == 0 and head(weight=True) == 0 and head(dv=True) == 0 and head(dv=True, dvp=True) == 0
    assert head(B_=0) == EINVAL and head(h_=0) == EINVAL and head(h_=512) == EINVAL and head(ld=h - 1) == EINVAL
    assert head(ldd=h - 1) == EINVAL and head(act=6) == EINVAL and head(act=-1) == EINVAL and head(loss_code=3) == EINVAL
    for k in ("mlp", "v", "z", "lin", "pred", "row_loss", "dmlp", "lp", "loss", "dvp"):
        assert head(**{k: True}) == EINVAL, k
    assert head(label=True, row_loss=True, dmlp=True, lp=True, loss=True, dv=True, dvp=True) == 0  # forward only
    assert lib.rg_drlinucb_head_partials(0, 3) == 0 and lib.rg_drlinucb_head_partials(8, 0) == 0
    assert lib.rg_drlinucb_head_partials(8, 512) == 0 and lib.rg_drlinucb_head_partials(8, 511) == 1
    assert lib.rg_drlinucb_head_partials(257, 5) == 5 and lib.rg_drlinucb_head_partials(257, 4) == 2
    x = torch.zeros(4, device=dev)
    assert lib.rg_drlinucb_activate(p(x), None, 0, 1, None) == EINVAL and lib.rg_drlinucb_activate(None, None, 4, 1, None) == EINVAL
    assert lib.rg_drlinucb_activate(p(x), None, 4, 6, None) == EINVAL and lib.rg_drlinucb_activate(p(x), None, 4, 1, None) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cb_deep_kernels_have_no_scratch(tmp_path):
    """cb_deep.hip compiled for gfx950 with the resource remarks on: no scratch, no spilled register (the solve keeps its
    8 x 8 share of the matrix in registers under compile-time indices), and the LDS the header states"""
    kernels = kernel_resources("cb_deep.hip", tmp_path)
    for want, n in (("linucb_solve_kernel", 4), ("drlinucb_head_kernel", 4), ("drlinucb_finish_kernel", 1),
                    ("drlinucb_activate_kernel", 1)):
        assert sum(want in k for k in kernels) == n, (want, list(kernels))
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        if "solve" in k:
            assert v["LDS Size [bytes/block]"] == (2 * 2 + 1) * 128 * 4, v
