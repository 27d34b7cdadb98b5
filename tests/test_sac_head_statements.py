"""The continuous-control kernels of reagent_amd/csrc/sac.hip against the float64 statements of tests/sac_refs.py.

The Gaussian head is held in two stages, as the reference itself is staged (get_log_prob takes the fp32 squashed action):
  stage A   action and squashed mean against float64 clamp(tanh(loc + noise * exp(clamp(scale_log)))), to 4 ulp of 1;
  stage B   log_prob against float64 get_log_prob evaluated AT THE KERNEL'S OWN fp32 ACTION BITS;
  backward  float64 autograd through the whole chain (sampling and get_log_prob share (loc, scale_log)).
An end-to-end float64 log-prob would be the wrong yardstick at saturation: float64 tanh clamps at another point than fp32.

Inputs are constructed from a target raw = loc + noise * sigma, so that the strata are planted and not left to chance:
interior rows (|raw| <= 2.5), near-saturated rows (elements at |raw| in {3, 4, 5.5, 6.5}), clamped rows ({9, 20}; the band
6.9-7.7, where the fp32 and float64 clamp decisions can differ, is avoided), scale_log probes at exactly +-2, one fp32 step
outside, and far outside.

Every bound is self-calibrating (tests/test_lstm_kernels.py, tests/test_pg_kernels.py): 4 x the error of torch fp32 on the
same formula against the float64 statement, floor 4 fp32 ulp of the quantity.  For the head the torch fp32 error is taken
per element stratum (bins of w = 1 - a^2 + eps) from a pool of B = 4096, A = 8 of the same generator, evaluated with torch
only.  Backward outputs are elementwise and are held to their element's entry; a row's log-prob is held to
sum_d e(stratum(b, d)) + (A - 1) u sum_d |term_d|, u = 2^-24 (the fp32 bound of summing A terms in any order)."""
import math

import numpy as np
import pytest
import torch

import reagent_amd._lib as L
import sac_refs as R
from reagent_amd import ops

F32, F64 = torch.float32, torch.float64
U = 2.0**-24
SENTINEL = -777.25
NAN = float("nan")
A_MAX = R.A_MAX


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _report(what, got, ref64, own32, bound):
    """elementwise: |got - ref64| <= bound.  Prints the worst element: kernel error, torch fp32 error, bound, ratio."""
    ref64 = ref64.detach().double()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref64).reshape(-1)
    ref64 = ref64.reshape(-1)
    err = (got.detach().cpu().double().reshape(-1) - ref64).abs()
    own = (own32.detach().double().reshape(-1) - ref64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
    i = int(ratio.argmax()) if ratio.numel() else 0
    print(f"{what}: kernel error {err[i]:.3e}, torch fp32 error {own.max():.3e}, bound {bound[i]:.3e}, ratio {ratio[i]:.3f}")
    assert bool(torch.isfinite(got).all()) and float(ratio[i]) <= 1.0, (what, float(err[i]), float(bound[i]), float(own.max()))
    return float(ratio[i])


def _close(what, got, ref64, own32):
    """the rule of tests/test_lstm_kernels.py::_close on one tensor: max error against max(4 x torch's own, 4 ulp of max)"""
    ref64 = ref64.detach().double()
    own = (own32.detach().double() - ref64).abs().max().item()
    bound = max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item()))
    return _report(what, got, ref64, own32, bound)


# ---- the generator of section "inputs that make the strata" ----------------------------------------------------------------
NEAR, CLAMPED = [3.0, 4.0, 5.5, 6.5], [9.0, 20.0]
PLANTS = {"near": [(v, s) for v in NEAR for s in (1.0, -1.0)], "clamped": [(v, s) for v in CLAMPED for s in (1.0, -1.0)]}
STRATA = ["interior", "raw3", "raw4", "raw5.5", "raw6.5", "clamped"]
# w = 1 - a^2 + eps at the planted levels: >= 2.66e-2 | 9.87e-3 | 1.34e-3 | 6.78e-5 | 1.00e-5 | 3.03e-6; the edges lie between
W_EDGES = [1.6e-2, 3.6e-3, 3.0e-4, 2.6e-5, 5.5e-6]
_TWO_UP = float(np.nextafter(np.float32(2), np.float32(np.inf)))
PROBES = [2.0, -2.0, _TWO_UP, -_TWO_UP, 5.0, -7.0]  # exactly +-2 (gradient passes: clamp is inclusive), one step outside, far


def stratum(action):
    w = 1.0 - action.detach().cpu().double() ** 2 + R.EPS
    s = torch.zeros_like(w, dtype=torch.int64)
    for e in W_EDGES:
        s += (w <= e).long()
    return s


def rows_per_wg(A):
    return 256 // A if A <= 256 else 256  # the row-per-thread forms run 256 rows per workgroup


def row_plans(B, A):
    """The kinds of the rows of a (B, A) case.  Planted rows: the first and last row of the first workgroup, the first row of
    the second, the last row of the batch, then rows 1, 2, ... until all (level, sign) plants fit; they alternate near /
    clamped.  One row at least stays interior; where that leaves fewer than two planted rows, several plans cover the kinds."""
    rpw = rows_per_wg(A)
    need = 2 * -(-len(PLANTS["near"]) // A)
    P = {p for p in (0, rpw - 1, rpw, B - 1) if 0 <= p < B}
    b = 1
    while len(P) < need and b < B:
        P.add(b)
        b += 1
    P = sorted(P)
    if len(P) == B:
        P = P[:-1]
    if not P:
        return [["interior"], ["near"], ["clamped"]]
    plans = []
    for v in range(1 if len(P) >= 2 else 2):
        kinds = ["interior"] * B
        for i, p in enumerate(P):
            kinds[p] = ("near", "clamped")[(i + v) % 2]
        plans.append(kinds)
    return plans


def _spread(n, A):
    """n distinct columns of A, d = 0 and d = A - 1 among them"""
    return sorted({round(j * (A - 1) / (n - 1)) for j in range(n)}) if n > 1 else [0]


def make_case(B, A, seed, kinds):
    """fp32 inputs whose raw = loc + noise * exp(clamp(scale_log)) hits the planted targets"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, dtype=F64, generator=g) * 2 - 1  # noqa: E731
    raw, loc, sl = u(B, A) * 2.5, (u(B, A) * 1.5).float(), (u(B, A) * 2.5).float()
    ga, glp = torch.randn(B, A, generator=g), torch.randn(B, generator=g)
    plants, seen = [], {"near": 0, "clamped": 0}
    for b, kind in enumerate(kinds):
        if kind == "interior":
            continue
        table = PLANTS[kind]
        for j, d in enumerate(_spread(min(len(table), A), A)):
            v, s = table[(seen[kind] * A + j) % len(table)]
            raw[b, d] = v * s
            plants.append((b, d, v, s))
        seen[kind] += 1
    interior_rows = [b for b, k in enumerate(kinds) if k == "interior"]
    probes = []
    if interior_rows:
        if A >= len(PROBES):
            cells = [(interior_rows[0], d) for d in _spread(len(PROBES), A)]
        else:
            cells = [(b, d) for b in interior_rows[:len(PROBES)] for d in range(A)][:len(PROBES)]
        for (b, d), v in zip(cells, PROBES):
            sl[b, d] = v
            probes.append((b, d, v))
            if abs(glp[b]) < 0.5:  # d_scale_log there is g_lp (r^2 - 1) + ...: large enough to show that it passes
                glp[b] = 0.5 if glp[b] >= 0 else -0.5
    sigma = sl.double().clamp(R.LOG_PROB_MIN, R.LOG_PROB_MAX).exp()
    noise = ((raw - loc.double()) / sigma).float()
    return dict(B=B, A=A, ls=torch.cat([loc, sl], 1), noise=noise, ga=ga, glp=glp, kinds=kinds, plants=plants, probes=probes,
                seed=seed)


def shape_cases(B, A, seed=None):
    seed = 1000 * A + B if seed is None else seed
    return [make_case(B, A, seed + 7 * i, kinds) for i, kinds in enumerate(row_plans(B, A))]


def _head_shapes():
    out = []
    for A in (1, 3, 7, 64, 65, 128, 129, 255, 256):
        r = 256 // A
        out += [(B, A) for B in sorted({r - 1, r, r + 1, 2 * r + 1}) if B >= 1]
    return out + [(B, A) for A in (257, 300) for B in (1, 255, 256, 257)]


HEAD_SHAPES = _head_shapes()
EMU_COST_LIMIT = 200_000  # threads x elements a thread loops over, per launch: what the interpreter takes in about a second
assert all(B * A <= EMU_COST_LIMIT for B, A in HEAD_SHAPES)  # (the cost rule: every head shape runs on the interpreter too)


# ---- calibration: torch fp32 against float64 on the pool, per element stratum ---------------------------------------------
_TABLES = None


def tables():
    """-> dict(lp, d_loc, d_sl: one entry per stratum, = max(4 x torch fp32 error, 4 ulp of the largest magnitude there),
    own_*: the raw torch fp32 errors, n: elements per stratum).  No kernel is launched."""
    global _TABLES
    if _TABLES is None:
        B, A = 4096, 8
        kinds = ["interior"] * B
        for i in range(0, B, 4):
            kinds[i] = ("near", "clamped")[(i // 4) % 2]
        c = make_case(B, A, 20240, kinds)
        a32, _ = R.gaussian_forward_ref(c["ls"], c["noise"], F32)
        _, t32 = R.gaussian_log_prob_ref(c["ls"], a32, F32)
        _, t64 = R.gaussian_log_prob_ref(c["ls"], a32, F64)   # stage B: float64 at the SAME fp32 action
        g32, _, _ = R.gaussian_backward_ref(c["ls"], c["noise"], c["ga"], c["glp"], dtype=F32)
        g64, a64, _ = R.gaussian_backward_ref(c["ls"], c["noise"], c["ga"], c["glp"], dtype=F64)
        s_b, s_g = stratum(a32), stratum(a64)
        T = {k: [] for k in ("lp", "d_loc", "d_sl", "own_lp", "own_d_loc", "own_d_sl", "n")}
        for i in range(len(STRATA)):
            for name, got, ref, s in (("lp", t32, t64, s_b), ("d_loc", g32[:, :A], g64[:, :A], s_g),
                                      ("d_sl", g32[:, A:], g64[:, A:], s_g)):
                m = s == i
                assert int(m.sum()) >= 256, (STRATA[i], int(m.sum()))
                own = (got.double() - ref)[m].abs().max().item()
                T["own_" + name].append(own)
                T[name].append(max(4.0 * own, 4.0 * _ulp(ref[m].abs().max().item())))
            T["n"].append(int((s_g == i).sum()))
        for k in ("lp", "d_loc", "d_sl"):
            print(f"pool {k}: " + ", ".join(f"{n} own {o:.3e} bound {e:.3e}" for n, o, e in zip(STRATA, T["own_" + k], T[k])))
        _TABLES = {k: torch.tensor(v, dtype=F64) if k != "n" else v for k, v in T.items()}
    return _TABLES


# ---- the two runners: the kernels, and torch fp32 on the same formula -------------------------------------------------------
def _wide(t, dev, pad=NAN, left=1, right=2):
    """t as a column view of a wider matrix (as self._xa[:, S:] is) -> (view, the wide matrix)"""
    w = torch.full((t.shape[0], t.shape[1] + left + right), pad, dtype=t.dtype, device=dev)
    w[:, left:left + t.shape[1]] = t.to(dev)
    return w[:, left:left + t.shape[1]], w


def _pads_untouched(wide, left, width):
    pads = torch.cat([wide[:, :left], wide[:, left + width:]], 1).cpu()
    return bool((pads == SENTINEL).all())


class KernelRunner:
    def __init__(self, dev):
        self.dev = dev

    def forward(self, ls, noise, want_lp=True, want_sm=True):
        B, A = noise.shape
        lsv, _ = _wide(ls, self.dev)
        act, act_w = _wide(torch.full((B, A), SENTINEL), self.dev, pad=SENTINEL)
        lp = torch.full((B,), NAN, device=self.dev) if want_lp else None
        sm = torch.full((B, A), NAN, device=self.dev) if want_sm else None
        ops.gaussian_head_forward(lsv, noise.to(self.dev), act, lp, sm)
        assert _pads_untouched(act_w, 1, A), "the forward wrote outside the action columns"
        return act.cpu().contiguous(), lp.cpu() if want_lp else None, sm.cpu() if want_sm else None

    def log_prob(self, ls, action):
        lsv, _ = _wide(ls, self.dev)
        av, _ = _wide(action, self.dev, left=2, right=1)
        lp = torch.full((action.shape[0],), NAN, device=self.dev)
        ops.gaussian_log_prob(lsv, av, lp)
        return lp.cpu()

    def backward(self, ls, noise, ga, glp, kld_coef=None, kld_on_mean=False):
        B, A = noise.shape
        lsv, _ = _wide(ls, self.dev)
        gav = _wide(ga, self.dev, left=3, right=1)[0] if ga is not None else None
        d, d_w = _wide(torch.full((B, 2 * A), SENTINEL), self.dev, pad=SENTINEL, left=2, right=3)
        ops.gaussian_head_backward(lsv, noise.to(self.dev), gav, glp.to(self.dev) if glp is not None else None, d,
                                   kld_coef.to(self.dev) if kld_coef is not None else None, kld_on_mean)
        assert _pads_untouched(d_w, 2, 2 * A), "the backward wrote outside d_loc_scale's columns"
        return d.cpu().contiguous()

    def kld(self, x, squash, mean, var, weight, loss0=None):
        A = mean.numel()
        xv, _ = _wide(x, self.dev)
        coef, terms = torch.full((2 * A,), NAN, device=self.dev), torch.full((A,), NAN, device=self.dev)
        kld = torch.full((1,), NAN, device=self.dev)
        loss = torch.tensor([loss0], device=self.dev) if loss0 is not None else None
        ops.sac_kld(xv, squash, mean.to(self.dev), var.to(self.dev), weight, coef, terms, kld, loss)
        return coef.cpu(), terms.cpu(), kld.cpu(), loss.cpu() if loss is not None else None


class TorchRunner:
    """torch fp32 on the same formulas: what every bound must let through"""

    def forward(self, ls, noise, want_lp=True, want_sm=True):
        a, sm = R.gaussian_forward_ref(ls, noise, F32)
        return a, R.gaussian_log_prob_ref(ls, a, F32)[0] if want_lp else None, sm if want_sm else None

    def log_prob(self, ls, action):
        return R.gaussian_log_prob_ref(ls, action, F32)[0]

    def backward(self, ls, noise, ga, glp, kld_coef=None, kld_on_mean=False):
        return R.gaussian_backward_ref(ls, noise, ga, glp, kld_coef, kld_on_mean, dtype=F32)[0]

    def kld(self, x, squash, mean, var, weight, loss0=None):
        xs = R.squash(x) if squash else x
        B = x.shape[0]
        kld, t = R.kld_value(xs, mean, var)
        coef = kld_coef_closed_form(xs.mean(0), xs.var(0), mean, var, weight, B)
        loss = torch.tensor([loss0]) + torch.tensor(weight, dtype=F32) * kld if loss0 is not None else None
        return coef.float(), t, kld.reshape(1), loss


def kld_coef_closed_form(m, v, mu, s2, weight, B):
    """d (weight * kld) / d x[b, d] = c0_d + c1_d x[b, d] -> cat(c0, c1); test_kld holds it to autograd of sac_trainer.py:285-304"""
    c1 = weight * (1.0 / s2 - 1.0 / v) / (B - 1)
    c0 = weight * (m - mu) / (B * s2) - c1 * m
    return torch.cat([c0, c1])


def given_actions(B, A, seed):
    """actions the forward did not produce: 0, +-1e-3, +-0.5, exactly +-(1 - eps) as fp32, and uniform interior values"""
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, A, generator=g) * 2 - 1) * 0.98
    vals = torch.tensor([0.0, 1e-3, -1e-3, 0.5, -0.5, A_MAX, -A_MAX], dtype=F32)
    flat = a.reshape(-1)
    idx = torch.arange(0, flat.numel(), 3)
    flat[idx] = vals[torch.arange(idx.numel()) % 7]
    flat[-1] = A_MAX  # d = A - 1 of the last row
    return a


# ---- the checks of one case -------------------------------------------------------------------------------------------------
def _lp_bound(ls, action, T):
    """-> (float64 log-prob at `action`, the row bound sum_d e(stratum) + (A - 1) u sum_d |term_d|)"""
    lp64, t64 = R.gaussian_log_prob_ref(ls, action, F64)
    A = action.shape[1]
    return lp64, T["lp"][stratum(action)].sum(1) + (A - 1) * U * t64.abs().sum(1)


def _kld_setup(run, case, on_mean):
    """embedding statistics and the coefficients of rg_sac_kld (the runner's) for this case"""
    B, A = case["B"], case["A"]
    g = torch.Generator().manual_seed(case["seed"] + 99)
    mean, var = torch.randn(A, generator=g) * 0.3, 0.2 + torch.rand(A, generator=g) * 0.5
    if on_mean:
        x, squash = case["ls"][:, :A].contiguous(), True
    else:
        x, squash = R.gaussian_forward_ref(case["ls"], case["noise"], F32)[0], False
    # c1 = weight (1 / s2 - 1 / v) / (B - 1): a weight in proportion to (B - 1) min_d v keeps the coefficients of the order of
    # g_a at every batch size (two rows can lie arbitrarily close together), so that the bound below stays a bound that bites
    v = (R.squash(x.double()) if squash else x.double()).var(0)
    return run.kld(x, squash, mean, var, float(np.float32(0.3 * (B - 1) * max(v.min().item(), 1e-6))))[0]


def check_head(run, case, counts=None):
    """all statements of the Gaussian head on one case; -> the worst ratio per check"""
    T = tables()
    B, A, ls, noise, ga, glp = (case[k] for k in ("B", "A", "ls", "noise", "ga", "glp"))
    tag = f"B={B} A={A}"
    out = {}
    # stage A
    act, lp, sm = run.forward(ls, noise)
    a64, sm64 = R.gaussian_forward_ref(ls, noise, F64)
    a32, sm32 = R.gaussian_forward_ref(ls, noise, F32)
    out["action"] = _report(f"action {tag}", act, a64, a32, 4 * _ulp(1.0))
    out["squashed_mean"] = _report(f"squashed_mean {tag}", sm, sm64, sm32, 4 * _ulp(1.0))
    for b, d, v, s in case["plants"]:
        if v in CLAMPED:
            assert act[b, d].item() == s * A_MAX, ("a clamped element is exactly the bound", b, d, act[b, d].item())
    # null outputs give the same action bits
    act_n, lp_n, sm_n = run.forward(ls, noise, want_lp=False, want_sm=False)
    assert lp_n is None and sm_n is None and torch.equal(_bits(act_n), _bits(act))
    # stage B, at the runner's own action bits
    lp64, bound = _lp_bound(ls, act, T)
    out["log_prob"] = _report(f"log_prob {tag}", lp, lp64, R.gaussian_log_prob_ref(ls, act, F32)[0], bound)
    # the log-prob of GIVEN actions
    given = given_actions(B, A, case["seed"] + 5)
    lpg64, bound_g = _lp_bound(ls, given, T)
    out["log_prob_given"] = _report(f"log_prob of given actions {tag}", run.log_prob(ls, given), lpg64,
                                    R.gaussian_log_prob_ref(ls, given, F32)[0], bound_g)
    # backward: float64 autograd through the full chain
    s64 = stratum(a64)
    e_loc, e_sl = T["d_loc"][s64], T["d_sl"][s64]
    variants = [("", ga, glp, None, False), (" g_a=None", None, glp, None, False), (" g_lp=None", ga, None, None, False)]
    if B >= 2:
        variants += [(" kld on the action", ga, glp, _kld_setup(run, case, False), False),
                     (" kld on the mean", ga, glp, _kld_setup(run, case, True), True)]
    clamped = torch.zeros(B, A, dtype=torch.bool)
    for b, d, v, s in case["plants"]:
        clamped[b, d] = v in CLAMPED
    sl_raw = ls[:, A:]
    outside = (sl_raw < R.LOG_PROB_MIN) | (sl_raw > R.LOG_PROB_MAX)
    for name, g_a, g_lp, coef, on_mean in variants:
        d = run.backward(ls, noise, g_a, g_lp, coef, on_mean)
        ref, _, _ = R.gaussian_backward_ref(ls, noise, g_a, g_lp, coef, on_mean, dtype=F64)
        own, _, _ = R.gaussian_backward_ref(ls, noise, g_a, g_lp, coef, on_mean, dtype=F32)
        b_loc, b_sl = e_loc, e_sl
        if coef is not None:
            cmag = (coef[:A].abs() + coef[A:].abs()).double()
            if on_mean:
                # the term (c0 + c1 m)(1 - t^2), m = clamp(t), t = tanh(loc), is added to d_loc alone.  With tanhf within 2 ulp
                # and one rounding in each of its five operations its error is below 16 u (|c0| + |c1|), as |t| < 1.
                b_loc = e_loc + 16 * U * cmag
            else:
                # c0 + c1 a joins g_a.  The head is linear in what reaches the action, and the pool's tables hold for g_a drawn
                # from N(0, 1) with every stratum's largest |g_a| above 1, so a further |c0 + c1 a| <= |c0| + |c1| widens
                # an element's error by at most that factor.
                b_loc, b_sl = e_loc * (1 + cmag), e_sl * (1 + cmag)
        out["d_loc" + name] = _report(f"d_loc{name} {tag}", d[:, :A], ref[:, :A], own[:, :A], b_loc)
        out["d_scale_log" + name] = _report(f"d_scale_log{name} {tag}", d[:, A:], ref[:, A:], own[:, A:], b_sl)
        # the clamp decisions, exactly: no gradient through a scale_log outside +-2, none through a clamped tanh
        assert bool((d[:, A:][outside] == 0).all()), f"d_scale_log{name}: a clamped scale_log has a gradient"
        assert bool((d[ref == 0] == 0).all()), f"backward{name}: the statement's exact zeros"
        if g_lp is None and coef is None:
            assert bool((d[:, :A][clamped] == 0).all() and (d[:, A:][clamped] == 0).all()), "a clamped tanh has a gradient"
        for b, dd, v in case["probes"]:
            if abs(v) == 2.0 and name == "":  # the clamp is inclusive: the gradient passes, and this input shows it
                assert ref[b, A + dd].abs() > 2 * float(b_sl[b, dd]), ("choose another seed", b, dd, v)
    if counts is not None:
        counts["interior_rows"] += sum(k == "interior" for k in case["kinds"])
        counts["rows"] += B
        for i, n in enumerate(STRATA):
            counts["bwd " + n] += int((s64 == i).sum())
            counts["lp " + n] += int((stratum(act) == i).sum())
        for _, _, v in case["probes"]:
            counts[f"scale_log {v:g}"] += 1
    return out


def _check_shape(run, B, A):
    counts = {k: 0 for k in ["rows", "interior_rows"] + [p + n for p in ("bwd ", "lp ") for n in STRATA]
              + [f"scale_log {v:g}" for v in PROBES]}
    worst = {}
    for case in shape_cases(B, A):
        for k, r in check_head(run, case, counts).items():
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"compared B={B} A={A}: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    assert counts["interior_rows"] >= 1 and all(counts[p + n] >= 1 for p in ("bwd ", "lp ") for n in STRATA), counts
    assert all(counts[f"scale_log {v:g}"] >= 1 for v in PROBES), counts
    return worst


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_gaussian_head_against_float64(backend, B, A):
    _check_shape(KernelRunner(backend.device), B, A)


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_torch_fp32_stays_inside_the_bounds(B, A):
    """no kernel: torch's fp32 restatement of every case passes the same checks, so the bounds do not reject the reference"""
    _check_shape(TorchRunner(), B, A)


def test_the_pool_covers_every_stratum():
    T = tables()
    assert len(T["n"]) == len(STRATA) and min(T["n"]) >= 256
    for k in ("lp", "d_loc", "d_sl"):
        assert bool((T[k] > 0).all()) and bool(torch.isfinite(T[k]).all())


def test_clamp_of_tanh_is_inclusive(backend):
    """da/dtanh at EXACTLY the bound is 1 (torch's clamp passes the gradient at the bound).  Float64 cannot say where fp32
    tanh reaches the bound, so this is a statement on the kernel's own action: raw sweeps [7.15, 7.45] in 4096 steps (loc = raw,
    noise = 0, so raw is exact), about 400 steps per fp32 value of tanh there, which makes tanh take every fp32 value from
    3.7 ulp below the bound (1 - 1.23e-6 at 7.15) to 4.4 ulp above it (1 - 7.5e-7 at 7.45).  With g_a = 1, g_lp = None,
    d_loc = da/draw: 1 - a^2 where a is below the bound; 0 at the far end; and in between, where a IS the bound, 1 - a^2 on
    the elements whose tanh equals the bound (about 400 of them), 0 on those whose tanh is beyond it."""
    B, A = 16, 256
    raw = torch.linspace(7.15, 7.45, B * A, dtype=F64).float().reshape(B, A)
    raw[1::2] = -raw[1::2]
    ls = torch.cat([raw, torch.zeros(B, A)], 1)
    noise, ones = torch.zeros(B, A), torch.ones(B, A)
    run = KernelRunner(backend.device)
    act, _, _ = run.forward(ls, noise)
    full = run.backward(ls, noise, ones, None)
    d = full[:, :A]
    at = act.abs() == A_MAX
    below = ~at
    assert bool((act.abs() <= A_MAX).all()) and int(below.sum()) >= 256 and int(at.sum()) >= 2048
    slope = 1.0 - act.double() ** 2
    assert bool(((d[below].double() - slope[below]).abs() <= _ulp(1.0)).all())
    passing = at & (d != 0)
    print(f"a == bound: {int(at.sum())} elements, gradient passes in {int(passing.sum())}")
    assert int(passing.sum()) >= 100, "no element whose tanh equals the bound passes its gradient"
    assert bool(((d[passing].double() - (1.0 - A_MAX**2)).abs() <= _ulp(1.0)).all())
    assert bool((d[raw.abs() >= 7.43] == 0).all()) and bool((full[:, A:][at & (d == 0)] == 0).all())


def test_backward_sees_the_eps_of_the_squash_correction(backend):
    """d lp / d a carries 2a / (1 - a^2 + eps).  The eps matters only near saturation (a tenth of the term at |raw| = 6.5), and
    there the pool's table is dominated by its small-sigma elements, so this case isolates it: sigma = e^2, g_a = None,
    g_lp = 1, |raw| in {4, 5.5, 6.5}; calibrated on the case itself, per level."""
    B, A = 12, 7
    g = torch.Generator().manual_seed(4)
    level = torch.tensor([4.0, 5.5, 6.5], dtype=F64)[torch.arange(B) % 3].reshape(B, 1).expand(B, A)
    sign = torch.where(torch.rand(B, A, generator=g) < 0.5, -1.0, 1.0).double()
    loc = ((torch.rand(B, A, dtype=F64, generator=g) * 2 - 1) * 1.5).float()
    sl = torch.full((B, A), 2.0)
    noise = ((level * sign - loc.double()) / math.exp(2.0)).float()
    ls, glp = torch.cat([loc, sl], 1), torch.ones(B)
    d = KernelRunner(backend.device).backward(ls, noise, None, glp)
    ref, _, _ = R.gaussian_backward_ref(ls, noise, None, glp, dtype=F64)
    own, _, _ = R.gaussian_backward_ref(ls, noise, None, glp, dtype=F32)
    for i, v in enumerate((4.0, 5.5, 6.5)):
        rows = torch.arange(B) % 3 == i
        _close(f"d_loc at sigma = e^2, |raw| = {v}", d[rows][:, :A], ref[rows][:, :A], own[rows][:, :A])
        _close(f"d_scale_log at sigma = e^2, |raw| = {v}", d[rows][:, A:], ref[rows][:, A:], own[rows][:, A:])


@pytest.mark.parametrize("A", [3, 65])
def test_a_row_depends_on_that_row_alone(backend, A):
    rpw = 256 // A
    B = 2 * rpw + 1
    case = shape_cases(B, A)[0]
    run = KernelRunner(backend.device)
    act, lp, sm = run.forward(case["ls"], case["noise"])
    given = given_actions(B, A, 3)
    lpg = run.log_prob(case["ls"], given)
    d = run.backward(case["ls"], case["noise"], case["ga"], case["glp"])
    for r in sorted({0, 1, rpw - 1, rpw, B - 2, B - 1}):
        one = slice(r, r + 1)
        a1, lp1, sm1 = run.forward(case["ls"][one], case["noise"][one])
        assert torch.equal(_bits(a1[0]), _bits(act[r])) and torch.equal(_bits(lp1[0]), _bits(lp[r])), r
        assert torch.equal(_bits(sm1[0]), _bits(sm[r])), r
        assert torch.equal(_bits(run.log_prob(case["ls"][one], given[one])[0]), _bits(lpg[r])), r
        d1 = run.backward(case["ls"][one], case["noise"][one], case["ga"][one], case["glp"][one])
        assert torch.equal(_bits(d1[0]), _bits(d[r])), r


def test_two_runs_give_the_same_bits(backend):
    case = shape_cases(7, 65)[0]
    run = KernelRunner(backend.device)
    f = lambda: (*run.forward(case["ls"], case["noise"]), run.backward(case["ls"], case["noise"], case["ga"], case["glp"]))  # noqa: E731
    for x, y in zip(f(), f()):
        assert torch.equal(_bits(x), _bits(y))


# ---- the loss heads -------------------------------------------------------------------------------------------------------
LOSS_BATCHES = [1, 255, 256, 257, 513]
LP_PROBES = [2.0, -2.0, _TWO_UP, -_TWO_UP, 7.0, -9.0]


def _lp_with_probes(B, g):
    lp = torch.randn(B, generator=g) * 2
    n = min(B, len(LP_PROBES))
    lp[:n] = torch.tensor(LP_PROBES[:n])
    return lp


def _partials_check(what, parts, terms64, bound_factor=255):
    """each partial against the float64 sum of ITS 256 rows; fp32 summation of 256 terms in any order is within
    255 u sum|terms| (the terms' own few roundings, at most 15 u |term| in the exponent mode, fit inside that too)"""
    B = terms64.numel()
    P = (B + 255) // 256
    assert parts.numel() == P
    pad = torch.zeros(P * 256, dtype=F64)
    pad[:B] = terms64
    ref, mag = pad.view(P, 256).sum(1), pad.view(P, 256).abs().sum(1)
    return _report(what, parts, ref, ref.float(), bound_factor * U * mag + 1e-300)


@pytest.mark.parametrize("B", LOSS_BATCHES)
def test_critic_head(backend, B, seed=0):
    dev = backend.device
    g = torch.Generator().manual_seed(B + seed)
    f = lambda: torch.randn(B, generator=g)  # noqa: E731
    q1, q2, q1t, q2t, reward = f(), f(), f(), f(), f()
    lpn = _lp_with_probes(B, g)
    nt = (torch.rand(B, generator=g) > 0.3).float()
    if B > 1:
        nt[1], nt[B - 1] = 0.0, 0.0
    alpha = torch.tensor([0.37], dtype=F64)
    P = ops.sac_partials(B)
    assert P == (B + 255) // 256
    for gamma in (0.0, 0.99):
        for has_q2 in (True, False):
            for has_q2t in (True, False):
                tag = f"B={B} gamma={gamma} q2={has_q2} q2_target={has_q2t}"
                new = lambda n=B: torch.full((n,), NAN, device=dev)  # noqa: E731
                tgt, dq1, l1 = new(), new(), new(P)
                dq2, l2 = (new(), new(P)) if has_q2 else (None, None)
                ops.sac_critic_head(q1.to(dev), q2.to(dev) if has_q2 else None, q1t.to(dev), q2t.to(dev) if has_q2t else None,
                                    lpn.to(dev), reward.to(dev), nt.to(dev), gamma, alpha.to(dev), tgt, dq1, dq2, l1, l2)
                y64, v32, mags = R.critic_head_ref(q1t, q2t if has_q2t else None, lpn, reward, nt, gamma, alpha)
                y32 = reward + torch.tensor(gamma, dtype=F32) * v32 * nt if gamma > 0 else reward
                # v is rounded once; gamma * v, * not_terminal and + reward round once each: 4 u of the terms = 2 ulp
                _report(f"target {tag}", tgt, y64, y32, 4 * U * mags)
                if gamma == 0.0:
                    assert torch.equal(_bits(tgt), _bits(reward))
                yk = tgt.cpu().double()
                for name, q, dq, lpart in (("1", q1, dq1, l1), ("2", q2, dq2, l2)):
                    if dq is None:
                        continue
                    # from the kernel's own target: q - y and / B round once each, 2 (q - y) is exact: 2 u = 1 ulp
                    dref = 2.0 * (q.double() - yk) / B
                    _report(f"dq{name} {tag}", dq, dref, (2.0 * (q - tgt.cpu()) / B), 2 * U * dref.abs() * (1 + 2.0**-20) + 1e-45)
                    _partials_check(f"loss{name} partials {tag}", lpart.cpu(), (q.double() - yk) ** 2)


def _grid(B, g):
    """values on a grid of 2^-10: their differences are exact in fp32, so fp32 and float64 agree on every comparison"""
    return torch.round(torch.randn(B, generator=g) * 1024) / 1024


ACTOR_CONFIGS = [  # crr_mode, crr_p0, crr_clamp, backprop_log_prob, with q2a
    (0, 0.0, 0.0, True, True), (0, 0.0, 0.0, False, True), (0, 0.0, 0.0, True, False),
    (1, 0.25, 0.0, True, True), (1, 0.25, 0.0, False, False),
    (2, 0.5, 3.0, True, True), (2, 0.5, 0.0, True, True), (2, 0.5, 3.0, False, False),
]


@pytest.mark.parametrize("B", LOSS_BATCHES)
def test_actor_head(backend, B, seed=0):
    dev = backend.device
    g = torch.Generator().manual_seed(100 + B + seed)
    lp = _lp_with_probes(B, g)
    q1a, q2a, v_cur = _grid(B, g), _grid(B, g), _grid(B, g)
    ties = torch.zeros(B, dtype=torch.bool)
    ties[::5] = True
    q2a[ties] = q1a[ties]
    alpha, target_entropy = torch.tensor([0.37], dtype=F64), -1.5
    P = ops.sac_partials(B)
    for crr_mode, p0, clampv, backprop, has_q2 in ACTOR_CONFIGS:
        tag = f"B={B} crr_mode={crr_mode} clamp={clampv} backprop={backprop} q2a={has_q2}"
        mq = torch.min(q1a, q2a) if has_q2 else q1a
        v = v_cur.clone()
        if crr_mode == 1:  # advantage == threshold exactly (weight 1), one grid step below it (weight 0)
            v[::3] = mq[::3] - p0
            v[1::3] = mq[1::3] - p0 + 2.0**-10
            assert bool(((mq - v)[::3] == p0).all())
        new = lambda n=B: torch.full((n,), NAN, device=dev)  # noqa: E731
        glp, d1, lpart, epart = new(), new(), new(P), new(P)
        d2 = new() if has_q2 else None
        ops.sac_actor_head(lp.to(dev), q1a.to(dev), q2a.to(dev) if has_q2 else None, alpha.to(dev), target_entropy, glp, d1, d2,
                           lpart, epart, v_cur=v.to(dev) if crr_mode else None, crr_mode=crr_mode, crr_p0=p0, crr_clamp=clampv,
                           backprop_log_prob=backprop)
        args = (lp, q1a, q2a if has_q2 else None)
        kw = dict(v_cur=v, crr_mode=crr_mode, crr_p0=p0, crr_clamp=clampv, backprop_log_prob=backprop)
        r64 = R.actor_head_ref(*args, alpha, target_entropy, **kw)
        r32 = R.actor_head_ref(*args, alpha.float(), target_entropy, dtype=F32, **kw)
        for name, got in (("g_lp", glp), ("dq1a", d1), ("dq2a", d2)):
            if got is None:
                continue
            _close(f"{name} {tag}", got, r64[name], r32[name])
            assert torch.equal(got.cpu() == 0, r64[name] == 0), f"{name} {tag}: the statement's exact zeros"
        if crr_mode == 0 and has_q2:  # torch.minimum's backward splits a tie evenly
            assert torch.equal(_bits(d1.cpu()[ties]), _bits(d2.cpu()[ties])) and bool((d1.cpu()[ties] != 0).all())
            assert bool(((d1.cpu() == 0) | (d2.cpu() == 0) | ties).all())
        _partials_check(f"loss partials {tag}", lpart.cpu(), r64["terms"])
        _partials_check(f"entropy partials {tag}", epart.cpu(), r64["ent"])


def test_alpha_grad_sums_more_than_256_partials(backend):
    dev = backend.device
    P, batch = 300, 300 * 256 - 5
    assert ops.sac_partials(batch) == P
    log_alpha = torch.tensor([math.log(0.37)], dtype=F64)
    # integers: every fp32 partial sum is exact in any order, so the result is exact in double
    parts = (torch.arange(P, dtype=F32) * 7 % 31) - 11 + torch.where(torch.arange(P) >= 256, 1000.0, 0.0)
    grad, loss = torch.full((1,), NAN, dtype=F64, device=dev), torch.full((1,), NAN, dtype=F64, device=dev)
    ops.sac_alpha_grad(parts.to(dev), batch, log_alpha.to(dev), grad, loss)
    m = parts.double().sum().item() / batch
    print(f"alpha grad (integers): kernel {grad.item()!r}, statement {-m!r}")
    assert grad.item() == -m and loss.item() == -(log_alpha.item() * m)
    # fp32 partials: 300 terms in any order are within 299 u sum|terms|
    g = torch.Generator().manual_seed(0)
    parts = torch.randn(P, generator=g) * 100
    ops.sac_alpha_grad(parts.to(dev), batch, log_alpha.to(dev), grad, None)
    ref = -(parts.double().sum() / batch)
    _report("alpha grad", grad.cpu(), ref.reshape(1), -(parts.sum().double() / batch).reshape(1),
            299 * U * parts.double().abs().sum().item() / batch)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("sched", [False, True])
def test_adam_f64_against_torch(backend, n, sched):
    dev = backend.device
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, dtype=F64, generator=g)
    p = torch.nn.Parameter(p0.clone())
    lr, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    pd, md, vd = p0.clone().to(dev), torch.zeros(n, dtype=F64, device=dev), torch.zeros(n, dtype=F64, device=dev)
    ex = torch.full((n,), NAN, dtype=F64, device=dev)
    steps = 4
    table = [x for t in range(1, steps + 1) for x in (1.0 - b1**t, math.sqrt(1.0 - b2**t))]
    for step in range(1, steps + 1):
        grad = torch.randn(n, dtype=F64, generator=g) * step
        p.grad = grad.clone()
        opt.step()
        if sched:
            s = torch.tensor([float(step - 1), lr, float(steps), 0.0] + table, dtype=F64).to(dev)
            ops.adam_step_f64_sched(pd, grad.to(dev), md, vd, b1, b2, eps, s, ex)
        else:
            ops.adam_step_f64(pd, grad.to(dev), md, vd, lr, b1, b2, eps, 1 - b1**step, (1 - b2**step) ** 0.5, ex)
        e_p = (pd.cpu() - p.detach()).abs().max().item()
        e_x = (ex.cpu() - p.detach().exp()).abs().max().item()
        print(f"adam f64 n={n} sched={sched} step {step}: param error {e_p:.3e}, exp error {e_x:.3e}, bound 1e-12")
        assert e_p <= 1e-12 and e_x <= 1e-12
        st = opt.state[p]
        assert (md.cpu() - st["exp_avg"]).abs().max().item() <= 1e-12 and (vd.cpu() - st["exp_avg_sq"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("B", [2, 255, 257])
@pytest.mark.parametrize("squashed", [False, True])
def test_kld(backend, B, squashed):
    """rg_sac_kld's arithmetic is float64; what it stores is fp32.  So coef and the per-dimension terms are held to one fp32
    rounding (u relative) of the float64 statement, kld to that plus the index-order fp32 sum of A stored terms, and loss_inout
    to the two roundings of loss + float(weight) * kld.  With squash the kernel's own fp32 tanh feeds the statistic: each x is
    then within dx = 4 ulp of 1 (stage A) of the statement's, which moves m by <= dx and v by <= 2 dx sqrt(B v / (B - 1))
    (Cauchy-Schwarz on sum (x - m) dx / (B - 1)); the bounds add the first-order effect of that on every output."""
    A = 5
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, A, generator=g) * (1.2 if squashed else 0.5)
    mean, var = torch.randn(A, generator=g) * 0.3, 0.2 + torch.rand(A, generator=g) * 0.5
    weight, loss0 = float(np.float32(0.3 * B)), 1.25  # (the kernel takes the weight as an fp32 number, as the fp32 reference does)
    r = R.kld_ref(x, squashed, mean, var, weight)
    m, v, mu, s2 = r["m"], r["v"], mean.double(), var.double()
    coef64 = kld_coef_closed_form(m, v, mu, s2, weight, B)
    # the closed form IS the autograd of sac_trainer.py:285-304
    lin = coef64[:A] + coef64[A:] * r["x"]
    assert (lin - r["grad"]).abs().max().item() <= 1e-12 * max(1.0, r["grad"].abs().max().item())
    dx = 4 * _ulp(1.0) if squashed else 0.0
    dm, dv = dx, 2 * dx * torch.sqrt(B * v / (B - 1))
    dc1 = weight * dv / (v * v * (B - 1))
    dc0 = weight * dm / (B * s2) + dc1 * m.abs() + coef64[A:].abs() * dm
    dterm = 0.5 * ((1.0 / s2 - 1.0 / v).abs() * dv + 2 * (m - mu).abs() / s2 * dm)
    tiny = 1e-12
    coef, terms, kld, loss = KernelRunner(backend.device).kld(x, squashed, mean, var, weight, loss0)  # x strided, NaN padding
    own = TorchRunner().kld(x, squashed, mean, var, weight, loss0)  # printed only: fp32 arithmetic is no yardstick for float64
    tag = f"B={B} squash={squashed}"
    _report(f"kld coef {tag}", coef, coef64, own[0], U * coef64.abs() + torch.cat([dc0, dc1]) + tiny)
    _report(f"kld terms {tag}", terms, r["terms"], own[1], U * r["terms"].abs() + dterm + tiny)
    tk = terms.double()
    _report(f"kld {tag}", kld, tk.sum().reshape(1), own[2], (A - 1) * U * tk.abs().sum().item() + tiny)
    w32 = float(np.float32(weight))
    _report(f"loss_inout {tag}", loss, (loss0 + w32 * kld.double()), own[3], 2 * U * (abs(loss0) + abs(w32 * kld.item())) + tiny)


# ---- exact kernels --------------------------------------------------------------------------------------------------------
def _td3_case(dev, B, A, every_branch=True):
    g = torch.Generator().manual_seed(B + A)
    na, noise = torch.rand(B, A, generator=g) * 2.4 - 1.2, torch.randn(B, A, generator=g)
    nav, _ = _wide(na, dev)
    out, out_w = _wide(torch.full((B, A), SENTINEL), dev, pad=SENTINEL, left=3, right=1)
    var, clip, lo, hi = 0.2, (-0.3, 0.5), -0.97, 0.99
    ops.td3_target_action(nav, noise.to(dev), var, clip, lo, hi, out)
    ref = R.td3_target_action_ref(na, noise, var, clip[0], clip[1], lo, hi)
    assert torch.equal(_bits(out), _bits(ref)), f"td3 target action B={B} A={A}: {(out.cpu() - ref).abs().max().item():.3e}"
    assert _pads_untouched(out_w, 3, A)
    n = noise * 0.2
    if every_branch:  # both noise clips and both action clamps are taken
        assert bool((n < -0.3).any() and (n > 0.5).any() and (ref == np.float32(lo)).any() and (ref == np.float32(hi)).any())


@pytest.mark.parametrize("B,A", [(1, 1), (255, 3), (257, 7), (5, 300)])
def test_td3_target_action_bits(backend, B, A):
    _td3_case(backend.device, B, A, every_branch=B * A >= 500)


@pytest.mark.gpu
def test_td3_target_action_grid_stride():
    """B * A just over 8192 * 256 elements: every thread of the capped grid takes a second element"""
    assert 8200 * 257 > 8192 * 256 and 8200 * 257 > EMU_COST_LIMIT  # (the cost rule: beyond what the interpreter is given)
    _td3_case("cuda", 8200, 257)


@pytest.mark.parametrize("B,C", [(1, 1), (255, 3), (300, 7)])
def test_add_cols_bits(backend, B, C):
    dev = backend.device
    g = torch.Generator().manual_seed(B)
    a, b = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    av, bv = _wide(a, dev)[0], _wide(b, dev, left=2, right=2)[0]
    for other in (bv, None):
        out, out_w = _wide(torch.full((B, C), SENTINEL), dev, pad=SENTINEL)
        ops.add_cols(av, other, out)
        ref = a + b if other is not None else a + 0.0
        assert torch.equal(_bits(out), _bits(ref)) and _pads_untouched(out_w, 1, C)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    p, s, lib, EINVAL = t.data_ptr(), L.stream_ptr(), L.lib(), -1

    def refuses(fn, base, bad):
        """`base` (keyword arguments in the entry point's order) is accepted; each change in `bad` is refused by code"""
        assert fn(*base.values(), s) == 0, (fn.__name__, "baseline")
        for change in bad:
            args = dict(base, **change)
            assert fn(*args.values(), s) == EINVAL, (fn.__name__, change)

    nul = lambda *ks: [{k: None} for k in ks]  # noqa: E731
    sizes = [{"batch": 0}, {"batch": -1}, {"A": 0}, {"A": -3}]
    refuses(lib.rg_gaussian_head_forward, dict(ls=p, ldls=2, noise=p, batch=1, A=1, action=p, lda=1, lp=p, sm=p),
            nul("ls", "noise", "action") + sizes)
    refuses(lib.rg_gaussian_log_prob, dict(ls=p, ldls=2, action=p, lda=1, batch=1, A=1, lp=p), nul("ls", "action", "lp") + sizes)
    refuses(lib.rg_gaussian_head_backward, dict(ls=p, ldls=2, noise=p, ga=p, ldga=1, glp=p, batch=1, A=1, d=p, ldd=2),
            nul("ls", "noise", "d") + sizes)
    refuses(lib.rg_gaussian_head_backward_kld,
            dict(ls=p, ldls=2, noise=p, ga=p, ldga=1, glp=p, batch=1, A=1, d=p, ldd=2, coef=p, on_mean=0),
            nul("ls", "noise", "d") + sizes)
    ones = torch.ones(64, device=dev)
    po = ones.data_ptr()
    refuses(lib.rg_sac_kld, dict(x=p, ldx=1, squash=0, batch=2, A=1, mean=po, var=po, weight=1.0, coef=p + 1024, terms=p + 2048,
                                 kld=None, loss=None),
            nul("x", "mean", "var", "coef", "terms") + [{"batch": 1}, {"batch": 0}, {"A": 0}, {"A": -1}])
    critic = dict(q1=p, q2=p, q1t=p, q2t=p, lpn=p, reward=p, nt=p, gamma=0.99, alpha=p, batch=1, target=p, dq1=p, dq2=p, l1=p, l2=p)
    refuses(lib.rg_sac_critic_head, critic,
            nul("q1", "q1t", "lpn", "reward", "nt", "alpha", "target", "dq1", "l1", "dq2", "l2") + [{"batch": 0}, {"batch": -1}])
    assert lib.rg_sac_critic_head(*dict(critic, q2=None, dq2=None, l2=None).values(), s) == 0
    actor = dict(lp=p, q1a=p, q2a=p, alpha=p, te=-1.0, batch=1, v_cur=p, crr_mode=0, p0=0.5, clamp=0.0, backprop=1, glp=p, d1=p,
                 d2=p, lpart=p, epart=p)
    refuses(lib.rg_sac_actor_head, actor,
            nul("lp", "q1a", "alpha", "glp", "d1", "lpart", "epart", "d2")
            + [{"batch": 0}, {"batch": -1}, {"crr_mode": -1}, {"crr_mode": 3}, {"crr_mode": 1, "v_cur": None},
               {"crr_mode": 2, "v_cur": None}, {"crr_mode": 2, "p0": 0.0}, {"crr_mode": 2, "p0": -1.0}])
    assert lib.rg_sac_actor_head(*dict(actor, crr_mode=2).values(), s) == 0
    assert lib.rg_sac_actor_head(*dict(actor, q2a=None, d2=None, v_cur=None).values(), s) == 0
    refuses(lib.rg_sac_alpha_grad, dict(parts=p, batch=1, log_alpha=p, grad=p + 1024, loss=None),
            nul("parts", "log_alpha", "grad") + [{"batch": 0}, {"batch": -1}])
    adam = dict(p=p, g=p + 1024, m=p + 2048, v=p + 3072, n=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, bc1=0.1, bc2=0.03, ex=None)
    refuses(lib.rg_adam_step_f64, adam, nul("p", "g", "m", "v") + [{"n": 0}, {"n": -1}, {"bc1": 0.0}])
    sch = torch.tensor([0.0, 1e-3, 1.0, 0.0, 0.1, 0.03], dtype=F64, device=dev)
    refuses(lib.rg_adam_step_f64_sched, dict(p=p, g=p + 1024, m=p + 2048, v=p + 3072, n=1, b1=0.9, b2=0.999, eps=1e-8,
                                             sched=sch.data_ptr(), ex=None),
            nul("p", "g", "m", "v", "sched") + [{"n": 0}, {"n": -1}])
    refuses(lib.rg_add_cols, dict(a=p, lda=1, b=None, ldb=0, batch=1, cols=1, out=p + 1024, ldo=1),
            nul("a", "out") + [{"batch": 0}, {"batch": -1}, {"cols": 0}, {"cols": -1}])

    def td3(next_actor=p, noise=p, out=p + 1024, batch=1, A=1):
        return lib.rg_td3_target_action(next_actor, 1, noise, 0.2, -0.5, 0.5, -1.0, 1.0, out, 1, batch, A, s)

    assert td3() == 0
    for change in nul("next_actor", "noise", "out") + sizes:
        assert td3(**change) == EINVAL, ("rg_td3_target_action", change)
    if dev != "cpu":
        torch.cuda.synchronize()
