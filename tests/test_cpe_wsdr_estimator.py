"""WeightedSequentialDoublyRobustEstimator (weighted sequential DR, num_j_steps = 1, and MAGIC, num_j_steps = 25) and its
simplex solver against the unmodified reference's records, on the interpreter and, under `-m gpu`, on the MI355X: the three
fixtures of tests/golden/cpe_wsdr (both values of the self-normalize flag) and the three of tests/golden/cpe_eval (reward and
every metric, flag set, as Evaluator.score_cpe calls it).  u = 2^-53.

Moments and weighted DR.  The any-order bound of tests/test_cpe_wsdr_kernels.py (derived there), against the float64 dense
statement (tests/cpe_wsdr_statement.py); the reference's recorded numbers are held to the same bound in the same assertion.
normalized = raw / score: the relative bounds of both plus 2 u.

Solver.  With g = 2 C x + d and lambda = g . x, the KKT conditions of min x' C x + d' x on the simplex are g_i = lambda on
the support and g_i >= lambda off it.  g is computed here in double from x: J products and additions per entry, error at most
(J + 2) u (2 ||C||_F ||x|| + ||d||) <= (J + 2) u scale with scale = 2 ||C||_F + ||d||_2 (x is on the simplex: ||x|| <= 1);
lambda adds J more.  The solver stops at 8 J u scale (its docstring), so the residual seen here is at most
KKT_FACTOR J u scale with KKT_FACTOR = 8 + 2 * 2 + 4 = 16 (the stop, twice the rounding of g and lambda here and in the
solver, and the final renormalisation of x by a sum within J u of 1 moving g by at most 2 J u ||C||).

MAGIC.  The exact minimiser is no worse than any feasible point: f(x_mine) <= f_ref (1 + J u), f the reference's own
objective (non-symmetric, quirk 2) at the reference's x clipped at 0 and renormalised.  min j_step_returns <= raw <= max.
|magic.raw - reference| as a share of max - min of the j-step returns is MEASURED, not derived: SLSQP's stop at its default
ftol = 1e-6 is the slack and differs per matrix, so the limit is PER FIXTURE: ten times the share measured on it
(MAGIC_SHARES, profiles/NOTES_r20.md), and never below SHARE_FLOOR = 2 J u max|j_step_returns| / (max - min), the rounding of
the two dot products x . j_step_returns of J terms being compared (several measured shares are exactly 0).

Standard error.  (1) The 50 bootstrap estimates replayed here with the documented draw recipe (torch.randperm(J)[:sample_size]
sorted, k = 0 .. 49, under the same torch.manual_seed) from the estimator's OWN moments give raw_std_error to 8 u relative
(np.std of the same 50 doubles: one sum and one square root apart at most).  (2) The same replay from the FLOAT64
STATEMENT's moments: a minimiser is not a Lipschitz function of its matrix with a constant one could write down, so the gap
between the two sets of 50 estimates is measured, as a share of max - min of the j-step returns; REPLAY_LIMIT is ten times
the largest seen over the twelve cases on the interpreter and on the MI355X (profiles/NOTES_r20.md), and raw_std_error is
held to the statement's standard deviation at the same limit (a standard deviation moves by at most the largest move of
its values).  (3) Where the bootstrap sample holds at least two j-steps, raw_std_error lies within 6 / sqrt(2 * 49) of
std_population, the standard deviation over 2 000 draws of the reference's own bootstrap step.  That bound is six standard
deviations of the sample standard deviation of 50 NORMAL values, sqrt((kurtosis - 1) / (4 * 49)) at kurtosis 3.  At wsdr_few
the sample is ONE j-step of 25 drawn uniformly, one of which lies far from the other 24: a kurtosis of 19.4 and 22.1 (the two
flags), at which six standard deviations are 184 % and 197 % and bound nothing.  There the test holds what is exact instead: every bootstrap estimate IS
one of the j-step returns, and (1) and (2).
"""
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

from cpe_wsdr_statement import dense_statement

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
STD_TOL = 6.0 / math.sqrt(2.0 * 49.0)
KKT_FACTOR = 16
# |magic.raw - reference| / (max - min of the j-step returns) as measured per fixture (the same digits on the interpreter and on
# the MI355X; profiles/NOTES_r20.md, "MAGIC against SLSQP"); the test's limit is ten times the fixture's own
MAGIC_SHARES = {
    "wsdr_long/1": 2.964e-02, "wsdr_long/0": 3.705e-04, "wsdr_zero_column/1": 1.381e-04, "wsdr_zero_column/0": 1.415e-01,
    "wsdr_few/1": 8.042e-09, "wsdr_few/0": 1.067e-08, "cpe_dqn_plain/reward": 0.0, "cpe_dqn_metrics_masks/reward": 3.956e-16,
    "cpe_dqn_metrics_masks/clicks": 9.098e-16, "cpe_dqn_metrics_masks/cost": 0.0, "cpe_qrdqn/reward": 9.002e-16,
    "cpe_qrdqn/m1": 1.931e-16,
}
TWO_J_STEPS_SHARE = 4.091e-09  # wsdr_few, self-normalized, num_j_steps = 2: measured the same way
# max |estimate from own moments - estimate from the float64 statement's moments| over the 50 bootstrap estimates, as a share
# of max - min of the j-step returns: ten times the largest measured (profiles/NOTES_r20.md, "Replay from the statement")
REPLAY_LIMIT = 10 * 5.660e-15  # largest seen: wsdr_long without self-normalisation (interpreter and MI355X alike)
SEED = 4321  # torch.manual_seed of the bootstrap draws
WSDR_CASES = [(n, f) for n in ("wsdr_long", "wsdr_zero_column", "wsdr_few") for f in (1, 0)]
EVAL_TARGETS = [("cpe_dqn_plain", "reward"), ("cpe_dqn_metrics_masks", "reward"), ("cpe_dqn_metrics_masks", "clicks"),
                ("cpe_dqn_metrics_masks", "cost"), ("cpe_qrdqn", "reward"), ("cpe_qrdqn", "m1")]
ALL = [("wsdr", n, f) for n, f in WSDR_CASES] + [("eval", n, t) for n, t in EVAL_TARGETS]
_CACHE, _STATEMENTS, _QUANTITIES = {}, {}, {}


def _fixture(folder, name):
    if (folder, name) not in _CACHE:
        with np.load(os.path.join(HERE, "golden", folder, name + ".npz")) as z:
            arrays = {k: z[k] for k in z.files}
        _CACHE[folder, name] = (json.loads(str(arrays["config_json"])), arrays)
    return _CACHE[folder, name]


def _lengths(mdp):
    mdp = mdp.reshape(-1)
    bounds = [0] + (np.nonzero(mdp[1:] != mdp[:-1])[0] + 1).tolist() + [len(mdp)]
    return [b - a for a, b in zip(bounds[:-1], bounds[1:])]


def _subsets(E, most=25):
    num_subsets = int(min(E / 2, most))
    interval = E / num_subsets
    return [int(i * interval) for i in range(num_subsets)] + [int(num_subsets * interval)]


def _j_steps(T, J):
    out = [float("inf")]
    if J > 1:
        out.append(-1)
    if J > 2:
        out.extend([i * (T // (J - 1)) for i in range(1, J - 1)])
    return out


class Case:
    """one (fixture, flag or target): the page on a device, its float64 statement, the reference's recorded estimates"""

    def __init__(self, kind, name, which):
        self.kind, self.name, self.which = kind, name, which
        self.c, self.arrays = _fixture("cpe_wsdr" if kind == "wsdr" else "cpe_eval", name)
        a = self.arrays
        self.flag = bool(which) if kind == "wsdr" else True
        self.gamma = self.c["gamma"] if kind == "wsdr" else self.c["rl"]["gamma"]
        self.lengths = _lengths(a["page_mdp_id"])
        A = a["page_action_mask"].shape[1]
        if kind == "wsdr" or which == "reward":
            self.rewards, self.values = a["page_logged_rewards"][:, 0], a["page_model_values"]
        else:
            i = self.c["cpe_metrics"].index(which)
            self.rewards, self.values = a["page_logged_metrics"][:, i], a["page_model_metrics_values"][:, i * A:(i + 1) * A]
        self.label = f"{name}/{which}"

    def recorded(self, J):
        if self.kind == "wsdr":
            return self.arrays.get(f"sn{self.which}_est_j{J}")
        return self.arrays[f"est_{self.which}_" + {1: "weighted_doubly_robust", 25: "magic"}[J]]

    def page(self, device):
        from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage

        a = self.arrays
        if self.kind == "wsdr":
            N = a["page_mdp_id"].shape[0]
            t = {k[5:]: torch.from_numpy(v).to(device) for k, v in a.items() if k.startswith("page_")}
            return EvaluationDataPage(model_rewards=torch.zeros_like(t["model_values"]),
                                      model_rewards_for_logged_action=torch.zeros(N, 1, device=device), **t)
        page = EvaluationDataPage(**{k[5:]: torch.from_numpy(v).to(device) for k, v in a.items() if k.startswith("page_")})
        if self.which != "reward":
            page = page.set_metric_as_reward(self.c["cpe_metrics"].index(self.which), self.c["num_actions"])
        return page

    def statement(self, J):
        key = (self.label, J)
        if key not in _STATEMENTS:
            a = self.arrays
            T, E = max(self.lengths), len(self.lengths)
            _STATEMENTS[key] = dense_statement(self.lengths, a["page_action_mask"], self.rewards, a["page_logged_propensities"],
                                               a["page_model_propensities"], self.values, self.gamma, self.flag,
                                               _j_steps(T, J), _subsets(E) if J > 1 else None)
        return _STATEMENTS[key]

    def K(self):
        T, E, A = max(self.lengths), len(self.lengths), self.arrays["page_action_mask"].shape[1]
        return T * (2 * A + 7) + E + A + 9


def _estimator(case):
    from reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator import WeightedSequentialDoublyRobustEstimator

    return WeightedSequentialDoublyRobustEstimator(case.gamma)


def _quantities(case, backend, J=25):
    key = (case.label, backend.name, J)
    if key not in _QUANTITIES:
        q = _estimator(case).device_quantities(case.page(backend.device), J, case.flag)
        _QUANTITIES[key] = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in q.items()}
    return _QUANTITIES[key]


def _within(label, got, want, mag, factor):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want))
    bound = factor * U * np.asarray(mag)
    print(f"WSDRERR {label} err={float(err.max()):.3e} bound={float(np.min(bound)):.3e}")
    assert (err <= bound).all(), (label, float(err.max()), float(np.min(bound)))


@pytest.mark.parametrize("kind,name,which", ALL)
def test_weighted_dr_against_float64_and_the_reference(backend, kind, name, which, caplog):
    case = Case(kind, name, which)
    want, ref = case.statement(1), case.recorded(1)
    E = len(case.lengths)
    factor = 2 * (case.K() + E) + 2
    with caplog.at_level(logging.WARNING, logger="reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator"):
        mine = _estimator(case).estimate(case.page(backend.device), 1, case.flag)
    warned = any("Can't normalize WSDR-CPE" in r.getMessage() for r in caplog.records)
    raw64, mag = want["j_step_returns"][0], want["j_step_returns_mag"][0]
    print(f"WSDRERR {case.label} weighted DR raw={mine.raw!r} ref={ref[0]!r} f64={raw64!r}")
    _within(case.label + " raw", [mine.raw, ref[0]], raw64, mag, factor)
    assert mine.raw_std_error == 0.0 and isinstance(mine.raw_std_error, float) and ref[2] == 0.0
    score, score_mag = want["logged_policy_score"], want["logged_policy_score_mag"]
    if score < 1e-6:  # quirk 8
        assert (name, which) == ("cpe_dqn_metrics_masks", "cost") and warned  # the reference's warning is logged
        assert mine.normalized == 0.0 and mine.normalized_std_error == 0.0 and ref[1] == 0.0 and ref[3] == 0.0
    else:
        n64 = raw64 / score
        rel = factor * U * (mag / abs(raw64) + score_mag / abs(score)) + 2 * U
        assert abs(mine.normalized - n64) <= rel * abs(n64) and abs(ref[1] - n64) <= rel * abs(n64)
        assert mine.normalized_std_error == 0.0 and not warned
    # E >= 1 is enough for num_j_steps = 1: the page's first episode alone
    from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage

    page = case.page(backend.device)
    n0 = case.lengths[0]
    one = EvaluationDataPage(**{k: (v[:n0] if torch.is_tensor(v) else v) for k, v in page.__dict__.items()})
    single = _estimator(case).estimate(one, 1, case.flag)
    assert math.isfinite(single.raw) and single.raw_std_error == 0.0


@pytest.mark.parametrize("kind,name,which", ALL)
def test_moments_against_float64_and_the_records(backend, kind, name, which):
    case = Case(kind, name, which)
    q, want = _quantities(case, backend), case.statement(25)
    E, K = len(case.lengths), case.K()
    T = max(case.lengths)
    assert q["j_steps"] == [int(min(j, T - 1)) for j in _j_steps(T, 25)]  # quirk 1
    assert q["subset_offsets"] == _subsets(E)                              # quirk 3
    sources = [("f64", want["j_step_returns"], want["infinite_step_returns"], want["covariance"])]
    if kind == "wsdr":
        a, p = case.arrays, f"sn{which}_"
        assert np.array_equal(a[p + "j_steps"][1:], np.array(_j_steps(T, 25)[1:], dtype=np.float64)) and np.isinf(a[p + "j_steps"][0])
        sources.append(("reference", a[p + "j_step_returns"], a[p + "infinite_step_returns"], a[p + "covariance"]))
    for label, jsr, inf, cov in sources:
        _within(f"{case.label} j_step_returns vs {label}", q["j_step_returns"], jsr, want["j_step_returns_mag"], 2 * (K + E) + 2)
        _within(f"{case.label} infinite_step_returns vs {label}", q["infinite_step_returns"], inf,
                want["infinite_step_returns_mag"], 2 * (K + E) + 2)
        _within(f"{case.label} covariance vs {label}", q["covariance"], cov, want["covariance_mag"], 4 * (K + E + 2))
    assert np.array_equal(q["covariance"], q["covariance"].T)
    if kind == "eval":  # quirk 1: T = 12 < 24, the interval is 0, 23 of the 25 j-steps are step 0: a singular covariance
        assert q["j_steps"] == [T - 1, -1] + [0] * 23 and np.linalg.matrix_rank(q["covariance"]) <= 3
        assert np.array_equal(q["ret"][2], q["ret"][24])
    if name == "cpe_dqn_metrics_masks":  # quirk 6: the fixture has sequence gaps of up to 3 and the discounts ignore them
        seq = case.arrays["page_sequence_number"].reshape(-1)
        mdp = case.arrays["page_mdp_id"].reshape(-1)
        assert (np.diff(seq)[np.diff(mdp) == 0] > 1).any()


def _kkt(C, d, x):
    J = len(x)
    g = 2.0 * (C @ x) + d
    lam = float(g @ x)
    scale = 2.0 * np.linalg.norm(C) + np.linalg.norm(d)
    tol = KKT_FACTOR * J * U * scale
    support = x > 0
    assert (x >= 0).all() and abs(x.sum() - 1.0) <= J * U
    assert np.abs(g[support] - lam).max() <= tol, (np.abs(g[support] - lam).max(), tol)
    assert (g[~support] >= lam - tol).all()


def test_solver_kkt_on_the_fixtures_and_on_singular_matrices(caplog):
    from reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator import magic_objective, solve_simplex_qp

    for name, f in WSDR_CASES:
        a = _fixture("cpe_wsdr", name)[1]
        C, b = a[f"sn{f}_covariance"], a[f"sn{f}_bias"]
        x = solve_simplex_qp(C, b * b)
        _kkt(0.5 * (C + C.T), b * b, x)
        f_mine, f_ref = magic_objective(x, C, b), float(a[f"sn{f}_f_ref"])
        print(f"WSDRERR {name} sn{f} f_mine={f_mine!r} f_ref={f_ref!r}")
        assert f_mine <= f_ref * (1 + 25 * U)
        # quirk 2: the reference's objective is the broadcast one, not x (cov + b b') x
        x_ref = a[f"sn{f}_x_ref"]
        assert magic_objective(x_ref, C, b) == f_ref
        assert magic_objective(x_ref, C, b) == pytest.approx(x_ref @ C @ x_ref + x_ref.sum() * ((b * b) @ x_ref), rel=1e-12)
        if name == "wsdr_long" and f == 1:  # (at x_ref the biased j-steps carry no weight: the uniform x tells the two apart)
            even = np.full(25, 1.0 / 25)
            assert magic_objective(even, C, b) == float(np.dot(np.dot(even, C + b.T * b), even.T))
            assert abs(even @ (C + np.outer(b, b)) @ even - magic_objective(even, C, b)) > 1e-2 * magic_objective(even, C, b)
    rng = np.random.default_rng(5)
    for trial in range(40):
        J = int(rng.integers(2, 33))
        rank = int(rng.integers(1, J))
        B = rng.standard_normal((J, rank))
        C = (B @ B.T) * 10.0 ** int(rng.integers(-6, 4))
        d = np.where(rng.random(J) < 0.5, 0.0, rng.random(J)) * np.abs(C).max()
        if trial % 3 == 0:  # duplicated j-steps: identical rows, columns and bias
            C[:, 1], d[1] = C[:, 0], d[0]
            C[1, :] = C[0, :]
            C[1, 1] = C[0, 0]
        _kkt(C, d, solve_simplex_qp(C, d))
    assert not any("solve_simplex_qp stopped" in r.getMessage() for r in caplog.records)  # every solve above ended at KKT
    # a solve cut short says so and still returns a feasible point
    a = _fixture("cpe_wsdr", "wsdr_long")[1]
    with caplog.at_level(logging.WARNING, logger="reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator"):
        x = solve_simplex_qp(a["sn1_covariance"], a["sn1_bias"] ** 2, max_iter=1)
    assert any("solve_simplex_qp stopped at the iteration limit" in r.getMessage() for r in caplog.records)
    assert (x >= 0).all() and abs(x.sum() - 1.0) <= 25 * U
    assert np.array_equal(solve_simplex_qp(np.array([[3.0]]), np.array([2.0])), np.ones(1))
    _kkt(np.zeros((4, 4)), np.array([1.0, 0.5, 0.5, 2.0]), solve_simplex_qp(np.zeros((4, 4)), np.array([1.0, 0.5, 0.5, 2.0])))


def _replay(q, seed, J, estimator):
    """the documented draw recipe (departure (c)) on given moments -> the 50 bootstrap estimates"""
    G = len(q["infinite_step_returns"])
    sample_size = int(0.5 * G)
    torch.manual_seed(seed)
    means = []
    for _ in range(50):
        idx = np.sort(torch.randperm(J)[:sample_size].numpy())
        means.append(estimator.compute_weighted_doubly_robust_point_estimate(
            q["j_step_returns"][idx], q["infinite_step_returns"], q["covariance"][np.ix_(idx, idx)])[0])
    return np.array(means)


def _share_limit(measured, returns):
    lo, hi = returns.min(), returns.max()
    return max(10.0 * measured, 2 * len(returns) * U * np.abs(returns).max() / (hi - lo))


@pytest.mark.parametrize("kind,name,which", ALL)
def test_magic_against_the_reference(backend, kind, name, which):
    case = Case(kind, name, which)
    est = _estimator(case)
    torch.manual_seed(SEED)
    mine = est.estimate(case.page(backend.device), 25, case.flag)
    q, ref = _quantities(case, backend), case.recorded(25)
    lo, hi = q["j_step_returns"].min(), q["j_step_returns"].max()
    share = abs(mine.raw - ref[0]) / (hi - lo)
    print(f"WSDRSHARE {case.label} {backend.name} raw={mine.raw!r} ref={ref[0]!r} share={share:.3e}")
    assert lo <= mine.raw <= hi
    assert share <= _share_limit(MAGIC_SHARES[case.label], q["j_step_returns"])
    # (1) the documented draws, replayed on the estimator's own moments under the same seed
    own = _replay(q, SEED, 25, est)
    assert mine.raw_std_error == pytest.approx(float(np.std(own)), rel=8 * U, abs=0.0)
    # (2) ... and on the float64 statement's moments
    want = case.statement(25)
    f64 = _replay(dict(j_step_returns=want["j_step_returns"], infinite_step_returns=want["infinite_step_returns"],
                       covariance=want["covariance"]), SEED, 25, est)
    gap = float(np.abs(own - f64).max() / (hi - lo))
    print(f"WSDRREPLAY {case.label} {backend.name} gap={gap:.3e} std={mine.raw_std_error!r} std_f64={float(np.std(f64))!r}")
    assert gap <= REPLAY_LIMIT
    assert abs(mine.raw_std_error - float(np.std(f64))) <= REPLAY_LIMIT * (hi - lo)
    G = len(q["infinite_step_returns"])
    assert G == int(min(len(case.lengths) / 2, 25))
    sample_size = int(0.5 * G)
    if kind == "wsdr" and sample_size >= 2:  # (3)
        population = float(case.arrays[f"sn{which}_std_population"])
        print(f"WSDRERR {case.label} std={mine.raw_std_error!r} ref={ref[2]!r} population={population!r}")
        assert abs(mine.raw_std_error - population) <= STD_TOL * population
        assert abs(ref[2] - population) <= STD_TOL * population
    if sample_size == 1:  # every bootstrap estimate is one j-step return
        assert name == "wsdr_few"
        assert all(v in q["j_step_returns"] for v in own)
    score = want["logged_policy_score"]
    if score < 1e-6:
        assert mine.normalized == 0.0 and mine.normalized_std_error == 0.0
    else:
        assert mine.normalized == pytest.approx(mine.raw / score, rel=1e-12)
        assert mine.normalized_std_error == pytest.approx(mine.raw_std_error / score, rel=1e-12)


def test_two_j_steps_and_the_bootstrap_sample_quirk(backend):
    """quirk 7: the bootstrap draws int(0.5 * subsets) of the J j-steps.  wsdr_few (two subsets: a sample of one j-step, so
    every bootstrap estimate IS one j-step return) runs with J = 2 and 25; on 40 episodes (20 subsets, a sample of 10) J = 2
    raises what np.random.choice raises in the reference."""
    few = Case("wsdr", "wsdr_few", 1)
    est = _estimator(few)
    torch.manual_seed(9)
    two = est.estimate(few.page(backend.device), 2, True)
    ref = few.recorded(2)
    q = _quantities(few, backend, 2)
    assert q["j_steps"] == [max(few.lengths) - 1, -1] and q["subset_offsets"] == [0, 2, 5]  # interval 2.5
    lo, hi = q["j_step_returns"].min(), q["j_step_returns"].max()
    share = abs(two.raw - ref[0]) / (hi - lo)
    print(f"WSDRSHARE wsdr_few/1 J=2 {backend.name} raw={two.raw!r} ref={ref[0]!r} share={share:.3e}")
    assert lo <= two.raw <= hi and share <= _share_limit(TWO_J_STEPS_SHARE, q["j_step_returns"])
    torch.manual_seed(9)
    picks = np.array([q["j_step_returns"][int(torch.randperm(2)[0])] for _ in range(50)])
    assert two.raw_std_error == pytest.approx(float(np.std(picks)), rel=8 * U, abs=0.0)
    long = Case("wsdr", "wsdr_long", 1)
    assert str(long.arrays["sn1_est_j2_error"]).startswith("Cannot take a larger sample than population")
    with pytest.raises(ValueError, match="Cannot take a larger sample than population"):
        _estimator(long).estimate(long.page(backend.device), 2, True)


def test_fewer_than_four_episodes_and_the_refusals(backend):
    import dataclasses

    from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage

    case = Case("wsdr", "wsdr_few", 1)
    page = case.page(backend.device)
    n3 = sum(case.lengths[:3])
    three = EvaluationDataPage(**{k: (v[:n3] if torch.is_tensor(v) else v) for k, v in page.__dict__.items()})
    est = _estimator(case)
    with pytest.raises(ValueError, match="at least 4 episodes"):
        est.estimate(three, 25, True)
    with pytest.raises(ValueError, match="at least 4 episodes"):
        est.estimate(three, 2, True)
    one = est.estimate(three, 1, True)
    assert math.isfinite(one.raw) and one.raw_std_error == 0.0
    with pytest.raises(ValueError, match="num_j_steps = 33"):
        est.estimate(page, 33, True)
    with pytest.raises(ValueError, match="num_j_steps = 0"):
        est.estimate(page, 0, True)
    with pytest.raises(ValueError, match="edp.mdp_id is None"):
        est.estimate(dataclasses.replace(page, mdp_id=None), 1, True)
    with pytest.raises(ValueError, match="edp.model_values is None"):
        est.estimate(dataclasses.replace(page, model_values=None), 1, True)
    assert est.estimate(page, 32, True).raw_std_error >= 0.0  # 32 j-steps are served


def test_static_functions_are_the_references():
    from reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator import (
        subset_offsets, T_QUANTILE_95, WeightedSequentialDoublyRobustEstimator as W)
    import cpe_wsdr_statement as S

    # (b) the table against scipy.stats.t.ppf(0.95, 1 .. 24) as the generator recorded it: the same doubles
    for name in ("wsdr_long", "wsdr_zero_column", "wsdr_few"):
        assert np.array_equal(np.array(T_QUANTILE_95), _fixture("cpe_wsdr", name)[1]["t_ppf_95"])
    x = [1.0, 2.5, 2.0, 4.0]
    m, se = np.mean(x), np.std(x, ddof=1) / 2.0
    low, high = W.confidence_bounds(x, 0.9)
    assert low == pytest.approx(m - se * T_QUANTILE_95[2], rel=1e-15) and high == pytest.approx(m + se * T_QUANTILE_95[2], rel=1e-15)
    with pytest.raises(ValueError, match="table of t quantiles"):
        W.confidence_bounds(x, 0.95)
    # quirk 5: a zero column gets 1 / n everywhere, padded rows included; in place, as the reference
    w = np.array([[2.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    got = W.normalize_importance_weights(w.copy(), True)
    assert np.array_equal(got, np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.0, 0.25, 0.25], [0.0, 0.25, 0.25]]))
    assert np.array_equal(got, S.normalize(w, True))
    assert np.array_equal(W.normalize_importance_weights(w.copy(), False), w / 4.0)
    buf = w.copy()
    assert W.normalize_importance_weights(buf, True) is buf
    # calculate_step_return against the dense statement's
    rng = np.random.default_rng(1)
    r, wn, w1, sv, ql = (rng.standard_normal((5, 7)) for _ in range(5))
    disc = 0.9 ** np.arange(7)
    for j in (-1, 0, 3, 6, float("inf")):
        assert np.allclose(W.calculate_step_return(r, disc, wn, w1, sv, ql, j), S.step_return(r, disc, wn, w1, sv, ql, j)[0],
                           rtol=1e-13, atol=1e-13)
    # quirks 3 and 4: the float interval, in Python; 57 episodes leave the last one out, an even integer split would not
    assert subset_offsets(57, 25)[-1] == 56 and subset_offsets(5, 25) == [0, 2, 5] and subset_offsets(4, 25) == [0, 2, 4]
    assert subset_offsets(67, 25) == [int(i * (67 / 25)) for i in range(26)] and len(subset_offsets(1000, 25)) == 26
