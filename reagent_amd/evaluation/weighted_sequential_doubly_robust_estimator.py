"""reagent/evaluation/weighted_sequential_doubly_robust_estimator.py (https://arxiv.org/pdf/1604.00923.pdf sections 5, 7, 8)
on a device-resident, sorted EvaluationDataPage: weighted sequential doubly-robust (``num_j_steps = 1``) and MAGIC
(``num_j_steps = 25``).

The reference pads every episode to the longest, holds dense [episodes, T, A] float64 cubes on the host, recomputes
everything for 25 episode subsets and calls scipy.optimize.minimize 51 times.  Here rg_cpe_wsdr (cpe_wsdr.hip) does all of
the row and episode arithmetic on the page where it lies, in double, with virtual padding, and leaves J + G + J * J + 1
doubles (j_step_returns, infinite_step_returns, the covariance of the j-step returns, the mean episode value), read back
once per estimate (the page's episode offsets and longest length cost one more synchronisation the first time a page
is seen and are kept for the next call on the same mdp_id tensor; the row quantities and cumulative weights are computed
again by every call, so score_cpe's two calls per target share only the former); the host part is the quadratic program over the J <= 32 j-step weights, in numpy alone (no scipy).

QUIRKS OF THE REFERENCE THAT ARE KEPT (a "corrected" version fails tests/test_cpe_wsdr_estimator.py):
 1. j_steps = [inf, -1, i * (T // (J - 1)) for i = 1 .. J - 2].  With T < J - 1 the interval is 0, J - 2 of the j-steps are
    step 0 and the covariance is singular.
 2. ``error = covariance + j_step_bias.T * j_step_bias`` broadcasts: b_k ** 2 is added to COLUMN k of every row; the
    objective is x . error . x with that non-symmetric matrix (``magic_objective``).
 3. num_subsets = int(min(E / 2, 25)); subset i is episodes int(i * interval) .. int((i + 1) * interval) - 1 with the FLOAT
    interval = E / num_subsets, computed on the host in Python exactly so (``subset_offsets``).
 4. If float rounding leaves the last episode out of every subset it stays out of the subsets and still counts in the whole
    set.
 5. A step whose weights sum to exactly 0 gets weight 1 / n for every episode of the set, padded ones included.
 6. Discounts go by step index (gamma ** t) and ignore gaps in sequence_number.
 7. The bootstrap draws int(0.5 * num_subsets) of the J J-STEPS (not of the subsets) without replacement, sorted, reuses the
    same infinite_step_returns and the sub-covariance, and takes np.std (ddof 0) over 50 draws.  Where that sample is larger
    than J (num_j_steps = 2 on a page of 12 episodes or more) np.random.choice raises ValueError("Cannot take a larger sample
    than population when 'replace=False'"), and so does estimate here, after the point estimate is made.
 8. The normalizer is the mean episode value; below 1e-6 the two normalized fields are 0.0 and the reference's warning is
    logged.

DEPARTURES FROM THE REFERENCE:
 (a) Exact minimiser.  The j-step weights are the exact minimiser of the convex program min x' cov x + (b * b)' x on the
     simplex, which is the reference's objective wherever sum x = 1, by the numpy active-set solver ``solve_simplex_qp``
     (singular cov included).  SLSQP started at the infeasible x = 0 and stopped at its default ftol = 1e-6 is not reproduced.
 (b) The quantile t_0.95(n - 1), n = 2 .. 25, comes from the table T_QUANTILE_95 of 24 doubles.
 (c) Bootstrap draws come from torch's default host generator: draw k of the 50 is
     ``torch.randperm(num_j_steps)[:sample_size]`` sorted ascending, k = 0 .. 49 in order, so torch.manual_seed reproduces
     them.  They are made only when the estimator runs with num_j_steps > 1, after the device results are read back.
 (d) Always double.  The reference is float32 throughout on a page whose episodes all have the same length (no padding value
     is ever inserted); here the arithmetic is double on the fp32 inputs always.
 (e) Fewer than four episodes: the reference divides by zero or propagates NaN there (one subset, a standard error of one
     value).  ``estimate(..., num_j_steps > 1, ...)`` raises ValueError naming "at least 4 episodes"; num_j_steps = 1 works
     for any E >= 1 and has raw_std_error exactly 0.0.

REFUSED, each by name: num_j_steps > 32 (RG_CPE_WSDR_MAX_J_STEPS), edp.mdp_id is None, edp.model_values is None.
"""
import logging

import numpy as np
import torch

from .. import ops
from .cpe import CpeEstimate
from .doubly_robust_estimator import _f32c, _rows
from .evaluation_data_page import EvaluationDataPage, episode_offsets

logger = logging.getLogger(__name__)

MAX_J_STEPS = ops.CPE_WSDR_MAX_J_STEPS

# t_0.95(df), df = 1 .. 24: the one-sided 95 % quantile of Student's t (scipy.stats.t.ppf(0.95, df); checked against the
# recorded values in tests/golden/cpe_wsdr)
T_QUANTILE_95 = (
    6.313751514800932, 2.919985580355516, 2.3533634348018264, 2.131846786326649, 2.0150483733330233, 1.9431802805153022,
    1.894578605061305, 1.8595480375228424, 1.8331129326536335, 1.8124611228107335, 1.7958848187036691, 1.782287555649159,
    1.7709333959867988, 1.7613101357748562, 1.7530503556925547, 1.74588367627624, 1.7396067260750672, 1.7340636066175354,
    1.729132811521367, 1.7247182429207857, 1.7207429028118775, 1.717144374380242, 1.7138715277470473, 1.7108820799094275,
)

_U = 2.0 ** -53


def subset_offsets(num_trajectories: int, max_subsets: int):
    """quirks 3 and 4 (:112-119): [G + 1] ints, subset i = episodes offsets[i] .. offsets[i + 1] - 1"""
    num_subsets = int(min(num_trajectories / 2, max_subsets))
    interval = num_trajectories / num_subsets
    # subset i ends where subset i + 1 begins: int((i + 1) * interval) is both
    return [int(i * interval) for i in range(num_subsets + 1)]


def reference_j_steps(trajectory_length: int, num_j_steps: int):
    """quirk 1 (:54-60), with inf as the reference writes it"""
    j_steps = [float("inf")]
    if num_j_steps > 1:
        j_steps.append(-1)
    if num_j_steps > 2:
        interval = trajectory_length // (num_j_steps - 1)
        j_steps.extend([i * interval for i in range(1, num_j_steps - 1)])
    return j_steps


def magic_objective(x, covariance, j_step_bias):
    """quirk 2: mse_loss(x, covariance + j_step_bias.T * j_step_bias) of the reference (:229, 352-353)"""
    error = np.asarray(covariance) + np.asarray(j_step_bias).T * np.asarray(j_step_bias)
    return float(np.dot(np.dot(x, error), np.asarray(x).T))


def solve_simplex_qp(C, d, max_iter=None):
    """The minimiser of x' C x + d' x over the simplex {x >= 0, sum x = 1}, C symmetric positive semi-definite (singular
    allowed), by a primal active-set method in numpy.

    On the free set F the step lives in {p : sum p = 0}, spanned by the orthonormal columns Z; the reduced Hessian
    H = Z' 2 C_FF Z is diagonalised (eigh).  Along eigen-directions with curvature the Newton step is taken; a direction
    without curvature but with slope is followed to the boundary (the objective is linear and falling there).  A step that
    would leave x >= 0 is cut at the first bound, whose index leaves F with x exactly 0.  At a minimiser of F, the index
    with the smallest gradient below the multiplier lambda joins F; if there is none the KKT conditions hold: with
    g = 2 C x + d, g_i = lambda on F and g_i >= lambda off it.  Everything stops at tol = 8 J u (2 ||C||_F + ||d||_2),
    u = 2^-53: the rounding of g itself is of that order.  A solve that ends otherwise (the iteration limit) logs a warning and
    returns the feasible point it has."""
    C = np.asarray(C, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    J = d.shape[0]
    assert C.shape == (J, J)
    if J == 1:
        return np.ones(1)
    C = 0.5 * (C + C.T)
    scale = 2.0 * float(np.linalg.norm(C)) + float(np.linalg.norm(d))
    tol = 8.0 * J * _U * scale
    x = np.zeros(J)
    x[int(np.argmin(np.diag(C) + d))] = 1.0
    free = x > 0
    max_iter = max_iter or 60 * J
    stopped_short = "the iteration limit"
    for _ in range(max_iter):
        g = 2.0 * (C @ x) + d
        idx = np.nonzero(free)[0]
        k = idx.size
        at_minimum = True
        if k > 1:
            # orthonormal basis of {p on F : sum p = 0}: the last k - 1 columns of a Householder reflection of the ones vector
            v = np.full(k, 1.0 / np.sqrt(k))
            v[0] += 1.0
            Q = np.eye(k) - np.outer(v, v) / v[0]
            Z = Q[:, 1:]
            r = Z.T @ g[idx]
            if float(np.linalg.norm(r)) > tol:
                at_minimum = False
                H = Z.T @ (2.0 * C[np.ix_(idx, idx)]) @ Z
                lam, V = np.linalg.eigh(0.5 * (H + H.T))
                rv = V.T @ r
                flat = lam <= 8.0 * J * _U * max(float(np.abs(lam).max()), scale)
                slope = flat & (np.abs(rv) > tol)
                if slope.any():
                    p = -(Z @ (V[:, slope] @ rv[slope]))
                    full = False
                else:
                    step = np.where(flat, 0.0, rv / np.where(flat, 1.0, lam))
                    p = -(Z @ (V @ step))
                    full = True
                neg = p < 0
                alpha, block = (1.0, -1) if full else (np.inf, -1)
                if neg.any():
                    ratios = np.where(neg, x[idx] / np.where(neg, -p, 1.0), np.inf)
                    b = int(np.argmin(ratios))
                    if ratios[b] < alpha:
                        alpha, block = float(ratios[b]), b
                if not np.isfinite(alpha):  # no curvature, no bound in the way: cannot happen with sum p = 0, p != 0
                    stopped_short = "a falling direction without a bound"
                    break
                x[idx] = x[idx] + alpha * p
                if block >= 0:
                    x[idx[block]] = 0.0
                    free[idx[block]] = False
                x[idx] = np.maximum(x[idx], 0.0)
                if full and block < 0 and float(np.linalg.norm(p)) <= 4.0 * J * _U:
                    at_minimum = True  # the Newton step no longer moves x: the residual is the rounding floor
                    g = 2.0 * (C @ x) + d
                if not at_minimum:
                    continue
        lam_f = float(np.dot(g[idx], x[idx]) / x[idx].sum())
        off = ~free
        if not off.any():
            stopped_short = None
            break
        cand = np.where(off, g, np.inf)
        i = int(np.argmin(cand))
        if cand[i] >= lam_f - tol:
            stopped_short = None
            break
        free[i] = True
    if stopped_short:
        logger.warning("solve_simplex_qp stopped at %s before the KKT conditions held (J = %d): the weights returned are "
                       "feasible but may not be the minimiser", stopped_short, J)
    x = np.where(free, np.maximum(x, 0.0), 0.0)
    return x / x.sum()


class WeightedSequentialDoublyRobustEstimator:
    NUM_SUBSETS_FOR_CB_ESTIMATES = 25
    CONFIDENCE_INTERVAL = 0.9
    NUM_BOOTSTRAP_SAMPLES = 50
    BOOTSTRAP_SAMPLE_PCT = 0.5

    def __init__(self, gamma):
        self.gamma = gamma
        self._episodes_of = None  # (mdp_id tensor, its version, offsets, longest episode): the last page's

    def _episodes(self, mdp_id: torch.Tensor):
        """-> (episode offsets [E + 1] int32 on the device, the longest episode's length).  Computing them synchronises with
        the device (torch.nonzero and one read-back of the maximum), so they are kept for the next call on the same mdp_id
        tensor: score_cpe calls estimate twice per target, and set_metric_as_reward pages share the tensor."""
        kept = self._episodes_of
        if kept is not None and kept[0] is mdp_id and kept[1] == mdp_id._version:
            return kept[2], kept[3]
        offsets = episode_offsets(mdp_id)
        longest = int((offsets[1:] - offsets[:-1]).max())
        self._episodes_of = (mdp_id, mdp_id._version, offsets, longest)
        return offsets, longest

    def device_quantities(self, edp: EvaluationDataPage, num_j_steps, whether_self_normalize_importance_weights):
        """rg_cpe_wsdr on the page -> dict(j_steps [J] ints, ret [J + 1, E] on the device, and on the host, after ONE
        read-back of the results: j_step_returns [J], infinite_step_returns [G], covariance [J, J], logged_policy_score).
        The page's episode structure costs one more synchronisation the first time a page is seen (_episodes); the row
        quantities and cumulative weights are computed again by every call."""
        if num_j_steps < 1 or num_j_steps > MAX_J_STEPS:
            raise ValueError(f"num_j_steps = {num_j_steps} is not served: 1 <= num_j_steps <= {MAX_J_STEPS}")
        if edp.mdp_id is None:
            raise ValueError("edp.mdp_id is None: the weighted sequential estimators need the page's episodes")
        if edp.model_values is None:
            raise ValueError("edp.model_values is None: the weighted sequential estimators need the model's values")
        offsets, trajectory_length = self._episodes(edp.mdp_id)
        num_trajectories = offsets.numel() - 1
        if num_j_steps > 1 and num_trajectories < 4:
            raise ValueError(f"MAGIC (num_j_steps > 1) needs at least 4 episodes for two subsets of two; the page has "
                             f"{num_trajectories}")
        J = int(num_j_steps)
        j_steps = [int(min(j, trajectory_length - 1)) for j in reference_j_steps(trajectory_length, J)]
        subsets = subset_offsets(num_trajectories, self.NUM_SUBSETS_FOR_CB_ESTIMATES) if J > 1 else None
        ret, out = ops.cpe_wsdr(_f32c(edp.model_propensities), _f32c(edp.action_mask), _rows(edp.model_values),
                                _f32c(edp.logged_propensities).reshape(-1), _rows(edp.logged_rewards), offsets,
                                trajectory_length, self.gamma, whether_self_normalize_importance_weights, j_steps, subsets)
        host = out.cpu().numpy()
        G = len(subsets) - 1 if J > 1 else 0
        return dict(j_steps=j_steps, ret=ret, subset_offsets=subsets, j_step_returns=host[:J],
                    infinite_step_returns=host[J:J + G],
                    covariance=host[J + G:J + G + J * J].reshape(J, J) if J > 1 else np.zeros((1, 1)),
                    logged_policy_score=float(host[-1]))

    def estimate(
        self,
        edp: EvaluationDataPage,
        num_j_steps,
        whether_self_normalize_importance_weights,
    ) -> CpeEstimate:
        """arXiv 1604.00923 sections 5, 7, 8.  num_j_steps = 1: the weighted sequential DR return of the whole set, standard
        error exactly 0.0.  More: MAGIC's blend of the j-step returns and the standard deviation of its 50 bootstrap blends."""
        q = self.device_quantities(edp, num_j_steps, whether_self_normalize_importance_weights)
        returns, J = q["j_step_returns"], int(num_j_steps)
        if J == 1:
            raw, std_error = float(returns[0]), 0.0
        else:
            subset_returns, covariance = q["infinite_step_returns"], q["covariance"]
            raw, _x = self.compute_weighted_doubly_robust_point_estimate(returns, subset_returns, covariance)
            sample_size = int(self.BOOTSTRAP_SAMPLE_PCT * len(subset_returns))
            if sample_size > J:  # quirk 7: what np.random.choice(J, sample_size, replace=False) raises in the reference
                raise ValueError("Cannot take a larger sample than population when 'replace=False'")
            blends = []
            for _ in range(self.NUM_BOOTSTRAP_SAMPLES):  # departure (c): the draw recipe
                picked = np.sort(torch.randperm(J)[:sample_size].numpy())
                blends.append(self.compute_weighted_doubly_robust_point_estimate(
                    returns[picked], subset_returns, covariance[np.ix_(picked, picked)])[0])
            std_error = float(np.std(blends))
        score = q["logged_policy_score"]
        can_normalize = score >= 1e-6  # quirk 8
        if not can_normalize:
            logger.warning("Can't normalize WSDR-CPE because of small or negative logged_policy_score")
        return CpeEstimate(raw=raw, normalized=raw / score if can_normalize else 0.0, raw_std_error=std_error,
                           normalized_std_error=std_error / score if can_normalize else 0.0)

    @staticmethod
    def j_step_bias(j_step_returns, infinite_step_returns):
        """:214-225: how far each j-step return lies outside the confidence bounds of the subsets' infinite-step returns"""
        low_bound, high_bound = WeightedSequentialDoublyRobustEstimator.confidence_bounds(
            infinite_step_returns, WeightedSequentialDoublyRobustEstimator.CONFIDENCE_INTERVAL)
        j_step_returns = np.asarray(j_step_returns, dtype=np.float64)
        bias = np.zeros(len(j_step_returns))
        lower, higher = j_step_returns < low_bound, j_step_returns > high_bound
        bias[lower] = low_bound - j_step_returns[lower]
        bias[higher] = j_step_returns[higher] - high_bound
        return bias

    def compute_weighted_doubly_robust_point_estimate(self, j_step_returns, infinite_step_returns, covariance):
        """:197-243 from the moments the device leaves -> (estimate, x).  An empty selection (a bootstrap of sample size 0)
        is np.dot of nothing: 0.0."""
        j_step_returns = np.asarray(j_step_returns, dtype=np.float64)
        if len(j_step_returns) == 0:
            return 0.0, np.zeros(0)
        bias = self.j_step_bias(j_step_returns, infinite_step_returns)
        x = solve_simplex_qp(covariance, bias * bias)
        return float(np.dot(x, j_step_returns)), x

    @staticmethod
    def normalize_importance_weights(importance_weights, whether_self_normalize_importance_weights):
        """:275-289 on a dense [episodes, T] numpy array, IN PLACE as the reference: divided by the column sums (a column that
        sums to exactly 0 becomes 1 / episodes in every row, quirk 5) or, without self-normalisation, by the episode count"""
        w = importance_weights
        episodes = w.shape[0]
        if not whether_self_normalize_importance_weights:
            w /= episodes
            return w
        column_sums = w.sum(axis=0)
        dead = column_sums == 0.0
        w[:, dead] = 1.0
        column_sums[dead] = episodes
        w /= column_sums
        return w

    @staticmethod
    def calculate_step_return(
        rewards,
        discounts,
        importance_weights,
        importance_weights_one_earlier,
        estimated_state_values,
        estimated_q_values,
        j_step,
    ):
        """:291-343 on dense [episodes, T] numpy arrays -> [episodes]: the importance-sampled rewards and the control variate
        up to step j, plus the direct-method value of step j + 1 where there is one"""
        rewards = np.asarray(rewards)
        steps = rewards.shape[1]
        k = int(min(j_step, steps - 1)) + 1
        weighted = np.asarray(discounts) * importance_weights
        weighted_earlier = np.asarray(discounts) * importance_weights_one_earlier
        q, v = np.asarray(estimated_q_values), np.asarray(estimated_state_values)
        head = (weighted[:, :k] * rewards[:, :k] - weighted[:, :k] * q[:, :k] + weighted_earlier[:, :k] * v[:, :k]).sum(axis=1)
        if k < steps:
            head = head + weighted_earlier[:, k] * v[:, k]
        return head

    @staticmethod
    def confidence_bounds(x, confidence):
        """:345-350 with the t quantile from T_QUANTILE_95 (departure (b)): confidence must be 0.9, 2 <= len(x) <= 25"""
        n = len(x)
        if abs(confidence - WeightedSequentialDoublyRobustEstimator.CONFIDENCE_INTERVAL) > 1e-12 or not 2 <= n <= 25:
            raise ValueError(f"confidence_bounds serves confidence 0.9 and 2 <= len(x) <= 25 (a table of t quantiles), "
                             f"not confidence {confidence}, len(x) {n}")
        x = np.asarray(x, dtype=np.float64)
        m = np.mean(x)
        se = np.std(x, ddof=1) / np.sqrt(n)
        h = se * T_QUANTILE_95[n - 2]
        return m - h, m + h
