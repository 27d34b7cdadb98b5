"""TEST INFRASTRUCTURE: a float64 numpy restatement of the DENSE computation of the reference's
WeightedSequentialDoublyRobustEstimator.estimate (weighted_sequential_doubly_robust_estimator.py:27-155), padded cubes and
all, shared by tests/test_cpe_wsdr_kernels.py and tests/test_cpe_wsdr_estimator.py (and timed as the host side by
profiles/microbench/cpe_wsdr.py).  It imports nothing of the package's estimator: the three static functions are restated
here as the reference writes them.

Every quantity comes with the sum of the absolute values of the terms it adds up, for the any-order bound of the tests."""
import itertools

import numpy as np


def to_dense(lengths, mask, rewards, logged_p, prop, values):
    """transform_to_equal_length_trajectories (:245-273) in float64: zip_longest padding with 0 (logged propensity: 1)"""
    ends = np.cumsum(lengths)
    trajectories = [np.arange(e - n, e) for n, e in zip(lengths, ends)]
    A = prop.shape[1]

    def pad(x, fill):
        return np.array(list(itertools.zip_longest(*[x[t] for t in trajectories], fillvalue=fill)),
                        dtype=np.float64).swapaxes(0, 1)

    f = lambda x: np.asarray(x, dtype=np.float64)
    return (pad(f(mask), np.zeros(A)), pad(f(rewards).reshape(-1), 0.0), pad(f(logged_p).reshape(-1), 1.0),
            pad(f(prop), np.zeros(A)), pad(f(values), np.zeros(A)))


def normalize(w, self_normalize):
    w = w.copy()
    if self_normalize:
        s = np.sum(w, axis=0)
        zeros = np.where(s == 0.0)[0]
        s[zeros] = len(w)
        w[:, zeros] = 1.0
        return w / s
    return w / w.shape[0]


def step_return(rewards, discounts, w, w_earlier, sv, ql, j_step, sv_abs=None, ql_abs=None):
    """calculate_step_return (:291-343) -> (returns [E], sum of |terms| [E]); sv_abs and ql_abs are the sums of |products|
    behind sv and ql (a sum over actions can cancel: the bound goes by its terms)"""
    sv_abs = np.abs(sv) if sv_abs is None else sv_abs
    ql_abs = np.abs(ql) if ql_abs is None else ql_abs
    T, E = rewards.shape[1], rewards.shape[0]
    j = int(min(j_step, T - 1))
    wd, wd1 = discounts * w, discounts * w_earlier
    a = wd[:, :j + 1] * rewards[:, :j + 1]
    dm = wd1[:, j + 1] * sv[:, j + 1] if j < T - 1 else np.zeros(E)
    b, c = wd[:, :j + 1] * ql[:, :j + 1], wd1[:, :j + 1] * sv[:, :j + 1]
    ret = np.sum(a, axis=1) + dm - np.sum(b - c, axis=1)
    dm_abs = np.abs(wd1[:, j + 1]) * sv_abs[:, j + 1] if j < T - 1 else np.zeros(E)
    mag = (np.sum(np.abs(a), axis=1) + dm_abs
           + np.sum(np.abs(wd[:, :j + 1]) * ql_abs[:, :j + 1] + np.abs(wd1[:, :j + 1]) * sv_abs[:, :j + 1], axis=1))
    return ret, mag


def _returns(ratio, rewards, sv, ql, discounts, self_normalize, j_steps, sv_abs, ql_abs):
    w = normalize(np.cumprod(ratio, axis=1), self_normalize)
    w1 = np.hstack([np.ones([len(w), 1]) * 1.0 / len(w), w[:, :-1]])
    pairs = [step_return(rewards, discounts, w, w1, sv, ql, j, sv_abs, ql_abs) for j in j_steps]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def dense_statement(lengths, mask, rewards, logged_p, prop, values, gamma, self_normalize, j_steps, subsets=None):
    """-> dict: ret [J + 1, E] (last row the episode values), j_step_returns [J], infinite_step_returns [G], covariance
    [J, J] and its numerators, logged_policy_score, and `*_mag`: the sums of |terms| behind each.  j_steps may hold inf."""
    actions, r, lp, tp, qv = to_dense(lengths, mask, rewards, logged_p, prop, values)
    E, T = r.shape
    tpl = np.sum(tp * actions, axis=2)
    ql = np.sum(qv * actions, axis=2)
    sv = np.sum(tp * qv, axis=2)
    ql_abs, sv_abs = np.sum(np.abs(qv * actions), axis=2), np.sum(np.abs(tp * qv), axis=2)
    ratio = tpl / lp
    discounts = np.power(float(gamma), np.arange(T, dtype=np.float64))
    ret, mag = _returns(ratio, r, sv, ql, discounts, self_normalize, j_steps, sv_abs, ql_abs)
    ev, ev_mag = np.sum(r * discounts, axis=1), np.sum(np.abs(r * discounts), axis=1)
    out = dict(T=T, ret=np.vstack([ret, ev]), ret_mag=np.vstack([mag, ev_mag]), j_step_returns=ret.sum(1),
               j_step_returns_mag=mag.sum(1), logged_policy_score=ev.mean(), logged_policy_score_mag=ev_mag.mean())
    if subsets is not None:
        inf, inf_mag = [], []
        for g in range(len(subsets) - 1):
            s = np.arange(subsets[g], subsets[g + 1])
            x, m = _returns(ratio[s], r[s], sv[s], ql[s], discounts, self_normalize, [float("inf")], sv_abs[s], ql_abs[s])
            inf.append(x[0].sum()), inf_mag.append(m[0].sum())
        out["infinite_step_returns"], out["infinite_step_returns_mag"] = np.array(inf), np.array(inf_mag)
        centred = ret - ret.mean(axis=1, keepdims=True)
        out["cov_numerators"] = centred @ centred.T
        # |centred product| <= (|ret_j| + |m_j|)(|ret_k| + |m_k|), each factor a sum of terms of size mag
        big = mag + np.abs(mag).mean(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):  # E == 1: 0 / 0, as np.cov of one observation
            out["covariance"] = out["cov_numerators"] / (E - 1)
            out["covariance_mag"] = (big @ big.T) / (E - 1)
    return out
