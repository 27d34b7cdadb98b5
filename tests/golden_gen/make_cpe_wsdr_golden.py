"""TEST INFRASTRUCTURE.  Generates tests/golden/cpe_wsdr/*.npz by running the UNMODIFIED reference's
WeightedSequentialDoublyRobustEstimator (reagent/evaluation/weighted_sequential_doubly_robust_estimator.py) through
oracle/stubs.py on EvaluationDataPages built directly from seeded tensors.  Run where the reference tree and scipy are present:
    python tests/golden_gen/make_cpe_wsdr_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_cpe_wsdr_golden.py --check    (regenerates them and compares with the committed files)

The fixtures of tests/golden/cpe_eval cannot test MAGIC's blend: there T = 12 < 24, the j-steps collapse (quirk 1 of the
estimator's docstring) and MAGIC equals weighted DR to 13 digits.  Here:
  wsdr_long         E = 40 episodes of 1 to 60 steps (one of length 1, the longest at least 48: a j-step interval of 2 at
                    least), A = 3, gamma 0.9; model_values are the true values of the target policy times 1 + BIAS plus noise,
                    propensity ratios spread widely.  Drawn again until the reference's MAGIC weights (self-normalized) put
                    more than 0.05 on two distinct j-steps at least and one bias term is non-zero.
  wsdr_zero_column  the same size; at step ZERO_STEP every episode still alive has target propensity 0 for its logged action,
                    so that step's and every later step's weights sum to exactly 0 (quirk 5)
  wsdr_few          E = 5 episodes of 1 to 12 steps: two subsets, interval 2.5, bootstrap sample size 1
Every case is run with both values of the self-normalize flag (sn0, sn1).  The pages are ragged, so the reference computes in
float64 (an equal-length page would be float32 throughout, departure (d)).

Layout: config_json; page_<field> for mdp_id, sequence_number [N, 1] int64, logged_propensities, logged_rewards [N, 1],
action_mask, model_propensities, model_values [N, A] float32 (sorted by episode); t_ppf_95 = scipy.stats.t.ppf(0.95, 1 .. 24);
and per flag, prefix sn<f>_:
  est_j<J>                 [raw, normalized, raw_std_error, normalized_std_error] for num_j_steps J in 1, 2, 25; where the
                           reference raises instead (J = 2 with more than 5 subsets: its bootstrap draws int(0.5 * subsets)
                           of the J j-steps without replacement), est_j<J>_error holds the ValueError's message
  j_steps                  [25] float64 as the reference lists them (inf first)
  j_step_returns [25], infinite_step_returns [G], covariance [25, 25], bias [25]   what the reference hands to its optimiser
  x_ref, f_ref             the optimiser's x clipped at 0 and renormalised to sum 1, and the reference's objective there
  x_raw                    the optimiser's x as returned
  bootstrap_means [50]     the reference's 50 bootstrap estimates
  std_population           the standard deviation over 2 000 draws of the reference's own bootstrap step
`check_inputs` names the conditions a draw misses; the whole case is drawn again with another seed until none is.
np.random.seed is fixed before every estimate.  The reference is read, never altered: its point-estimate method is wrapped on
an instance to see its arguments and results, and its optimiser call is repeated here with the same arguments to see x.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "cpe_wsdr")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "cpe_wsdr_signatures.json")

GAMMA = 0.9
BIAS = 0.15
ZERO_STEP = 5
NUM_J_STEPS = (1, 2, 25)
POPULATION_DRAWS = 2000
STD_TOLERANCE = 6.0 / np.sqrt(2.0 * 49.0)  # six standard deviations of a sample standard deviation at 50 draws
CASES = {
    "wsdr_long": dict(episodes=40, max_length=60, longest_at_least=48, num_actions=3, zero_step=None, seed=7100),
    "wsdr_zero_column": dict(episodes=40, max_length=60, longest_at_least=48, num_actions=3, zero_step=ZERO_STEP, seed=7200),
    "wsdr_few": dict(episodes=5, max_length=12, longest_at_least=2, num_actions=3, zero_step=None, seed=7300),
}
PAGE_FIELDS = ("mdp_id", "sequence_number", "logged_propensities", "logged_rewards", "action_mask", "model_propensities",
               "model_values")


def _draw(c, seed):
    """-> dict of the page's tensors (sorted by episode) and the episode lengths"""
    g = torch.Generator().manual_seed(seed)
    E, A = c["episodes"], c["num_actions"]
    lengths = [1, int(torch.randint(c["longest_at_least"], c["max_length"] + 1, (1,), generator=g))]
    lengths += torch.randint(1, c["max_length"] + 1, (E - 2,), generator=g).tolist()
    lengths = [lengths[i] for i in torch.randperm(E, generator=g).tolist()]
    N = sum(lengths)
    logged_policy = torch.softmax(0.7 * torch.randn(N, A, generator=g), 1)
    target_policy = torch.softmax(1.5 * torch.randn(N, A, generator=g), 1)
    logged = torch.multinomial(logged_policy, 1, generator=g).reshape(-1)
    base = torch.linspace(0.2, 1.0, A)
    rewards = base[logged] + 0.3 * torch.randn(N, generator=g)
    rows = torch.arange(N)
    if c["zero_step"] is not None:
        start = 0
        for n in lengths:
            if n > c["zero_step"]:
                x = start + c["zero_step"]
                target_policy[x, logged[x]] = 0.0
                target_policy[x] /= target_policy[x].sum()
            start += n
    # the target policy's true values where every step's reward depends on its action alone: q_t(a) = base[a] + gamma v_{t+1}
    q = torch.zeros(N, A)
    start = 0
    for n in lengths:
        v = 0.0
        for x in range(start + n - 1, start - 1, -1):
            q[x] = base + GAMMA * v
            v = float((target_policy[x] * q[x]).sum())
        start += n
    model_values = q * (1.0 + BIAS) + 0.05 * torch.randn(N, A, generator=g)
    mdp = torch.repeat_interleave(torch.arange(len(lengths)) + 500, torch.tensor(lengths))
    seq = torch.cat([torch.arange(n) + 1 for n in lengths])
    page = dict(mdp_id=mdp.reshape(N, 1).to(torch.int64), sequence_number=seq.reshape(N, 1).to(torch.int64),
                logged_propensities=logged_policy[rows, logged].reshape(N, 1), logged_rewards=rewards.reshape(N, 1),
                action_mask=torch.nn.functional.one_hot(logged, A).float(), model_propensities=target_policy,
                model_values=model_values)
    return page, lengths


def _reference_page(page):
    from reagent.evaluation.evaluation_data_page import EvaluationDataPage

    N = page["mdp_id"].shape[0]
    return EvaluationDataPage(model_rewards=torch.zeros_like(page["model_values"]),
                              model_rewards_for_logged_action=torch.zeros(N, 1), **page)


def _run_reference(page, flag):
    """-> arrays of one value of the self-normalize flag"""
    import scipy as sp
    import scipy.optimize  # noqa: F401
    from reagent.evaluation import weighted_sequential_doubly_robust_estimator as ref

    edp = _reference_page(page)
    out = {}
    for J in NUM_J_STEPS:
        est = ref.WeightedSequentialDoublyRobustEstimator(GAMMA)
        calls = []
        inner = est.compute_weighted_doubly_robust_point_estimate

        def seen(j_steps, num_j_steps, j_step_returns, infinite_step_returns, j_step_return_trajectories, _inner=inner,
                 _calls=calls):
            value = _inner(j_steps, num_j_steps, j_step_returns, infinite_step_returns, j_step_return_trajectories)
            _calls.append((list(j_steps), np.array(j_step_returns), np.array(infinite_step_returns),
                           np.array(j_step_return_trajectories), value))
            return value

        est.compute_weighted_doubly_robust_point_estimate = seen
        np.random.seed(1234 + J)
        try:
            e = est.estimate(edp, J, bool(flag))
        except ValueError as error:  # int(0.5 * num_subsets) > J: np.random.choice cannot draw that many without replacement
            out[f"est_j{J}_error"] = np.array(str(error))
            continue
        out[f"est_j{J}"] = np.array([e.raw, e.normalized, e.raw_std_error, e.normalized_std_error], dtype=np.float64)
        if J != 25:
            continue
        j_steps, jsr, inf, traj, value = calls[0]
        low, high = ref.WeightedSequentialDoublyRobustEstimator.confidence_bounds(inf, 0.9)
        bias = np.maximum(low - jsr, 0.0) + np.maximum(jsr - high, 0.0)  # the distance outside [low, high]
        cov = np.cov(traj)
        error = cov + bias.T * bias  # (quirk 2 of the estimator's docstring: b_k ** 2 on column k)
        # the reference's optimiser call with the reference's arguments: SLSQP from x = 0, default tolerances
        res = sp.optimize.minimize(fun=ref.mse_loss, x0=np.zeros(J), args=(error,), bounds=[(0, 1)] * J,
                                   constraints=[dict(type="eq", fun=lambda x: np.sum(x) - 1.0)])
        x_raw = np.array(res.x)
        assert float(np.dot(x_raw, jsr)) == value, "the repeated optimiser call is not the reference's"
        x_ref = np.clip(x_raw, 0.0, None)
        x_ref = x_ref / x_ref.sum()
        out.update(j_steps=np.array(j_steps, dtype=np.float64), j_step_returns=jsr, infinite_step_returns=inf, covariance=cov,
                   bias=bias, x_raw=x_raw, x_ref=x_ref, f_ref=np.array(ref.mse_loss(x_ref, error)),
                   bootstrap_means=np.array([c[4] for c in calls[1:]], dtype=np.float64))
        assert len(calls) == 51
        # the reference's own bootstrap step (:163-176), POPULATION_DRAWS times
        sample_size = int(0.5 * len(inf))
        rng_state = np.random.get_state()
        np.random.seed(99)
        draws = []
        for _ in range(POPULATION_DRAWS):
            idx = np.random.choice(J, sample_size, replace=False)
            idx.sort()
            draws.append(inner(j_steps=[j_steps[i] for i in idx], num_j_steps=sample_size, j_step_returns=jsr[idx],
                               infinite_step_returns=inf, j_step_return_trajectories=traj[idx]))
        np.random.set_state(rng_state)
        out["std_population"] = np.array(np.std(draws))
    return out


def check_inputs(name, c, page, lengths, arrays):
    """the conditions the committed fixtures hold -> list of the ones this draw misses"""
    bad = []
    if 1 not in lengths or max(lengths) < c["longest_at_least"] or len(set(lengths)) < 2:
        bad.append("no episode of length 1, or the longest too short, or all lengths equal")
    for f in (0, 1):
        got, want = arrays[f"sn{f}_est_j25"][2], float(arrays[f"sn{f}_std_population"])
        if not abs(got - want) <= STD_TOLERANCE * want:
            bad.append(f"sn{f}: the reference's standard error {got} is outside {STD_TOLERANCE:.3f} of {want}")
    if name == "wsdr_long":
        x, j = arrays["sn1_x_ref"], arrays["sn1_j_steps"]
        if len(set(j[x > 0.05].tolist())) < 2:
            bad.append("the MAGIC weights do not put more than 0.05 on two distinct j-steps")
        if not (arrays["sn1_bias"] != 0).any():
            bad.append("every bias term is zero")
        if max(lengths) // 24 < 2:
            bad.append("the j-step interval is below 2")
    if c["zero_step"] is not None:
        alive = sum(n > c["zero_step"] for n in lengths)
        if alive < 2 or alive == len(lengths):
            bad.append("the zero column has fewer than two episodes alive, or none padded")
        start, zero = 0, True
        for n in lengths:
            if n > c["zero_step"]:
                x = start + c["zero_step"]
                zero &= float((page["model_propensities"][x] * page["action_mask"][x]).sum()) == 0.0
            start += n
        if not zero:
            bad.append("a live episode has a non-zero target propensity at the zero step")
    return bad


def generate(name):
    from oracle import reference_harness as rh

    rh._install()
    import scipy.stats

    c = CASES[name]
    for attempt in range(200):
        seed = c["seed"] + attempt
        page, lengths = _draw(c, seed)
        arrays = {"page_" + k: page[k].numpy().copy() for k in PAGE_FIELDS}
        for f in (0, 1):
            arrays.update({f"sn{f}_{k}": v for k, v in _run_reference(page, f).items()})
        bad = check_inputs(name, c, page, lengths, arrays)
        if not bad:
            break
    assert not bad, (name, bad)
    arrays["t_ppf_95"] = np.array([scipy.stats.t.ppf(0.95, k) for k in range(1, 25)], dtype=np.float64)
    arrays["config_json"] = np.array(json.dumps(dict(c, gamma=GAMMA, bias=BIAS, drawn_seed=seed, episode_lengths=lengths)))
    return arrays


SURFACE = [
    ("reagent.evaluation.weighted_sequential_doubly_robust_estimator.WeightedSequentialDoublyRobustEstimator",
     ["__init__", "estimate", "normalize_importance_weights", "calculate_step_return", "confidence_bounds"]),
    ("reagent.evaluation.evaluator.Evaluator", ["__init__", "score_cpe"]),
]
CONSTANTS = ("NUM_SUBSETS_FOR_CB_ESTIMATES", "CONFIDENCE_INTERVAL", "NUM_BOOTSTRAP_SAMPLES", "BOOTSTRAP_SAMPLE_PCT")


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) and the
    estimator's four constants and the evaluator's number of j-steps"""
    from oracle import reference_harness as rh

    rh._install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"](SURFACE)
    from reagent.evaluation.evaluator import Evaluator
    from reagent.evaluation.weighted_sequential_doubly_robust_estimator import WeightedSequentialDoublyRobustEstimator as W

    rec["constants"] = {k: repr(getattr(W, k)) for k in CONSTANTS}
    rec["constants"]["NUM_J_STEPS_FOR_MAGIC_ESTIMATOR"] = repr(Evaluator.NUM_J_STEPS_FOR_MAGIC_ESTIMATOR)
    return rec


def main():
    check = "--check" in sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    failed = []
    for name in CASES:
        arrays = generate(name)
        path = os.path.join(OUT, name + ".npz")
        if check:
            with np.load(path) as old:
                same = sorted(old.files) == sorted(arrays) and all(
                    old[k].dtype == arrays[k].dtype and np.array_equal(old[k], arrays[k], equal_nan=old[k].dtype.kind == "f")
                    for k in arrays)
            print(name, "identical" if same else "DIFFERS")
            if not same:
                failed.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", name, os.path.getsize(path) // 1024, "KiB", json.loads(str(arrays["config_json"]))["drawn_seed"])
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("cpe_wsdr_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("cpe_wsdr_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote cpe_wsdr_signatures.json")


if __name__ == "__main__":
    main()
