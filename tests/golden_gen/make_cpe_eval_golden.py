"""TEST INFRASTRUCTURE.  Generates tests/golden/cpe_eval/*.npz by running the UNMODIFIED reference's counterfactual policy
evaluation (reagent/evaluation: EvaluationDataPage, Evaluator and its estimators; the trainers' validation_step and
gather_eval_data) through oracle/stubs.py on seeded synthetic validation batches.  Run where the reference tree is present:
    python tests/golden_gen/make_cpe_eval_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_cpe_eval_golden.py --check    (regenerates them and compares with the committed files)

Every fixture is BATCHES = 3 validation batches of ROWS = 41 rows.  The 123 rows are episodes of 1 to 12 steps (one of
length 1 at least) whose rows arrive SHUFFLED over the three batches, so `sort` matters and an episode crosses a batch
border.  The networks are as constructed (seeded): evaluation does not depend on training.

Cases:
  cpe_dqn_plain           DQNTrainer, A = 3, no extra metrics, gamma 0.9
  cpe_dqn_metrics_masks   DQNTrainer, A = 4, two extra metrics, the second with a negative mean (the `normalizer = 0` branch),
                          impossible actions (the logged one always possible), rl_temperature 0.5, reward boosts, sequence
                          gaps of 1 to 3
  cpe_qrdqn               QRDQNTrainer, 5 atoms, one extra metric

Layout: config_json; sd_<network>_<key> for the state_dicts of q_network, reward_network, q_network_cpe;
  b<i>_batch_<key>       the validation batch i as DiscreteDqnInput.from_dict reads it (mdp_id, sequence_number [41, 1] int64)
  b<i>_page_<field>      every field of the page validation_step returned for it (fields that are None are absent)
  page_<field>           the gathered page after append, sort, compute_values
  est_<target>_<estimator>   [raw, normalized, raw_std_error, normalized_std_error] (float64) for target = "reward" and every
                         extra metric's name, estimator in ESTIMATORS (weighted_doubly_robust and magic are recorded for the
                         change that builds them; nothing reads them yet)
  q_value_means, q_value_stds, action_distribution   [A] float64, in action order

`check_inputs` names the conditions a draw misses; the whole fixture is drawn again with another seed until none is.
np.random.seed is fixed before evaluate_post_training (the reference's bootstrap draws from numpy's global generator).
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
OUT = os.path.join(GOLDEN, "cpe_eval")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "cpe_eval_signatures.json")

BATCHES, ROWS = 3, 41
ESTIMATORS = ("direct_method", "inverse_propensity", "doubly_robust", "sequential_doubly_robust", "weighted_doubly_robust",
              "magic")
CHECKED = ESTIMATORS[:4]
_BASE = dict(state_dim=6, sizes=[16, 12], activations=["relu", "leaky_relu"], num_atoms=None, cpe_metrics=[],
             p_impossible=0.0, max_gap=1, lr=0.003, double_q=True)
CASES = {
    "cpe_dqn_plain": dict(_BASE, num_actions=3, rl=dict(gamma=0.9, target_update_rate=0.1, maxq_learning=True), seed=6100),
    "cpe_dqn_metrics_masks": dict(_BASE, num_actions=4, cpe_metrics=["clicks", "cost"], p_impossible=0.3, max_gap=3,
                                  rl=dict(gamma=0.85, target_update_rate=0.1, maxq_learning=True, temperature=0.5,
                                          reward_boost={"1": 0.5, "2": -0.25}), seed=6200),
    "cpe_qrdqn": dict(_BASE, num_actions=3, num_atoms=5, cpe_metrics=["m1"],
                      rl=dict(gamma=0.95, target_update_rate=0.1, maxq_learning=True), seed=6300),
}
NEGATIVE_METRIC = 1  # index of the extra metric drawn with a negative mean, where there are two
GAP = 1e-3           # the two best masked action scores of a row are at least this far apart
STD_TOLERANCE = 6.0 / np.sqrt(2.0 * 999.0)  # six standard deviations of a sample standard deviation at K = 1000


def _np(t):
    return t.detach().cpu().numpy().copy()


def _draw(c, seed):
    """-> list of BATCHES dicts under DiscreteDqnInput.from_dict's keys (rows shuffled over the batches), episode lengths"""
    g = torch.Generator().manual_seed(seed)
    N, A, S = BATCHES * ROWS, c["num_actions"], c["state_dim"]
    lengths = [1]
    while sum(lengths) < N:
        lengths.append(min(int(torch.randint(1, 13, (1,), generator=g)), N - sum(lengths)))
    mdp, seq = [], []
    for e, n in enumerate(lengths):
        start = int(torch.randint(0, 5, (1,), generator=g))
        gaps = torch.randint(1, c["max_gap"] + 1, (n,), generator=g)
        mdp += [100 + e] * n
        seq += (start + torch.cumsum(gaps, 0)).tolist()
    order = torch.randperm(N, generator=g)
    mdp = torch.tensor(mdp, dtype=torch.int64)[order].reshape(N, 1)
    seq = torch.tensor(seq, dtype=torch.int64)[order].reshape(N, 1)
    logged = torch.randint(A, (N,), generator=g)
    action = torch.nn.functional.one_hot(logged, A).float()
    pam = torch.ones(N, A)
    if c["p_impossible"] > 0:
        pam = (torch.rand(N, A, generator=g) >= c["p_impossible"]).float()
        pam[torch.arange(N), logged] = 1.0
    full = {
        "state_features": torch.randn(N, S, generator=g), "next_state_features": torch.randn(N, S, generator=g),
        "reward": 0.2 + torch.rand(N, 1, generator=g) + 0.3 * torch.randn(N, 1, generator=g),
        "time_diff": torch.ones(N, 1), "step": torch.ones(N, 1),
        "not_terminal": torch.ones(N, 1), "action": action,
        "next_action": torch.nn.functional.one_hot(torch.randint(A, (N,), generator=g), A).float(),
        "possible_actions_mask": pam, "possible_next_actions_mask": torch.ones(N, A),
        "mdp_id": mdp, "sequence_number": seq,
        "action_probability": 0.2 + 0.8 * torch.rand(N, 1, generator=g),
    }
    n_extra = len(c["cpe_metrics"])
    if n_extra:
        metrics = torch.rand(N, n_extra, generator=g)
        if n_extra > NEGATIVE_METRIC:
            metrics[:, NEGATIVE_METRIC] -= 1.0
        full["metrics"] = metrics
    batches = [{k: v[i * ROWS:(i + 1) * ROWS].clone() for k, v in full.items()} for i in range(BATCHES)]
    return batches, lengths


def _targets(c):
    return ["reward"] + list(c["cpe_metrics"])


def _estimator_inputs(arrays, c, t):
    """the gathered page's columns the estimates of target t (0 = reward, i = extra metric i - 1) are made of, float64"""
    A = c["num_actions"]
    f = lambda k: arrays["page_" + k].astype(np.float64)
    if t == 0:
        return f("logged_rewards")[:, 0], f("model_rewards"), f("model_values"), f("model_rewards_for_logged_action")[:, 0]
    i = t - 1
    # (set_metric_as_reward leaves model_rewards_for_logged_action the REWARD's: the reference's DR of a metric uses it)
    return (f("logged_metrics")[:, i], f("model_metrics")[:, i * A:(i + 1) * A], f("model_metrics_values")[:, i * A:(i + 1) * A],
            f("model_rewards_for_logged_action")[:, 0])


def float64_rows(arrays, c, t):
    """dm, ips, dr rows [N] and the per-episode sequential-DR values and episode values in float64 from the gathered page"""
    r, mr, mv, mrl = _estimator_inputs(arrays, c, t)
    p = arrays["page_model_propensities"].astype(np.float64)
    m = arrays["page_action_mask"].astype(np.float64)
    lp = arrays["page_logged_propensities"].astype(np.float64)[:, 0]
    iw = (p * m).sum(1) / lp
    dm = (p * mr).sum(1)
    ips, dr = iw * r, iw * (r - mrl) + dm
    sv, ql = (p * mv).sum(1), (mv * m).sum(1)
    mdp = arrays["page_mdp_id"].reshape(-1)
    gamma = float(np.float32(c["rl"]["gamma"]))
    bounds = [0] + (np.nonzero(mdp[1:] != mdp[:-1])[0] + 1).tolist() + [len(mdp)]
    sdr, ev = [], []
    for b, e in zip(bounds[:-1], bounds[1:]):
        d = v = 0.0
        for j in range(e - 1, b - 1, -1):
            d = sv[j] + iw[j] * (r[j] + gamma * d - ql[j])
            v = v * gamma + r[j]
        sdr.append(d)
        ev.append(v)
    return dict(direct_method=dm, inverse_propensity=ips, doubly_robust=dr, sequential_doubly_robust=np.array(sdr),
                episode_value=np.array(ev), logged=r)


def check_inputs(c, batches, lengths, arrays):
    """the conditions the committed fixtures hold -> list of the ones this draw misses"""
    bad = []
    if 1 not in lengths or max(lengths) < 8:
        bad.append("no episode of length 1 or none of 8 and more")
    ids = [set(b["mdp_id"].reshape(-1).tolist()) for b in batches]
    if not any(ids[i] & ids[j] for i in range(BATCHES) for j in range(i + 1, BATCHES)):
        bad.append("no episode crosses a batch border")
    key = [(int(m), int(s)) for b in batches for m, s in zip(b["mdp_id"].reshape(-1), b["sequence_number"].reshape(-1))]
    if key == sorted(key):
        bad.append("the rows arrive sorted")
    for i, b in enumerate(batches):
        pam, act = b["possible_actions_mask"], b["action"]
        if not (pam * act).sum(1).eq(1).all():
            bad.append("a logged action is impossible")
        q = arrays[f"b{i}_page_optimal_q_values"].astype(np.float64) + -1e9 * (1.0 - pam.numpy().astype(np.float64))
        top = np.sort(q, axis=1)[:, ::-1]
        if (top[:, 0] - top[:, 1] < GAP).any():
            bad.append("a row whose two best actions are within the gap")
    if c["p_impossible"] > 0 and not any((b["possible_actions_mask"] == 0).any() for b in batches):
        bad.append("no impossible action")
    for t, name in enumerate(_targets(c)):
        rows = float64_rows(arrays, c, t)
        mean = rows["logged"].mean()
        negative = t - 1 == NEGATIVE_METRIC
        if negative and not (mean < -0.1 and rows["episode_value"].mean() < -0.1):
            bad.append("the negative metric's mean is not negative")
        if not negative and not (mean > 0.1 and rows["episode_value"].mean() > 0.1):
            bad.append(f"the logged mean of {name} is not clearly positive")
        for est in CHECKED:
            x = rows[est]
            want = np.sqrt(x.var() / int(0.25 * len(x)))
            got = arrays[f"est_{name}_{est}"][2]
            if not abs(got - want) <= STD_TOLERANCE * want:
                bad.append(f"the reference's standard error of {name} {est} is {got}, outside 13.4 % of {want}")
    return bad


def _generate_once(c, seed):
    from oracle import reference_harness as rh

    rh._install()
    import reagent.core.types as rlt
    from reagent.evaluation.evaluation_data_page import EvaluationDataPage  # noqa: F401

    batches, lengths = _draw(c, seed)
    tr = rh.build_dqn(c["state_dim"], c["num_actions"], c["sizes"], c["activations"], c["rl"], c["lr"], double_q=c["double_q"],
                      seed=seed, num_atoms=c["num_atoms"], cpe_metrics=list(c["cpe_metrics"]))
    arrays = {}
    for net in ("q_network", "reward_network", "q_network_cpe"):
        for k, v in getattr(tr, net).state_dict().items():
            arrays[f"sd_{net}_{k}"] = _np(v)
    if not hasattr(tr, "on_gpu"):
        tr.on_gpu = False
    pages = []
    for i, b in enumerate(batches):
        for k, v in b.items():
            arrays[f"b{i}_batch_{k}"] = _np(v)
        page = tr.validation_step({k: v.clone() for k, v in b.items()}, i)
        assert isinstance(page, EvaluationDataPage)
        for k, v in page.__dict__.items():
            if isinstance(v, torch.Tensor):
                arrays[f"b{i}_page_{k}"] = _np(v)
        pages.append(page)
    gathered = tr.gather_eval_data(pages)
    for k, v in gathered.__dict__.items():
        if isinstance(v, torch.Tensor):
            arrays[f"page_{k}"] = _np(v)
    np.random.seed(seed)
    details = tr.evaluator.evaluate_post_training(gathered)
    sets = {"reward": details.reward_estimates}
    sets.update(details.metric_estimates)
    assert list(sets) == _targets(c), (list(sets), _targets(c))
    for name, s in sets.items():
        for est in ESTIMATORS:
            e = getattr(s, est)
            arrays[f"est_{name}_{est}"] = np.array([e.raw, e.normalized, e.raw_std_error, e.normalized_std_error], dtype=np.float64)
    actions = [str(i) for i in range(c["num_actions"])]
    for k in ("q_value_means", "q_value_stds", "action_distribution"):
        arrays[k] = np.array([getattr(details, k)[a] for a in actions], dtype=np.float64)
    return batches, lengths, arrays


def generate(name):
    c = CASES[name]
    for attempt in range(200):
        seed = c["seed"] + attempt
        batches, lengths, arrays = _generate_once(c, seed)
        bad = check_inputs(c, batches, lengths, arrays)
        if not bad:
            break
    assert not bad, (name, bad)
    arrays["config_json"] = np.array(json.dumps(dict(c, drawn_seed=seed, episode_lengths=lengths)))
    return arrays


SURFACE = [
    ("reagent.evaluation.evaluation_data_page.EvaluationDataPage",
     ["__init__", "create_from_training_batch", "create_from_tensors_dqn", "append", "sort", "compute_values",
      "compute_values_for_mdps", "validate", "set_metric_as_reward"]),
    ("reagent.evaluation.cpe.CpeEstimate", ["__new__"]),
    ("reagent.evaluation.cpe.CpeEstimateSet", ["__new__", "check_estimates_exist", "log", "fill_empty_with_zero"]),
    ("reagent.evaluation.cpe.CpeDetails", ["__init__", "log"]),
    ("reagent.evaluation.doubly_robust_estimator.DoublyRobustHP", ["__new__"]),
    ("reagent.evaluation.doubly_robust_estimator.DoublyRobustEstimator", ["estimate"]),
    ("reagent.evaluation.sequential_doubly_robust_estimator.SequentialDoublyRobustEstimator", ["__init__", "estimate"]),
    ("reagent.evaluation.evaluator.Evaluator", ["__init__", "evaluate_post_training", "score_cpe"]),
    ("reagent.training.dqn_trainer.DQNTrainer", ["validation_step", "gather_eval_data", "validation_epoch_end"]),
    ("reagent.training.qrdqn_trainer.QRDQNTrainer", ["validation_step", "gather_eval_data", "validation_epoch_end"]),
]


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default), the field order of
    EvaluationDataPage, CpeEstimate, CpeEstimateSet and DoublyRobustHP, and bootstrapped_std_error_of_mean's parameters"""
    from oracle import reference_harness as rh

    rh._install()
    import dataclasses

    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"](SURFACE)
    fn = "reagent.evaluation.cpe.bootstrapped_std_error_of_mean"
    rec[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    from reagent.evaluation.cpe import CpeEstimate, CpeEstimateSet
    from reagent.evaluation.doubly_robust_estimator import DoublyRobustHP
    from reagent.evaluation.evaluation_data_page import EvaluationDataPage

    rec["fields"] = {
        "EvaluationDataPage": [f.name for f in dataclasses.fields(EvaluationDataPage)],
        "CpeEstimate": list(CpeEstimate._fields), "CpeEstimateSet": list(CpeEstimateSet._fields),
        "DoublyRobustHP": list(DoublyRobustHP._fields),
        "DoublyRobustHP_defaults": {k: repr(v) for k, v in DoublyRobustHP._field_defaults.items()},
    }
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
            print("wrote", name, sum(a.nbytes for a in arrays.values()) // 1024, "KiB",
                  json.loads(str(arrays["config_json"]))["drawn_seed"])
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("cpe_eval_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("cpe_eval_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote cpe_eval_signatures.json")


if __name__ == "__main__":
    main()
