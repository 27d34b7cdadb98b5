"""TEST INFRASTRUCTURE.  Generates tests/golden/cb_eval/*.npz by running the UNMODIFIED reference trainers with an attached
PolicyEvaluator (reagent/evaluation/cb) through oracle/stubs.py plus the shims of make_cb_golden._install, on seeded
synthetic bandit batches.  Run where the reference tree is present:
    python tests/golden_gen/make_cb_eval_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_cb_eval_golden.py --check    (regenerates them and compares with the committed files)

Every fixture is EPOCHS = 2 epochs of STEPS = 4 evaluated training steps and an epoch end, A = 4 arms, B = 37 rows a batch;
d = 6 features for the LinUCB cases, the stack 9-8-5 for the deep one.  The stubbed Lightning module has no global_step, so
the generator sets it (the running step index) before every step and epoch end.

Cases:
  eval_plain           no weights, no arm_presence, no log-probabilities, no clip: the size quirk shows
  eval_full            weights, arm_presence, action_log_probability, max_importance_weight = 3 (some rows clipped, some not),
                       eval_model_update_critical_weight = 60 (the frozen model is replaced mid-epoch), gamma = 0.9
  eval_presence_ties   arm_presence without log-probabilities (1 / slate size), the frozen model replaced before every step
                       but the first; rows 0 and 1 of step e1_s1 have two arms with identical features that are the model's
                       top two: in row 0 the logged arm is the lower index (accepted), in row 1 the higher (rejected)
  eval_deep            DeepRepresentLinUCBTrainer on a plain 9-8-5 stack, critical weight 70

Layout: config_json; log_json (every call the recording logger received, in order: {"step", "metrics"}); signatures aside.
  per epoch e and step s:  e<e>_s<s>_batch_<key> (the keys CBInput.from_dict reads); _ucb [B, A] and _model_actions [B, 1] of
      the frozen model; _importance_weight [B, 1]; _ev_<buffer> for the nine local buffers and num_eval_model_updates;
      _eval_avg_A, _eval_sum_weight of the frozen model (for the conditioning check); the scorer's buffers after the step:
      _cur_avg_A, _cur_avg_b, _cur_sum_weight, _cur_num_obs; the deep case also _loss and _sd_<key> for its state_dict
  per epoch e, after its end:  e<e>_end_ev_<buffer> for every buffer of the evaluator (the frozen model's aside),
      e<e>_end_avg_reward [1], e<e>_end_<buffer> for the scorer's state_dict
  after the last epoch: final_ev_<key> for the evaluator's whole state_dict (eval_model.* included), and ONE further step on
      a further batch: x_batch_<key>, x_ucb, x_model_actions, x_importance_weight, x_ev_<buffer>, x_cur_*.

`check_inputs` names the conditions a draw misses; the whole fixture is drawn again with another seed until none is.
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

from make_cb_golden import _install, _np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "cb_eval")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "cb_eval_signatures.json")

D, ARMS, BATCH, EPOCHS, STEPS = 6, 4, 37, 2, 4
_BASE = dict(deep=False, d=D, arms=ARMS, batch=BATCH, epochs=EPOCHS, steps=STEPS, weights=False, presence=False, logp=False,
             max_importance_weight=None, critical_weight=None, ties=False, gamma=1.0, ucb_alpha=1.0, l2_reg_lambda=1.0)
_DEEP = dict(deep=True, d=9, sizes=[8, 5], activations=["relu", "linear"], lr=1e-3, weight_decay=0.0, loss_type="mse",
             output_activation="linear", use_batch_norm=False, normalize_output=True, use_layer_norm=False,
             use_skip_connections=False, nn_e2e=True)
CASES = {
    "eval_plain": dict(_BASE, seed=5100),
    "eval_full": dict(_BASE, weights=True, presence=True, logp=True, max_importance_weight=3.0, critical_weight=60.0,
                      gamma=0.9, ucb_alpha=1.5, l2_reg_lambda=0.5, seed=5200),
    "eval_presence_ties": dict(_BASE, presence=True, critical_weight=30.0, ties=True, ucb_alpha=2.0, seed=5300),
    "eval_deep": dict(_BASE, **_DEEP, critical_weight=70.0, seed=5400),
}
TIE_STEP, TIE_ARMS = (1, 1), (1, 3)  # (epoch, step) of the planted rows 0 and 1; the two arms with identical features
MAX_COND = 100.0
GAP = 1e-3
MODEL_KEYS = ("output_activation", "l2_reg_lambda", "ucb_alpha", "gamma", "use_batch_norm", "normalize_output",
              "use_layer_norm", "use_skip_connections", "nn_e2e")
LOCAL = ("sum_weight_all_data_local", "sum_reward_weighted_all_data_local", "sum_size_weighted_all_data_local",
         "sum_reward_importance_weighted_accepted_local", "sum_reward_weighted_accepted_local", "sum_weight_accepted_local",
         "sum_importance_weight_accepted_local", "sum_size_weighted_accepted_local", "sum_weight_since_update_local")
BUFFERS_STEP = ("cur_avg_A", "cur_avg_b", "cur_sum_weight", "cur_num_obs")


def _draw(c, seed):
    """the fixture's inputs: per step (and one further step) a dict under CBInput.from_dict's keys"""
    g = torch.Generator().manual_seed(seed)
    d, A, B = c["d"], c["arms"], c["batch"]
    theta = torch.randn(d, generator=g) / (d ** 0.5 if c["deep"] else 1.0)
    batches = []
    for i in range(c["epochs"] * c["steps"] + 1):
        x = torch.randn(B, A, d, generator=g)
        b = {"context_arm_features": x}
        if c["presence"]:
            b["arm_presence"] = (torch.rand(B, A, generator=g) < 0.7)
        action = torch.randint(0, A, (B, 1), generator=g)
        if c["ties"] and i == TIE_STEP[0] * c["steps"] + TIE_STEP[1]:
            lo, hi = TIE_ARMS
            for row, logged in ((0, lo), (1, hi)):
                x[row, lo] = 3.0 * torch.randn(d, generator=g)
                x[row, hi] = x[row, lo]
                b["arm_presence"][row, lo] = b["arm_presence"][row, hi] = True
                action[row, 0] = logged
        if c["presence"]:  # the logged arm is present
            b["arm_presence"][torch.arange(B), action.reshape(-1)] = True
        b["action"] = action
        chosen = torch.gather(x, 1, action.unsqueeze(-1).expand(-1, 1, d)).squeeze(1)
        b["reward"] = (chosen @ theta + 0.3 * torch.randn(B, generator=g)).reshape(B, 1)
        if c["weights"]:
            b["weight"] = 0.5 + torch.rand(B, 1, generator=g)
        if c["logp"]:
            b["action_log_probability"] = torch.log(0.1 + 0.9 * torch.rand(B, 1, generator=g))
        batches.append(b)
    return batches


def _steps(c):
    return [f"e{e}_s{s}_" for e in range(c["epochs"]) for s in range(c["steps"])] + ["x_"]


def check_inputs(c, batches, arrays):
    """the conditions the committed fixtures hold -> list of the ones this draw misses"""
    bad = []
    d = (c["sizes"][-1] + 1) if c["deep"] else c["d"]
    eye = torch.eye(d, dtype=torch.float64)

    def cond(A, sw, where):
        A = torch.from_numpy(A).double()
        if float(torch.linalg.cond(A + c["l2_reg_lambda"] * eye / float(sw))) > MAX_COND:
            bad.append("cond(A_extended) above %g at %s" % (MAX_COND, where))

    for b, pre in zip(batches, _steps(c)):
        B = len(b["action"])
        present = b["arm_presence"].numpy() if "arm_presence" in b else np.ones((B, c["arms"]), dtype=bool)
        if not present[np.arange(B), b["action"].reshape(-1).numpy()].all():
            bad.append("a logged action's arm is absent")
        # acceptance must not hinge on rounding: every row's two largest ucb among its present arms are the same bits (a
        # planted tie) or GAP * (1 + max|ucb|) apart.  No row is left out.
        ucb = arrays[pre + "ucb"]
        top = np.sort(np.where(present, ucb, -np.inf), axis=1)[:, ::-1]
        if c["arms"] > 1:
            gap = top[:, 0] - top[:, 1]
            tied = top[:, 0] == top[:, 1]
            if not (tied | (gap >= GAP * (1.0 + np.abs(ucb).max()))).all():
                bad.append("a row whose two best arms are within the gap at " + pre)
            planted = np.zeros(B, dtype=bool)
            if c["ties"] and pre == "e%d_s%d_" % TIE_STEP:
                planted[:2] = True
                lo, hi = TIE_ARMS
                if not ((ucb[:2, lo] == ucb[:2, hi]) & (ucb[:2, lo] == top[:2, 0])).all():
                    bad.append("a planted tie is not its row's maximum")
            if (tied & ~planted).any():
                bad.append("a tie that was not planted at " + pre)
        iw = arrays[pre + "importance_weight"].reshape(-1)
        if (iw > 0).sum() < 3 or (iw == 0).sum() < 3:
            bad.append("fewer than 3 accepted or 3 rejected rows at " + pre)
        if np.isnan(iw).any():
            bad.append("a NaN importance weight")
        clip = c["max_importance_weight"]
        if clip is not None:
            raw = 1.0 / np.exp(b["action_log_probability"].double().numpy().reshape(-1))
            if (np.abs(raw - clip) < 1e-3 * clip).any():
                bad.append("a 1 / p within 1e-3 of the clip")
            if pre != "x_" and (not (raw > clip).any() or not (raw < clip).any()):
                bad.append("no clipped or no unclipped row at " + pre)
        if float(arrays[pre + "eval_sum_weight"][0]) > 1e-3:  # (the model as constructed inverts lambda * I / 1e-5: condition 1)
            cond(arrays[pre + "eval_avg_A"], arrays[pre + "eval_sum_weight"][0], pre + "eval model")
    for e in range(c["epochs"]):
        cond(arrays[f"e{e}_end_avg_A"], float(arrays[f"e{e}_end_sum_weight"][0]) / c["gamma"], f"e{e}_end")
    if c["critical_weight"] is not None:
        last = "e%d_s%d_" % (c["epochs"] - 1, c["steps"] - 1)
        ends = [int(arrays["e%d_s%d_ev_num_eval_model_updates" % (e, c["steps"] - 1)][0]) for e in range(c["epochs"])]
        firsts = [int(arrays["e%d_s0_ev_num_eval_model_updates" % e][0]) for e in range(c["epochs"])]
        mid = sum(ends[e] - firsts[e] for e in range(c["epochs"]))  # updates at a step other than an epoch's first
        if mid < 2:
            bad.append("fewer than two mid-epoch updates of the eval model (%s)" % arrays[last + "ev_num_eval_model_updates"])
    return bad


class _Recorder:
    def __init__(self):
        self.calls = []

    def log_metrics(self, metrics, step=None):
        self.calls.append({"step": step, "metrics": dict(metrics)})


def _generate_once(c, seed):
    _install()
    import reagent.core.types as rlt
    import reagent.training.cb.base_trainer as bt
    from reagent.evaluation.cb.policy_evaluator import PolicyEvaluator
    from reagent.gym.policies.policy import Policy

    batches = _draw(c, seed)
    torch.manual_seed(seed)
    opt = None
    arrays = {}
    if c["deep"]:
        from reagent.models.deep_represent_linucb import DeepRepresentLinearRegressionUCB
        from reagent.training.cb.deep_represent_linucb_trainer import DeepRepresentLinUCBTrainer

        scorer = DeepRepresentLinearRegressionUCB(c["d"], list(c["sizes"]), list(c["activations"]),
                                                  **{k: c[k] for k in MODEL_KEYS})
        tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=c["lr"], weight_decay=c["weight_decay"],
                                        loss_type=c["loss_type"], eval_model_update_critical_weight=c["critical_weight"])
        opt = tr.configure_optimizers()
        for name, v in scorer.state_dict().items():
            arrays[f"init_{name}"] = _np(v)
    else:
        from reagent.models.linear_regression import LinearRegressionUCB
        from reagent.training.cb.linucb_trainer import LinUCBTrainer

        scorer = LinearRegressionUCB(c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"], gamma=c["gamma"])
        tr = LinUCBTrainer(Policy(scorer=scorer, sampler=None), eval_model_update_critical_weight=c["critical_weight"])
    rec = _Recorder()
    ev = PolicyEvaluator(scorer, logger=rec, max_importance_weight=c["max_importance_weight"])
    tr.attach_eval_module(ev)
    seen = {}
    real_actions, real_step = bt.get_model_actions, tr.cb_training_step

    def recording_actions(scores, mask=None, **k):  # (names of the modules' namespaces: the reference's files stay as they are)
        out = real_actions(scores, mask, **k)
        seen["ucb"], seen["model_actions"] = scores.detach().clone(), out.detach().clone()
        return out

    def recording_step(batch, *a, **k):
        seen["importance_weight"] = batch.importance_weight.detach().clone()
        return real_step(batch, *a, **k)

    bt.get_model_actions = recording_actions
    tr.cb_training_step = recording_step

    def step(b, pre, i):
        tr.global_step = i
        for k, v in b.items():
            arrays[f"{pre}batch_{k}"] = _np(v)
        if opt is not None:
            opt.zero_grad()
        loss = tr.training_step(rlt.CBInput.from_dict({k: v.clone() for k, v in b.items()}), i)
        if opt is not None:
            loss.backward()
            opt.step()
            arrays[f"{pre}loss"] = _np(loss).reshape(1)
            for name, v in scorer.state_dict().items():
                arrays[f"{pre}sd_{name}"] = _np(v)
        arrays[f"{pre}ucb"] = _np(seen["ucb"])
        arrays[f"{pre}model_actions"] = _np(seen["model_actions"]).astype(np.int64)
        arrays[f"{pre}importance_weight"] = _np(seen["importance_weight"])
        for name in LOCAL + ("num_eval_model_updates",):
            arrays[f"{pre}ev_{name}"] = _np(getattr(ev, name))
        arrays[f"{pre}eval_avg_A"] = _np(ev.eval_model.avg_A)
        arrays[f"{pre}eval_sum_weight"] = _np(ev.eval_model.sum_weight)
        for name in BUFFERS_STEP:
            arrays[f"{pre}{name}"] = _np(getattr(scorer, name))

    try:
        i = 0
        for e in range(c["epochs"]):
            for s in range(c["steps"]):
                step(batches[i], f"e{e}_s{s}_", i)
                i += 1
            tr.global_step = i
            tr.on_train_epoch_end()
            for name, v in ev.state_dict().items():
                if not name.startswith("eval_model."):
                    arrays[f"e{e}_end_ev_{name}"] = _np(v)
            arrays[f"e{e}_end_avg_reward"] = np.array([ev.get_avg_reward()], dtype=np.float64)
            for name, v in scorer.state_dict().items():
                arrays[f"e{e}_end_{name}"] = _np(v)
        for name, v in ev.state_dict().items():
            arrays[f"final_ev_{name}"] = _np(v)
        arrays["n_log_calls_before_x"] = np.array([len(rec.calls)], dtype=np.int64)
        step(batches[i], "x_", i)
    finally:
        bt.get_model_actions = real_actions
    arrays["log_json"] = np.array(json.dumps(rec.calls))
    return batches, arrays


def generate(name):
    c = CASES[name]
    for attempt in range(200):
        seed = c["seed"] + attempt
        batches, arrays = _generate_once(c, seed)
        bad = check_inputs(c, batches, arrays)
        if not bad:
            break
    assert not bad, (name, bad)
    arrays["config_json"] = np.array(json.dumps(dict(c, drawn_seed=seed)))
    return arrays


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) for the evaluator
    classes and add_importance_weights, the evaluator's state_dict as constructed (key -> shape, dtype; the frozen model's
    aside), metric_prefix, EPSILON and the keys log_metrics hands its logger"""
    _install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    methods = ["__init__", "ingest_batch", "_aggregate_across_instances", "get_avg_reward", "update_eval_model",
               "attach_logger", "log_metrics", "get_formatted_result_string"]
    rec = ns["surface"]([("reagent.evaluation.cb.base_evaluator.BaseOfflineEval", methods),
                         ("reagent.evaluation.cb.policy_evaluator.PolicyEvaluator", methods)])
    fn = "reagent.evaluation.cb.utils.add_importance_weights"
    rec[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    import reagent.evaluation.cb.policy_evaluator as pe
    from reagent.models.linear_regression import LinearRegressionUCB

    log = _Recorder()
    ev = pe.PolicyEvaluator(LinearRegressionUCB(3), logger=log)
    key = "reagent.evaluation.cb.policy_evaluator.PolicyEvaluator"
    rec[key]["state_dict"] = {k: [list(v.shape), str(v.dtype), float(v.reshape(-1)[0])] for k, v in ev.state_dict().items()
                              if not k.startswith("eval_model.")}
    rec[key]["metric_prefix"] = ev.metric_prefix
    rec[key]["EPSILON"] = pe.EPSILON
    ev.log_metrics(step=0)
    rec[key]["logged_keys"] = list(log.calls[0]["metrics"])
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
        print("cb_eval_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("cb_eval_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote cb_eval_signatures.json")


if __name__ == "__main__":
    main()
