"""TEST INFRASTRUCTURE.  Generates tests/golden/cb/*.npz by running the UNMODIFIED reference LinUCBTrainer on a
LinearRegressionUCB (through oracle/stubs.py plus the four shims of `_install`) on seeded synthetic bandit batches.  Run
where the reference tree is present:
    python tests/golden_gen/make_cb_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_cb_golden.py --check    (regenerates them and compares with the committed files)

Every fixture is EPOCHS epochs of STEPS training steps and an epoch end (on_train_epoch_end: _calculate_coefs and the
discount of the total weight), d = 6 features, A = 4 arms, B = 37 rows a batch.

Layout: config_json; heldout_x [5, A, d] (and heldout_presence [5, A] where the case masks arms);
  per epoch e and step s:  e<e>_s<s>_batch_<key> (the keys CBInput.from_dict reads), and the epoch's buffers AFTER the step:
      e<e>_s<s>_cur_avg_A, _cur_avg_b, _cur_sum_weight, _cur_num_obs
  per epoch e, after its end:  e<e>_end_<buffer> for every buffer of the scorer's state_dict (dummy_param included), the
      reference's forward on heldout_x: e<e>_heldout_pred_label / _pred_sigma / _ucb [5, A], and its get_model_actions on
      that ucb (under heldout_presence): e<e>_heldout_actions [5, 1].

`generate(name)` returns the arrays without writing them; `check_inputs` names the conditions a draw misses, and the
whole fixture is drawn again with another seed until none is missed.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "cb")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "cb_signatures.json")

D, ARMS, BATCH, EPOCHS, STEPS, HELDOUT = 6, 4, 37, 2, 3, 5
_BASE = dict(d=D, arms=ARMS, batch=BATCH, epochs=EPOCHS, steps=STEPS, heldout=HELDOUT, weights=False, presence=False,
             gamma=1.0, ucb_alpha=1.0, l2_reg_lambda=1.0)
CASES = {
    "linucb_plain": dict(_BASE, seed=3100),
    "linucb_weighted_discount": dict(_BASE, weights=True, gamma=0.9, ucb_alpha=1.5, l2_reg_lambda=0.5, seed=3200),
    "linucb_mean_only": dict(_BASE, ucb_alpha=0.0, presence=True, seed=3300),
}
MAX_COND = 100.0
BUFFERS_STEP = ("cur_avg_A", "cur_avg_b", "cur_sum_weight", "cur_num_obs")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _install():
    """oracle.stubs.install_gym() plus what the contextual-bandit modules import beyond it (oracle/ is frozen, so the four
    shims live here): pytorch_lightning.utilities.distributed (ReduceOp, an identity sync_ddp_if_available),
    pytorch_lightning.loggers.LightningLoggerBase, torchrec.metrics.metric_module.RecMetricModule, and a bypass package
    for reagent.gym.policies (whose __init__ imports every policy and, through them, gym)."""
    import types

    from oracle import stubs

    stubs.install_gym()
    if getattr(sys.modules.get("reagent.gym.policies"), "_oracle_stub", False):
        return
    dist = types.ModuleType("pytorch_lightning.utilities.distributed")
    dist.ReduceOp = type("ReduceOp", (), {"SUM": "sum"})
    dist.sync_ddp_if_available = lambda result, group=None, reduce_op=None: result
    sys.modules["pytorch_lightning.utilities.distributed"] = dist
    sys.modules["pytorch_lightning.utilities"].distributed = dist
    loggers = sys.modules["pytorch_lightning.loggers"]
    if not hasattr(loggers, "LightningLoggerBase"):
        loggers.LightningLoggerBase = sys.modules["pytorch_lightning.loggers.base"].LightningLoggerBase
    sys.modules["torchrec.metrics.metric_module"].RecMetricModule = type("RecMetricModule", (), {})
    pol = types.ModuleType("reagent.gym.policies")
    pol.__path__ = [os.path.join(stubs.runtime_root(), "reagent", "gym", "policies")]
    pol._oracle_stub = True
    sys.modules["reagent.gym.policies"] = pol


def _draw(c, seed):
    """the fixture's inputs: per step a dict under CBInput.from_dict's keys, and the held-out features (arm 2 of rows 0 and
    3 a copy of arm 1: an exact tie) with their presence mask"""
    g = torch.Generator().manual_seed(seed)
    d, A, B = c["d"], c["arms"], c["batch"]
    theta = torch.randn(d, generator=g)
    batches = []
    for _ in range(c["epochs"] * c["steps"]):
        x = torch.randn(B, A, d, generator=g)
        b = {"context_arm_features": x}
        if c["presence"]:
            b["arm_presence"] = (torch.rand(B, A, generator=g) < 0.7)
        action = torch.randint(0, A, (B, 1), generator=g)
        if c["presence"]:  # the logged arm is present
            b["arm_presence"][torch.arange(B), action.reshape(-1)] = True
        b["action"] = action
        chosen = torch.gather(x, 1, action.unsqueeze(-1).expand(-1, 1, d)).squeeze(1)
        b["reward"] = (chosen @ theta + 0.3 * torch.randn(B, generator=g)).reshape(B, 1)
        if c["weights"]:
            b["weight"] = 0.5 + torch.rand(B, 1, generator=g)
            b["importance_weight"] = 0.25 + 1.5 * torch.rand(B, 1, generator=g)
        batches.append(b)
    held = torch.randn(c["heldout"], A, d, generator=g)
    held[0, 2] = held[0, 1]
    held[3, 2] = held[3, 1]
    presence = None
    if c["presence"]:
        presence = torch.rand(c["heldout"], A, generator=g) < 0.7
        presence[:, 1:3] = True
    return batches, held, presence


def check_inputs(c, batches, arrays):
    """the conditions the committed fixtures hold -> list of the ones this draw misses"""
    bad = []
    for b in batches:
        if "arm_presence" in b and not b["arm_presence"][torch.arange(len(b["action"])), b["action"].reshape(-1)].all():
            bad.append("a logged action's arm is absent")
    for e in range(c["epochs"]):
        A = torch.from_numpy(arrays[f"e{e}_end_avg_A"]).double()
        # (after the epoch end sum_weight carries the discount already: the matrix inverted used the undiscounted one)
        sw = float(arrays[f"e{e}_end_sum_weight"][0]) / c["gamma"]
        ext = A + c["l2_reg_lambda"] * torch.eye(c["d"], dtype=torch.float64) / sw
        if float(torch.linalg.cond(ext)) > MAX_COND:
            bad.append("cond(A_extended) above %g" % MAX_COND)
        if np.isnan(arrays[f"e{e}_heldout_pred_sigma"]).any():
            bad.append("a NaN pred_sigma")
        ucb = arrays[f"e{e}_heldout_ucb"]
        tie = (ucb[:, 1] == ucb[:, 2])
        if not tie.any():
            bad.append("no exact tie in the held-out scores")
        present = arrays.get("heldout_presence", np.ones_like(ucb, dtype=bool))
        top = np.where(present, ucb, -np.inf).max(1)
        if not (tie & (ucb[:, 1] == top)).any():
            bad.append("no held-out row whose tie is its maximum")
    return bad


def _generate_once(c, seed):
    _install()
    import reagent.core.types as rlt
    from reagent.gym.policies.policy import Policy
    from reagent.models.linear_regression import LinearRegressionUCB
    from reagent.training.cb.linucb_trainer import LinUCBTrainer
    from reagent.training.cb.utils import get_model_actions

    batches, held, presence = _draw(c, seed)
    scorer = LinearRegressionUCB(c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"], gamma=c["gamma"])
    tr = LinUCBTrainer(Policy(scorer=scorer, sampler=None))
    arrays = {"heldout_x": _np(held)}
    if presence is not None:
        arrays["heldout_presence"] = _np(presence)
    i = 0
    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            b = batches[i]
            for k, v in b.items():
                arrays[f"e{e}_s{s}_batch_{k}"] = _np(v)
            tr.training_step(rlt.CBInput.from_dict({k: v.clone() for k, v in b.items()}), i)
            for name in BUFFERS_STEP:
                arrays[f"e{e}_s{s}_{name}"] = _np(getattr(scorer, name))
            i += 1
        tr.on_train_epoch_end()
        for name, v in scorer.state_dict().items():
            arrays[f"e{e}_end_{name}"] = _np(v)
        with torch.no_grad():
            out = scorer(held.clone())
            actions = get_model_actions(out["ucb"], presence)
        for k in ("pred_label", "pred_sigma", "ucb"):
            arrays[f"e{e}_heldout_{k}"] = _np(out[k])
        arrays[f"e{e}_heldout_actions"] = _np(actions).astype(np.int64)
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
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) for the two
    trainer classes, the scorer, the two functions of cb/utils.py and CBInput (with its fields and prototype shape)"""
    import dataclasses

    _install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"]([
        ("reagent.training.cb.linucb_trainer.LinUCBTrainer",
         ["__init__", "configure_optimizers", "update_params", "cb_training_step", "apply_discounting_multiplier",
          "on_train_epoch_end"]),
        ("reagent.training.cb.base_trainer.BaseCBTrainerWithEval",
         ["__init__", "_check_input", "attach_eval_module", "cb_training_step", "training_step", "on_train_epoch_end"]),
        ("reagent.models.linear_regression.LinearRegressionUCB",
         ["__init__", "_calculate_coefs", "calculate_coefs_if_necessary", "_forward_no_coefs_check", "forward",
          "forward_inference", "input_prototype"]),
        ("reagent.core.types.CBInput", ["input_prototype", "from_dict"]),
    ])
    for fn in ("reagent.training.cb.utils.add_chosen_arm_features", "reagent.training.cb.utils.get_model_actions",
               "reagent.models.linear_regression.batch_quadratic_form",
               "reagent.models.linear_regression.matrix_inv_fallback_pinv"):
        rec[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    import reagent.core.types as rlt
    from reagent.models.linear_regression import LinearRegressionUCB

    rec["reagent.core.types.CBInput"]["fields"] = [f.name for f in dataclasses.fields(rlt.CBInput)]
    proto = rlt.CBInput.input_prototype(context_dim=2, batch_size=7, arm_features_dim=5, num_arms=3)
    rec["reagent.core.types.CBInput"]["prototype_shape"] = list(proto.context_arm_features.shape)
    m = LinearRegressionUCB(3)
    rec["reagent.models.linear_regression.LinearRegressionUCB"]["state_dict"] = {
        k: [list(v.shape), str(v.dtype), float(v.reshape(-1)[0])] for k, v in m.state_dict().items()}
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
            print("wrote", name, sum(a.nbytes for a in arrays.values()) // 1024, "KiB")
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("cb_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("cb_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote cb_signatures.json")


if __name__ == "__main__":
    main()
