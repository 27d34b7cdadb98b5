"""TEST INFRASTRUCTURE.  Generates tests/golden/cb_disjoint/*.npz by running the UNMODIFIED reference DisjointLinUCBTrainer
on a DisjointLinearRegressionUCB (through oracle/stubs.py plus the shims of make_cb_golden._install) on seeded synthetic
per-arm sub-batches.  Run where the reference tree is present:
    python tests/golden_gen/make_disjoint_cb_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_disjoint_cb_golden.py --check    (regenerates them and compares with the committed files)

Every fixture is EPOCHS epochs of STEPS training steps and an epoch end (on_train_epoch_end: _estimate_coefs and the discount
of A and b), d = 6 features, 4 arms, a List[CBInput] of one sub-batch per arm a step.

Layout: config_json; heldout_x [5, d] (and heldout_presence [5, arms] where the case masks arms);
  per epoch e, step s and arm a:  e<e>_s<s>_a<a>_x [n, d], _reward [n, 1] and, where given, _weight [n, 1] (n may be 0);
  the epoch's buffers AFTER the step:  e<e>_s<s>_cur_A, _cur_b, _cur_num_obs;
  per epoch e, after its end:  e<e>_end_<name> for every entry of the scorer's state_dict (dummy_param included), the
      reference's forward on heldout_x: e<e>_heldout_scores [5, arms], and its get_model_actions on them (under
      heldout_presence): e<e>_heldout_actions [5, 1].

`generate(name)` returns the arrays without writing them; `check_inputs` names the conditions a draw misses, and the whole
fixture is drawn again with the next seed until none is missed.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_cb_golden import _install, _np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "cb_disjoint")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "disjoint_cb_signatures.json")

D, ARMS, EPOCHS, STEPS, HELDOUT = 6, 4, 2, 3, 5
_BASE = dict(d=D, arms=ARMS, epochs=EPOCHS, steps=STEPS, heldout=HELDOUT, sizes=[37, 37, 37, 37], weights=False,
             presence=False, twin_arms=False, empty=[], no_weight=[], gamma=1.0, ucb_alpha=1.0, l2_reg_lambda=1.0)
CASES = {
    "dlinucb_plain": dict(_BASE, seed=4100),
    # arms 1 and 2 get the same rows every step (an exact tie in every score); arm 3 has no rows in step 1 of each epoch;
    # arm 0 comes without weights in (epoch 0, step 2) while the others carry theirs
    "dlinucb_weighted_ragged": dict(_BASE, sizes=[37, 11, 11, 5], weights=True, twin_arms=True, gamma=0.9, ucb_alpha=1.5,
                                    l2_reg_lambda=0.5, empty=[[0, 1, 3], [1, 1, 3]], no_weight=[[0, 2, 0]], seed=4200),
    # the means alone under a presence mask; arm 3 gets no rows at all in epoch 0: its state stays zero, inv_A = I / lambda
    "dlinucb_mean_only": dict(_BASE, ucb_alpha=0.0, presence=True, empty=[[0, 0, 3], [0, 1, 3], [0, 2, 3]], seed=4300),
}
MAX_COND = 100.0
BUFFERS_STEP = ("cur_A", "cur_b", "cur_num_obs")


def _draw(c, seed):
    """the fixture's inputs: per step a list of per-arm dicts (x, reward, weight or None), and the held-out rows with their
    presence mask"""
    g = torch.Generator().manual_seed(seed)
    d, arms = c["d"], c["arms"]
    theta = torch.randn(arms, d, generator=g)
    steps = []
    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            subs = []
            for a in range(arms):
                n = 0 if [e, s, a] in c["empty"] else c["sizes"][a]
                x = torch.randn(n, d, generator=g)
                sub = {"x": x, "reward": (x @ theta[a] + 0.3 * torch.randn(n, generator=g)).reshape(n, 1), "weight": None}
                if c["weights"]:
                    w = 0.5 + torch.rand(n, 1, generator=g)
                    sub["weight"] = None if [e, s, a] in c["no_weight"] else w
                subs.append(sub)
            if c["twin_arms"]:
                subs[2] = {k: None if v is None else v.clone() for k, v in subs[1].items()}
            steps.append(subs)
    held = torch.randn(c["heldout"], d, generator=g)
    presence = None
    if c["presence"]:
        presence = torch.rand(c["heldout"], arms, generator=g) < 0.7
        presence[:, 1] = True
    return steps, held, presence


def check_inputs(c, arrays):
    """the conditions the committed fixtures hold -> list of the ones this draw misses"""
    bad = []
    eye = torch.eye(c["d"], dtype=torch.float64)
    for e in range(c["epochs"]):
        A = torch.from_numpy(arrays[f"e{e}_end_A"]).double() / c["gamma"]  # (recorded after the discount)
        for a in range(c["arms"]):
            if float(torch.linalg.cond(A[a] + c["l2_reg_lambda"] * eye)) > MAX_COND:
                bad.append("cond(A + lambda I) above %g" % MAX_COND)
        scores = arrays[f"e{e}_heldout_scores"]
        if np.isnan(scores).any():
            bad.append("a NaN score")
        if c["twin_arms"]:
            if not (scores[:, 1] == scores[:, 2]).all():
                bad.append("the twin arms' scores differ")
            present = arrays.get("heldout_presence", np.ones_like(scores, dtype=bool))
            top = np.where(present, scores, -np.inf).max(1)
            if not (present[:, 1] & (scores[:, 1] == top)).any():
                bad.append("no held-out row whose tie is its maximum")
    return bad


def _generate_once(c, seed):
    _install()
    import reagent.core.types as rlt
    from reagent.gym.policies.policy import Policy
    from reagent.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
    from reagent.training.cb.disjoint_linucb_trainer import DisjointLinUCBTrainer
    from reagent.training.cb.utils import get_model_actions

    steps, held, presence = _draw(c, seed)
    scorer = DisjointLinearRegressionUCB(c["arms"], c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"],
                                         gamma=c["gamma"])
    tr = DisjointLinUCBTrainer(Policy(scorer=scorer, sampler=None))
    arrays = {"heldout_x": _np(held)}
    if presence is not None:
        arrays["heldout_presence"] = _np(presence)
    i = 0
    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            batch = []
            for a, sub in enumerate(steps[i]):
                arrays[f"e{e}_s{s}_a{a}_x"] = _np(sub["x"])
                arrays[f"e{e}_s{s}_a{a}_reward"] = _np(sub["reward"])
                if sub["weight"] is not None:
                    arrays[f"e{e}_s{s}_a{a}_weight"] = _np(sub["weight"])
                batch.append(rlt.CBInput(context_arm_features=sub["x"].clone(), reward=sub["reward"].clone(),
                                         weight=None if sub["weight"] is None else sub["weight"].clone()))
            tr.training_step(batch, i)
            for name in BUFFERS_STEP:
                arrays[f"e{e}_s{s}_{name}"] = _np(getattr(scorer, name))
            i += 1
        tr.on_train_epoch_end()
        for name, v in scorer.state_dict().items():
            arrays[f"e{e}_end_{name}"] = _np(v)
        with torch.no_grad():
            scores = scorer(held.clone())
            actions = get_model_actions(scores, presence)
        arrays[f"e{e}_heldout_scores"] = _np(scores)
        arrays[f"e{e}_heldout_actions"] = _np(actions).astype(np.int64)
    return arrays


def generate(name):
    import warnings

    c = CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the reference's torch.tensor(y) on a tensor)
        for attempt in range(200):
            seed = c["seed"] + attempt
            arrays = _generate_once(c, seed)
            bad = check_inputs(c, arrays)
            if not bad:
                break
    assert not bad, (name, bad)
    arrays["config_json"] = np.array(json.dumps(dict(c, drawn_seed=seed)))
    return arrays


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) for the trainer,
    the scorer and batch_quadratic_form_multi_arms, and the scorer's state_dict (names, shapes, dtypes, first values)"""
    _install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"]([
        ("reagent.training.cb.disjoint_linucb_trainer.DisjointLinUCBTrainer",
         ["__init__", "configure_optimizers", "update_params", "_check_input", "cb_training_step",
          "apply_discounting_multiplier", "on_train_epoch_end"]),
        ("reagent.models.disjoint_linucb_predictor.DisjointLinearRegressionUCB",
         ["__init__", "input_prototype", "_estimate_coefs", "forward"]),
    ])
    fn = "reagent.models.disjoint_linucb_predictor.batch_quadratic_form_multi_arms"
    rec[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    from reagent.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB

    m = DisjointLinearRegressionUCB(2, 3)
    own = rec["reagent.models.disjoint_linucb_predictor.DisjointLinearRegressionUCB"]
    own["state_dict"] = {k: [list(v.shape), str(v.dtype), float(v.reshape(-1)[0])] for k, v in m.state_dict().items()}
    own["prototype_shape"] = list(m.input_prototype().shape)
    own["cur_num_obs"] = [list(m.cur_num_obs.shape), str(m.cur_num_obs.dtype)]
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
                    old[k].dtype == arrays[k].dtype and old[k].shape == arrays[k].shape
                    and np.array_equal(old[k], arrays[k], equal_nan=old[k].dtype.kind == "f") for k in arrays)
            print(name, "identical" if same else "DIFFERS")
            if not same:
                failed.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", name, sum(a.nbytes for a in arrays.values()) // 1024, "KiB")
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("disjoint_cb_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("disjoint_cb_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote disjoint_cb_signatures.json")


if __name__ == "__main__":
    main()
