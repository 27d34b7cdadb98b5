"""TEST INFRASTRUCTURE.  Generates tests/golden/cb_deep/*.npz by running the UNMODIFIED reference
DeepRepresentLinUCBTrainer on a DeepRepresentLinearRegressionUCB (through oracle/stubs.py plus the shims of
make_cb_golden._install) on seeded synthetic bandit batches.  Run where the reference tree is present:
    python tests/golden_gen/make_deep_cb_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_deep_cb_golden.py --check    (regenerates them and compares with the committed files)

Every fixture is EPOCHS epochs of STEPS training steps and an epoch end, F = 9 raw features, an MLP of sizes [8, 8, 5]
(relu, relu, linear), A = 4 arms, B = 37 rows a batch.  Lightning's loop is emulated as
    optimizer.zero_grad(); loss = trainer.training_step(batch, i); loss.backward(); optimizer.step()
with the one optimizer configure_optimizers() returns.

Layout: config_json; heldout_x [5, A, F] (and heldout_presence [5, A] where the case masks arms);
  init_<name>: the scorer's state_dict as constructed (the MLP's random initialisation included);
  per epoch e and step s:  e<e>_s<s>_batch_<key> (the keys CBInput.from_dict reads); e<e>_s<s>_loss; what the scorer's
      forward returned inside the step, e<e>_s<s>_pred_label [B] and e<e>_s<s>_mlp_out_with_ones [B, 6]; AFTER the
      optimizer's step: e<e>_s<s>_sd_<name> for every entry of the scorer's state_dict (parameters, batch-norm statistics,
      LinUCB buffers) and e<e>_s<s>_adam_<name>_exp_avg / _exp_avg_sq / _step for every parameter Adam holds state for;
  per epoch e, after its end:  e<e>_end_<name> for the state_dict; the eval()-mode forward on heldout_x:
      e<e>_heldout_pred_label / _pred_sigma / _ucb [5, A], e<e>_heldout_mlp_out_with_ones [5, A, 6]; get_model_actions on
      that ucb (under heldout_presence): e<e>_heldout_actions [5, 1].

The layer-normed representation of drlinucb_sigmoid_bce_layernorm sums to zero in every row, so its avg_A is singular along
(0, 1, ..., 1) and the smallest eigenvalue of A_extended is l2_reg_lambda / sum_weight exactly: that case takes
l2_reg_lambda = 8 to keep cond(A_extended) under MAX_COND up to the last solve (sum_weight = 222).

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
OUT = os.path.join(GOLDEN, "cb_deep")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "deep_cb_signatures.json")

F, SIZES, ACTS, ARMS, BATCH, EPOCHS, STEPS, HELDOUT = 9, [8, 8, 5], ["relu", "relu", "linear"], 4, 37, 2, 3, 5
_BASE = dict(F=F, sizes=SIZES, activations=ACTS, arms=ARMS, batch=BATCH, epochs=EPOCHS, steps=STEPS, heldout=HELDOUT,
             weights=False, presence=False, gamma=1.0, ucb_alpha=1.0, l2_reg_lambda=1.0, lr=1e-3, weight_decay=0.0,
             loss_type="mse", output_activation="linear", use_batch_norm=True, normalize_output=True, use_layer_norm=False,
             use_skip_connections=True, nn_e2e=True, unit_labels=False)
_PLAIN = dict(use_batch_norm=False, use_skip_connections=False)
CASES = {
    "drlinucb_defaults": dict(_BASE, seed=4100),
    "drlinucb_plain_coefs_weighted": dict(_BASE, **_PLAIN, nn_e2e=False, weights=True, gamma=0.9, ucb_alpha=1.5,
                                          l2_reg_lambda=0.5, weight_decay=1e-3, seed=4200),
    "drlinucb_sigmoid_bce_layernorm": dict(_BASE, use_batch_norm=False, output_activation="sigmoid", loss_type="cross_entropy",
                                           unit_labels=True, use_layer_norm=True, l2_reg_lambda=8.0, seed=4300),
    "drlinucb_mae_mean_only": dict(_BASE, loss_type="mae", ucb_alpha=0.0, presence=True, seed=4400),
}
MAX_COND = 100.0
MODEL_KEYS = ("output_activation", "l2_reg_lambda", "ucb_alpha", "gamma", "use_batch_norm", "normalize_output",
              "use_layer_norm", "use_skip_connections", "nn_e2e")


def _draw(c, seed):
    """the fixture's inputs: per step a dict under CBInput.from_dict's keys, and the held-out features (arm 2 of rows 0 and
    3 a copy of arm 1: an exact tie) with their presence mask"""
    g = torch.Generator().manual_seed(seed)
    d, A, B = c["F"], c["arms"], c["batch"]
    theta = torch.randn(d, generator=g) / d ** 0.5
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
        r = chosen @ theta + 0.3 * torch.randn(B, generator=g)
        b["reward"] = (torch.sigmoid(r) if c["unit_labels"] else r).reshape(B, 1)
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


def check_inputs(c, batches, arrays, probes):
    """the conditions the committed fixtures hold -> list of the ones this draw misses.  probes: per step the
    pre-activations of the MLP's relu layers"""
    bad = []
    d = c["sizes"][-1] + 1
    eye = torch.eye(d, dtype=torch.float64)

    def cond(prefix, discounted):
        A = torch.from_numpy(arrays[prefix + "avg_A"]).double()
        sw = float(arrays[prefix + "sum_weight"][0]) / (c["gamma"] if discounted else 1.0)
        if float(torch.linalg.cond(A + c["l2_reg_lambda"] * eye / sw)) > MAX_COND:
            bad.append("cond(A_extended) above %g at %s" % (MAX_COND, prefix))

    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            if e > 0 or s > 0:  # (the very first solve inverts lambda * I / 2e-5: condition 1)
                cond(f"e{e}_s{s}_sd_", False)
            pred, label = arrays[f"e{e}_s{s}_pred_label"], arrays[f"e{e}_s{s}_batch_reward"].reshape(-1)
            if c["loss_type"] == "mae" and (np.abs(pred - label) < 1e-3).any():
                bad.append("an mae residual within 1e-3 of its kink")
            if c["output_activation"] == "sigmoid" and not ((pred >= 0.02) & (pred <= 0.98)).all():
                bad.append("a sigmoid output outside [0.02, 0.98]")
        cond(f"e{e}_end_", True)
        ucb = arrays[f"e{e}_heldout_ucb"]
        if np.isnan(arrays[f"e{e}_heldout_pred_sigma"]).any():
            bad.append("a NaN pred_sigma")
        tie = (ucb[:, 1] == ucb[:, 2])
        if not tie.any():
            bad.append("no exact tie in the held-out scores")
        present = arrays.get("heldout_presence", np.ones_like(ucb, dtype=bool))
        top = np.where(present, ucb, -np.inf).max(1)
        if not (tie & (ucb[:, 1] == top)).any():
            bad.append("no held-out row whose tie is its maximum")
    for pre in probes:
        if (pre.abs() < 1e-4).any():
            bad.append("a pre-activation within 1e-4 of a relu kink")
            break
    for b in batches:
        if "arm_presence" in b and not b["arm_presence"][torch.arange(len(b["action"])), b["action"].reshape(-1)].all():
            bad.append("a logged action's arm is absent")
    return bad


def _generate_once(c, seed):
    _install()
    import reagent.core.types as rlt
    from reagent.gym.policies.policy import Policy
    from reagent.models.deep_represent_linucb import DeepRepresentLinearRegressionUCB
    from reagent.training.cb.deep_represent_linucb_trainer import DeepRepresentLinUCBTrainer
    from reagent.training.cb.utils import get_model_actions

    batches, held, presence = _draw(c, seed)
    torch.manual_seed(seed)
    scorer = DeepRepresentLinearRegressionUCB(c["F"], list(c["sizes"]), list(c["activations"]),
                                              **{k: c[k] for k in MODEL_KEYS})
    tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=c["lr"], weight_decay=c["weight_decay"],
                                    loss_type=c["loss_type"])
    opt = tr.configure_optimizers()
    names = {id(p): n for n, p in scorer.named_parameters()}
    probes, seen = [], []
    for m in scorer.deep_represent_layers.modules():  # the relu layers' inputs, for check_inputs
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_hook(lambda mod, inp, out: probes.append(inp[0].detach().clone()))
    inner = scorer.forward

    def recording_forward(*a, **k):  # (an attribute of the instance: the reference's classes stay as they are)
        out = inner(*a, **k)
        seen.append(out)
        return out

    scorer.forward = recording_forward
    arrays = {"heldout_x": _np(held)}
    if presence is not None:
        arrays["heldout_presence"] = _np(presence)
    for name, v in scorer.state_dict().items():
        arrays[f"init_{name}"] = _np(v)
    i = 0
    for e in range(c["epochs"]):
        scorer.train()
        for s in range(c["steps"]):
            b = batches[i]
            for k, v in b.items():
                arrays[f"e{e}_s{s}_batch_{k}"] = _np(v)
            opt.zero_grad()
            loss = tr.training_step(rlt.CBInput.from_dict({k: v.clone() for k, v in b.items()}), i)
            loss.backward()
            opt.step()
            arrays[f"e{e}_s{s}_loss"] = _np(loss).reshape(1)
            arrays[f"e{e}_s{s}_pred_label"] = _np(seen[-1]["pred_label"])
            arrays[f"e{e}_s{s}_mlp_out_with_ones"] = _np(seen[-1]["mlp_out_with_ones"])
            for name, v in scorer.state_dict().items():
                arrays[f"e{e}_s{s}_sd_{name}"] = _np(v)
            for p, st in opt.state.items():
                for k in ("exp_avg", "exp_avg_sq", "step"):
                    arrays[f"e{e}_s{s}_adam_{names[id(p)]}_{k}"] = _np(torch.as_tensor(st[k])).reshape(
                        -1 if k == "step" else st[k].shape)
            i += 1
        tr.on_train_epoch_end()
        for name, v in scorer.state_dict().items():
            arrays[f"e{e}_end_{name}"] = _np(v)
        scorer.eval()
        n_probes = len(probes)
        with torch.no_grad():
            out = scorer(held.clone())
            actions = get_model_actions(out["ucb"], presence)
        del probes[n_probes:]  # (the held-out rows may sit on a kink: nothing is differentiated there)
        for k in ("pred_label", "pred_sigma", "ucb", "mlp_out_with_ones"):
            arrays[f"e{e}_heldout_{k}"] = _np(out[k])
        arrays[f"e{e}_heldout_actions"] = _np(actions).astype(np.int64)
    return batches, arrays, probes


def generate(name):
    c = CASES[name]
    for attempt in range(200):
        seed = c["seed"] + attempt
        batches, arrays, probes = _generate_once(c, seed)
        bad = check_inputs(c, batches, arrays, probes)
        if not bad:
            break
    assert not bad, (name, bad)
    arrays["config_json"] = np.array(json.dumps(dict(c, drawn_seed=seed)))
    return arrays


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) for the trainer
    and the scorer, LOSS_TYPES' names and the scorer's state_dict as constructed (key -> shape, dtype)"""
    _install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"]([
        ("reagent.training.cb.deep_represent_linucb_trainer.DeepRepresentLinUCBTrainer",
         ["__init__", "configure_optimizers", "cb_training_step", "update_params", "apply_discounting_multiplier",
          "on_train_epoch_end", "training_step"]),
        ("reagent.models.deep_represent_linucb.DeepRepresentLinearRegressionUCB",
         ["__init__", "forward", "forward_inference", "input_prototype", "_calculate_coefs", "calculate_coefs_if_necessary"]),
    ])
    from reagent.models.deep_represent_linucb import DeepRepresentLinearRegressionUCB
    from reagent.training.cb.supervised_trainer import LOSS_TYPES

    rec["reagent.training.cb.supervised_trainer.LOSS_TYPES"] = sorted(LOSS_TYPES)
    torch.manual_seed(0)
    key = "reagent.models.deep_represent_linucb.DeepRepresentLinearRegressionUCB"
    rec[key]["state_dict"] = {}
    for tag, kw in (("defaults", {}), ("plain", dict(use_batch_norm=False, use_skip_connections=False)),
                    ("layer_norm", dict(use_batch_norm=False, use_skip_connections=False, use_layer_norm=True))):
        m = DeepRepresentLinearRegressionUCB(F, list(SIZES), list(ACTS), **kw)
        rec[key]["state_dict"][tag] = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
        rec[key].setdefault("parameters", {})[tag] = [n for n, _ in m.named_parameters()]
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
        print("deep_cb_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("deep_cb_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote deep_cb_signatures.json")


if __name__ == "__main__":
    main()
