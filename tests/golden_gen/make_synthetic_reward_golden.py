"""TEST INFRASTRUCTURE.  Generates tests/golden/synthetic_reward/*.npz by running the UNMODIFIED reference SyntheticRewardNet,
its three fully connected / recurrent nets and RewardNetTrainer (through oracle/stubs.py) on seeded synthetic batches
(reagent_amd.synthetic.synthetic_reward_batch).  Run where the reference tree is present:

    python tests/golden_gen/make_synthetic_reward_golden.py            (writes the fixtures)
    python tests/golden_gen/make_synthetic_reward_golden.py --check    (regenerates them and compares with the committed files)

A step is what the reference's train_step_gen and Lightning do: the yielded loss, zero_grad, backward,
torch.optim.Adam.step().  Data only: inputs, the initial state_dict and recorded results.  Layout (golden_util.Golden):
config_json; names_json (the state_dict keys = the parameter names, in parameters() order); init_<i>; per step s
step<s>_batch_<key>, step<s>_loss, step<s>_kept (the rows the threshold kept), step<s>_grad_<i>, step<s>_param_<i>,
step<s>_m_<i> and step<s>_v_<i> (Adam's exp_avg and exp_avg_sq after the step); held_batch_<key> and held_predicted_reward,
held_mask, held_output = the net on a held-out batch after the last step; val_loss = validation_step's return on it and
val_report_<key> what it logged; record_json = RewardNetworkTrainerParameters' fields with their defaults,
SyntheticRewardNetworkOutput's fields, LossFunction's members, the signatures of the nets, the trainer, ngram and _gen_mask.

A condition, not a measurement: where a case sets reward_ignore_threshold, the reference keeps at least 1 and at most B - 1
rows under it on every step (asserted here, on the CPU), so the filter is exercised both ways.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "synthetic_reward")
T, B, S, A = 5, 12, 4, 3

CASES = {
    # (a) single-step [16, 8] relu, sigmoid last, MSE
    "single_step_mse": dict(net="single", sizes=[16, 8], activations=["relu", "relu"], last="sigmoid", loss="MSE", seed=41),
    # (b) n-gram of 3, [16] with layer norm, leaky_relu last, SmoothL1 under a reward_ignore_threshold
    "ngram3_layer_norm_smoothl1_threshold": dict(net="ngram", sizes=[16], activations=["relu"], last="leaky_relu", context=3,
                                                 layer_norm=True, loss="SmoothL1Loss", threshold=2.0, seed=42),
    # (c) the sequence net: two layers, H = 8, L1
    "sequence_two_layers_l1": dict(net="sequence", hidden=8, layers=2, last="linear", loss="L1Loss", sequence=True, seed=43),
    # (d) single-step on binary rewards, sigmoid, BCE
    "single_step_bce": dict(net="single", sizes=[16, 8], activations=["relu", "relu"], last="sigmoid", loss="BCELoss",
                            binary=True, seed=44),
    # (e) n-gram of 5 with no hidden layer: the head reads the n-gram rows
    "ngram5_no_hidden": dict(net="ngram", sizes=[], activations=[], last="leaky_relu", context=5, loss="MSE", seed=45),
}
STEPS, LR = 4, 0.01


def _np(t):
    return t.detach().cpu().numpy().copy()


def batch_of(c, s):
    from reagent_amd import synthetic

    return synthetic.synthetic_reward_batch(T, B, S, A, seed=c["seed"] * 100 + s, binary_reward=c.get("binary", False),
                                            sequence=c.get("sequence", False))


def build_net(c, M):
    """the case's net from module M (the reference's models.synthetic_reward, or this package's)"""
    if c["net"] == "single":
        net = M.SingleStepSyntheticRewardNet(S, A, c["sizes"], c["activations"], c["last"], use_layer_norm=c.get("layer_norm", False))
    elif c["net"] == "ngram":
        net = M.NGramFullyConnectedNetwork(S, A, c["sizes"], c["activations"], c["last"], c["context"],
                                           use_layer_norm=c.get("layer_norm", False))
    else:
        net = M.SequenceSyntheticRewardNet(S, A, c["hidden"], c["layers"], False, c["last"])
    return M.SyntheticRewardNet(net)


class _Reporter:
    def __init__(self):
        self.seen = {}

    def log(self, **kw):
        self.seen.update(kw)


def generate(name):
    from oracle import stubs

    stubs.install()
    import reagent.core.types as rlt
    import reagent.models.synthetic_reward as M
    from reagent.optimizer.union import Optimizer__Union
    from reagent.training.reward_network_trainer import LossFunction, RewardNetTrainer

    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = build_net(c, M)
    tr = RewardNetTrainer(net, optimizer=Optimizer__Union.default(lr=LR), loss_type=LossFunction[c["loss"]],
                          reward_ignore_threshold=c.get("threshold"))
    reporter = _Reporter()
    tr.set_reporter(reporter)
    (made,) = tr.configure_optimizers()
    opt = made["optimizer"]
    named = list(net.named_parameters())
    assert [id(p) for _, p in named] == [id(p) for g in opt.param_groups for p in g["params"]]
    assert [n for n, _ in named] == list(net.state_dict().keys())
    arrays = {"names_json": np.array(json.dumps([n for n, _ in named]))}
    for i, (_, p) in enumerate(named):
        arrays[f"init_{i}"] = _np(p)

    def to_input(b):
        empty = torch.tensor([])
        return rlt.MemoryNetworkInput(state=rlt.FeatureData(b["state"]), action=rlt.FeatureData(b["action"]),
                                      valid_step=b["valid_step"], reward=b["reward"], next_state=empty, step=empty,
                                      not_terminal=empty, time_diff=empty)

    for s in range(STEPS):
        b = batch_of(c, s)
        v = b["valid_step"]
        assert v.min() == 1 and v.max() == T
        for k, val in b.items():
            arrays[f"step{s}_batch_{k}"] = _np(val)
        shown = b["reward"] / v if c["loss"] == "BCELoss" else b["reward"]
        kept = B if c.get("threshold") is None else int((shown <= c["threshold"]).sum())
        if c.get("threshold") is not None:
            assert 1 <= kept <= B - 1, (name, s, kept)
        arrays[f"step{s}_kept"] = np.asarray(kept, dtype=np.int64)
        gen = tr.train_step_gen(to_input(b), s)
        loss = next(gen)
        opt.zero_grad()
        loss.backward()
        arrays[f"step{s}_loss"] = _np(loss)
        assert float(reporter.seen.pop("loss")) == float(loss.detach()) and not reporter.seen
        for i, (_, p) in enumerate(named):
            arrays[f"step{s}_grad_{i}"] = _np(p.grad)
        opt.step()
        assert next(gen, None) is None
        for i, (_, p) in enumerate(named):
            arrays[f"step{s}_param_{i}"] = _np(p)
            arrays[f"step{s}_m_{i}"] = _np(opt.state[p]["exp_avg"])
            arrays[f"step{s}_v_{i}"] = _np(opt.state[p]["exp_avg_sq"])
    held = batch_of(c, STEPS)
    for k, val in held.items():
        arrays[f"held_batch_{k}"] = _np(val)
    with torch.no_grad():
        out = net(to_input(held))
        assert [f.name for f in dataclasses.fields(out)] == ["predicted_reward", "mask", "output"]
        arrays["held_predicted_reward"], arrays["held_mask"], arrays["held_output"] = _np(out.predicted_reward), _np(out.mask), _np(out.output)
        # (inside no_grad, as Lightning runs validation: the reference gates its threshold filter on pred.requires_grad)
        arrays["val_loss"] = np.asarray(tr.validation_step(to_input(held), 0), dtype=np.float64)
    for k, val in reporter.seen.items():
        arrays[f"val_report_{k}"] = np.asarray(val, dtype=np.float64)
    arrays["config_json"] = np.array(json.dumps(dict(c, T=T, B=B, S=S, A=A, steps=STEPS, lr=LR)))
    arrays["record_json"] = np.array(json.dumps(record(), sort_keys=True))
    return arrays


def record():
    """RewardNetworkTrainerParameters' fields with their defaults (the optimizer's as its factory's name),
    SyntheticRewardNetworkOutput's fields, LossFunction's members, and the signatures of the nets, the trainer, ngram and
    _gen_mask as tests/test_reference_signatures.py reduces them (name, kind, default)"""
    import reagent.core.types as rlt
    from reagent.core.configuration import make_config_class
    from reagent.training.reward_network_trainer import LossFunction, RewardNetTrainer

    # reagent/training/parameters.py:131-133, restated: that module imports every trainer (and gym) to build the others'
    @make_config_class(RewardNetTrainer.__init__, blocklist=["reward_net"])
    class RewardNetworkTrainerParameters:
        pass

    def default(f):
        if f.default is not dataclasses.MISSING:
            return repr(f.default)
        return f"{type(f.default_factory()).__name__}.default()"

    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    nets = "reagent.models.synthetic_reward."
    signatures = ns["surface"]([
        (nets + "SyntheticRewardNet", ["__init__", "forward", "export_mlp"]),
        (nets + "SingleStepSyntheticRewardNet", ["__init__", "forward"]),
        (nets + "NGramFullyConnectedNetwork", ["__init__", "forward"]),
        (nets + "SequenceSyntheticRewardNet", ["__init__", "forward"]),
        ("reagent.training.reward_network_trainer.RewardNetTrainer",
         ["__init__", "configure_optimizers", "train_step_gen", "validation_step", "validation_epoch_end", "warm_start_components"]),
    ])
    for fn in (nets + "ngram", nets + "_gen_mask"):
        signatures[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    return {
        "signatures": signatures,
        "RewardNetworkTrainerParameters": [[f.name, default(f)] for f in dataclasses.fields(RewardNetworkTrainerParameters)],
        "SyntheticRewardNetworkOutput": [f.name for f in dataclasses.fields(rlt.SyntheticRewardNetworkOutput)],
        "LossFunction": {m.name: m.value for m in LossFunction},
    }


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
                    old[k].dtype == arrays[k].dtype and np.array_equal(old[k], arrays[k]) for k in arrays)
            print(name, "identical" if same else "DIFFERS")
            if not same:
                failed.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", name, os.path.getsize(path) // 1024, "KiB")
    if check:
        sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
