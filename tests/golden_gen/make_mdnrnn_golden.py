"""TEST INFRASTRUCTURE.  Generates tests/golden/mdnrnn/*.npz and tests/golden/reference_records/world_model_signatures.json
by running the UNMODIFIED reference MemoryNetwork / MDNRNNTrainer (through oracle/stubs.py) on seeded synthetic batches
(reagent_amd.synthetic.memory_network_batch).  Run where the reference tree is present:

    python tests/golden_gen/make_mdnrnn_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_mdnrnn_golden.py --check    (regenerates them and compares with the committed files)

A step is what the reference's train_step_gen and Lightning do with one optimizer: get_loss(batch, state_dim), zero_grad,
backward, torch.optim.Adam(lr = params.learning_rate).step().
Layout (golden_util.Golden): config_json; names_json (the parameters' names in parameters() order); init_<i>; per step s
step<s>_batch_<key>, step<s>_loss_{gmm,bce,mse,loss}, step<s>_grad_<i> (the gradients the step applied) and step<s>_param_<i>
(the parameters after it; `params_last_step_only` keeps them for the last step alone).  `forward`: the eight fields of
MemoryNetwork.forward on a held-out batch after the last step (fwd_*), and the seven values of MDNRNN.forward on the same
batch with a non-zero hidden (hid_h0, hid_c0 -> hid_*).
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
OUT = os.path.join(GOLDEN, "mdnrnn")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "world_model_signatures.json")

CASES = {
    # (1) the defaults' shape in small; not_terminal mixed
    "mdnrnn_defaults_small": dict(L=2, G=5, H=16, S=6, A=3, T=5, B=7, steps=4, seed=11, params={}),
    # (2) one layer, one gaussian, weighted losses; the forward's outputs
    "mdnrnn_one_gaussian_weighted": dict(L=1, G=1, H=8, S=4, A=2, T=3, B=9, steps=4, seed=22, forward=True,
                                         params=dict(next_state_loss_weight=0.5, not_terminal_loss_weight=2.0,
                                                     reward_loss_weight=0.25, learning_rate=0.003)),
    # (3) fit_only_one_next_step; B crosses the 32-row tile, H is no multiple of 32
    "mdnrnn_one_next_step": dict(L=3, G=3, H=33, S=5, A=2, T=4, B=33, steps=4, seed=33, params_last_step_only=True,
                                 params=dict(fit_only_one_next_step=True)),
    # (4) the degenerate sequence
    "mdnrnn_t1_b1": dict(L=2, G=2, H=4, S=3, A=2, T=1, B=1, steps=4, seed=44, params=dict(learning_rate=0.01)),
}
LOSSES = ("gmm", "bce", "mse", "loss")


def _np(t):
    return t.detach().cpu().numpy().copy()


def batch_of(c, s):
    from reagent_amd import synthetic

    return synthetic.memory_network_batch(c["T"], c["B"], c["S"], c["A"], seed=c["seed"] * 100 + s)


def trainer_parameters(c, cls):
    return cls(hidden_size=c["H"], num_hidden_layers=c["L"], num_gaussians=c["G"], action_dim=c["A"], **c["params"])


def generate(name):
    from oracle import stubs

    stubs.install()
    import reagent.core.types as rlt
    from reagent.core.parameters import MDNRNNTrainerParameters
    from reagent.models.world_model import MemoryNetwork
    from reagent.training.world_model.mdnrnn_trainer import MDNRNNTrainer

    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = MemoryNetwork(state_dim=c["S"], action_dim=c["A"], num_hiddens=c["H"], num_hidden_layers=c["L"],
                        num_gaussians=c["G"])
    tr = MDNRNNTrainer(net, trainer_parameters(c, MDNRNNTrainerParameters))
    opt = tr.configure_optimizers()[0]
    named = list(net.mdnrnn.named_parameters())
    assert [id(p) for _, p in named] == [id(p) for g in opt.param_groups for p in g["params"]]
    arrays = {"names_json": np.array(json.dumps([n for n, _ in named]))}
    for i, (_, p) in enumerate(named):
        arrays[f"init_{i}"] = _np(p)
    for s in range(c["steps"]):
        b = batch_of(c, s)
        for k, v in b.items():
            if v is not None:
                arrays[f"step{s}_batch_{k}"] = _np(v)
        losses = tr.get_loss(rlt.MemoryNetworkInput.from_dict(b), c["S"])
        opt.zero_grad()
        losses["loss"].backward()
        for k in LOSSES:
            arrays[f"step{s}_loss_{k}"] = _np(losses[k])
        for i, (_, p) in enumerate(named):
            arrays[f"step{s}_grad_{i}"] = _np(p.grad)
        opt.step()
        if not c.get("params_last_step_only") or s == c["steps"] - 1:
            for i, (_, p) in enumerate(named):
                arrays[f"step{s}_param_{i}"] = _np(p)
    if c.get("forward"):
        b = batch_of(c, c["steps"])
        with torch.no_grad():
            out = net(rlt.FeatureData(b["state"]), rlt.FeatureData(b["action"]))
            for k, v in out.__dict__.items():
                arrays[f"fwd_{k}"] = _np(v)
            g = torch.Generator().manual_seed(c["seed"] + 1)
            h0 = torch.randn(c["L"], c["B"], c["H"], generator=g) * 0.5
            c0 = torch.randn(c["L"], c["B"], c["H"], generator=g)
            mus, sigmas, logpi, reward, not_terminal, all_h, (h_n, c_n) = net.mdnrnn(b["action"], b["state"], (h0, c0))
        arrays["hid_h0"], arrays["hid_c0"] = _np(h0), _np(c0)
        for k, v in dict(mus=mus, sigmas=sigmas, logpi=logpi, reward=reward, not_terminal=not_terminal,
                         all_steps_hidden=all_h, h_n=h_n, c_n=c_n).items():
            arrays[f"hid_{k}"] = _np(v)
    arrays["config_json"] = np.array(json.dumps(c))
    return arrays


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default) for the four
    classes, gmm_loss and transpose; MDNRNNTrainerParameters' fields with their defaults; the fields of MemoryNetworkInput
    and MemoryNetworkOutput; the state_dict keys of a MemoryNetwork with two layers"""
    import dataclasses

    from oracle import stubs

    stubs.install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    rec = ns["surface"]([
        ("reagent.models.mdn_rnn.MDNRNN", ["__init__", "forward", "get_initial_hidden_state"]),
        ("reagent.models.mdn_rnn.MDNRNNMemoryPool", ["__init__", "deque_sample", "sample_memories", "insert_into_memory"]),
        ("reagent.models.world_model.MemoryNetwork", ["__init__", "input_prototype", "forward"]),
        ("reagent.training.world_model.mdnrnn_trainer.MDNRNNTrainer",
         ["__init__", "configure_optimizers", "train_step_gen", "validation_step", "test_step", "get_loss"]),
    ])
    for fn in ("reagent.models.mdn_rnn.gmm_loss", "reagent.models.mdn_rnn.transpose"):
        rec[fn] = {"__call__": ns["params"](ns["resolve"](fn))}
    import reagent.core.types as rlt
    from reagent.core.parameters import MDNRNNTrainerParameters
    from reagent.models.mdn_rnn import MDNRNNMemorySample
    from reagent.models.world_model import MemoryNetwork

    rec["reagent.core.parameters.MDNRNNTrainerParameters"] = {
        "fields": [[f.name, repr(f.default)] for f in dataclasses.fields(MDNRNNTrainerParameters)]}
    for cls in (rlt.MemoryNetworkInput, rlt.MemoryNetworkOutput):
        rec[f"reagent.core.types.{cls.__name__}"] = {"fields": [f.name for f in dataclasses.fields(cls)]}
    rec["reagent.models.mdn_rnn.MDNRNNMemorySample"] = {"fields": list(MDNRNNMemorySample._fields)}
    net = MemoryNetwork(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=2, num_gaussians=2)
    rec["reagent.models.world_model.MemoryNetwork"]["state_dict"] = {k: list(v.shape) for k, v in net.state_dict().items()}
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
                    old[k].dtype == arrays[k].dtype and np.array_equal(old[k], arrays[k]) for k in arrays)
            print(name, "identical" if same else "DIFFERS")
            if not same:
                failed.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", name, os.path.getsize(path) // 1024, "KiB")
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("world_model_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("world_model_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote world_model_signatures.json")


if __name__ == "__main__":
    main()
