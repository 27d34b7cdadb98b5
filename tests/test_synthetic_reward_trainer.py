"""RewardNetTrainer and the synthetic-reward nets against the unmodified reference (tests/golden/synthetic_reward/*.npz, made
by tests/golden_gen/make_synthetic_reward_golden.py).

Each fixture is replayed through the generator path (training_step + backward + optimizer step) and through
train_step_native.  Tolerances, the rule tests/test_seq2reward_trainer.py applies to its fixtures, restated: losses
1e-4 |ref| + 2e-6, every parameter after every step 2e-5 absolute (no element exempted), Adam's moments and the net's outputs
on the held-out batch 1e-4 of the tensor's largest magnitude + 2e-6.  The first step's gradients, taken at the reference's own
initial parameters, are held to the moments' rule against the recording."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from golden_util import Golden
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.models import synthetic_reward as M
from reagent_amd.optimizer import Optimizer__Union
from reagent_amd.training import LossFunction, RewardNetTrainer, RewardNetworkTrainerParameters, plumbing

CASES = ["single_step_mse", "ngram3_layer_norm_smoothl1_threshold", "sequence_two_layers_l1", "single_step_bce",
         "ngram5_no_hidden"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _near(got, ref, what):
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    assert got.shape == ref.shape and (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 2e-6, (what, got, ref)


class _Reporter:
    def __init__(self):
        self.seen = {}
        self.best = []

    def log(self, **kw):
        self.seen.update(kw)

    def update_best_model(self, score, model):
        self.best.append((score, model))


def _build(c):
    S, A = c["S"], c["A"]
    if c["net"] == "single":
        net = M.SingleStepSyntheticRewardNet(S, A, c["sizes"], c["activations"], c["last"], use_layer_norm=c.get("layer_norm", False))
    elif c["net"] == "ngram":
        net = M.NGramFullyConnectedNetwork(S, A, c["sizes"], c["activations"], c["last"], c["context"],
                                           use_layer_norm=c.get("layer_norm", False))
    else:
        net = M.SequenceSyntheticRewardNet(S, A, c["hidden"], c["layers"], False, c["last"])
    return M.SyntheticRewardNet(net)


def _make(g, dev, load=True):
    """-> (net, trainer) at the fixture's initial weights, loaded as a state_dict under the reference's keys"""
    c = g.cfg
    torch.manual_seed(c["seed"])
    net = _build(c)
    names = json.loads(str(g.a("names_json")))
    assert list(net.state_dict().keys()) == names and [n for n, _ in net.named_parameters()] == names
    if load:
        net.load_state_dict({n: g.t(f"init_{i}") for i, n in enumerate(names)}, strict=True)
    net = net.to(dev)
    tr = RewardNetTrainer(net, optimizer=Optimizer__Union.default(lr=c["lr"]), loss_type=LossFunction[c["loss"]],
                          reward_ignore_threshold=c.get("threshold"))
    return net, tr.to(dev)


def _batch(g, prefix, dev):
    pre = f"{prefix}_batch_"
    b = {k[len(pre):]: g.t(k) for k in g.z.files if k.startswith(pre)}
    return b, synthetic.to_synthetic_reward_input(b, dev)


def _replay(name, dev, native, reporter=True):
    g = Golden(os.path.join("synthetic_reward", name))
    c = g.cfg
    net, tr = _make(g, dev)
    rep = _Reporter()
    if reporter:
        tr.set_reporter(rep)
    (opt,) = tr.native_optimizers() if native else [o["optimizer"] for o in tr.configure_optimizers()]
    params = list(net.parameters())
    out = []
    for s in range(c["steps"]):
        _, batch = _batch(g, f"step{s}", dev)
        if native:
            loss = tr.train_step_native(batch)["loss"].detach().cpu()
        else:
            loss = tr.training_step(batch, s)
            opt.zero_grad()
            loss.backward()
            opt.step()
            loss = loss.detach().cpu()
        grads = [p.grad.detach().cpu().clone() for p in params]
        ref = g.t(f"step{s}_loss").item()
        assert abs(loss.item() - ref) <= 1e-4 * abs(ref) + 2e-6, (name, s, loss.item(), ref)
        if s == 0:
            for i, gr in enumerate(grads):
                _near(gr, g.t(f"step0_grad_{i}"), (name, "grad", i))
        for i, p in enumerate(params):
            err = (p.detach().cpu() - g.t(f"step{s}_param_{i}")).abs().max().item()
            assert err <= 2e-5, (name, s, i, err)
            _near(opt.state[p]["exp_avg"].cpu(), g.t(f"step{s}_m_{i}"), (name, s, i, "exp_avg"))
            _near(opt.state[p]["exp_avg_sq"].cpu(), g.t(f"step{s}_v_{i}"), (name, s, i, "exp_avg_sq"))
        if reporter and not native:  # the generator path hands the reporter the reference's key and value
            assert set(rep.seen) == {"loss"} and rep.seen.pop("loss").item() == loss.item()
        out.append((loss, [p.detach().cpu().clone() for p in params] + [opt.state[p]["exp_avg"].cpu().clone() for p in params]))
    assert tr.all_batches_processed == c["steps"] and not rep.seen
    return out, net, tr, g


@pytest.mark.parametrize("native", [False, True], ids=["generator", "native"])
@pytest.mark.parametrize("name", CASES)
def test_replay_matches_the_reference(backend, name, native):
    _, net, tr, g = _replay(name, backend.device, native)
    c, dev = g.cfg, backend.device
    b, held = _batch(g, "held", dev)
    out = net(held)
    assert isinstance(out, rlt.SyntheticRewardNetworkOutput)
    assert out.predicted_reward.shape == (c["B"], 1) and out.mask.shape == out.output.shape == (c["B"], c["T"])
    _near(out.predicted_reward.cpu(), g.t("held_predicted_reward"), (name, "predicted_reward"))
    _near(out.output.cpu(), g.t("held_output"), (name, "output"))
    assert torch.equal(out.mask.cpu(), g.t("held_mask"))
    assert torch.equal(out.mask.cpu(), M._gen_mask(b["valid_step"], c["B"], c["T"]))
    alone = net.export_mlp()(held.state.float_features, held.action.float_features)  # the net without mask and sum
    assert torch.equal(_bits(alone), _bits(out.output))
    rep = _Reporter()
    tr.set_reporter(rep)
    val = tr.validation_step(held, 0)
    assert isinstance(val, float)
    _near(val, g.t("val_loss"), (name, "validation_step"))
    recorded = {k[len("val_report_"):]: g.t(k) for k in g.z.files if k.startswith("val_report_")}
    assert set(rep.seen) == set(recorded) == {"eval_rewards", "eval_pred_rewards", "eval_loss"}
    for k, v in recorded.items():
        _near(rep.seen[k], v, (name, k))
    tr.validation_epoch_end([val, val + 2.0])
    assert rep.best == [(val + 1.0, net)]
    assert tr.warm_start_components() == ["reward_net"]


@pytest.mark.parametrize("name", CASES)
def test_both_paths_give_the_same_bits(backend, name):
    (a, *_), (b, *_) = _replay(name, backend.device, False), _replay(name, backend.device, True, reporter=False)
    for (la, pa), (lb, pb) in zip(a, b):
        assert torch.equal(_bits(la), _bits(lb))
        for x, y in zip(pa, pb):
            assert torch.equal(_bits(x), _bits(y))


def test_fields_defaults_and_state_dict_keys_against_the_record():
    g = Golden(os.path.join("synthetic_reward", CASES[0]))
    rec = json.loads(str(g.a("record_json")))

    def default(f):
        if f.default is not dataclasses.MISSING:
            return repr(f.default)
        return f"{type(f.default_factory()).__name__}.default()"

    assert [[f.name, default(f)] for f in dataclasses.fields(RewardNetworkTrainerParameters)] == rec["RewardNetworkTrainerParameters"]
    assert [f.name for f in dataclasses.fields(rlt.SyntheticRewardNetworkOutput)] == rec["SyntheticRewardNetworkOutput"]
    assert {m.name: m.value for m in LossFunction} == rec["LossFunction"]
    # the signatures, as tests/test_reference_signatures.py reduces them; a parameter the reference defaults through
    # field(default_factory=...) defaults to None here and the constructor builds it (reagent_amd/training/parameters.py)
    from test_reference_signatures import _PARAMS

    ns = {}
    exec(_PARAMS, ns)
    checked = 0
    for path, methods in rec["signatures"].items():
        obj = ns["resolve"](path.replace("reagent.", "reagent_amd.", 1))
        for m, want in methods.items():
            got = json.loads(json.dumps(ns["params"](obj if m == "__call__" else getattr(obj, m))))
            assert [g[:2] for g in got] == [w[:2] for w in want], (path, m, got, want)
            for g_, w_ in zip(got, want):
                assert g_[2] == w_[2] or (w_[2][0] == "factory" and g_[2] == ["value", "None"]), (path, m, g_, w_)
            checked += 1
    assert checked == 17
    p = RewardNetworkTrainerParameters()
    assert p.asdict().keys() == {"optimizer", "loss_type", "reward_ignore_threshold", "weighted_by_inverse_propensity"}
    for name in CASES:  # the keys (_make); the single-step and sequence nets draw the reference's initial weights, bit for bit
        g = Golden(os.path.join("synthetic_reward", name))
        net, _ = _make(g, "cpu", load=False)
        for i, p in enumerate(net.parameters()):
            assert p.shape == g.t(f"init_{i}").shape
            if g.cfg["net"] != "ngram":  # (the n-gram net is the package's FullyConnectedNetwork: the same law, its own draw)
                assert torch.equal(_bits(p), _bits(g.t(f"init_{i}"))), (name, i)


def test_state_dict_moves_either_way(backend):
    g = Golden(os.path.join("synthetic_reward", "sequence_two_layers_l1"))
    net, _ = _make(g, backend.device)
    lstm = torch.nn.LSTM(7, 8, 2)
    lstm.load_state_dict({k[len("net.lstm."):]: v for k, v in net.state_dict().items() if k.startswith("net.lstm.")}, strict=True)
    fc_out = torch.nn.Linear(8, 1)
    fc_out.load_state_dict({k[len("net.fc_out."):]: v for k, v in net.state_dict().items() if k.startswith("net.fc_out.")}, strict=True)
    b, held = _batch(g, "held", backend.device)
    with torch.no_grad():
        want = fc_out(lstm(torch.cat((b["state"], b["action"]), dim=-1))[0]).squeeze(2).transpose(0, 1)
    got = net(held).output
    assert (got.cpu() - want).abs().max() < 1e-5


def test_validation_does_not_apply_the_threshold(backend):
    g = Golden(os.path.join("synthetic_reward", "ngram3_layer_norm_smoothl1_threshold"))
    dev = backend.device
    net, tr = _make(g, dev)
    _, batch = _batch(g, "step0", dev)
    kept = int(g.a("step0_kept"))
    assert 1 <= kept < g.cfg["B"]
    train = tr._forward(batch, training=True)
    assert int(train["n_kept"].item()) == kept
    val = tr.validation_step(batch, 0)
    free = RewardNetTrainer(net, loss_type=LossFunction.SmoothL1Loss).to(dev)  # no threshold at all
    assert val == free.validation_step(batch, 0) and val != train["loss"].item()
    out = net(batch)
    want = torch.nn.SmoothL1Loss()(out.predicted_reward.cpu(), batch.reward.cpu()).item()
    assert abs(val - want) <= 1e-5 * abs(want)
    # a threshold below every reward: the reference's assertion, where the loss is read
    low = RewardNetTrainer(net, loss_type=LossFunction.SmoothL1Loss, reward_ignore_threshold=-1e9).to(dev)
    low.set_reporter(_Reporter())
    with pytest.raises(AssertionError, match="reward ignore threshold set too small"):
        next(low.train_step_gen(batch, 0))
    low.set_reporter(None)
    loss = next(low.train_step_gen(batch, 0))  # nobody listens: the NaN stays on the device
    assert torch.isnan(loss)


def test_nothing_moves_to_the_host_without_a_reporter(backend):
    g = Golden(os.path.join("synthetic_reward", "single_step_mse"))
    dev = backend.device
    net, tr = _make(g, dev)
    _, batch = _batch(g, "step0", dev)
    (opt,) = [o["optimizer"] for o in tr.configure_optimizers()]
    tr.train_step_native(batch)  # (first use builds the slabs and optimizers)
    tr.training_step(batch, 0).backward()
    opt.step()
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        for fn in ("item", "tolist", "numpy", "cpu"):
            mp.setattr(torch.Tensor, fn, lambda self, *a, _fn=fn, **k: calls.append(_fn) or self)
        tr.train_step_native(batch)
        loss = tr.training_step(batch, 1)
        opt.zero_grad()
        loss.backward()
    assert calls == []
    tr.set_reporter(_Reporter())
    list(tr.train_step_gen(batch, 2))
    assert set(tr.reporter.seen) == {"loss"}


def test_refusals_by_name(backend):
    dev = backend.device
    ok = dict(state_dim=4, action_dim=3, lstm_hidden_size=8, lstm_num_layers=1, lstm_bidirectional=False, last_layer_activation="linear")
    for change, text in ((dict(lstm_bidirectional=True), "lstm_bidirectional"), (dict(lstm_hidden_size=257), "lstm_hidden_size 257"),
                         (dict(lstm_num_layers=5), "lstm_num_layers 5"), (dict(last_layer_activation="gelu"), "activation gelu")):
        with pytest.raises(NotImplementedError, match=text):
            M.SequenceSyntheticRewardNet(**dict(ok, **change))
    M.SequenceSyntheticRewardNet(**dict(ok, lstm_hidden_size=256, lstm_num_layers=4))
    with pytest.raises(NotImplementedError, match="context_size 4"):
        M.NGramFullyConnectedNetwork(4, 3, [8], ["relu"], "linear", 4)
    with pytest.raises(NotImplementedError, match="activation gelu"):
        M.NGramFullyConnectedNetwork(4, 3, [8], ["gelu"], "linear", 3)
    with pytest.raises(NotImplementedError, match="use_batch_norm"):
        M.SingleStepSyntheticRewardNet(4, 3, [8], ["relu"], "linear", use_batch_norm=True)
    with pytest.raises(NotImplementedError, match="activation swish"):
        M.SingleStepSyntheticRewardNet(4, 3, [8], ["relu"], "swish")
    with pytest.raises(NotImplementedError, match="reagent_amd SingleStepSyntheticRewardNet"):
        M.SyntheticRewardNet(torch.nn.Linear(7, 1))
    assert not hasattr(M, "NGramConvolutionalNetwork") and not hasattr(M, "TransformerSyntheticRewardNet")
    net = M.SyntheticRewardNet(M.SingleStepSyntheticRewardNet(4, 3, [8], ["relu"], "linear")).to(dev)
    with pytest.raises(NotImplementedError, match="reagent_amd SyntheticRewardNet"):
        RewardNetTrainer(torch.nn.Linear(7, 1))
    with pytest.raises(NotImplementedError, match="reagent_amd SyntheticRewardNet"):
        RewardNetTrainer(net.net)
    batch = synthetic.to_synthetic_reward_input(synthetic.synthetic_reward_batch(3, 5, 4, 3, seed=1), dev)
    weighted = RewardNetTrainer(net, weighted_by_inverse_propensity=True).to(dev)
    with pytest.raises(NotImplementedError, match="Sampling weighting not implemented for"):
        next(weighted.train_step_gen(batch, 0))
    with pytest.raises(NotImplementedError, match="Sampling weighting not implemented for"):
        weighted.validation_step(batch, 0)
    tr = RewardNetTrainer(net).to(dev)

    class PreprocessedRankingInput:
        slate_reward = torch.zeros(5, 1)

    with pytest.raises(NotImplementedError, match="PreprocessedRankingInput batches are not supported"):
        next(tr.train_step_gen(PreprocessedRankingInput(), 0))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.enable_data_parallel()
    with pytest.raises(NotImplementedError, match="HIP graph"):
        plumbing.enable_graph_mode(tr)
    (o,) = tr.configure_optimizers()
    assert type(o["optimizer"]).__name__ == "FusedAdam"
    assert [id(p) for p in o["optimizer"].param_groups[0]["params"]] == [id(p) for p in net.parameters()]
    out = net(batch)  # outside a trainer with grad mode on: no graph, and a backward that says so
    with pytest.raises(NotImplementedError, match="outside autograd"):
        out.predicted_reward.sum().backward()


def test_synthetic_batch():
    b = synthetic.synthetic_reward_batch(5, 12, 4, 3, seed=1)
    assert b["state"].shape == (5, 12, 4) and b["action"].shape == (5, 12, 3) and b["reward"].shape == (12, 1)
    v = b["valid_step"]
    assert v.shape == (12, 1) and v.dtype == torch.int64 and v.min() == 1 and v.max() == 5
    assert torch.equal(synthetic.synthetic_reward_batch(5, 12, 4, 3, seed=1)["reward"], b["reward"])  # seeded
    binary = synthetic.synthetic_reward_batch(5, 12, 4, 3, seed=1, binary_reward=True)
    assert (binary["reward"] >= 0).all() and (binary["reward"] <= v).all()
    seq = synthetic.synthetic_reward_batch(5, 12, 4, 3, seed=1, sequence=True)
    assert torch.equal(seq["state"], b["state"]) and not torch.equal(seq["reward"], b["reward"])
    x = synthetic.to_synthetic_reward_input(b)
    assert isinstance(x, rlt.MemoryNetworkInput) and torch.equal(x.valid_step, v) and torch.equal(x.reward, b["reward"])


def test_training_lowers_the_eval_loss(backend):
    """a short learning check at tiny sizes: the n-gram net of one step on the linear task"""
    dev = backend.device
    torch.manual_seed(0)
    net = M.SyntheticRewardNet(M.NGramFullyConnectedNetwork(4, 3, [16], ["relu"], "linear", 1)).to(dev)
    tr = RewardNetTrainer(net, optimizer=Optimizer__Union.default(lr=0.02)).to(dev)
    held = synthetic.to_synthetic_reward_input(synthetic.synthetic_reward_batch(4, 32, 4, 3, seed=999), dev)
    before = tr.validation_step(held, 0)
    for s in range(40):
        tr.train_step_native(synthetic.to_synthetic_reward_input(synthetic.synthetic_reward_batch(4, 32, 4, 3, seed=s), dev))
    after = tr.validation_step(held, 0)
    print(f"eval loss {before:.3f} -> {after:.3f}")
    assert np.isfinite(after) and after < before
