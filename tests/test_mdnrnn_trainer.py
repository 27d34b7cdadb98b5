"""MDNRNNTrainer / MemoryNetwork / MDNRNN against the unmodified reference (tests/golden/mdnrnn/*.npz, made by
tests/golden_gen/make_mdnrnn_golden.py) and against the reference's lines in float64 (tests/mdnrnn_statement.py).

Each fixture is replayed through the generator path (training_step + backward + optimizer step) and through
train_step_native.  Tolerances, as in tests/test_pdqn_trainer.py / test_pg_trainers.py: losses 1e-4 |ref| + 2e-6, every
parameter after every recorded step 2e-5 absolute (no element exempted).  Gradients are held to the self-calibrating bound of
tests/test_pg_kernels.py against the float64 statement evaluated at the parameters the step started from; at step 0, where
those are the reference's own, the fixture's gradient is additionally within bound + the fp32 statement's error of ours."""
import dataclasses
import json
import logging
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Golden
from mdnrnn_statement import Statement, close
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.core.parameters import MDNRNNTrainerParameters
from reagent_amd.models.mdn_rnn import MDNRNN, MDNRNNMemoryPool, MDNRNNMemorySample, gmm_loss, transpose  # noqa: F401
from reagent_amd.models.world_model import MemoryNetwork
from reagent_amd.training import plumbing
from reagent_amd.training.world_model import MDNRNNTrainer

CASES = ["mdnrnn_defaults_small", "mdnrnn_one_gaussian_weighted", "mdnrnn_one_next_step", "mdnrnn_t1_b1"]
LOSSES = ("gmm", "bce", "mse", "loss")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "world_model_signatures.json")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _make(g, dev):
    c = g.cfg
    torch.manual_seed(c["seed"])
    net = MemoryNetwork(state_dim=c["S"], action_dim=c["A"], num_hiddens=c["H"], num_hidden_layers=c["L"],
                        num_gaussians=c["G"])
    names = json.loads(str(g.a("names_json")))
    assert [n for n, _ in net.mdnrnn.named_parameters()] == names
    for i, p in enumerate(net.mdnrnn.parameters()):  # the same seed gives the reference's initial weights, bit for bit
        assert torch.equal(_bits(p), _bits(g.t(f"init_{i}"))), names[i]
    net = net.to(dev)
    params = MDNRNNTrainerParameters(hidden_size=c["H"], num_hidden_layers=c["L"], num_gaussians=c["G"], action_dim=c["A"],
                                     **c["params"])
    return net, MDNRNNTrainer(net, params), params


def _batch(g, s, dev):
    b = g.batch(s)
    b["step"] = None
    return b, synthetic.to_memory_network_input(b, dev)


def _statement_grads(net, c, params, b, dtype):
    """the reference's lines in dtype at the network's current parameters -> (losses, gradients in parameters() order)"""
    m = Statement(c["S"], c["A"], c["H"], c["L"], c["G"])
    m.load_state_dict({k: v.detach().cpu() for k, v in net.mdnrnn.state_dict().items()})
    m = m.to(dtype)
    bd = {k: v.to(dtype) for k, v in b.items() if v is not None}
    losses = m.losses(bd, (params.next_state_loss_weight, params.not_terminal_loss_weight, params.reward_loss_weight),
                      last_step_only=params.fit_only_one_next_step)
    losses[3].backward()
    return torch.stack([x.detach() for x in losses]), [p.grad for p in m.parameters()]


def _replay(name, dev, native, ratios=None):
    """-> per step (losses [4], parameters after the step), all on the host"""
    g = Golden(os.path.join("mdnrnn", name))
    c = g.cfg
    net, tr, params = _make(g, dev)
    opt = None if native else tr.configure_optimizers()[0]
    seen = []

    class Reporter:
        def log(self, **kw):
            seen.append(kw)

    tr.set_reporter(Reporter())
    out = []
    for s in range(c["steps"]):
        b, batch = _batch(g, s, dev)
        l64, g64 = _statement_grads(net, c, params, b, torch.float64)
        l32, g32 = _statement_grads(net, c, params, b, torch.float32)
        if native:
            losses = tr.train_step_native(batch)
            got = torch.stack([losses[k].detach().cpu() for k in LOSSES])
        else:
            loss = tr.training_step(batch, s)
            opt.zero_grad()
            loss.backward()
            logged = seen.pop()  # the generator path hands the four losses to the reporter, as the reference does
            assert set(logged) == set(LOSSES) and logged["loss"] == loss.item()
            got = torch.stack([torch.tensor(logged[k], dtype=torch.float32) for k in LOSSES])
        grads = [p.grad.detach().cpu().clone() for p in net.mdnrnn.parameters()]
        if not native:
            opt.step()
        close(got, l64, l32.detach(), f"{name} step {s} losses")
        for i, k in enumerate(LOSSES):
            ref = g.t(f"step{s}_loss_{k}").item()
            assert abs(got[i].item() - ref) <= 1e-4 * abs(ref) + 2e-6, (name, s, k, got[i].item(), ref)
        for i, (gr, a, b32) in enumerate(zip(grads, g64, g32)):
            bound, own = close(gr, a, b32, f"{name} step {s} grad {i}", ratios)
            if s == 0:
                assert (gr.double() - g.t(f"step0_grad_{i}").double()).abs().max().item() <= bound + own, (name, i)
        after = [p.detach().cpu().clone() for p in net.mdnrnn.parameters()]
        if g.has(f"step{s}_param_0"):
            for i, p in enumerate(after):
                err = (p - g.t(f"step{s}_param_{i}")).abs().max().item()
                assert err <= 2e-5, (name, s, i, err)
        out.append((got, after))
    assert tr.all_batches_processed == c["steps"]
    return out


@pytest.mark.parametrize("native", [False, True], ids=["generator", "native"])
@pytest.mark.parametrize("name", CASES)
def test_replay_matches_the_reference(backend, name, native):
    ratios = []
    _replay(name, backend.device, native, ratios)
    print(f"{name}: largest gradient error-to-bound ratio {max(ratios):.3f}")


@pytest.mark.parametrize("name", CASES)
def test_both_paths_give_the_same_bits(backend, name):
    a, b = _replay(name, backend.device, False), _replay(name, backend.device, True)
    for (la, pa), (lb, pb) in zip(a, b):
        assert torch.equal(_bits(la[3]), _bits(lb[3]))
        for x, y in zip(pa, pb):
            assert torch.equal(_bits(x), _bits(y))


def test_forward_outputs(backend):
    """MemoryNetwork.forward on a held-out batch, and MDNRNN.forward with a non-zero hidden, at the reference's last
    parameters: ours against the float64 statement under the bound the reference's own fp32 outputs calibrate"""
    g = Golden(os.path.join("mdnrnn", "mdnrnn_one_gaussian_weighted"))
    c, dev = g.cfg, backend.device
    net, _, _ = _make(g, dev)
    with torch.no_grad():
        for i, p in enumerate(net.mdnrnn.parameters()):
            p.copy_(g.t(f"step{c['steps'] - 1}_param_{i}"))
    b = synthetic.memory_network_batch(c["T"], c["B"], c["S"], c["A"], seed=c["seed"] * 100 + c["steps"])
    m = Statement(c["S"], c["A"], c["H"], c["L"], c["G"])
    m.load_state_dict({k: v.detach().cpu() for k, v in net.mdnrnn.state_dict().items()})
    m = m.double()
    with torch.no_grad():
        r64 = m(b["action"].double(), b["state"].double())
        hid64 = m(b["action"].double(), b["state"].double(), (g.t("hid_h0").double(), g.t("hid_c0").double()))
    out = net(rlt.FeatureData(b["state"].to(dev)), rlt.FeatureData(b["action"].to(dev)))
    assert isinstance(out, rlt.MemoryNetworkOutput)
    fields = dict(mus=r64[0], sigmas=r64[1], logpi=r64[2], reward=r64[3], not_terminal=r64[4], all_steps_lstm_hidden=r64[5],
                  last_step_lstm_hidden=r64[6][0], last_step_lstm_cell=r64[6][1])
    assert set(fields) == {f.name for f in dataclasses.fields(out)}
    for k, ref in fields.items():
        got = getattr(out, k)
        assert got.shape == ref.shape == g.t(f"fwd_{k}").shape, k
        close(got, ref, g.t(f"fwd_{k}"), f"forward {k}")
    got = net.mdnrnn(b["action"].to(dev), b["state"].to(dev), (g.t("hid_h0").to(dev), g.t("hid_c0").to(dev)))
    assert len(got) == 7 and len(got[6]) == 2
    flat = dict(mus=got[0], sigmas=got[1], logpi=got[2], reward=got[3], not_terminal=got[4], all_steps_hidden=got[5],
                h_n=got[6][0], c_n=got[6][1])
    ref = dict(mus=hid64[0], sigmas=hid64[1], logpi=hid64[2], reward=hid64[3], not_terminal=hid64[4],
               all_steps_hidden=hid64[5], h_n=hid64[6][0], c_n=hid64[6][1])
    for k in flat:
        assert flat[k].shape == ref[k].shape, k
        close(flat[k], ref[k], g.t(f"hid_{k}"), f"forward with hidden {k}")
    h0, c0 = net.mdnrnn.get_initial_hidden_state(batch_size=3)
    assert h0.shape == c0.shape == (c["L"], 3, c["H"]) and not h0.any() and not c0.any()
    proto = net.input_prototype()
    assert proto[0].float_features.shape == (1, 1, c["S"]) and proto[1].float_features.shape == (1, 1, c["A"])


def test_validation_and_test_steps(backend):
    g = Golden(os.path.join("mdnrnn", "mdnrnn_defaults_small"))
    net, tr, _ = _make(g, backend.device)
    _, batch = _batch(g, 0, backend.device)
    seen = []

    class Reporter:
        def log(self, **kw):
            seen.append(kw)

    tr.set_reporter(Reporter())
    before = [p.detach().clone() for p in net.parameters()]
    for step, prefix in ((tr.validation_step, "eval_"), (tr.test_step, "test_")):
        loss = step(batch, 0)
        logged = seen.pop()
        assert set(logged) == {prefix + k for k in LOSSES} and not seen
        for k in LOSSES:
            ref = g.t(f"step0_loss_{k}").item()
            assert isinstance(logged[prefix + k], float) and abs(logged[prefix + k] - ref) <= 1e-4 * abs(ref) + 2e-6, k
        assert loss.item() == logged[prefix + "loss"] and not loss.requires_grad
    assert all(p.grad is None for p in net.parameters())
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters()))
    with torch.no_grad():  # get_loss without state_dim: the gmm term undivided
        l = tr.get_loss(batch)
    assert set(l) == set(LOSSES)
    assert abs(l["loss"].item() - (l["gmm"].item() + l["bce"].item() + l["mse"].item())) <= 1e-5 * abs(l["loss"].item())
    l = tr.get_loss(batch, g.cfg["S"])  # with autograd: "loss" carries the kernels' backward
    assert l["loss"].requires_grad and not l["gmm"].requires_grad
    next(tr.train_step_gen(batch, 0))
    assert set(seen.pop()) == set(LOSSES)


def test_state_dict_round_trip_with_the_references_names(backend):
    rec = json.load(open(SIGNATURES))["reagent.models.world_model.MemoryNetwork"]["state_dict"]
    torch.manual_seed(3)
    net = MemoryNetwork(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=2, num_gaussians=2)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == rec
    m = Statement(3, 2, 4, 2, 2)  # torch's own modules under the reference's names
    m.load_state_dict(net.mdnrnn.state_dict(), strict=True)
    torch.manual_seed(4)
    other = MemoryNetwork(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=2, num_gaussians=2).to(backend.device)
    other.mdnrnn.load_state_dict(m.state_dict(), strict=True)
    for a, b in zip(net.parameters(), other.parameters()):
        assert torch.equal(_bits(a), _bits(b))
    a, s = torch.randn(2, 3, 2), torch.randn(2, 3, 3)
    with torch.no_grad():
        ref = m(a, s)
    got = other.mdnrnn(a.to(backend.device), s.to(backend.device))
    assert (got[0].cpu() - ref[0]).abs().max() < 1e-5 and (got[5].cpu() - ref[5]).abs().max() < 1e-5


def test_memory_network_input():
    b = synthetic.memory_network_batch(4, 5, 3, 2, seed=1)
    x = rlt.MemoryNetworkInput.from_dict(dict(b, mdp_id=torch.arange(5)))
    assert len(x) == 5 and x.batch_size() == 5 and x.valid_step is None and x.step is None
    assert torch.equal(x.extras.mdp_id, torch.arange(5)) and x.extras.sequence_number is None
    assert x.action.float_features.shape == (4, 5, 2) and x.state.float_features.shape == (4, 5, 3)
    flat = rlt.MemoryNetworkInput.from_dict({k: (v[0] if v is not None else None) for k, v in b.items()})
    assert len(flat) == 5
    flat.state.float_features = torch.zeros(3)
    with pytest.raises(NotImplementedError):
        len(flat)
    assert [f.name for f in dataclasses.fields(rlt.MemoryNetworkInput)] == \
        json.load(open(SIGNATURES))["reagent.core.types.MemoryNetworkInput"]["fields"]
    assert [f.name for f in dataclasses.fields(rlt.MemoryNetworkOutput)] == \
        json.load(open(SIGNATURES))["reagent.core.types.MemoryNetworkOutput"]["fields"]
    assert b["not_terminal"].unique().numel() == 2  # mixed


def test_feature_data_takes_sequences_with_one_warning(caplog):
    rlt._warned_3d = False
    with caplog.at_level(logging.WARNING, logger=rlt.__name__):
        rlt.FeatureData(torch.zeros(2, 3, 4))
        rlt.FeatureData(torch.zeros(5, 3, 4))
    assert len([r for r in caplog.records if "should be 2D" in r.getMessage()]) == 1
    for shape in ((3,), (2, 3, 4, 5)):
        with pytest.raises(ValueError, match="float_features should be 2D"):
            rlt.FeatureData(torch.zeros(*shape))
    rlt.FeatureData(torch.zeros(2, 3))


def test_signatures_match_the_reference():
    """every parameter the reference's callables take, in its order, with its kind and default (this package's MDNRNN adds
    keyword-only refusals after them)"""
    from test_reference_signatures import _PARAMS

    ns = {}
    exec(_PARAMS, ns)
    rec = json.load(open(SIGNATURES))
    checked = 0
    for path, methods in rec.items():
        ours = path.replace("reagent.", "reagent_amd.", 1)
        if "fields" in methods:
            continue
        obj = ns["resolve"](ours)
        for m, want in methods.items():
            if m == "state_dict":
                continue
            got = json.loads(json.dumps(ns["params"](obj if m == "__call__" else getattr(obj, m))))
            assert got[:len(want)] == want, (path, m, got, want)
            assert all(p[1] == "KEYWORD_ONLY" for p in got[len(want):]), (path, m, got)
            checked += 1
    assert checked == 18
    want = rec["reagent.core.parameters.MDNRNNTrainerParameters"]["fields"]
    assert [[f.name, repr(f.default)] for f in dataclasses.fields(MDNRNNTrainerParameters)] == want
    assert list(MDNRNNMemorySample._fields) == rec["reagent.models.mdn_rnn.MDNRNNMemorySample"]["fields"]


def test_memory_pool_samples_the_references_indices():
    pool = MDNRNNMemoryPool(max_replay_memory_size=6)
    rng = np.random.RandomState(0)
    for i in range(8):  # two more than fit: the oldest two leave
        pool.insert_into_memory(rng.randn(4, 3).astype(np.float32) + i, rng.randn(4, 2).astype(np.float32),
                                rng.randn(4, 3).astype(np.float32), np.full(4, float(i), dtype=np.float32),
                                np.ones(4, dtype=np.float32))
    assert pool.memory_size == 6 and pool.accu_memory_num == 8
    np.random.seed(5)
    want = np.random.randint(6, size=7)
    np.random.seed(5)
    b = pool.sample_memories(7)
    assert isinstance(b, rlt.MemoryNetworkInput) and len(b) == 7 and b.step is None
    assert b.state.float_features.shape == (4, 7, 3) and b.action.float_features.shape == (4, 7, 2)
    assert b.reward.shape == (4, 7) and torch.equal(b.reward[0], torch.as_tensor(want + 2, dtype=torch.float32))
    assert torch.equal(b.time_diff, torch.ones(4, 7)) and b.reward.dtype == torch.float32
    x, y = transpose(torch.zeros(2, 3), torch.zeros(4, 5, 6))
    assert x.shape == (3, 2) and y.shape == (5, 4, 6)


def test_refusals_by_name(backend):
    ok = dict(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=1, num_gaussians=2)
    for change, text in ((dict(num_hiddens=257), "num_hiddens 257"), (dict(num_hiddens=0), "num_hiddens 0"),
                         (dict(num_hidden_layers=5), "num_hidden_layers 5"), (dict(num_gaussians=33), "num_gaussians 33"),
                         (dict(state_dim=500, action_dim=13), "state_dim \\+ action_dim = 513"),
                         (dict(dropout=0.1), "dropout"), (dict(bidirectional=True), "bidirectional"),
                         (dict(proj_size=2), "proj_size")):
        with pytest.raises(NotImplementedError, match=text):
            MDNRNN(**dict(ok, **change))
    MDNRNN(**dict(ok, num_hiddens=256, num_hidden_layers=4, num_gaussians=32))
    net = MemoryNetwork(**ok).to(backend.device)
    tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=4, num_hidden_layers=1, num_gaussians=2))
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.enable_data_parallel()
    with pytest.raises(NotImplementedError, match="HIP graph"):
        plumbing.enable_graph_mode(tr)
    with pytest.raises(NotImplementedError, match="reagent_amd MemoryNetwork"):
        MDNRNNTrainer(torch.nn.Linear(2, 2), MDNRNNTrainerParameters())
    batch = synthetic.to_memory_network_input(synthetic.memory_network_batch(2, 3, 3, 2), backend.device)
    with pytest.raises(NotImplementedError, match="state_dim=7"):
        tr.get_loss(batch, 7)
    opt = tr.configure_optimizers()
    assert len(opt) == 1 and opt[0].param_groups[0]["lr"] == 0.001
    assert [id(p) for p in opt[0].param_groups[0]["params"]] == [id(p) for p in net.mdnrnn.parameters()]
