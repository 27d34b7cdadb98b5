"""Seq2RewardTrainer / CompressModelTrainer / Seq2RewardNetwork against the unmodified reference (tests/golden/seq2reward/*.npz,
made by tests/golden_gen/make_seq2reward_golden.py) and against the reference's lines in float64 (tests/seq2reward_statement.py).

Each fixture is replayed through the generator path (training_step + backward + optimizer step per optimizer) and through
train_step_native.  Tolerances, as in tests/test_mdnrnn_trainer.py: losses 1e-4 |ref| + 2e-6, every parameter after every step
2e-5 absolute (no element exempted); Adam's moments, which that file does not record, 1e-4 of the tensor's largest magnitude +
2e-6.  Gradients are held to the self-calibrating bound (mdnrnn_statement.close) against the float64 statement evaluated at the
parameters the step started from; at step 0, where those are the reference's own, the fixture's gradient is additionally
within bound + the fp32 statement's error of ours."""
import dataclasses
import json
import os

import pytest
import torch

import seq2reward_statement as ST
from golden_util import GOLDEN, Golden
from mdnrnn_statement import close
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.core.parameters import Seq2RewardTrainerParameters
from reagent_amd.models.fully_connected_network import FloatFeatureFullyConnected
from reagent_amd.models.seq2reward_model import Seq2RewardNetwork
from reagent_amd.training import plumbing
from reagent_amd.training.utils import gen_permutations
from reagent_amd.training.world_model import CompressModelTrainer, Seq2RewardTrainer
from reagent_amd.training.world_model import seq2reward_trainer as S

CASES = ["seq2reward_one_layer_view_q", "seq2reward_two_layers", "seq2reward_short_plan", "seq2reward_t1_b1"]
COMPRESS = "compress_two_layers"
SIGNATURES = os.path.join(GOLDEN, "reference_records", "seq2reward_signatures.json")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _near(got, ref, what):
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    assert got.shape == ref.shape and (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 2e-6, (what, got, ref)


class _Reporter:
    def __init__(self):
        self.seen = []

    def log(self, **kw):
        self.seen.append(kw)


def _params(c):
    return Seq2RewardTrainerParameters(multi_steps=c["K"], action_names=[f"a{i}" for i in range(c["A"])],
                                       step_predict_net_size=16, **c["params"])


def _network(g, dev):
    c = g.cfg
    torch.manual_seed(c["seed"])
    net = Seq2RewardNetwork(state_dim=c["S"], action_dim=c["A"], num_hiddens=c["H"], num_hidden_layers=c["L"])
    assert [n for n, _ in net.named_parameters()] == json.loads(str(g.a("net_names_json")))
    for i, p in enumerate(net.parameters()):  # the same seed gives the reference's initial weights, bit for bit
        assert torch.equal(_bits(p), _bits(g.t(f"init_net_{i}"))), i
    return net.to(dev)


def _make(g, dev):
    """-> (network, trainer, the trained groups [(name, parameters)]) at the fixture's initial weights"""
    c = g.cfg
    net = _network(g, dev)
    if "compress" in c:
        mlp = FloatFeatureFullyConnected(c["S"], c["A"], c["compress"], ["relu"] * len(c["compress"]))
        tr = CompressModelTrainer(mlp, net, _params(c))
        groups = [("mlp", list(mlp.parameters()))]
    else:
        tr = Seq2RewardTrainer(net, _params(c))
        groups = [("net", list(net.parameters())), ("step", list(tr.step_predict_network.parameters()))]
    names = json.loads(str(g.a("names_json")))
    with torch.no_grad():
        for group, ps in groups:
            assert len(ps) == len(names[group])
            for i, p in enumerate(ps):
                p.copy_(g.t(f"init_{group}_{i}"))
    tr.to(dev)
    return net, tr, groups


def _batch(g, prefix, dev):
    pre = f"{prefix}_batch_"
    b = {k[len(pre):]: g.t(k) for k in g.z.files if k.startswith(pre)}
    b["step"] = None
    return b, synthetic.to_seq2reward_input(b, dev)


def _statement(net, c, dtype):
    m = ST.Statement(c["S"], c["A"], c["H"], c["L"])
    m.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return m.to(dtype)


def _statement_grads(net, groups, c, b, dtype, group):
    """the reference's lines in dtype at the current parameters -> (loss, gradients of the group's parameters)"""
    bd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items() if v is not None}
    if group == "net":
        m = _statement(net, c, dtype)
        loss = m.mse_loss(bd, c["params"].get("gamma", 1.0))
        ps = list(m.parameters())
    else:
        ps = [p.detach().cpu().to(dtype).requires_grad_(True) for p in dict(groups)[group]]
        if group == "step":
            loss = ST.step_entropy_loss(ps, bd)
        else:
            with torch.no_grad():
                target = ST.flat_q(_statement(net, c, dtype), bd["state"][0], gen_permutations(c["K"], c["A"]))
            loss = torch.nn.functional.mse_loss(ST.mlp(ps, bd["state"][0]), target)
    loss.backward()
    return loss.detach(), [p.grad for p in ps]


LOSS_OF = {"net": "mse", "step": "step_entropy", "mlp": "mse"}


def _replay(name, dev, native, ratios=None, reporter=True):
    """-> per step (losses, parameters and moments after the step), all on the host; checks them against the recording"""
    g = Golden(os.path.join("seq2reward", name))
    c = g.cfg
    net, tr, groups = _make(g, dev)
    rep = _Reporter()
    if reporter:
        tr.set_reporter(rep)
    opts = tr.native_optimizers() if native else [o["optimizer"] for o in tr.configure_optimizers()]
    out = []
    for s in range(c["steps"]):
        b, batch = _batch(g, f"step{s}", dev)
        want = {grp: (_statement_grads(net, groups, c, b, torch.float64, grp), _statement_grads(net, groups, c, b, torch.float32, grp))
                for grp, _ in groups}
        losses, grads = {}, {}
        if native:
            got = tr.train_step_native(batch)
            losses = {k: v.detach().cpu() for k, v in got.items()}
            # (each segment's gradients are still published when the step returns: the two networks are disjoint)
            grads = {grp: [p.grad.detach().cpu().clone() for p in ps] for grp, ps in groups}
        else:
            for k, ((grp, ps), opt) in enumerate(zip(groups, opts)):
                loss = tr.training_step(batch, s, k)
                opt.zero_grad()
                loss.backward()
                grads[grp] = [p.grad.detach().cpu().clone() for p in ps]
                opt.step()
                losses[grp] = loss.detach().cpu()
        if "compress" in c:
            lv = {"mlp": losses["mse_loss"] if native else losses["mlp"]}
        else:
            lv = {"net": losses["mse_loss"] if native else losses["net"], "step": losses["step_entropy_loss"] if native else losses["step"]}
        for grp, ps in groups:
            (l64, g64), (l32, g32) = want[grp]
            close(lv[grp], l64, l32, f"{name} step {s} {grp} loss")
            ref = g.t(f"step{s}_loss_{LOSS_OF[grp]}").item()
            assert abs(lv[grp].item() - ref) <= 1e-4 * abs(ref) + 2e-6, (name, s, grp, lv[grp].item(), ref)
            for i, (gr, a, b32) in enumerate(zip(grads[grp], g64, g32)):
                bound, own = close(gr, a, b32, f"{name} step {s} grad {grp} {i}", ratios)
                if s == 0:
                    assert (gr.double() - g.t(f"step0_grad_{grp}_{i}").double()).abs().max().item() <= bound + own, (name, grp, i)
        after = {}
        for (grp, ps), opt in zip(groups, opts):
            for i, p in enumerate(ps):
                err = (p.detach().cpu() - g.t(f"step{s}_param_{grp}_{i}")).abs().max().item()
                assert err <= 2e-5, (name, s, grp, i, err)
                _near(opt.state[p]["exp_avg"].cpu(), g.t(f"step{s}_m_{grp}_{i}"), (name, s, grp, i, "exp_avg"))
                _near(opt.state[p]["exp_avg_sq"].cpu(), g.t(f"step{s}_v_{grp}_{i}"), (name, s, grp, i, "exp_avg_sq"))
            after[grp] = [p.detach().cpu().clone() for p in ps] + [opt.state[p]["exp_avg"].cpu().clone() for p in ps]
        if reporter and not native:  # the generator path hands the reporter the reference's keys and values
            logged = rep.seen.pop()
            assert not rep.seen
            recorded = {k[len(f"step{s}_report_"):]: g.t(k) for k in g.z.files if k.startswith(f"step{s}_report_")}
            assert set(logged) == set(recorded), (sorted(logged), sorted(recorded))
            for k, v in recorded.items():
                _near(logged[k], v, (name, s, k))
        out.append((lv, after))
    assert tr.all_batches_processed == c["steps"] and not rep.seen
    return out, net, tr, g


@pytest.mark.parametrize("native", [False, True], ids=["generator", "native"])
@pytest.mark.parametrize("name", CASES + [COMPRESS])
def test_replay_matches_the_reference(backend, name, native):
    ratios = []
    _, net, tr, g = _replay(name, backend.device, native, ratios)
    print(f"{name}: largest gradient error-to-bound ratio {max(ratios):.3f}")
    c, dev = g.cfg, backend.device
    b, held = _batch(g, "held", dev)
    # planning at the parameters the replay ended with: the recording, and the float64 statement at OUR parameters
    q = S.get_Q(net, held.state.float_features[0], gen_permutations(c["K"], c["A"]))
    _near(q.cpu(), g.t("held_q"), (name, "held_q"))
    permut = gen_permutations(c["K"], c["A"])
    close(q, ST.flat_q(_statement(net, c, torch.float64), b["state"][0].double(), permut),
          ST.flat_q(_statement(net, c, torch.float32), b["state"][0], permut), f"{name} get_Q")
    rep = _Reporter()
    tr.set_reporter(rep)
    val = tr.validation_step(held, 0)
    assert len(val) == 4 and all(isinstance(v, (float, list)) for v in val)
    for i, v in enumerate(val):
        _near(v, g.t(f"val_{i}"), (name, "validation_step", i))
    dist = 3 if "compress" not in c else 2
    assert val[dist] == g.t(f"val_{dist}").tolist()  # the action distribution: equal
    logged = rep.seen.pop()
    recorded = {k[len("val_report_"):]: g.t(k) for k in g.z.files if k.startswith("val_report_")}
    assert set(logged) == set(recorded) and all(k.startswith("eval_") for k in logged)
    for k, v in recorded.items():
        _near(logged[k], v, (name, k))


@pytest.mark.parametrize("name", CASES + [COMPRESS])
def test_both_paths_give_the_same_bits(backend, name):
    (a, *_), (b, *_) = _replay(name, backend.device, False), _replay(name, backend.device, True, reporter=False)
    for (la, pa), (lb, pb) in zip(a, b):
        for grp in la:
            assert torch.equal(_bits(la[grp]), _bits(lb[grp])), grp
            for x, y in zip(pa[grp], pb[grp]):
                assert torch.equal(_bits(x), _bits(y)), grp


def test_the_embeddings_gradient_reaches_map_linear(backend):
    """every layer starts from map_linear(state[0]): its gradient is the sum of the layers' dh0, within the bound of
    autograd's on the float64 statement, and not zero"""
    g = Golden(os.path.join("seq2reward", "seq2reward_two_layers"))
    c, dev = g.cfg, backend.device
    net, tr, groups = _make(g, dev)
    b, batch = _batch(g, "step0", dev)
    loss = tr.get_mse_loss(batch)
    assert loss.requires_grad
    loss.backward()
    (_, g64), (_, g32) = (_statement_grads(net, groups, c, b, dt, "net") for dt in (torch.float64, torch.float32))
    names = [n for n, _ in net.named_parameters()]
    for n in ("map_linear.weight", "map_linear.bias"):
        i = names.index(n)
        gr = dict(net.named_parameters())[n].grad
        assert gr.abs().max().item() > 1e-3
        close(gr, g64[i], g32[i], n)
    assert c["L"] == 2


def test_state_dict_round_trip_with_a_torch_lstm(backend):
    rec = json.load(open(SIGNATURES))["reagent.models.seq2reward_model.Seq2RewardNetwork"]["state_dict"]
    torch.manual_seed(3)
    net = Seq2RewardNetwork(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=2)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == rec
    m = ST.Statement(3, 2, 4, 2)  # torch's own nn.LSTM and nn.Linear under the reference's names
    m.load_state_dict(net.state_dict(), strict=True)
    torch.manual_seed(4)
    other = Seq2RewardNetwork(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=2).to(backend.device)
    other.load_state_dict(m.state_dict(), strict=True)
    lstm = torch.nn.LSTM(2, 4, 2)
    lstm.load_state_dict({k[len("rnn."):]: v for k, v in other.state_dict().items() if k.startswith("rnn.")}, strict=True)
    for a, b in zip(net.parameters(), other.parameters()):
        assert torch.equal(_bits(a), _bits(b))
    s, a = torch.randn(3, 5, 3), torch.randn(3, 5, 2)
    v = torch.tensor([1, 3, 2, 3, 1])
    with torch.no_grad():
        ref, ref_v = m(s, a), m(s, a, v)
    dev = backend.device
    got = other(rlt.FeatureData(s.to(dev)), rlt.FeatureData(a.to(dev)))
    assert isinstance(got, rlt.Seq2RewardOutput) and got.acc_reward.shape == (5, 1) and not got.acc_reward.requires_grad
    assert (got.acc_reward.cpu() - ref).abs().max() < 1e-5
    got_v = other(rlt.FeatureData(s.to(dev)), rlt.FeatureData(a.to(dev)), v.to(dev))
    assert (got_v.acc_reward.cpu() - ref_v).abs().max() < 1e-5
    h0, c0 = other.get_initial_hidden_state(s[0][None].to(dev), batch_size=5)
    assert h0.shape == c0.shape == (2, 5, 4) and not c0.any() and torch.equal(h0[0], h0[1])
    assert (h0[0].cpu() - m.map_linear(s[0]).detach()).abs().max() < 1e-5
    proto = other.input_prototype()
    assert proto[0].float_features.shape == (1, 1, 3) and proto[1].float_features.shape == (1, 1, 2)


def test_nothing_moves_to_the_host_without_a_reporter(backend):
    """train_step_native and the generator path with no reporter call none of Tensor.item / tolist / numpy (the reference
    calls .cpu().item() on every loss on every step)"""
    g = Golden(os.path.join("seq2reward", "seq2reward_one_layer_view_q"))
    dev = backend.device
    net, tr, groups = _make(g, dev)
    _, batch = _batch(g, "step0", dev)
    opts = [o["optimizer"] for o in tr.configure_optimizers()]
    tr.train_step_native(batch)  # (first use builds the slabs and optimizers)
    for k, opt in enumerate(opts):
        tr.training_step(batch, 0, k).backward()
        opt.step()
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        for fn in ("item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, fn, lambda self, *a, _fn=fn, **k: calls.append(_fn) or 0.0)
        tr.train_step_native(batch)
        for k, opt in enumerate(opts):
            loss = tr.training_step(batch, 1, k)
            opt.zero_grad()
            loss.backward()
    assert calls == []
    tr.set_reporter(_Reporter())
    list(tr.train_step_gen(batch, 2))
    assert set(tr.reporter.seen.pop()) == {"mse_loss", "step_entropy_loss", "q_values"}


def test_reporter_keys_of_the_compress_trainer(backend):
    g = Golden(os.path.join("seq2reward", COMPRESS))
    net, tr, _ = _make(g, backend.device)
    _, batch = _batch(g, "step0", backend.device)
    tr.set_reporter(_Reporter())
    loss = next(tr.train_step_gen(batch, 0))
    logged = tr.reporter.seen.pop()
    assert set(logged) == {"mse_loss", "accuracy"} and logged["mse_loss"] == loss.item() and 0.0 <= logged["accuracy"] <= 1.0
    with torch.no_grad():
        mse, acc = tr.get_loss(batch)
    assert not mse.requires_grad and mse.shape == () and acc.shape == ()
    first = CompressModelTrainer.extract_state_first_step(batch)
    assert isinstance(first, rlt.FeatureData) and first.float_features.shape == (g.cfg["B"], g.cfg["S"])
    assert tr.warm_start_components() == [] and Seq2RewardTrainer(net, _params(g.cfg)).warm_start_components() == ["seq2reward_network"]


def test_signatures_match_the_reference():
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
    assert checked == 21

    def default(f):
        return repr(f.default_factory()) if f.default is dataclasses.MISSING else repr(f.default)

    want = rec["reagent.core.parameters.Seq2RewardTrainerParameters"]["fields"]
    assert [[f.name, default(f)] for f in dataclasses.fields(Seq2RewardTrainerParameters)] == want
    assert [f.name for f in dataclasses.fields(rlt.Seq2RewardOutput)] == rec["reagent.core.types.Seq2RewardOutput"]["fields"]
    p = gen_permutations(2, 3)
    assert p.shape == (2, 9, 3) and p.dtype == torch.float32 and gen_permutations(1, 4).shape == (1, 4, 4)
    assert p.argmax(-1).t().tolist() == [[i, j] for i in range(3) for j in range(3)] and torch.equal(p.sum(-1), torch.ones(2, 9))
    assert torch.equal(gen_permutations(1, 4)[0], torch.eye(4))


def test_synthetic_batch():
    b = synthetic.seq2reward_batch(4, 9, 3, 3, seed=1)
    assert b["action"].shape == (4, 9, 3) and torch.equal(b["action"].sum(-1), torch.ones(4, 9))
    v = b["valid_step"]
    assert v.shape == (9, 1) and v.dtype == torch.int64 and v.min() == 1 and v.max() == 4 and v.unique().numel() > 2
    assert b["reward"].shape == (4, 9)
    again = synthetic.seq2reward_batch(4, 9, 3, 3, seed=1)
    assert torch.equal(again["reward"], b["reward"])  # seeded
    x = synthetic.to_seq2reward_input(b)
    assert isinstance(x, rlt.MemoryNetworkInput) and torch.equal(x.valid_step, v) and len(x) == 9
    assert synthetic.seq2reward_batch(4, 9, 3, 3, seed=1, max_valid_step=2)["valid_step"].max() == 2


def test_refusals_by_name(backend):
    dev = backend.device
    ok = dict(state_dim=3, action_dim=2, num_hiddens=4, num_hidden_layers=1)
    for change, text in ((dict(num_hiddens=257), "num_hiddens 257"), (dict(num_hiddens=0), "num_hiddens 0"),
                         (dict(num_hidden_layers=5), "num_hidden_layers 5"), (dict(num_hidden_layers=0), "num_hidden_layers 0")):
        with pytest.raises(NotImplementedError, match=text):
            Seq2RewardNetwork(**dict(ok, **change))
    Seq2RewardNetwork(**dict(ok, num_hiddens=256, num_hidden_layers=4))
    net = Seq2RewardNetwork(**ok).to(dev)
    mlp = FloatFeatureFullyConnected(3, 2, [8], ["relu"]).to(dev)
    names = lambda n: [f"a{i}" for i in range(n)]  # noqa: E731
    P = Seq2RewardTrainerParameters
    for make in (lambda p: Seq2RewardTrainer(net, p), lambda p: CompressModelTrainer(mlp, net, p)):
        with pytest.raises(NotImplementedError, match="0 actions"):
            make(P(action_names=[]))
        with pytest.raises(NotImplementedError, match="33 actions"):
            make(P(action_names=names(33)))
        with pytest.raises(NotImplementedError, match=r"2 \*\* 21 action sequences"):
            make(P(action_names=names(2), multi_steps=21))
        with pytest.raises(NotImplementedError, match=r"2 \*\* 0 action sequences"):
            make(P(action_names=names(2), multi_steps=0))
        with pytest.raises(NotImplementedError, match="multi_steps 33"):
            make(P(action_names=names(1), multi_steps=33))
        S.check_planning_limits(2, 20, "limits"), S.check_planning_limits(32, 4, "limits")  # 2^20 sequences: the most
        tr = make(P(action_names=names(2), multi_steps=2))
        with pytest.raises(NotImplementedError, match="data-parallel"):
            tr.enable_data_parallel()
        with pytest.raises(NotImplementedError, match="HIP graph"):
            plumbing.enable_graph_mode(tr)
    with pytest.raises(NotImplementedError, match="reagent_amd Seq2RewardNetwork"):
        Seq2RewardTrainer(torch.nn.LSTM(2, 4), P(action_names=names(2)))
    with pytest.raises(NotImplementedError, match="reagent_amd Seq2RewardNetwork"):
        CompressModelTrainer(mlp, ST.Statement(3, 2, 4, 1), P(action_names=names(2)))
    with pytest.raises(NotImplementedError, match="FloatFeatureFullyConnected"):
        CompressModelTrainer(torch.nn.Linear(3, 2), net, P(action_names=names(2)))
    tr = Seq2RewardTrainer(net, P(action_names=names(2), multi_steps=2, learning_rate=0.01))
    opts = tr.configure_optimizers()
    assert len(opts) == 2 and all(type(o["optimizer"]).__name__ == "FusedAdam" for o in opts)
    assert [o["optimizer"].param_groups[0]["lr"] for o in opts] == [0.01, 0.01]
    assert [id(p) for p in opts[0]["optimizer"].param_groups[0]["params"]] == [id(p) for p in net.parameters()]
    assert [id(p) for p in opts[1]["optimizer"].param_groups[0]["params"]] == [id(p) for p in tr.step_predict_network.parameters()]
    assert [l.weight.shape for l in tr.step_predict_network.linears()] == [(64, 3), (64, 64), (2, 64)]
    ct = CompressModelTrainer(mlp, net, P(action_names=names(2), compress_model_learning_rate=0.02))
    (o,) = ct.configure_optimizers()
    assert o["optimizer"].param_groups[0]["lr"] == 0.02
