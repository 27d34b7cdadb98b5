"""BanditRewardNetTrainer and BayesByBackpropTrainer against the unmodified reference (tests/golden/cfeval/*.npz and
tests/golden/reference_records/cfeval_signatures.json, made by tests/golden_gen/make_cfeval_golden.py).

Each fixture is replayed through the generator path (training_step + backward + optimizer step) and through
train_step_native; the Bayesian cases are fed the reference's recorded Normal(0, 1) draws through the net's noise_source.
Tolerances are tests/test_synthetic_reward_trainer.py's: losses 1e-4 |ref| + 2e-6, every parameter after every step 2e-5
absolute (no element exempted), Adam's moments and held-out outputs 1e-4 of the tensor's largest magnitude + 2e-6."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Golden
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.models import FullyConnectedDQN
from reagent_amd.models.probabilistic_fully_connected_network import FullyConnectedProbabilisticNetwork, LinearBBB
from reagent_amd.optimizer import Optimizer__Union
from reagent_amd.training import BanditRewardNetTrainer, LossFunction, plumbing
from reagent_amd.training import cfeval
from reagent_amd.training.cfeval.bayes_by_backprop_trainer import BayesByBackpropTrainer

CASES = ["bandit_mse_plain", "bandit_smoothl1_ips_threshold", "bandit_l1", "bbb_defaults", "bbb_layernorm_wide"]


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


def _make(g, dev, load=True):
    """-> (net, trainer) at the fixture's initial parameters, loaded as a state_dict under the reference's names"""
    c = g.cfg
    torch.manual_seed(c["seed"])
    if c["kind"] == "bbb":
        net = FullyConnectedProbabilisticNetwork(c["layers"], c["activations"], c["prior_var"], noise_tol=c.get("noise_tol", 0.1),
                                                 use_layer_norm=c.get("layer_norm", False))
    else:
        net = FullyConnectedDQN(c["S"], c["A"], c["sizes"], c["activations"])
    names = json.loads(str(g.a("names_json")))
    assert [n for n, _ in net.named_parameters()] == names
    if load:
        net.load_state_dict({n: g.t(f"init_{i}") for i, n in enumerate(names)}, strict=False)
    net = net.to(dev)
    opt = Optimizer__Union.default(lr=c["lr"])
    if c["kind"] == "bbb":
        tr = BayesByBackpropTrainer(net, optimizer=opt)
    else:
        tr = BanditRewardNetTrainer(net, optimizer=opt, loss_type=LossFunction[c["loss"]], reward_ignore_threshold=c.get("threshold"),
                                    weighted_by_inverse_propensity=c.get("ips", False))
    return net, tr.to(dev)


def _batch(g, prefix, dev):
    pre = f"{prefix}_batch_"
    b = {k[len(pre):]: g.t(k).to(dev) for k in g.z.files if k.startswith(pre)}
    return rlt.BanditRewardModelInput(state=rlt.FeatureData(b["state"]), action=b["action"], reward=b["reward"],
                                      action_prob=b.get("action_prob"))


def _feed(net, g, prefix):
    """the recorded draws under `prefix`, handed out in order; asserts the shapes asked for"""
    draws = g.seq(f"{prefix}_eps_")
    assert draws

    def source(shape):
        e = draws.pop(0)
        assert tuple(e.shape) == tuple(shape)
        return e

    net.noise_source = source
    return draws


def _replay(name, dev, native, reporter=True):
    g = Golden(os.path.join("cfeval", name))
    c = g.cfg
    bbb = c["kind"] == "bbb"
    net, tr = _make(g, dev)
    rep = _Reporter()
    if reporter:
        tr.set_reporter(rep)
    (opt,) = tr.native_optimizers() if native else [o["optimizer"] for o in tr.configure_optimizers()]
    params = list(net.parameters())
    out = []
    for s in range(c["steps"]):
        batch = _batch(g, f"step{s}", dev)
        left = _feed(net, g, f"step{s}") if bbb else []
        if native:
            res = tr.train_step_native(batch)
            loss = res["loss"].detach().cpu()
            unweighted = res.get("unweighted_loss")
        else:
            loss = tr.training_step(batch, s)
            opt.zero_grad()
            loss.backward()
            opt.step()
            loss = loss.detach().cpu()
            unweighted = rep.seen.get("unweighted_loss")
        assert not left
        ref = g.t(f"step{s}_loss").item()
        print(f"{name} step {s}: loss {loss.item():.7g} (reference {ref:.7g})")
        assert abs(loss.item() - ref) <= 1e-4 * abs(ref) + 2e-6, (name, s, loss.item(), ref)
        if c.get("ips") and (native or reporter):
            _near(unweighted.cpu(), g.t(f"step{s}_unweighted_loss"), (name, s, "unweighted_loss"))
        if bbb:
            for got, key in zip(net.elbo_terms(), ("log_prior", "log_post", "log_like")):
                _near(got.cpu(), g.t(f"step{s}_{key}"), (name, s, key))
        if s == 0:
            for i, p in enumerate(params):
                _near(p.grad.detach().cpu(), g.t(f"step0_grad_{i}"), (name, "grad", i))
        for i, p in enumerate(params):
            err = (p.detach().cpu() - g.t(f"step{s}_param_{i}")).abs().max().item()
            assert err <= 2e-5, (name, s, i, err)
            _near(opt.state[p]["exp_avg"].cpu(), g.t(f"step{s}_m_{i}"), (name, s, i, "exp_avg"))
            _near(opt.state[p]["exp_avg_sq"].cpu(), g.t(f"step{s}_v_{i}"), (name, s, i, "exp_avg_sq"))
        if reporter and not native:  # the generator path hands the reporter the reference's keys
            assert set(rep.seen) == ({"loss", "unweighted_loss"} if c.get("ips") else {"loss"})
            assert rep.seen["loss"].item() == loss.item()
            rep.seen.clear()
        out.append((loss, [p.detach().cpu().clone() for p in params] + [opt.state[p]["exp_avg"].cpu().clone() for p in params]))
    assert tr.all_batches_processed == c["steps"] and not rep.seen
    return out, net, tr, g


@pytest.mark.parametrize("native", [False, True], ids=["generator", "native"])
@pytest.mark.parametrize("name", CASES)
def test_replay_matches_the_reference(backend, name, native):
    _, net, tr, g = _replay(name, backend.device, native)
    c, dev = g.cfg, backend.device
    held = _batch(g, "held", dev)
    rep = _Reporter()
    tr.set_reporter(rep)
    if c["kind"] == "bbb":
        left = _feed(net, g, "val")
    val = tr.validation_step(held, 0)
    assert isinstance(val, float)
    _near(val, g.t("val_loss"), (name, "validation_step"))
    recorded = {k[len("val_report_"):]: g.t(k) for k in g.z.files if k.startswith("val_report_")}
    assert set(rep.seen) == set(recorded)
    for k, v in recorded.items():
        _near(rep.seen[k], v, (name, k))
    if c["kind"] == "bbb":
        assert not left and set(recorded) == {"eval_loss"}
        _feed(net, g, "fwd")
        x = torch.cat([held.action, held.state.float_features], 1)
        out = net(x)
        assert out.shape == (c["B"], 1)
        _near(out.cpu(), g.t("fwd_out"), (name, "forward"))
        with pytest.raises(NotImplementedError, match="outside autograd"):
            out.sum().backward()
    else:
        assert {"eval_rewards", "eval_pred_rewards", "eval_loss"} <= set(recorded)
        assert ("eval_unweighted_loss" in recorded) == bool(c.get("ips"))
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


def test_the_planted_tie_has_a_zero_gradient(backend):
    """bandit_l1, step 0, row 0: a zero state at zero biases predicts 0 exactly, the reward is 0, and torch's L1 gradient
    there is 0"""
    g = Golden(os.path.join("cfeval", "bandit_l1"))
    net, tr = _make(g, backend.device)
    batch = _batch(g, "step0", backend.device)
    r = tr._forward(batch, training=True)
    assert r["predicted_reward"][0, 0].item() == 0.0 == batch.reward[0, 0].item()
    assert torch.equal(r["dq"][0].cpu(), torch.zeros(g.cfg["A"]))
    assert (r["dq"][1:].abs().sum(1) > 0).all()


def test_a_seed_reproduces_a_drawn_run(backend):
    g = Golden(os.path.join("cfeval", "bbb_defaults"))
    dev = backend.device
    runs = []
    for seed in (7, 7, 8):
        net, tr = _make(g, dev)
        torch.manual_seed(seed)
        losses = [tr.train_step_native(_batch(g, f"step{s}", dev))["loss"].cpu().clone() for s in range(2)]
        runs.append((losses, [p.detach().cpu().clone() for p in net.parameters()]))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]))
    assert not torch.equal(runs[0][0][0], runs[2][0][0])
    assert not torch.equal(_bits(runs[0][0][0]), _bits(runs[0][0][1]))  # a fresh draw on every step


def test_surface_against_the_record():
    rec = json.load(open(os.path.join(GOLDEN, "reference_records", "cfeval_signatures.json")))
    fields = [[f.name, repr(f.default) if f.default is not dataclasses.MISSING else "required"]
              for f in dataclasses.fields(rlt.BanditRewardModelInput)]
    assert fields == rec["BanditRewardModelInput"]

    class Keys(dict):
        asked = []

        def __getitem__(self, k):
            self.asked.append(k)
            return super().__getitem__(k)

        def get(self, k, default=None):
            self.asked.append(k)
            return super().get(k, default)

    d = Keys(state_features=torch.zeros(2, 3), action=torch.zeros(2, 2), reward=torch.zeros(2, 1))
    made = rlt.BanditRewardModelInput.from_dict(d)
    assert d.asked == rec["from_dict_keys"] and made.batch_size() == 2 and made.action_prob is None
    assert list(cfeval.__all__) == rec["cfeval_all"] and cfeval.BanditRewardNetTrainer is BanditRewardNetTrainer
    from test_reference_signatures import _PARAMS

    ns = {}
    exec(_PARAMS, ns)
    checked = 0
    for path, methods in rec["signatures"].items():
        obj = ns["resolve"](path.replace("reagent.", "reagent_amd.", 1))
        for m, want in methods.items():
            got = json.loads(json.dumps(ns["params"](getattr(obj, m))))
            assert [g[:2] for g in got] == [w[:2] for w in want], (path, m, got, want)
            for g_, w_ in zip(got, want):
                assert g_[2] == w_[2] or (w_[2][0] == "factory" and g_[2] == ["value", "None"]), (path, m, g_, w_)
            checked += 1
    assert checked == 17
    plain = FullyConnectedProbabilisticNetwork([6, 16, 16, 1], ["relu", "relu", "linear"], 1.0)
    assert list(plain.state_dict().keys()) == rec["state_dict_keys"]["plain"]
    ln = FullyConnectedProbabilisticNetwork([6, 16, 1], ["relu", "linear"], 1.0, use_layer_norm=True, normalize_output=True)
    assert list(ln.state_dict().keys()) == rec["state_dict_keys"]["layer_norm"]
    assert all(isinstance(m, LinearBBB) for m in plain.linear_bbbs) and plain.linear_bbbs[1] is plain.dnn[2]
    # the initial law: w_mu and w_rho ~ N(0, gain^2 / dim_in), the biases' mu and rho zero
    torch.manual_seed(0)
    wide = FullyConnectedProbabilisticNetwork([400, 300, 1], ["relu", "linear"], 1.0)
    l = wide.linear_bbbs[0]
    for w in (l.w_mu, l.w_rho):
        assert abs(w.std().item() / (2.0 / 400) ** 0.5 - 1.0) < 0.02 and abs(w.mean().item()) < 1e-3
    assert not l.b_mu.any() and not l.b_rho.any()
    assert wide.input_prototype().shape == (1, 400)


def test_state_dict_moves_either_way(backend):
    g = Golden(os.path.join("cfeval", "bbb_layernorm_wide"))
    dev = backend.device
    net, _ = _make(g, dev)
    again = FullyConnectedProbabilisticNetwork(g.cfg["layers"], g.cfg["activations"], g.cfg["prior_var"], noise_tol=g.cfg["noise_tol"],
                                               use_layer_norm=True)
    again.load_state_dict(net.state_dict(), strict=True)
    again = again.to(dev)
    x = torch.cat([g.t("held_batch_action"), g.t("held_batch_state")], 1).to(dev)
    outs = []
    for n in (net, again):
        _feed(n, g, "fwd")
        outs.append(n(x))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # the same state_dict read by a plain torch statement of the reference's forward, under its keys
    sd = {k: v.cpu().double() for k, v in again.state_dict().items()}
    eps = [e.double() for e in g.seq("fwd_eps_")]
    h = x.cpu().double()
    for i, k in enumerate((0, 3, 6)):
        w = sd[f"dnn.{k}.w_mu"] + torch.log1p(torch.exp(sd[f"dnn.{k}.w_rho"])) * eps[2 * i]
        b = sd[f"dnn.{k}.b_mu"] + torch.log1p(torch.exp(sd[f"dnn.{k}.b_rho"])) * eps[2 * i + 1]
        h = torch.nn.functional.linear(h, w, b)
        if i < 2:
            h = torch.relu(torch.nn.functional.layer_norm(h, h.shape[1:], sd[f"dnn.{k + 1}.weight"], sd[f"dnn.{k + 1}.bias"]))
    _near(outs[1].cpu(), h, "forward against the torch statement")


def test_validation_does_not_apply_the_threshold(backend):
    g = Golden(os.path.join("cfeval", "bandit_smoothl1_ips_threshold"))
    dev = backend.device
    net, tr = _make(g, dev)
    batch = _batch(g, "step0", dev)
    kept = int(g.a("step0_kept"))
    assert 1 <= kept < g.cfg["B"]
    train = tr._forward(batch, training=True)
    assert int(train["n_kept"].item()) == kept
    val = tr.validation_step(batch, 0)
    free = BanditRewardNetTrainer(net, loss_type=LossFunction.SmoothL1Loss, weighted_by_inverse_propensity=True).to(dev)
    assert val == free.validation_step(batch, 0) and val != train["loss"].item()
    pred = tr._forward(batch, training=False)["predicted_reward"].cpu()
    want = (torch.nn.SmoothL1Loss(reduction="none")(pred, batch.reward.cpu()) / batch.action_prob.cpu()).mean().item()
    assert abs(val - want) <= 1e-5 * abs(want)
    low = BanditRewardNetTrainer(net, loss_type=LossFunction.SmoothL1Loss, reward_ignore_threshold=-1e9).to(dev)
    low.set_reporter(_Reporter())
    with pytest.raises(AssertionError, match="reward ignore threshold set too small"):
        next(low.train_step_gen(batch, 0))
    low.set_reporter(None)
    loss = next(low.train_step_gen(batch, 0))  # nobody listens: the NaN stays on the device
    assert torch.isnan(loss)


@pytest.mark.parametrize("name", ["bandit_smoothl1_ips_threshold", "bbb_defaults"])
def test_nothing_moves_to_the_host_without_a_reporter(backend, name):
    g = Golden(os.path.join("cfeval", name))
    dev = backend.device
    net, tr = _make(g, dev)
    batch = _batch(g, "step0", dev)
    if g.cfg["kind"] == "bbb":
        net.noise_source = lambda shape: torch.zeros(shape)  # (the drawn path reads torch's host generator for its seed)
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
    assert "loss" in tr.reporter.seen


def test_refusals_by_name(backend):
    dev = backend.device
    P = FullyConnectedProbabilisticNetwork
    with pytest.raises(NotImplementedError, match="use_batch_norm"):
        P([4, 8, 1], ["relu", "linear"], 1.0, use_batch_norm=True)
    with pytest.raises(NotImplementedError, match="dropout_ratio 0.1"):
        P([4, 8, 1], ["relu", "linear"], 1.0, dropout_ratio=0.1)
    with pytest.raises(NotImplementedError, match="activation gelu"):
        P([4, 8, 1], ["gelu", "linear"], 1.0)
    with pytest.raises(NotImplementedError, match="9 layers"):
        P([4] * 9 + [1], ["relu"] * 8 + ["linear"], 1.0)
    P([4] * 8 + [1], ["relu"] * 7 + ["linear"], 1.0, min_std=0.5, orthogonal_init=True)  # eight layers; both accepted, ignored
    wide = P([4, 8, 2], ["relu", "linear"], 1.0).to(dev)
    with pytest.raises(NotImplementedError, match="last layer of 2 outputs"):
        wide.sample_elbo(torch.zeros(3, 4, device=dev), torch.zeros(3, 1, device=dev), 1)
    for t in (wide.log_prior(), wide.log_post(), *wide.elbo_terms()):  # nothing drawn yet: NaN, not stale memory
        assert torch.isnan(t).all()
    assert wide(torch.zeros(3, 4, device=dev)).shape == (3, 2)
    assert torch.isfinite(wide.log_prior()) and torch.isfinite(wide.log_post())
    bnet = P([5, 8, 1], ["relu", "linear"], 1.0).to(dev)
    dqn = FullyConnectedDQN(3, 2, [8], ["relu"]).to(dev)
    for cls, net in ((BanditRewardNetTrainer, dqn), (BayesByBackpropTrainer, bnet)):
        with pytest.raises(NotImplementedError, match="LossFunction.BCELoss"):
            cls(net, loss_type=LossFunction.BCELoss)
        with pytest.raises(NotImplementedError, match="reward_net must be a reagent_amd"):
            cls(torch.nn.Linear(3, 2))
        tr = cls(net).to(dev)
        with pytest.raises(NotImplementedError, match="enable_data_parallel"):
            tr.enable_data_parallel()
        with pytest.raises(NotImplementedError, match="HIP graph"):
            plumbing.enable_graph_mode(tr)
        (o,) = tr.configure_optimizers()
        assert type(o["optimizer"]).__name__ == "FusedAdam"
    with pytest.raises(NotImplementedError, match="FullyConnectedDQN"):
        BanditRewardNetTrainer(bnet)
    with pytest.raises(NotImplementedError, match="FullyConnectedProbabilisticNetwork"):
        BayesByBackpropTrainer(dqn)
    with pytest.raises(NotImplementedError, match="weighted_by_inverse_propensity"):
        BayesByBackpropTrainer(bnet, weighted_by_inverse_propensity=True)
    batch = synthetic.bandit_reward_batch(5, 3, 2, seed=1, device=dev)
    weighted = BanditRewardNetTrainer(dqn, weighted_by_inverse_propensity=True).to(dev)
    with pytest.raises(AssertionError):  # the reference's `assert batch.action_prob is not None`
        next(weighted.train_step_gen(batch, 0))


def test_synthetic_batch():
    b = synthetic.bandit_reward_batch(12, 4, 3, seed=1, with_propensities=True)
    assert isinstance(b, rlt.BanditRewardModelInput) and b.batch_size() == 12
    assert b.state.float_features.shape == (12, 4) and b.action.shape == (12, 3) and b.reward.shape == b.action_prob.shape == (12, 1)
    assert torch.equal(b.action.sum(1), torch.ones(12)) and ((b.action == 0) | (b.action == 1)).all()
    assert (b.action_prob > 0).all() and (b.action_prob <= 1).all()
    assert torch.equal(synthetic.bandit_reward_batch(12, 4, 3, seed=1).reward, b.reward)  # seeded
    assert synthetic.bandit_reward_batch(12, 4, 3, seed=1).action_prob is None
    assert not torch.equal(synthetic.bandit_reward_batch(12, 4, 3, seed=2).reward, b.reward)


def test_bayes_by_backprop_learns_the_toy(backend):
    """the reference's own toy (reagent/test/training/test_probabilistic.py): y = -x^4 + 3 x^2 - 5 sin x + 1 on six points in
    [-2, 2]; the loss's moving average falls, and the predictive variance is larger far from the data than inside it"""
    dev = backend.device
    torch.manual_seed(0)
    x = torch.linspace(-2, 2, 6).reshape(-1, 1)
    y = -x ** 4 + 3 * x ** 2 - 5 * torch.sin(x) + 1
    net = FullyConnectedProbabilisticNetwork([2, 32, 1], ["relu", "linear"], 1.0, noise_tol=0.1).to(dev)
    tr = BayesByBackpropTrainer(net, optimizer=Optimizer__Union.default(lr=0.1)).to(dev)
    # (action first: the action column is the toy's x, the state one column of zeros)
    batch = rlt.BanditRewardModelInput(state=rlt.FeatureData(torch.zeros(6, 1, device=dev)), action=x.to(dev), reward=y.to(dev))
    losses = torch.stack([tr.train_step_native(batch)["loss"].clone() for _ in range(300)]).cpu()
    first, last = losses[:30].mean().item(), losses[-30:].mean().item()
    print(f"loss, mean of the first 30 steps {first:.1f}, of the last 30 {last:.1f}")
    assert np.isfinite(last) and last < first
    probe = torch.tensor([[-25.0, 0.0], [0.0, 0.0]], device=dev)
    draws = torch.stack([net(probe).detach().cpu() for _ in range(100)])
    var = draws.var(0).view(-1)
    print(f"predictive variance at x = -25: {var[0].item():.3g}, at x = 0: {var[1].item():.3g}")
    assert var[0] > var[1]


# ---- the reference's own float32 against float64 --------------------------------------------------------------------------
def _restated_steps(dtype, layers, prior_var, noise_tol, layer_norm, names, init, batches, draws, lr):
    """The Bayes-by-backprop step of the reference (probabilistic_fully_connected_network.py:87-105, :190-213, one draw) and
    torch.optim.Adam restated in plain torch at `dtype`, from given initial parameters, batches (x, y) and draws -> the
    loss of every step and the parameters after every step"""
    from torch.distributions import Normal

    p = {n: torch.nn.Parameter(t.detach().clone().to(dtype)) for n, t in zip(names, init)}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    bbb = sorted({int(n.split(".")[1]) for n in names if n.endswith("w_mu")})
    prior = Normal(torch.zeros((), dtype=dtype), torch.tensor(prior_var, dtype=dtype))
    losses, params = [], []
    for (x, y), eps in zip(batches, draws):
        h, log_prior, log_post = x.to(dtype), 0, 0
        for i, k in enumerate(bbb):
            mu, rho, bmu, brho = (p[f"dnn.{k}.{s}"] for s in ("w_mu", "w_rho", "b_mu", "b_rho"))
            w = mu + torch.log(1 + torch.exp(rho)) * eps[2 * i].to(dtype)
            b = bmu + torch.log(1 + torch.exp(brho)) * eps[2 * i + 1].to(dtype)
            log_prior = log_prior + torch.sum(prior.log_prob(w)) + torch.sum(prior.log_prob(b))
            log_post = log_post + Normal(mu.data, torch.log(1 + torch.exp(rho))).log_prob(w).sum() \
                + Normal(bmu.data, torch.log(1 + torch.exp(brho))).log_prob(b).sum()
            h = torch.nn.functional.linear(h, w, b)
            if i < len(bbb) - 1:
                if layer_norm:
                    h = torch.nn.functional.layer_norm(h, h.shape[1:], p[f"dnn.{k + 1}.weight"], p[f"dnn.{k + 1}.bias"])
                h = torch.relu(h)
        log_like = Normal(h.reshape(-1), noise_tol).log_prob(y.to(dtype).reshape(-1)).sum()
        loss = log_post - log_prior - log_like
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
        params.append([v.detach().clone() for v in p.values()])
    return losses, params


def _within_the_float32_bounds(got, want, what):
    """the issue's bounds on a float32 run against float64: 2.5e-7 relative on the loss, 1.6e-7 absolute on every parameter"""
    for s, ((l32, p32), (l64, p64)) in enumerate(zip(zip(*got), zip(*want))):
        rel = abs(l32.double().item() - l64.item()) / abs(l64.item())
        err = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
        print(f"{what} step {s}: loss off by {rel:.3e} relative, parameters by {err:.3e}")
        assert rel <= 2.5e-7 and err <= 1.6e-7, (what, s, rel, err)


@pytest.mark.parametrize("name", ["bbb_defaults", "bbb_layernorm_wide"])
def test_the_fixtures_float32_runs_sit_inside_the_float64_bounds(name):
    """the fixture's data through the float64 restatement: the float32 restatement AND the reference's own recorded float32
    run stay within the bounds, two orders inside the replay's 1e-4 and 2e-5 (a fixture that does not gets another seed)"""
    g = Golden(os.path.join("cfeval", name))
    c = g.cfg
    names = json.loads(str(g.a("names_json")))
    init = [g.t(f"init_{i}") for i in range(len(names))]
    batches = [(torch.cat([g.t(f"step{s}_batch_action"), g.t(f"step{s}_batch_state")], 1), g.t(f"step{s}_batch_reward"))
               for s in range(c["steps"])]
    draws = [g.seq(f"step{s}_eps_") for s in range(c["steps"])]
    args = (c["layers"], c["prior_var"], c.get("noise_tol", 0.1), c.get("layer_norm", False), names, init, batches, draws, c["lr"])
    want = _restated_steps(torch.float64, *args)
    _within_the_float32_bounds(_restated_steps(torch.float32, *args), want, name + " restated")
    recorded = ([g.t(f"step{s}_loss") for s in range(c["steps"])],
                [[g.t(f"step{s}_param_{i}") for i in range(len(names))] for s in range(c["steps"])])
    _within_the_float32_bounds(recorded, want, name + " recorded")


# (layers, lr) -> (seed, batch).  The bounds are a few float32 ulp of the loss and about one of a parameter near 1, so not every
# draw of the data stays inside them; as the issue has it for the fixtures, the seed moves and the bound does not.  Each seed
# below is the first of 1, 2, ... at which the float32 run stays within 0.75 of both bounds.
RESTATED = {("6-16-16-1", 0.01): (13, 8), ("6-16-16-1", 0.001): (165, 8), ("33-65-34-1", 0.01): (59, 33),
            ("33-65-34-1", 0.001): (1, 33), ("3-1", 0.01): (1, 8), ("3-1", 0.001): (1, 8)}


@pytest.mark.parametrize("lr", [0.01, 0.001])
@pytest.mark.parametrize("layers", [[6, 16, 16, 1], [33, 65, 34, 1], [3, 1]], ids=lambda l: "-".join(map(str, l)))
def test_float32_restatement_stays_within_the_float64_bounds(layers, lr):
    """a float32 torch restatement of the Bayes-by-backprop step against float64 over four Adam steps, on seeded data"""
    seed, B = RESTATED["-".join(map(str, layers)), lr]
    torch.manual_seed(seed)
    net = FullyConnectedProbabilisticNetwork(layers, ["relu"] * (len(layers) - 2) + ["linear"], 1.0)
    names = [n for n, _ in net.named_parameters()]
    init = [p.detach().clone() for p in net.parameters()]
    batches = [(torch.randn(B, layers[0]), torch.randn(B, 1)) for _ in range(4)]
    draws = [[torch.randn(s) for l in net.linear_bbbs for s in (l.w_mu.shape, l.b_mu.shape)] for _ in range(4)]
    args = (layers, 1.0, 0.1, False, names, init, batches, draws, lr)
    _within_the_float32_bounds(_restated_steps(torch.float32, *args), _restated_steps(torch.float64, *args), f"{layers} lr {lr}")
