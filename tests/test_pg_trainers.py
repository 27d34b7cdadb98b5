"""ReinforceTrainer and PPOTrainer against golden vectors of the reference's trainers (tests/golden/pg/*.npz, made by
tests/golden_gen/make_pg_golden.py from the unmodified reference): REINFORCE's generator path and native step, PPO's
`training_step` fed the recorded trajectories and minibatch orders; a packed PPO update against the same trainer fed one
trajectory at a time; the conditions the fixture inputs hold; the surface (signatures, parameter classes, input type,
acting side, what is refused).
Tolerances are those of tests/test_pdqn_trainer.py: losses 1e-4 * |ref| + 2e-6, parameters of every network 2e-5 absolute
after every step / update."""
import dataclasses
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Golden
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.gym.policies import Policy, SoftmaxActionSampler
from reagent_amd.models import DuelingQNetwork, FloatFeatureFullyConnected, FullyConnectedDQN
from reagent_amd.optimizer import Optimizer__Union
from reagent_amd.training import PPOTrainer, PPOTrainerParameters, ReinforceTrainer, ReinforceTrainerParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REINFORCE = ["reinforce_whiten", "reinforce_offpolicy_clip", "reinforce_baseline"]
PPO = ["ppo_clip_entropy", "ppo_baseline"]
MARGIN = 1e-3


def _generator_module():
    spec = importlib.util.spec_from_file_location("make_pg_golden", os.path.join(ROOT, "tests", "golden_gen", "make_pg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(g, device, **override):
    c = dict(g.cfg, **override)
    scorer = FullyConnectedDQN(c["state_dim"], c["num_actions"], c["sizes"], c["activations"])
    value = FloatFeatureFullyConnected(c["state_dim"], 1, c["sizes"], c["activations"]) if c["value_net"] else None
    with torch.no_grad():
        for p, init in zip(scorer.parameters(), g.seq("init_policy_")):
            p.copy_(init)
        if value is not None:
            for p, init in zip(value.parameters(), g.seq("init_value_")):
                p.copy_(init)
    policy = Policy(scorer=scorer.to(device), sampler=SoftmaxActionSampler(temperature=c["temperature"]))
    common = dict(gamma=c["gamma"], optimizer=Optimizer__Union.default(lr=c["lr"]),
                  optimizer_value_net=Optimizer__Union.default(lr=c["lr"]), reward_clip=c["reward_clip"],
                  normalize=c["normalize"], subtract_mean=c["subtract_mean"], offset_clamp_min=c["offset_clamp_min"],
                  value_net=value.to(device) if value is not None else None)
    if c["algo"] == "reinforce":
        tr = ReinforceTrainer(policy, off_policy=c["off_policy"], clip_param=c["clip_param"], **common)
    else:
        tr = PPOTrainer(policy, update_freq=c["update_freq"], update_epochs=c["update_epochs"],
                        ppo_batch_size=c["ppo_batch_size"], ppo_epsilon=c["ppo_epsilon"], entropy_weight=c["entropy_weight"],
                        **common)
    return tr.to(device)


def check(tr, g, prefix, tol=2e-5):
    nets = dict(policy=tr.scorer)
    if tr.value_net is not None:
        nets["value"] = tr.value_net
    for n, net in nets.items():
        for i, p in enumerate(net.parameters()):
            err = (p.detach().cpu() - g.t(f"{prefix}{n}_{i}")).abs().max().item()
            assert err <= tol, (prefix, n, i, err)


def check_loss(got, ref, what):
    ref = float(ref)
    assert abs(float(got) - ref) <= 1e-4 * abs(ref) + 2e-6, (what, float(got), ref)


def lightning_like_step(tr, opts, batch, batch_idx):
    losses = []
    for i, opt in enumerate(opts):
        loss = tr.training_step(batch, batch_idx, i)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return losses


@pytest.mark.parametrize("name", REINFORCE)
def test_reinforce_generator_path_matches_reference(backend, name):
    g = Golden("pg/" + name)
    tr = build(g, backend.device)
    opts = [o["optimizer"] for o in tr.configure_optimizers()]
    assert len(opts) == (2 if g.cfg["value_net"] else 1)
    if g.cfg["value_net"]:  # the value net's optimizer first
        assert opts[0].param_groups[0]["params"][0] is next(tr.value_net.parameters())
    for s in range(g.cfg["steps"]):
        losses = lightning_like_step(tr, opts, synthetic.to_pg_input(g.batch(s), backend.device), s)
        if g.cfg["value_net"]:
            check_loss(losses[0], g.t(f"step{s}_value_loss"), f"step{s}_value_loss")
        check_loss(losses[-1], g.t(f"step{s}_loss"), f"step{s}_loss")
        check(tr, g, f"step{s}_")
    assert tr.all_batches_processed == g.cfg["steps"]


@pytest.mark.parametrize("name", REINFORCE)
def test_reinforce_native_step_matches_reference(backend, name):
    g = Golden("pg/" + name)
    tr = build(g, backend.device)
    for s in range(g.cfg["steps"]):
        out = tr.train_step_native(synthetic.to_pg_input(g.batch(s), backend.device))
        assert set(out) == {"loss", "value_loss"} and (out["value_loss"] is not None) == g.cfg["value_net"]
        check_loss(out["loss"].item(), g.t(f"step{s}_loss"), f"step{s}_loss")
        if g.cfg["value_net"]:
            check_loss(out["value_loss"].item(), g.t(f"step{s}_value_loss"), f"step{s}_value_loss")
        check(tr, g, f"step{s}_")
        ref_l = g.t(f"step{s}_ref_log_prob")  # the kernel's by-products against the reference's own, before the step
        assert (tr._log_prob.cpu() - ref_l).abs().max() <= 1e-5
        assert (tr._advantage.cpu() - g.t(f"step{s}_ref_advantage")).abs().max() <= 1e-5


def _ppo_trajectories(g, u):
    out = []
    for j in range(g.cfg["update_freq"]):
        pre = f"update{u}_traj{j}_batch_"
        out.append({k[len(pre):]: g.t(k) for k in g.z.files if k.startswith(pre)})
    return out


@pytest.mark.parametrize("name", PPO)
def test_ppo_training_step_matches_reference(backend, name):
    g = Golden("pg/" + name)
    c = g.cfg
    tr = build(g, backend.device)
    reported, orders = [], []

    class Reporter:
        def log(self, **kw):
            reported.append(kw)

    tr.set_reporter(Reporter())
    tr._minibatch_order = lambda n: orders.pop(0)
    n_mb = c["update_epochs"] * -(-c["update_freq"] // c["ppo_batch_size"])
    for u in range(c["updates"]):
        orders[:] = list(g.t(f"update{u}_orders"))
        del reported[:]
        for j, d in enumerate(_ppo_trajectories(g, u)):
            assert len(tr.traj_buffer) == j
            batch = {k: v.to(backend.device) for k, v in d.items()}
            tr.training_step(batch if j % 2 else rlt.PolicyGradientInput.from_dict(batch), j)  # (a dict is accepted as well)
        assert tr.traj_buffer == [] and orders == [] and len(reported) == n_mb
        for m, r in enumerate(reported):
            assert set(r) == {"ppo_loss", "value_net_loss"} and r["ppo_loss"].shape == r["value_net_loss"].shape == (1,)
            check_loss(r["ppo_loss"].item(), g.t(f"update{u}_ppo_loss")[m], f"update{u} minibatch {m} ppo_loss")
            check_loss(r["value_net_loss"].item(), g.t(f"update{u}_value_net_loss")[m], f"update{u} minibatch {m} value_net_loss")
        check(tr, g, f"update{u}_")
    if c["update_freq"] % c["ppo_batch_size"]:  # the last minibatch of an epoch is short
        assert c["update_freq"] // c["ppo_batch_size"] >= 1


def test_packed_ppo_update_equals_one_trajectory_at_a_time(backend):
    """three trajectories of different lengths in ONE packed update against the same trainer fed them one at a time through
    `_trajectory_to_losses` with the losses summed, the value net stepped first (ppo_trainer.py:386-402); 2e-5 on every
    parameter.  With a value net, masks and an entropy bonus, so that every per-trajectory quantity takes part."""
    g = Golden("pg/ppo_baseline")
    dev = backend.device
    trajs = [synthetic.to_pg_input(synthetic.pg_trajectory(n, 6, 4, seed=70 + n, with_mask=True), dev) for n in (5, 17, 9)]
    packed = build(g, dev, update_freq=3, ppo_batch_size=3, entropy_weight=0.01)
    packed._minibatch_order = lambda n: torch.arange(n)
    for j, t in enumerate(trajs):
        packed.training_step(t, j)
    assert packed.traj_buffer == []
    single = build(g, dev, update_freq=3, ppo_batch_size=1, entropy_weight=0.01)
    value_opt, ppo_opt = single.get_optimizers()
    losses = [single._trajectory_to_losses(t) for t in trajs]
    assert all(set(l) == {"ppo_loss", "value_net_loss"} for l in losses)
    value_loss = torch.stack([l["value_net_loss"] for l in losses]).sum()
    value_opt.zero_grad()
    single.manual_backward(value_loss)
    value_opt.step()
    ppo_loss = torch.stack([l["ppo_loss"] for l in losses]).sum()
    ppo_opt.zero_grad()
    single.manual_backward(ppo_loss)
    ppo_opt.step()
    check_loss(packed._ploss.item(), ppo_loss.item(), "ppo_loss")
    check_loss(packed._vloss.item(), value_loss.item(), "value_net_loss")
    for a, b in zip(packed.parameters(), single.parameters()):
        assert (a.detach().cpu() - b.detach().cpu()).abs().max() <= 2e-5
    moved = max((a.detach().cpu() - i).abs().max().item() for a, i in zip(packed.scorer.parameters(), g.seq("init_policy_")))
    assert moved > 1e-3  # (the update did something)


def test_a_loss_built_before_a_weight_step_refuses_its_backward(backend):
    """`_trajectory_to_losses` keeps each trajectory's output gradients, not the weights autograd would have saved: a
    backward after the network's own optimizer step raises; the other network's step in between is the reference's order"""
    g = Golden("pg/ppo_baseline")
    dev = backend.device
    tr = build(g, dev, update_freq=2, ppo_batch_size=1)
    trajs = [synthetic.to_pg_input(synthetic.pg_trajectory(n, 6, 4, seed=80 + n, with_mask=True), dev) for n in (6, 11)]
    value_opt, ppo_opt = tr.get_optimizers()
    first, second, third = [tr._trajectory_to_losses(t) for t in (trajs[0], trajs[1], trajs[0])]
    value_opt.zero_grad()
    tr.manual_backward(first["value_net_loss"])  # (repeats the value net's forward on trajectory 0)
    value_opt.step()
    with pytest.raises(RuntimeError, match="value network's weights changed"):
        tr.manual_backward(second["value_net_loss"])
    ppo_opt.zero_grad()
    tr.manual_backward(first["ppo_loss"] + second["ppo_loss"])  # the value net's step does not touch these
    ppo_opt.step()
    with pytest.raises(RuntimeError, match="policy network's weights changed"):
        tr.manual_backward(third["ppo_loss"])


def _hold(c, trajs):
    for b in trajs:
        a = b["action"].argmax(1)
        if c["with_mask"]:
            m = b["possible_actions_mask"]
            assert (m[torch.arange(len(a)), a] == 1).all() and (m.sum(1) >= 2).all()
        else:
            assert "possible_actions_mask" not in b
        assert c["reward_clip"] >= 1e6 or (b["reward"] > c["reward_clip"]).any()
        assert c["min_len"] <= len(a) <= c["max_len"] and (not c["normalize"] or len(a) >= 2)
        assert b["action"].dtype == torch.int64 and (b["action"].sum(1) == 1).all()


def test_fixture_inputs_hold_their_conditions():
    """stated here on the committed files, independently of the generator's own check: no logged action is masked and
    every masked row allows at least two actions; off-policy REINFORCE keeps l - old 1e-3 away from log clip and has at
    least two rows with a positive advantage on each side of it (offset_clamp_min leaves no negative one); PPO keeps
    every rho 1e-3 away from 1 +- epsilon in every minibatch and, per update,
    has at least two rows clipped on each side with an advantage of each sign; a reward above reward_clip where one is
    set; whitened trajectories of length >= 2"""
    for name in REINFORCE:
        g = Golden("pg/" + name)
        c = g.cfg
        assert (c["state_dim"], c["num_actions"], c["sizes"], c["lr"], c["steps"]) == (6, 4, [24, 16], 0.003, 4)
        for s in range(c["steps"]):
            b = g.batch(s)
            _hold(c, [b])
            if c["off_policy"]:
                d = g.t(f"step{s}_ref_log_prob").double() - b["log_prob"].double()
                lc = math.log(c["clip_param"])
                adv = g.t(f"step{s}_ref_advantage")
                assert c["offset_clamp_min"] and (adv >= 0).all() and (adv == 0).any()  # no negative advantage to be had
                assert ((d - lc).abs() >= MARGIN).all()
                assert ((d > lc) & (adv > 0)).sum() >= 2 and ((d < lc) & (adv > 0)).sum() >= 2
        assert os.path.getsize(os.path.join(GOLDEN, "pg", name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "td3_twin.npz"))
    assert Golden("pg/reinforce_whiten").cfg["temperature"] == 0.7 and Golden("pg/reinforce_whiten").cfg["with_mask"]
    assert Golden("pg/reinforce_baseline").cfg["reward_clip"] == 0.8 and Golden("pg/reinforce_baseline").cfg["value_net"]
    c = Golden("pg/reinforce_offpolicy_clip").cfg
    assert (c["normalize"], c["subtract_mean"], c["offset_clamp_min"], c["clip_param"]) == (False, True, True, 2.0)
    for name in PPO:
        g = Golden("pg/" + name)
        c = g.cfg
        eps = c["ppo_epsilon"]
        n_mb = c["update_epochs"] * -(-c["update_freq"] // c["ppo_batch_size"])
        for u in range(c["updates"]):
            trajs = _ppo_trajectories(g, u)
            _hold(c, trajs)
            assert len({len(t["reward"]) for t in trajs}) > 1  # lengths differ inside an update
            orders = g.t(f"update{u}_orders")
            assert orders.shape == (c["update_epochs"], c["update_freq"])
            assert all(sorted(o.tolist()) == list(range(c["update_freq"])) for o in orders)
            rhos, advs = [], []
            for m in range(n_mb):
                e, k = divmod(m, -(-c["update_freq"] // c["ppo_batch_size"]))
                idx = orders[e][k * c["ppo_batch_size"]:(k + 1) * c["ppo_batch_size"]].tolist()
                old = torch.cat([trajs[i]["log_prob"] for i in idx])
                assert torch.equal(old, g.t(f"update{u}_mb{m}_old_log_prob"))  # the minibatch is what the order says
                rho = torch.exp(g.t(f"update{u}_mb{m}_ref_log_prob").double() - old.double())
                assert ((rho - (1 - eps)).abs() >= MARGIN).all() and ((rho - (1 + eps)).abs() >= MARGIN).all()
                rhos.append(rho)
                advs.append(g.t(f"update{u}_mb{m}_ref_advantage"))
            assert not g.has(f"update{u}_mb{n_mb}_ref_log_prob")
            rho, adv = torch.cat(rhos), torch.cat(advs)
            for on in (rho < 1 - eps, rho > 1 + eps):
                assert (on & (adv > 0)).sum() >= 2 and (on & (adv < 0)).sum() >= 2
        assert os.path.getsize(os.path.join(GOLDEN, "pg", name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "td3_twin.npz"))
    c = Golden("pg/ppo_baseline").cfg
    assert c["update_freq"] % c["ppo_batch_size"] != 0 and c["value_net"] and c["with_mask"]  # a short last minibatch
    c = Golden("pg/ppo_clip_entropy").cfg
    assert (c["update_freq"], c["update_epochs"], c["ppo_batch_size"], c["entropy_weight"]) == (4, 2, 2, 0.01)


def test_generator_check_agrees_with_the_committed_fixtures():
    mod = _generator_module()
    for name in REINFORCE + PPO:
        g = Golden("pg/" + name)
        assert g.cfg == mod.CASES[name]
    for name in REINFORCE:
        g = Golden("pg/" + name)
        for s in range(g.cfg["steps"]):
            l = g.t(f"step{s}_ref_log_prob") if g.cfg["off_policy"] else None
            assert mod.check_inputs(g.cfg, [g.batch(s)], l, g.t(f"step{s}_ref_advantage")) == []


def _reference_present():
    from oracle import stubs

    return os.path.isdir(os.path.join(stubs.REFERENCE_ROOT, "reagent"))


@pytest.mark.parametrize("name", REINFORCE + PPO)
def test_fixture_is_what_the_reference_produces(name):
    """where the reference tree is present: regenerate the fixture in memory and compare it with the committed file"""
    if not _reference_present():
        pytest.skip("reference tree not present")
    arrays = _generator_module().generate(name)
    z = np.load(os.path.join(GOLDEN, "pg", name + ".npz"), allow_pickle=False)
    assert set(arrays) == set(z.files)
    for k, v in arrays.items():
        if k == "config_json":
            assert json.loads(str(v)) == json.loads(str(z[k]))
        elif v.dtype.kind in "bi":
            assert np.array_equal(v, z[k]), k
        else:
            np.testing.assert_allclose(v, z[k], rtol=1e-6, atol=1e-7, err_msg=k)


# ---- surface ------------------------------------------------------------------------------------------------------
OWN = {
    "reagent.training.reinforce_trainer.ReinforceTrainer": "reagent_amd.training.ReinforceTrainer",
    "reagent.training.ppo_trainer.PPOTrainer": "reagent_amd.training.PPOTrainer",
    "reagent.gym.policies.policy.Policy": "reagent_amd.gym.policies.Policy",
    "reagent.gym.policies.samplers.discrete_sampler.SoftmaxActionSampler": "reagent_amd.gym.policies.SoftmaxActionSampler",
    "reagent.core.types.PolicyGradientInput": "reagent_amd.core.types.PolicyGradientInput",
}


def _record():
    return json.load(open(os.path.join(GOLDEN, "reference_records", "policy_gradient_signatures.json")))


def test_signatures_equal_the_reference_record():
    from test_reference_signatures import _PARAMS, _same

    ns = {}
    exec(_PARAMS, ns)
    rec = _record()
    assert set(rec) == set(OWN) | {"reagent.training.parameters.ReinforceTrainerParameters",
                                   "reagent.training.parameters.PPOTrainerParameters"}
    for ref_path, own_path in OWN.items():
        methods = sorted(m for m in rec[ref_path] if m not in ("fields", "prototype_shapes"))
        own = ns["surface"]([(own_path, methods)])[own_path]
        for m in methods:
            assert _same(rec[ref_path][m], own[m]), (own_path, m, rec[ref_path][m], own[m])
    assert set(rec["reagent.training.ppo_trainer.PPOTrainer"]) >= {"_trajectory_to_losses", "_check_input", "training_step",
                                                                    "update_model", "_update_model", "get_optimizers"}
    if _reference_present():
        assert _generator_module().signatures() == rec


def _fields(cls):
    out = []
    for f in dataclasses.fields(cls):
        if f.default is not dataclasses.MISSING:
            out.append([f.name, ["value", repr(f.default)]])
        elif f.default_factory is not dataclasses.MISSING:
            out.append([f.name, ["factory", type(f.default_factory()).__name__]])
        else:
            out.append([f.name, ["required"]])
    return out


def test_parameter_classes_equal_the_reference_record():
    rec = _record()
    assert _fields(ReinforceTrainerParameters) == rec["reagent.training.parameters.ReinforceTrainerParameters"]["fields"]
    assert _fields(PPOTrainerParameters) == rec["reagent.training.parameters.PPOTrainerParameters"]["fields"]
    p = PPOTrainerParameters()
    assert "policy" not in p.asdict() and "value_net" not in p.asdict() and p.ppo_epsilon == 0.2 and p.actions == []
    scorer = FullyConnectedDQN(4, 3, [8], ["relu"])
    tr = PPOTrainer(Policy(scorer, SoftmaxActionSampler()), **dict(p.asdict(), normalize=False),
                    value_net=FloatFeatureFullyConnected(4, 1, [8], ["relu"]))
    assert tr.update_freq == 1 and tr.value_net is not None
    r = ReinforceTrainerParameters(gamma=0.5)
    assert ReinforceTrainer(Policy(scorer, SoftmaxActionSampler()), **r.asdict()).gamma == 0.5


def test_policy_gradient_input_and_the_acting_side(emu_lib):
    rec = _record()["reagent.core.types.PolicyGradientInput"]
    assert [f.name for f in dataclasses.fields(rlt.PolicyGradientInput)] == rec["fields"]
    proto = rlt.PolicyGradientInput.input_prototype(action_dim=3, batch_size=7, state_dim=5)
    shapes = rec["prototype_shapes"]
    assert list(proto.state.float_features.shape) == shapes["state"] and list(proto.action.shape) == shapes["action"]
    assert list(proto.reward.shape) == shapes["reward"] and list(proto.log_prob.shape) == shapes["log_prob"]
    assert list(proto.possible_actions_mask.shape) == shapes["possible_actions_mask"]
    assert str(proto.action.dtype) == shapes["action_dtype"] and len(proto) == 7
    d = synthetic.pg_trajectory(9, 5, 3, seed=1, with_mask=True)
    b = rlt.PolicyGradientInput.from_dict(d)
    assert len(b) == 9 and b.next_state is None and b.not_terminal is None
    assert torch.equal(b.state.float_features, d["observation"]) and torch.equal(b.possible_actions_mask, d["possible_actions_mask"])
    b = rlt.PolicyGradientInput.from_dict(dict(d, next_observation=d["observation"], not_terminal=torch.ones(9)))
    assert torch.equal(b.next_state.float_features, d["observation"]) and b.not_terminal.shape == (9,)
    # the acting side: masked actions are never drawn, log_prob is the categorical's, update() decays to the floor
    scorer = FullyConnectedDQN(5, 3, [8], ["relu"])
    sampler = SoftmaxActionSampler(temperature=2.0, temperature_decay=0.5, minimum_temperature=0.75)
    policy = Policy(scorer, sampler)
    mask = torch.tensor([[1.0, 0.0, 1.0]]).repeat(64, 1)
    out = policy.act(rlt.FeatureData(torch.randn(64, 5)), mask)
    assert out.action.shape == (64, 3) and out.action[:, 1].sum() == 0 and out.log_prob.shape == (64,)
    scores = torch.randn(6, 3)
    onehot = torch.nn.functional.one_hot(torch.tensor([0, 1, 2, 2, 1, 0]), 3)
    want = torch.log_softmax(scores / 2.0, dim=1)[torch.arange(6), onehot.argmax(1)]
    assert torch.allclose(sampler.log_prob(scores, onehot), want)
    p = torch.softmax(scores / 2.0, dim=1)
    assert torch.allclose(sampler.entropy(scores), -(p * p.log()).sum(1).mean())
    sampler.update()
    assert sampler.temperature == 1.0
    sampler.update()
    assert sampler.temperature == 0.75
    with pytest.raises(AssertionError):
        SoftmaxActionSampler(temperature=0.0)


def _policy(S=5, A=3, scorer=None):
    return Policy(scorer if scorer is not None else FullyConnectedDQN(S, A, [8], ["relu"]), SoftmaxActionSampler())


def test_unsupported_configurations_are_refused(emu_lib):
    traj = synthetic.to_pg_input(synthetic.pg_trajectory(7, 5, 3, seed=2))
    value = lambda: FloatFeatureFullyConnected(5, 1, [8], ["relu"])  # noqa: E731
    # the reference's own errors
    with pytest.raises(RuntimeError, match="Can't apply a baseline and reward normalization"):
        ReinforceTrainer(_policy(), value_net=value())
    with pytest.raises(AssertionError, match="value baseline and normalize"):
        PPOTrainer(_policy(), value_net=value())
    with pytest.raises(AssertionError, match="requires a value_net"):
        PPOTrainer(_policy(), td_error_advantage=True)
    with pytest.raises(AssertionError, match="ppo_epsilon"):
        PPOTrainer(_policy(), ppo_epsilon=1.5)
    # what this package leaves out, each by name
    with pytest.raises(NotImplementedError, match="td_error_advantage"):
        PPOTrainer(_policy(), normalize=False, value_net=value(), td_error_advantage=True)
    with pytest.raises(NotImplementedError, match="do_log_metrics"):
        ReinforceTrainer(_policy(), do_log_metrics=True)
    dueling = DuelingQNetwork.make_fully_connected(5, 3, [8], ["relu"])
    for cls in (ReinforceTrainer, PPOTrainer):
        with pytest.raises(NotImplementedError, match="FullyConnectedDQN"):
            cls(_policy(scorer=dueling))
        with pytest.raises(NotImplementedError, match="data-parallel"):
            cls(_policy()).enable_data_parallel()

    @dataclasses.dataclass
    class WithGraph(rlt.PolicyGradientInput):
        graph: object = None

    graph_traj = WithGraph(**{f.name: getattr(traj, f.name) for f in dataclasses.fields(traj)}, graph=object())
    with pytest.raises(NotImplementedError, match="graph"):
        ReinforceTrainer(_policy()).train_step_native(graph_traj)
    with pytest.raises(NotImplementedError, match="graph"):
        PPOTrainer(_policy()).training_step(graph_traj, 0)
    ppo = PPOTrainer(_policy())
    ppo.logger = object()
    with pytest.raises(NotImplementedError, match="logger"):
        ppo.training_step(traj, 0)
    from reagent_amd.training.plumbing import enable_graph_mode

    for tr in (ReinforceTrainer(_policy()), PPOTrainer(_policy())):
        with pytest.raises(NotImplementedError, match="HIP graph"):
            enable_graph_mode(tr)
        tr._graph_mode = True  # (however it got there)
        with pytest.raises(NotImplementedError, match="HIP graph"):
            tr.train_step_native(traj) if isinstance(tr, ReinforceTrainer) else tr.training_step(traj, 0)
    with pytest.raises(NotImplementedError, match="manually"):
        next(PPOTrainer(_policy()).train_step_gen(traj, 0))
    # and the supported ones run
    assert torch.isfinite(ReinforceTrainer(_policy()).train_step_native(traj)["loss"]).all()
    ok = PPOTrainer(_policy(), update_freq=2)
    ok.training_step(traj, 0)
    assert len(ok.traj_buffer) == 1
    ok.training_step(traj, 1)
    assert ok.traj_buffer == [] and torch.isfinite(ok._ploss).all()
