"""CEMTrainer over two MDNRNNTrainers: the members train exactly as they do alone, through the generator path and through
train_step_native; the planner sees a training step on its next call; CEMPolicy's output; the constructor signatures."""
import copy
import json
import os

import numpy as np
import torch

from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.core.parameters import CEMTrainerParameters, MDNRNNTrainerParameters
from reagent_amd.gym.policies import CEMPolicy
from reagent_amd.models.cem_planner import CEMPlannerNetwork
from reagent_amd.models.world_model import MemoryNetwork
from reagent_amd.training import CEMTrainer
from reagent_amd.training.world_model import MDNRNNTrainer

HERE = os.path.dirname(os.path.abspath(__file__))
SIGNATURES = os.path.join(HERE, "golden", "reference_records", "cem_signatures.json")
S, A, H, LAYERS, G = 3, 2, 8, 2, 3


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _nets(dev, seed=0):
    torch.manual_seed(seed)
    return [MemoryNetwork(S, A, H, LAYERS, G).to(dev) for _ in range(2)]


def _planner(nets, discrete=False, **kw):
    bounds = {} if discrete else dict(action_upper_bounds=np.ones(A), action_lower_bounds=-np.ones(A))
    return CEMPlannerNetwork(nets, kw.pop("iterations", 3), 24, 1, 6, 4, S, A, discrete, True, 0.9, **bounds, **kw)


def _trainer(nets):
    p = MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=LAYERS, num_gaussians=G, action_dim=A, learning_rate=0.01)
    params = CEMTrainerParameters(plan_horizon_length=4, num_world_models=2, cem_population_size=24, cem_num_iterations=3,
                                  ensemble_population_size=1, num_elites=6, mdnrnn=p)
    members = [MDNRNNTrainer(n, p) for n in nets]
    return CEMTrainer(_planner(nets), members, params), members, p


def _batch(dev):
    return synthetic.to_memory_network_input(synthetic.memory_network_batch(4, 6, S, A, seed=3), dev)


def _state_of(net, opt):
    ps = list(net.mdnrnn.parameters())
    return [p.detach().cpu().clone() for p in ps], [opt.state[p]["exp_avg"].detach().cpu().clone() for p in ps], \
        [opt.state[p]["exp_avg_sq"].detach().cpu().clone() for p in ps]


def _alone(dev, i, batch):
    """member i trained alone for one step through the generator path -> (parameters, exp_avg, exp_avg_sq)"""
    net = _nets(dev)[i]
    tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=LAYERS, num_gaussians=G, action_dim=A,
                                                    learning_rate=0.01))
    opt = tr.configure_optimizers()[0]
    loss = tr.training_step(batch, 0)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return _state_of(net, opt)


def test_members_train_as_they_do_alone_on_both_paths(backend):
    dev = backend.device
    batch = _batch(dev)
    nets = _nets(dev)
    tr, members, _ = _trainer(nets)
    opts = tr.configure_optimizers()
    assert len(opts) == 2
    for o, n in zip(opts, nets):  # both optimizers, in order: each holds its own member's parameters
        held = {id(p) for g in o.param_groups for p in g["params"]}
        assert held == {id(p) for p in n.mdnrnn.parameters()}
    for k, o in enumerate(opts):
        loss = tr.training_step(batch, 0, optimizer_idx=k)
        o.zero_grad()
        loss.backward()
        o.step()
    assert tr.all_batches_processed == 1
    gen = [_state_of(n, o) for n, o in zip(nets, opts)]
    nets2 = _nets(dev)
    tr2, members2, _ = _trainer(nets2)
    out = tr2.train_step_native(batch)
    assert len(out) == 2 and set(out[0]) == {"gmm", "bce", "mse", "loss"} and tr2.all_batches_processed == 1
    nat = [_state_of(n, m._native_opt) for n, m in zip(nets2, members2)]
    for i in range(2):
        alone = _alone(dev, i, batch)
        for group_a, group_g, group_n in zip(alone, gen[i], nat[i]):
            for x, y, z in zip(group_a, group_g, group_n):
                assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z))


def test_the_planner_sees_a_training_step(backend):
    dev = backend.device
    nets = _nets(dev)
    with torch.no_grad():  # planted: action[0] drives every gate of layer 0, so the plan depends on the weights
        for n in nets:
            n.mdnrnn.rnn.weight_ih_l0[:, 0] += 1.0
    tr, members, _ = _trainer(nets)
    state = rlt.FeatureData(torch.randn(1, S, generator=torch.Generator().manual_seed(1)))
    torch.manual_seed(5)
    before = tr.cem_planner_network(state)
    tr.train_step_native(_batch(dev))
    torch.manual_seed(5)
    after = tr.cem_planner_network(state)
    fresh = _planner([copy.deepcopy(n) for n in nets])
    torch.manual_seed(5)
    want = fresh(state)
    assert torch.equal(after.view(torch.int64), want.view(torch.int64))
    assert not torch.equal(after, before)


def test_cem_policy(backend):
    nets = _nets(backend.device)
    state = rlt.FeatureData(torch.randn(1, S))
    out = CEMPolicy(_planner(nets), False).act(state)
    assert isinstance(out, rlt.ActorOutput) and out.action.shape == (1, A) and out.log_prob.shape == () and out.log_prob.item() == 0.0
    out = CEMPolicy(_planner(nets, discrete=True), True).act(state, possible_actions_mask=None)
    assert out.action.shape == (1, A) and out.action.sum().item() == 1.0 and out.action.dtype == torch.float32
    assert out.log_prob.item() == 0.0


def test_signatures_match_the_reference():
    from test_reference_signatures import _PARAMS

    ns = {}
    exec(_PARAMS, ns)
    rec = json.load(open(SIGNATURES))
    # cross_entropy_method.py:35-43, which does not import where the record is made (it pulls in the model managers)
    rec["reagent_amd.gym.policies.cem_policy.CEMPolicy"] = {
        "__init__": [["cem_planner_network", "POSITIONAL_OR_KEYWORD", ["required"]], ["discrete_action", "POSITIONAL_OR_KEYWORD", ["required"]]],
        "act": [["obs", "POSITIONAL_OR_KEYWORD", ["required"]], ["possible_actions_mask", "POSITIONAL_OR_KEYWORD", ["value", "None"]]]}
    checked = 0
    for path, methods in rec.items():
        obj = ns["resolve"](path.replace("reagent.", "reagent_amd.", 1))
        for m, want in methods.items():
            got = json.loads(json.dumps(ns["params"](getattr(obj, m))))
            assert got[:len(want)] == want, (path, m, got, want)
            assert all(p[1] == "KEYWORD_ONLY" or p[2] != ["required"] for p in got[len(want):]), (path, m, got)  # ours: optional
            checked += 1
    assert checked == 14
