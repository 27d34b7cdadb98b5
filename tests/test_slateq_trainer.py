"""SlateQTrainer against golden vectors of the reference's SlateQTrainer (tests/golden/slateq/slateq_*.npz, made by
tests/golden_gen/make_slateq_golden.py from the unmodified reference under the Lightning-loop emulation): the generator
path and the native step; the conditions the fixture inputs hold; the surface (signatures, parameter class, input type,
what is refused).
Tolerances are those of tests/test_pdqn_trainer.py: losses 1e-4 * |ref| + 2e-6, parameters of every network 2e-5 absolute
after every step, reporter fields 2e-5 relative to the largest magnitude, with equal shapes."""
import dataclasses
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, Golden
from reagent_amd import synthetic
from reagent_amd.core import types as rlt
from reagent_amd.core.parameters import EvaluationParameters, RLParameters, SlateOptMethod, SlateOptParameters
from reagent_amd.models import FullyConnectedCritic
from reagent_amd.optimizer import Optimizer__Union
from reagent_amd.training import NextSlateValueNormMethod, SlateQTrainer, SlateQTrainerParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["slateq_single_sarsa_timediff", "slateq_single_maxq", "slateq_multi_sarsa_norm_next",
         "slateq_multi_maxq_norm_current_timediff"]


def _generator_module():
    spec = importlib.util.spec_from_file_location("make_slateq_golden",
                                                  os.path.join(ROOT, "tests", "golden_gen", "make_slateq_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(g, device):
    c = g.cfg
    mk = lambda: FullyConnectedCritic(c["state_dim"], c["doc_dim"], c["sizes"], c["activations"])  # noqa: E731
    q, qt = mk(), mk()
    with torch.no_grad():
        for net in (q, qt):
            for p, init in zip(net.parameters(), g.seq("init_q_")):
                p.copy_(init)
    tr = SlateQTrainer(q.to(device), qt.to(device), c["slate_size"], rl=RLParameters(**c["rl"]),
                       optimizer=Optimizer__Union.default(lr=c["lr"]), slate_opt_parameters=SlateOptParameters(),
                       discount_time_scale=c["discount_time_scale"], single_selection=c["single_selection"],
                       next_slate_value_norm_method=NextSlateValueNormMethod(c["norm"]))
    return tr.to(device)


def check(tr, g, s, tol=2e-5):
    for n, net in dict(q=tr.q_network, target=tr.q_network_target).items():
        for i, p in enumerate(net.parameters()):
            err = (p.detach().cpu() - g.t(f"step{s}_{n}_{i}")).abs().max().item()
            assert err <= tol, (s, n, i, err)


def check_loss(got, g, key):
    ref = float(g.t(key))
    assert abs(float(got) - ref) <= 1e-4 * abs(ref) + 2e-6, (key, float(got), ref)


def lightning_like_step(tr, opts, batch, batch_idx):
    losses = []
    for i, opt in enumerate(opts):
        loss = tr.training_step(batch, batch_idx, i)
        if loss is not None:
            opt.zero_grad()
            loss.backward()
            opt.step()
        losses.append(None if loss is None else loss.detach())
    return losses


@pytest.mark.parametrize("name", CASES)
def test_generator_path_matches_reference(backend, name):
    g = Golden("slateq/" + name)
    tr = build(g, backend.device)
    opts = [o["optimizer"] for o in tr.configure_optimizers()]
    assert [type(o).__name__ for o in opts] == ["FusedAdam", "SoftUpdate"]
    seen = {}

    class Reporter:
        def log(self, **kw):
            seen.update(kw)

    tr.set_reporter(Reporter())
    for s in range(g.cfg["steps"]):
        seen.clear()
        d = g.batch(s)
        batch = synthetic.to_slateq_input(d, backend.device)
        next_action = batch.next_action.clone()
        losses = lightning_like_step(tr, opts, batch, s)
        assert len(losses) == 2
        check_loss(losses[0], g, f"step{s}_td_loss")
        check(tr, g, s)
        assert torch.equal(batch.next_action, next_action)  # terminal rows are zeroed inside the kernel, not in the batch
        want = {k[len(f"step{s}_report_"):]: g.t(k) for k in g.z.files if k.startswith(f"step{s}_report_")}
        assert set(seen) == set(want) == {"td_loss", "model_values_on_logged_actions"}
        for k, ref in want.items():
            assert tuple(seen[k].shape) == tuple(ref.shape), k
            assert (seen[k].cpu() - ref).abs().max() <= 2e-5 * max(1.0, ref.abs().max().item()), k
        n = int(d["reward_mask"].sum())
        assert tuple(want["model_values_on_logged_actions"].shape) == ((n,) if g.cfg["single_selection"] else (g.cfg["batch"], 1))
    assert tr.all_batches_processed == g.cfg["steps"]


@pytest.mark.parametrize("name", CASES)
def test_native_step_matches_reference(backend, name):
    g = Golden("slateq/" + name)
    tr = build(g, backend.device)
    for s in range(g.cfg["steps"]):
        out = tr.train_step_native(synthetic.to_slateq_input(g.batch(s), backend.device))
        assert set(out) == {"td_loss"}
        check_loss(out["td_loss"].item(), g, f"step{s}_td_loss")
        check(tr, g, s)
        if g.cfg["rl"]["maxq_learning"]:  # the slate the reference's scores select, in descending order
            want = torch.sort(g.t(f"step{s}_ref_scores"), dim=1, descending=True, stable=True).indices[:, :g.cfg["slate_size"]]
            assert torch.equal(tr._next_idx.cpu(), want)


def test_fixture_inputs_hold_their_conditions():
    """stated here on the committed files, independently of the generator's own check: every state and next state has a
    present candidate; in the non-single cases at least two states per batch have fewer than K present candidates in the
    normalising state; every batch has at least two terminal rows, each with a non-zero logged next_action index; every
    reward_mask has an all-false row and a true entry; in the maxq cases neighbouring scores among the K + 1 largest of a row
    differ by at least 1e-3 of the row's largest magnitude unless both are exactly 0"""
    for i, name in enumerate(CASES):
        g = Golden("slateq/" + name)
        c = g.cfg
        K = c["slate_size"]
        assert (c["batch"], c["num_candidates"], K, c["steps"]) == (16, 7, 3, 4)
        assert c["single_selection"] == (i < 2) and c["rl"]["maxq_learning"] == bool(i % 2)
        for s in range(c["steps"]):
            b = g.batch(s)
            assert b["item_mask"].dtype == b["next_item_mask"].dtype == b["reward_mask"].dtype == torch.bool
            assert b["item_mask"].any(1).all() and b["next_item_mask"].any(1).all()
            if i >= 2:
                norm = b["next_item_mask"] if c["norm"] == "norm_by_next_slate_size" else b["item_mask"]
                assert int((norm.sum(1) < K).sum()) >= 2
            terminal = b["not_terminal"][:, 0] == 0
            assert int(terminal.sum()) >= 2 and (b["next_action"][terminal] != 0).any(1).all()
            assert (~b["reward_mask"]).all(1).any() and b["reward_mask"].any()
            assert g.has(f"step{s}_ref_scores") == bool(i % 2)
            if i % 2:
                scores = g.t(f"step{s}_ref_scores")
                lead = torch.sort(scores, dim=1, descending=True).values[:, :K + 1]
                gap, both_zero = lead[:, :-1] - lead[:, 1:], (lead[:, :-1] == 0) & (lead[:, 1:] == 0)
                assert ((gap >= 1e-3 * scores.abs().max(1, keepdim=True).values) | both_zero).all()
                if i == 3:  # padded documents (exact zeros) reach the slate
                    assert ((lead[:, :K] == 0).any(1)).any()
        assert c["discount_time_scale"] == (2.0 if i in (0, 3) else None)
        if c["discount_time_scale"]:
            assert len(set(g.batch(0)["time_diff"].reshape(-1).tolist())) > 1
        assert os.path.getsize(os.path.join(GOLDEN, "slateq", name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "td3_twin.npz"))
    assert Golden("slateq/" + CASES[2]).cfg["norm"] == "norm_by_next_slate_size"
    assert Golden("slateq/" + CASES[3]).cfg["norm"] == "norm_by_current_slate_size"


def test_generator_check_agrees_with_the_committed_fixtures():
    """the generator's own `check_inputs` (what it holds a new batch to) passes on every committed batch"""
    mod = _generator_module()
    for name in CASES:
        g = Golden("slateq/" + name)
        assert g.cfg == mod.CASES[name]
        for s in range(g.cfg["steps"]):
            scores = g.t(f"step{s}_ref_scores") if g.has(f"step{s}_ref_scores") else None
            assert mod.check_inputs(g.cfg, g.batch(s), scores) == []


def _reference_present():
    from oracle import stubs

    return os.path.isdir(os.path.join(stubs.REFERENCE_ROOT, "reagent"))


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_what_the_reference_produces(name):
    """where the reference tree is present: regenerate the fixture in memory and compare it with the committed file"""
    if not _reference_present():
        pytest.skip("reference tree not present")
    arrays = _generator_module().generate(name)
    z = np.load(os.path.join(GOLDEN, "slateq", name + ".npz"), allow_pickle=False)
    assert set(arrays) == set(z.files)
    for k, v in arrays.items():
        if k == "config_json":
            assert json.loads(str(v)) == json.loads(str(z[k]))
        elif v.dtype.kind in "bi":
            assert np.array_equal(v, z[k]), k
        else:
            np.testing.assert_allclose(v, z[k], rtol=1e-6, atol=1e-7, err_msg=k)


def test_signatures_equal_the_reference_record():
    """constructor / method parameter names, order and defaults against tests/golden/reference_records/
    slate_q_signatures.json (the reference's, recorded by the fixture generator), reduced and compared as
    tests/test_reference_signatures.py does; the parameter class's field order; rlt.SlateQInput's field names"""
    from test_reference_signatures import _PARAMS, _same

    ns = {}
    exec(_PARAMS, ns)
    rec = json.load(open(os.path.join(GOLDEN, "reference_records", "slate_q_signatures.json")))
    ref_path, own_path = "reagent.training.slate_q_trainer.SlateQTrainer", "reagent_amd.training.SlateQTrainer"
    assert set(rec) == {ref_path} and set(rec[ref_path]) == {"__init__", "train_step_gen", "configure_optimizers"}
    own = ns["surface"]([(own_path, sorted(rec[ref_path]))])[own_path]
    for m, ref in rec[ref_path].items():
        assert _same(ref, own[m]), (m, ref, own[m])
    p = SlateQTrainerParameters()
    assert list(p.asdict()) == ["rl", "optimizer", "slate_opt_parameters", "discount_time_scale", "single_selection",
                                "next_slate_value_norm_method", "minibatch_size", "evaluation"]
    assert isinstance(p.rl, RLParameters) and p.rl.maxq_learning is False and p.single_selection is True
    assert p.evaluation == EvaluationParameters(calc_cpe_in_training=False) and p.minibatch_size == 1024
    assert p.next_slate_value_norm_method is NextSlateValueNormMethod.NORM_BY_CURRENT_SLATE_SIZE
    q = FullyConnectedCritic(4, 2, [8], ["relu"])
    tr = SlateQTrainer(q, q, 2)
    assert tr.rl_parameters.maxq_learning is False and tr.maxq_learning is False
    names = [f.name for f in dataclasses.fields(rlt.SlateQInput)]
    assert names == ["state", "next_state", "reward", "time_diff", "step", "not_terminal", "action", "next_action",
                     "reward_mask", "extras"]
    assert [f.name for f in dataclasses.fields(rlt.DocList)] == ["float_features", "mask", "value"]


def test_doc_list_and_input_types():
    feats = torch.arange(24.0).reshape(2, 4, 3)
    docs = rlt.DocList(feats)
    assert docs.mask.dtype == torch.bool and docs.mask.all() and docs.mask.shape == (2, 4)
    assert torch.equal(docs.value, torch.ones(2, 4))
    action = torch.tensor([[3, 0], [1, 1]])
    docs = rlt.DocList(feats, torch.tensor([[True, False, True, True], [False, True, True, False]]), torch.rand(2, 4))
    sel = docs.select_slate(action)
    assert torch.equal(sel.float_features, torch.stack([feats[0, [3, 0]], feats[1, [1, 1]]]))
    assert torch.equal(sel.mask, torch.tensor([[True, True], [True, True]]))
    assert torch.equal(sel.value, torch.stack([docs.value[0, [3, 0]], docs.value[1, [1, 1]]]))
    assert torch.equal(sel.as_feature_data().float_features, sel.float_features.reshape(4, 3))
    with pytest.raises(AssertionError):
        rlt.DocList(torch.zeros(3, 2))
    d = synthetic.slateq_batch(8, 5, 3, 6, 2, seed=3)
    b = rlt.SlateQInput.from_dict(d)
    assert b.step is None and torch.equal(b.reward, d["position_reward"]) and len(b) == 8
    assert torch.equal(b.next_state.candidate_docs.mask, d["next_item_mask"])
    assert torch.equal(b.state.candidate_docs.value, d["item_probability"]) and b.action.dtype == torch.int64


def _small(device, **kw):
    q = FullyConnectedCritic(5, 3, [8], ["relu"]).to(device)
    tr = SlateQTrainer(q, q.get_target_network().to(device), 2, **kw)
    return tr, synthetic.to_slateq_input(synthetic.slateq_batch(8, 5, 3, 6, 2, seed=3), device)


def test_other_slate_optimisation_methods_are_refused(emu_lib):
    for method in (SlateOptMethod.GREEDY, SlateOptMethod.EXACT):
        tr, b = _small("cpu", rl=RLParameters(maxq_learning=True), slate_opt_parameters=SlateOptParameters(method=method))
        with pytest.raises(NotImplementedError, match="SlateQ with optimization method other than TOP_K is not implemented."):
            tr.train_step_native(b)
        opts = [o["optimizer"] for o in tr.configure_optimizers()]
        with pytest.raises(NotImplementedError, match="other than TOP_K"):
            lightning_like_step(tr, opts, b, 0)
    tr, b = _small("cpu", rl=RLParameters(maxq_learning=True), slate_opt_parameters=SlateOptParameters())
    assert torch.isfinite(tr.train_step_native(b)["td_loss"]).all()
    tr, b = _small("cpu", single_selection=False, next_slate_value_norm_method="something else")
    with pytest.raises(NotImplementedError, match="has not been implemented"):
        tr.train_step_native(b)


def test_data_parallel_is_refused(emu_lib):
    tr, b = _small("cpu")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.enable_data_parallel()
    with pytest.raises(AssertionError, match="learning input"):
        tr.train_step_native(synthetic.to_parametric_input(synthetic.parametric_batch(4, 5, 3, 2)))
