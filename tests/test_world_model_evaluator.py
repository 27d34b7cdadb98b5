"""The world-model evaluators (reagent_amd/evaluation/world_model_evaluator.py) on a two-layer MemoryNetwork, against the
reference's evaluate lines restated in float64 (tests/mdnrnn_statement.py's model and get_loss on cloned, overwritten batches)
under the self-calibrating bound, the fp32 evaluation of the same lines calibrating it."""
import pytest
import torch

from mdnrnn_statement import Statement, close
from reagent_amd import synthetic
from reagent_amd.core.parameters import MDNRNNTrainerParameters
from reagent_amd.evaluation.world_model_evaluator import (FeatureImportanceEvaluator, FeatureSensitivityEvaluator,
                                                          LossEvaluator)
from reagent_amd.models import mdn_rnn
from reagent_amd.models.world_model import MemoryNetwork
from reagent_amd.training import plumbing
from reagent_amd.training.world_model import MDNRNNTrainer

S, A, H, LAYERS, G, T, B = 5, 3, 33, 2, 2, 3, 33
STATE_STARTS, ACTION_STARTS = [0, 1, 3], [0, 2]  # state 1:3 is a two-column enum; state 3:5 and action 0:2 are blocks too
WEIGHTS = (1.0, 1.0, 1.0)


@pytest.fixture
def setup(backend):
    torch.manual_seed(4)
    net = MemoryNetwork(state_dim=S, action_dim=A, num_hiddens=H, num_hidden_layers=LAYERS, num_gaussians=G).to(backend.device)
    tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=LAYERS, num_gaussians=G, action_dim=A))
    b = synthetic.memory_network_batch(T, B, S, A, seed=2)
    b["state"][:, :, 0] = 0.625  # a constant feature: replacing it by its mean changes nothing
    b["state"][:, :, 1:3] = (torch.arange(T * B).view(T, B, 1) % 3 == torch.tensor([0, 1])).float()
    return tr, b, synthetic.to_memory_network_input(b, backend.device)


def _statement_loss(tr, b, dtype):
    m = Statement(S, A, H, LAYERS, G)
    m.load_state_dict({k: v.detach().cpu() for k, v in tr.memory_network.mdnrnn.state_dict().items()})
    m = m.to(dtype)
    with torch.no_grad():
        return torch.stack(m.losses({k: v.to(dtype) for k, v in b.items() if v is not None}, WEIGHTS))


def _importance_lines(tr, b, dtype, discrete):
    """FeatureImportanceEvaluator.evaluate of the reference in dtype -> loss increases, action features first"""
    def value(cols):  # compute_median_feature_value
        if cols.shape[1] == 1:
            return cols.mean(dim=0)
        counts = cols.sum(dim=0)
        first = int((counts == torch.median(counts)).nonzero()[0])
        return (torch.arange(cols.shape[1]) == first).to(cols.dtype)

    base = _statement_loss(tr, b, dtype)[3]
    out = []
    for key, dim, starts in (("action", A, ACTION_STARTS), ("state", S, STATE_STARTS)):
        bounds = (list(range(A)) if discrete and key == "action" else starts) + [dim]
        for i, (s, e) in enumerate(zip(bounds, bounds[1:])):
            rows = b[key].to(dtype).reshape(T * B, dim).clone()
            if discrete and key == "action":
                rows[:] = (torch.arange(A) == i).to(dtype)
            else:
                rows[:, s:e] = value(rows[:, s:e])
            out.append(_statement_loss(tr, dict(b, **{key: rows.view(T, B, dim)}), dtype)[3] - base)
    return torch.stack(out)


@pytest.mark.parametrize("discrete", [False, True])
def test_feature_importance(setup, monkeypatch, discrete):
    tr, b, batch = setup
    ev = FeatureImportanceEvaluator(tr, discrete, len(STATE_STARTS), A if discrete else len(ACTION_STARTS),
                                    list(range(A)) if discrete else ACTION_STARTS, STATE_STARTS)
    got = ev.evaluate(batch)["feature_loss_increase"]
    n_action = A if discrete else len(ACTION_STARTS)
    assert got.dtype.name == "float32" and got.shape == (n_action + len(STATE_STARTS),) and got[n_action] == 0.0
    ref64, ref32 = (_importance_lines(tr, b, d, discrete) for d in (torch.float64, torch.float32))
    close(torch.as_tensor(got), ref64, ref32, f"feature_loss_increase discrete={discrete}")
    monkeypatch.setattr(mdn_rnn, "SWEEP_WORKSPACE_BYTES", 1)  # one variant per chunk
    assert ev.evaluate(batch)["feature_loss_increase"].tobytes() == got.tobytes()


def test_loss_evaluator_and_feature_sensitivity(setup):
    tr, b, batch = setup
    got = LossEvaluator(tr, S).evaluate(batch)
    ref64, ref32 = (_statement_loss(tr, b, d) for d in (torch.float64, torch.float32))
    close(torch.tensor([got[k] for k in ("gmm", "bce", "mse", "loss")]), ref64, ref32, "LossEvaluator")
    torch.manual_seed(11)
    sens = FeatureSensitivityEvaluator(tr, len(STATE_STARTS), STATE_STARTS).evaluate(batch)["feature_sensitivity"]
    torch.manual_seed(11)
    perm = torch.randperm(B)

    def statement(dtype):
        m = Statement(S, A, H, LAYERS, G)
        m.load_state_dict({k: v.detach().cpu() for k, v in tr.memory_network.mdnrnn.state_dict().items()})
        m = m.to(dtype)
        with torch.no_grad():
            mus, shuffled = (m(a.to(dtype), b["state"].to(dtype))[0] for a in (b["action"], b["action"][:, perm, :]))
        bounds = STATE_STARTS + [S]
        return torch.stack([(shuffled[..., s:e] - mus[..., s:e]).abs().sum(dim=3).mean() for s, e in zip(bounds, bounds[1:])])

    close(torch.as_tensor(sens), statement(torch.float64), statement(torch.float32), "feature_sensitivity")


def test_refusals_by_name(setup):
    tr, _, batch = setup
    with pytest.raises(NotImplementedError, match="must be a reagent_amd MDNRNNTrainer"):
        LossEvaluator(torch.nn.Linear(2, 2), S)
    with pytest.raises(ValueError, match="sorted_state_feature_start_indices .* is not sorted inside the vector"):
        FeatureImportanceEvaluator(tr, False, 3, 2, ACTION_STARTS, [0, 3, 1]).evaluate(batch)
    with pytest.raises(ValueError, match="sorted_action_feature_start_indices .* is not sorted inside the vector"):
        FeatureImportanceEvaluator(tr, False, 3, 2, [0, A], STATE_STARTS).evaluate(batch)
    tr._graph_mode = True  # (what plumbing.enable_graph_mode sets on a trainer that allows capture)
    for ev in (FeatureImportanceEvaluator(tr, False, 3, 2, ACTION_STARTS, STATE_STARTS), FeatureSensitivityEvaluator(tr, 3, STATE_STARTS)):
        with pytest.raises(NotImplementedError, match="HIP graph"):
            ev.evaluate(batch)
    with pytest.raises(NotImplementedError, match="HIP graph"):
        plumbing.enable_graph_mode(tr)
