"""Feature importance by perturbation (reagent_amd/csrc/feature_importance.hip: rg_fi_sweep, rg_fi_finish) and its module
(reagent_amd/evaluation/feature_importance).  The statement is plain float64 torch: materialise x_v, run the stack, mean |delta|,
one rounding.  Exact where bits are the statement; otherwise 4 x the worst error of the EXISTING per-layer PREC_F32 forward on
the materialised perturbed batches against float64 on the same inputs (layer 0's sum is reassociated), that path's result rounded
to fp32 as a result is.  NaN fills every pitch padding."""
import numpy as np
import pytest
import torch

import reagent_amd._lib as L
import reagent_amd.evaluation.feature_importance.feature_importance_perturbation as fi_module
from fc_refs import act64, ints, same_bits
from reagent_amd import ops
from reagent_amd.core.parameters import NormalizationParameters
from reagent_amd.evaluation.feature_importance import FeatureImportancePerturbation, create_default_perturb_fn
from reagent_amd.models import FullyConnectedDQN
from reagent_amd.models.dueling_q_network import DuelingQNetwork
from reagent_amd.prediction.predictor_wrapper import DiscreteDqnWithPreprocessor, ServingFeatureData
from reagent_amd.preprocessing import Preprocessor

MODES = sorted(L.FI_REDUCE, key=L.FI_REDUCE.get)  # max_q, logged_action, per_action
NARROW = [(0, 1), (1, 4), (2, 5), (4, 5)]  # widths 1 and 3, two blocks at the last columns of D = 5


def _padded(t, pad=3):
    big = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def _case(dims, B, V, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: ints(g, *s).float()) if integer else (lambda *s: torch.randn(*s, generator=g))
    Ws = [draw(o, i) * (1.0 if integer else i ** -0.5) for i, o in zip(dims, dims[1:])]
    bs = [draw(o) for o in dims[1:]]
    perm = torch.stack([torch.randperm(B, generator=g) for _ in range(V)])
    mask = torch.nn.functional.one_hot(torch.randint(dims[-1], (B,), generator=g), dims[-1]).float()
    return draw(B, dims[0]), Ws, bs, perm, mask


def _layer(dev, h, W, b, act):
    y = _padded(torch.empty(h.shape[0], W.shape[0], device=dev))
    ops.fc_forward(h, W.to(dev), b.to(dev), L.ACT[act], L.PREC_F32, y32=y)
    return y


def _forward(dev, x, Ws, bs, acts):
    """the existing per-layer PREC_F32 launches -> z0, q"""
    q = _padded(x.to(dev))
    z0 = _layer(dev, q, Ws[0], bs[0], "linear")
    for W, b, a in zip(Ws, bs, acts):
        q = _layer(dev, q, W, b, a)
    return z0, q


def _pred(q, mode, mask):
    q = q.double()
    return q.max(dim=1, keepdim=True)[0] if mode == "max_q" else (q * mask.double()).sum(1, keepdim=True) if mode == "logged_action" else q


def _stack64(x, Ws, bs, acts):
    h = x.double()
    for W, b, a in zip(Ws, bs, acts):
        h = act64(h @ W.double().T + b.double(), a)
    return h


def _variant(x, perm, s, e):
    xv = x.clone()
    xv[:, s:e] = x[perm, s:e]
    return xv


def _statement(x, Ws, bs, acts, perm, table, mode, mask, run=_stack64):
    base = _pred(run(x, Ws, bs, acts), mode, mask)
    return torch.stack([(_pred(run(_variant(x, p, s, e), Ws, bs, acts), mode, mask) - base).abs().mean(0)
                        for p, (s, e) in zip(perm, table)])


def _sweep(dev, x, Ws, bs, acts, perm, table, mode, mask):
    z0, q = _forward(dev, x, Ws, bs, acts)
    V, B, C = len(table), x.shape[0], Ws[-1].shape[0] if mode == "per_action" else 1
    reduce = L.FI_REDUCE[mode]
    partials = torch.full((ops.fi_partials(B, V, Ws[-1].shape[0], reduce),), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((V, C), float("nan"), device=dev)
    ops.fi_sweep(_padded(x.to(dev)), z0, perm.to(torch.int32).to(dev), torch.tensor(table, dtype=torch.int32).to(dev),
                 [W.to(dev) for W in Ws], [b.to(dev) for b in bs], [L.ACT[a] for a in acts], q,
                 _padded(mask.to(dev)) if mode == "logged_action" else None, reduce, max(e - s for s, e in table), partials)
    ops.fi_finish(partials, B, out)
    return out.cpu()


def _bound(dev, x, Ws, bs, acts, perm, table, mode, mask, ref):
    existing = _statement(x, Ws, bs, acts, perm, table, mode, mask, run=lambda *a: _forward(dev, *a)[1].cpu())
    worst = (existing.float().double() - ref).abs().max().item()  # (rounded to fp32 as a result is: inside the measured figure)
    print(f"{mode}: existing per-layer path worst |error| {worst:.3e}, new path allowed 4 x that")
    return 4 * worst


@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("dims", [[5, 33, 16, 3], [40, 64, 3]])
def test_identity_perm_and_empty_block_are_exactly_zero(backend, dims, B):
    D = dims[0]
    table = [(0, D), (D - 2, D - 2), (0, D), (1, 2)]  # identity over everything, empty, two real variants
    acts = ["tanh"] * (len(dims) - 2) + ["linear"]
    x, Ws, bs, perm, mask = _case(dims, B, len(table), 3 * B + D)
    perm[0] = torch.arange(B)
    for mode in MODES:
        got = _sweep(backend.device, x, Ws, bs, acts, perm, table, mode, mask)
        assert same_bits(got[:2], torch.zeros_like(got[:2])), (mode, got)
        assert not got.isnan().any() and (B == 1 or (got[2:] > 0).all()), (mode, got)


@pytest.mark.parametrize("mode", MODES)
def test_integer_operands_give_the_float64_statement_bit_for_bit(backend, mode):
    dims, B, acts = [5, 33, 16, 3], 33, ["relu", "relu", "linear"]
    x, Ws, bs, perm, mask = _case(dims, B, len(NARROW), 17, integer=True)
    got = _sweep(backend.device, x, Ws, bs, acts, perm, NARROW, mode, mask)
    assert same_bits(got, _statement(x, Ws, bs, acts, perm, NARROW, mode, mask).float()), got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims,table", [([5, 33, 16, 3], NARROW), ([40, 64, 3], [(0, 1), (2, 37), (8, 40), (37, 40)]),
                                        ([5, 512, 33, 3], NARROW)])
def test_random_operands_within_the_float64_bound(backend, dims, table, mode):
    B, acts = 33, (["tanh", "leaky_relu", "tanh"] * 2)[:len(dims) - 2] + ["linear"]
    x, Ws, bs, perm, mask = _case(dims, B, len(table), 100 + dims[1])
    got = _sweep(backend.device, x, Ws, bs, acts, perm, table, mode, mask).double()
    ref = _statement(x, Ws, bs, acts, perm, table, mode, mask)
    bound = _bound(backend.device, x, Ws, bs, acts, perm, table, mode, mask, ref)
    print(f"{mode} {dims}: new path worst |error| {(got - ref).abs().max().item():.3e}")
    assert ((got - ref).abs() <= bound).all(), (got - ref).abs() / bound


PRED = {"max_q": lambda q, d: q.max(dim=1, keepdim=True)[0], "per_action": lambda q, d: q,
        "logged_action": lambda q, d: (q * d["action"]).sum(1, keepdim=True)}  # the sentinels as pred_fn bodies


def _module(dev, sizes=(33, 16), **kw):
    norm = {1: NormalizationParameters(feature_type="CONTINUOUS", mean=0.5, stddev=2.0),
            2: NormalizationParameters(feature_type="CONTINUOUS", mean=-1.0, stddev=0.5),
            3: NormalizationParameters(feature_type="ENUM", possible_values=[10, 11, 12]),
            4: NormalizationParameters(feature_type="BINARY")}
    pre = Preprocessor(norm, device=dev)
    torch.manual_seed(2)
    net = FullyConnectedDQN(pre.num_output_features, 3, list(sizes), ["relu", "tanh"][:len(sizes)], **kw).to(dev)
    return DiscreteDqnWithPreprocessor(net, pre), pre


def _loader(dev, B=33, batches=2):
    g = torch.Generator().manual_seed(8)
    out = []
    for _ in range(batches):  # columns in the Preprocessor's order: BINARY 4, CONTINUOUS 1, 2, ENUM 3
        v = torch.randn(B, 4, generator=g)
        v[:, 3] = torch.randint(10, 13, (B,), generator=g).float()
        out.append({"state_features": (v.to(dev), (torch.rand(B, 4, generator=g) > 0.2).to(torch.uint8).to(dev)),
                    "action": torch.nn.functional.one_hot(torch.randint(3, (B,), generator=g), 3).float().to(dev)})
    return out


@pytest.mark.parametrize("mode", MODES)
def test_module_matches_the_reference_loop_and_repeats_to_the_bit(backend, monkeypatch, mode):
    dev = backend.device
    model, pre = _module(dev)
    ids, data = pre.sorted_features, _loader(dev)

    def through_the_model(m, d):
        return PRED[mode](m(ServingFeatureData(float_features_with_presence=d["state_features"])), d)

    def run(pred_fn, cap=None):
        if cap is not None:  # a workspace cap below one variant's partials: the sweep goes variant by variant
            monkeypatch.setattr(fi_module, "WORKSPACE_CAP_BYTES", cap)
        torch.manual_seed(5)
        fi = FeatureImportancePerturbation(model, ids, data, pred_fn, create_default_perturb_fn("state_features"), repeat=2)
        df = fi.compute_feature_importance()
        assert list(df.columns) == ["feature_id", "feature_importance"] and df["feature_importance"].is_monotonic_decreasing
        return df.set_index("feature_id")["feature_importance"].reindex(ids).to_numpy(), fi

    (native, fi), (again, _), loop = run(mode), run(mode, cap=1), torch.tensor(run(through_the_model)[0]).double()
    assert np.array_equal(native, again) and pre.column_blocks() == [(0, 1), (1, 2), (2, 3), (3, 6)]
    if mode == "per_action":
        per = fi.per_action_importance  # [F, A], each rounded to fp32: its row mean is the column within those roundings
        assert per.shape == (4, 3) and np.allclose(per.double().mean(1).numpy(), native, rtol=2.0 ** -22, atol=0)
    with pytest.raises(ValueError, match="leading input columns"):
        FeatureImportancePerturbation(model, ids[::-1], data, mode).compute_feature_importance()
    # the float64 statement on the same normalized batches and the same randperm stream
    lin = model.model.fc.linears()
    Ws, bs = [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin]
    torch.manual_seed(5)
    ref = torch.zeros(len(ids), dtype=torch.float64)
    for d in data:
        x = pre(*d["state_features"]).cpu()
        for _ in range(2):
            perm = [torch.randperm(x.shape[0]) for _ in ids]
            ref += _statement(x, Ws, bs, ["relu", "tanh", "linear"], perm, pre.column_blocks(), mode, d["action"].cpu()).mean(1) / 4
    bound = 4 * (loop - ref).abs().max()  # (the loop's values are fp32 already)
    assert ((torch.tensor(native).double() - ref).abs() <= bound).all(), (native, loop, ref)


@pytest.mark.parametrize("name,make", [
    ("batch norm", lambda: _module("cpu", use_batch_norm=True)[0]), ("layer norm", lambda: _module("cpu", use_layer_norm=True)[0]),
    ("a dueling head", lambda: DiscreteDqnWithPreprocessor(DuelingQNetwork.make_fully_connected(6, 3, [8, 8], ["relu", "relu"]),
                                                           None)),
    ("a foreign model", lambda: torch.nn.Linear(6, 3)), ("a hidden width of 513", lambda: _module("cpu", sizes=(513,))[0])])
def test_refusals_by_name(name, make):
    with pytest.raises(NotImplementedError, match=name):
        FeatureImportancePerturbation(make(), [4, 1, 2, 3], [], "max_q").compute_feature_importance()
