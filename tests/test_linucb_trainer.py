"""LinUCBTrainer on the three fixtures of the unmodified reference (tests/golden/cb/*.npz, tests/golden_gen/make_cb_golden.py):
two epochs of three steps, step by step, on the interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24.

After every step the epoch's buffers are held to the float64 restatement of linucb_trainer.py:64-75 with the per-entry
bounds of tests/test_cb_kernels.py, carried from step to step (the earlier steps' bound shrinks by the factor the earlier
average does: bound' = bound * (1 - s_w / W) + (B + 2) u sum|w x_i x_j| / W + 8 u |value|); the reference's recorded
buffers are held to the same bounds.

After every epoch end inv_avg_A, _coefs and the held-out outputs are held to the reference's within TOL.  TOL is 4 x the
reference's OWN distance (max-abs over the largest entry, the worse of the two epochs) from the float64 inverse of the
float64 A_extended built from its recorded avg_A, avg_b and sum_weight -- 4 x because the LAPACK build and the last bits of
avg_A differ.  Measured (profiles/NOTES_r12.md):
                                inv_avg_A   _coefs      pred_label  pred_sigma  ucb
    linucb_plain                8.320e-08   9.453e-08   1.148e-07   7.271e-08   1.135e-07
    linucb_weighted_discount    6.844e-08   1.195e-07   5.761e-08   8.084e-08   7.415e-08
    linucb_mean_only            6.970e-08   1.386e-07   1.711e-07   0 (exact)   1.711e-07
"""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cb")
U = 2.0 ** -24
CASES = ["linucb_plain", "linucb_weighted_discount", "linucb_mean_only"]
KEYS = ("inv_avg_A", "_coefs", "pred_label", "pred_sigma", "ucb")
MEASURED = {  # the reference against float64, see the module docstring
    "linucb_plain": (8.320e-08, 9.453e-08, 1.148e-07, 7.271e-08, 1.135e-07),
    "linucb_weighted_discount": (6.844e-08, 1.195e-07, 5.761e-08, 8.084e-08, 7.415e-08),
    "linucb_mean_only": (6.970e-08, 1.386e-07, 1.711e-07, 0.0, 1.711e-07),
}
TOL = {name: {k: 4.0 * m for k, m in zip(KEYS, row)} for name, row in MEASURED.items()}
BATCH_KEYS = ("context_arm_features", "arm_presence", "action", "reward", "weight", "importance_weight")


def _load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        g = {k: f[k] for k in f.files}
    return g, json.loads(str(g["config_json"]))


def _batch(g, e, s, dev):
    from reagent_amd.core.types import CBInput

    d = {k: torch.from_numpy(g[f"e{e}_s{s}_batch_{k}"]).to(dev) for k in BATCH_KEYS if f"e{e}_s{s}_batch_{k}" in g}
    return CBInput.from_dict(d)


def _trainer(c, dev):
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.linear_regression import LinearRegressionUCB
    from reagent_amd.training import LinUCBTrainer

    scorer = LinearRegressionUCB(c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"], gamma=c["gamma"]).to(dev)
    return LinUCBTrainer(Policy(scorer=scorer, sampler=None)), scorer


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _t64(a):
    return torch.from_numpy(np.asarray(a)).double()


class _Statement:
    """the epoch's averages in float64 from the fixture's batches, with the bound carried along"""

    def __init__(self, d, sum_weight):
        self.A, self.b, self.sw = torch.zeros(d, d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64), sum_weight
        self.bound_A, self.bound_b, self.bound_sw = torch.zeros_like(self.A), torch.zeros_like(self.b), U * sum_weight

    def step(self, g, e, s):
        x3, action = _t64(g[f"e{e}_s{s}_batch_context_arm_features"]), torch.from_numpy(g[f"e{e}_s{s}_batch_action"])
        B, _, d = x3.shape
        x = torch.gather(x3, 1, action.view(B, 1, 1).expand(-1, 1, d)).squeeze(1)
        y = _t64(g[f"e{e}_s{s}_batch_reward"]).reshape(B)
        w = torch.ones(B, dtype=torch.float64)
        if f"e{e}_s{s}_batch_weight" in g:  # effective_weight: the fp32 product of the two, as the reference forms it
            w = (torch.from_numpy(g[f"e{e}_s{s}_batch_weight"]) * torch.from_numpy(g[f"e{e}_s{s}_batch_importance_weight"]))
            w = w.double().reshape(B)
        s_w = w.sum()
        self.sw = self.sw + s_w
        keep = 1.0 - s_w / self.sw
        self.A = self.A * keep + x.t() @ (x * w[:, None]) / self.sw
        self.b = self.b * keep + x.t() @ (w * y) / self.sw
        absA, absb = x.abs().t() @ (x.abs() * w[:, None]), x.abs().t() @ (w * y).abs()
        self.bound_A = self.bound_A * keep + (B + 2) * U * absA / self.sw + 8 * U * self.A.abs()
        self.bound_b = self.bound_b * keep + (B + 2) * U * absb / self.sw + 8 * U * self.b.abs()
        self.bound_sw = self.bound_sw + (B + 2) * U * w.abs().sum() + 8 * U * self.sw
        return B

    def check(self, who, A, b, sw):
        for name, got, ref, bound in (("cur_avg_A", A, self.A, self.bound_A), ("cur_avg_b", b, self.b, self.bound_b),
                                      ("cur_sum_weight", sw, self.sw.reshape(1), self.bound_sw.reshape(1))):
            err = (torch.as_tensor(got).double().cpu() - ref).abs()
            assert (err <= bound).all(), (who, name, (err / bound.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("name", CASES)
def test_fixture_step_by_step(backend, name):
    from reagent_amd.training.cb import get_model_actions

    dev = backend.device
    g, c = _load(name)
    tr, scorer = _trainer(c, dev)
    held = torch.from_numpy(g["heldout_x"]).to(dev)
    presence = torch.from_numpy(g["heldout_presence"]).to(dev) if "heldout_presence" in g else None
    num_obs, i, carried = 0, 0, {}
    for e in range(c["epochs"]):
        st = _Statement(c["d"], 1e-5 if e == 0 else 0.0)  # float32(1e-5) as constructed; exactly 0 after an epoch end
        if e == 0:
            st.sw = float(np.float32(1e-5))
        seen = 0
        for s in range(c["steps"]):
            assert tr.training_step(_batch(g, e, s, dev), i) is None
            seen += st.step(g, e, s)
            st.check(("ours", e, s), scorer.cur_avg_A, scorer.cur_avg_b, scorer.cur_sum_weight)
            st.check(("reference", e, s), g[f"e{e}_s{s}_cur_avg_A"], g[f"e{e}_s{s}_cur_avg_b"], g[f"e{e}_s{s}_cur_sum_weight"])
            assert scorer.cur_num_obs.item() == seen == g[f"e{e}_s{s}_cur_num_obs"].item()
            assert torch.equal(scorer.cur_avg_A, scorer.cur_avg_A.t())
            i += 1
        num_obs += seen
        last_A, last_b, last_sw = st.bound_A, st.bound_b, st.bound_sw
        tr.on_train_epoch_end()
        ref = lambda k: torch.from_numpy(g[f"e{e}_end_{k}"])  # noqa: E731
        # the all-data averages are the reference's weighted mean of the earlier average and the epoch's (reduce_avg): each
        # side is within the epoch's bound of the float64 statement, so they are within twice it of each other, plus the four
        # roundings of the mean itself
        # (and the earlier epochs' allowance, carried whole: the mean's weights add up to 1)
        for k, bound in (("avg_A", last_A), ("avg_b", last_b)):
            got, want = getattr(scorer, k).cpu().double(), ref(k).double()
            carried[k] = carried.get(k, 0.0) + 2 * bound + 8 * U * want.abs()
            assert ((got - want).abs() <= carried[k]).all(), (e, k)
        carried["sw"] = carried.get("sw", 0.0) + 2 * float(last_sw) + 8 * U * abs(ref("sum_weight").item())
        assert abs(scorer.sum_weight.item() - ref("sum_weight").item()) <= carried["sw"]
        assert scorer.num_obs.item() == num_obs == ref("num_obs").item()
        for k in ("cur_avg_A", "cur_avg_b", "cur_sum_weight", "cur_num_obs"):
            assert torch.equal(getattr(scorer, k).cpu(), torch.zeros_like(ref(k))) and not ref(k).any()
        assert torch.equal(scorer.coefs_valid_for_avg_A, scorer.avg_A)
        out = scorer(held)
        assert not scorer._coefs_dirty  # (the epoch end calculated the coefficients; forward did not have to)
        tol = TOL[name]
        for k in ("inv_avg_A", "_coefs"):
            r = _rel(getattr(scorer, k), ref(k))
            print(name, e, k, f"{r:.3e} of {tol[k]:.3e}")
            assert r <= tol[k], (e, k, r)
        for k in ("pred_label", "pred_sigma", "ucb"):
            want = g[f"e{e}_heldout_{k}"]
            assert out[k].shape == want.shape
            r = _rel(out[k], want) if np.abs(want).max() > 0 else out[k].abs().max().item()
            print(name, e, k, f"{r:.3e} of {tol[k]:.3e}")
            assert r <= tol[k], (e, k, r)
        want_actions = torch.from_numpy(g[f"e{e}_heldout_actions"])
        assert torch.equal(get_model_actions(out["ucb"], presence).cpu(), want_actions)
        both = scorer.forward_with_actions(held, arm_presence=presence)
        assert torch.equal(both["model_actions"].cpu(), want_actions) and torch.equal(both["ucb"], out["ucb"])
        same = scorer.forward_inference(held)
        assert all(torch.equal(same[k], out[k]) for k in out)


@pytest.mark.parametrize("name", CASES)
def test_measured_tolerances_are_the_references_own_error(name):
    """MEASURED is what the committed fixture says: the reference's recorded inverse, coefficients and held-out outputs
    against the float64 inverse of the float64 A_extended of its recorded averages"""
    g, c = _load(name)
    worst = dict.fromkeys(KEYS, 0.0)
    for e in range(c["epochs"]):
        A, b = _t64(g[f"e{e}_end_avg_A"]), _t64(g[f"e{e}_end_avg_b"])
        sw_after = _t64(g[f"e{e}_end_sum_weight"])  # (recorded after the discount; the matrix inverted saw it before)
        ext = A + c["l2_reg_lambda"] * torch.eye(c["d"], dtype=torch.float64) / (sw_after / c["gamma"])
        assert torch.linalg.cond(ext).item() <= 100
        inv = torch.linalg.inv(ext)
        coefs = inv @ b
        x = _t64(g["heldout_x"])
        label = x @ coefs
        sigma = (((x @ inv) * x).sum(-1) / sw_after).sqrt() if c["ucb_alpha"] != 0 else torch.zeros_like(label)
        want = dict(zip(KEYS, (inv, coefs, label, sigma, label + c["ucb_alpha"] * sigma)))
        got = dict(zip(KEYS, (g[f"e{e}_end_inv_avg_A"], g[f"e{e}_end__coefs"], g[f"e{e}_heldout_pred_label"],
                              g[f"e{e}_heldout_pred_sigma"], g[f"e{e}_heldout_ucb"])))
        for k in KEYS:
            worst[k] = max(worst[k], _rel(got[k], want[k]) if want[k].abs().max() > 0 else float(np.abs(got[k]).max()))
    for k, m in zip(KEYS, MEASURED[name]):
        assert worst[k] == pytest.approx(m, rel=2e-3, abs=0), (k, worst[k], m)


@pytest.mark.parametrize("name", CASES)
def test_reference_state_dict_loads_and_scores_like_the_trained_model(backend, name):
    """the state_dict the reference's scorer had at the end (every buffer and dummy_param, under the reference's names) loads
    strictly, needs no recalculation, and scores the held-out features like the model trained here from the same batches"""
    dev = backend.device
    g, c = _load(name)
    tr, trained = _trainer(c, dev)
    i = 0
    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            tr.training_step(_batch(g, e, s, dev), i)
            i += 1
        tr.on_train_epoch_end()
    _, loaded = _trainer(c, dev)
    last = c["epochs"] - 1
    sd = {k[len(f"e{last}_end_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"e{last}_end_")}
    assert set(sd) == set(loaded.state_dict())
    assert all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in loaded.state_dict().items())
    loaded.load_state_dict(sd, strict=True)
    assert not loaded._coefs_dirty
    held = torch.from_numpy(g["heldout_x"]).to(dev)
    a, b = loaded(held), trained(held)
    for k in ("pred_label", "pred_sigma", "ucb"):
        want = g[f"e{last}_heldout_{k}"]
        for out in (a, b):
            r = _rel(out[k], want) if np.abs(want).max() > 0 else out[k].abs().max().item()
            assert r <= TOL[name][k], (k, r)
    # and back: a model constructed here has the reference's initial buffers (recorded with its signatures)
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_records", "cb_signatures.json")))
    init = rec["reagent.models.linear_regression.LinearRegressionUCB"]["state_dict"]
    from reagent_amd.models.linear_regression import LinearRegressionUCB

    own = LinearRegressionUCB(3).state_dict()
    assert set(own) == set(init)
    for k, (shape, dtype, first) in init.items():
        assert list(own[k].shape) == shape and str(own[k].dtype) == dtype and float(own[k].reshape(-1)[0]) == first, k
    dirty = LinearRegressionUCB(c["d"])
    sd["cur_avg_A"] = sd["cur_avg_A"].clone()
    sd["cur_avg_A"][0, 0] = 1.0
    dirty.load_state_dict(sd)
    assert dirty._coefs_dirty  # an epoch in progress: the next forward recalculates, as the reference's comparison decides


def test_a_step_is_the_two_accumulate_launches_and_nothing_else(backend, monkeypatch):
    """training_step on a [B, A, d] batch calls rg_linucb_accumulate once (its main and finishing launch) with the
    features and the logged action as they are, and no torch operation that launches anything (views aside): the gathered
    [B, d] copy is never made, nothing is read back"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from reagent_amd import ops

    dev = backend.device
    g, c = _load("linucb_plain")
    tr, scorer = _trainer(c, dev)
    batch = _batch(g, 0, 0, dev)
    tr.training_step(batch, 0)  # (the first step allocates the workspace)
    calls, seen = [], []
    real = ops.linucb_accumulate

    def counted(x, y, w, *a, action=None, **k):
        calls.append((x.data_ptr(), x.shape, None if action is None else action.data_ptr(), w))
        return real(x, y, w, *a, action=action, **k)

    monkeypatch.setattr(ops, "linucb_accumulate", counted)
    for name in ("linucb_score", "linucb_workspace"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.__name__ if hasattr(func, "__name__") else str(func))
            return func(*args, **(kwargs or {}))

    with Recorder():
        tr.training_step(batch, 1)
    x = batch.context_arm_features
    assert calls == [(x.data_ptr(), x.shape, batch.action.data_ptr(), None)]
    views = ("view", "reshape", "_unsafe_view", "alias", "detach", "squeeze", "unsqueeze", "expand", "t", "transpose")
    assert [f for f in seen if f.split(".")[0] not in views] == [], seen
    assert scorer.cur_num_obs.item() == 2 * len(batch)


def test_refusals(backend):
    import torch.nn as nn

    from reagent_amd.core.types import CBInput
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.linear_regression import LinearRegressionUCB
    from reagent_amd.training import LinUCBTrainer
    from reagent_amd.training.cb import add_chosen_arm_features, get_model_actions

    dev = backend.device
    g, c = _load("linucb_plain")
    tr, scorer = _trainer(c, dev)
    batch = _batch(g, 0, 0, dev)
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.attach_eval_module(object())
    tr.eval_module = object()
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.training_step(batch, 0)
    tr.eval_module = None
    policy = Policy(scorer=scorer, sampler=None)
    with pytest.raises(NotImplementedError, match="recmetric_module"):
        LinUCBTrainer(policy, recmetric_module=object(), log_every_n_steps=5)
    with pytest.raises(AssertionError, match="if and only if"):
        LinUCBTrainer(policy, log_every_n_steps=5)
    with pytest.raises(NotImplementedError, match="randomize_ties"):
        get_model_actions(torch.zeros(2, 3, device=dev), randomize_ties=True)
    with pytest.raises(NotImplementedError, match=r"List\[CBInput\]"):
        tr.training_step([batch, batch], 0)
    with pytest.raises(NotImplementedError, match=r"List\[CBInput\]"):
        add_chosen_arm_features([batch, batch])
    with pytest.raises(AssertionError, match="LinearRegressionUCB"):
        LinUCBTrainer(Policy(scorer=nn.Linear(c["d"], 1), sampler=None))
    with pytest.raises(NotImplementedError, match="512"):
        LinearRegressionUCB(513)
    with pytest.raises(ValueError, match="input_dim"):
        tr.training_step(CBInput(context_arm_features=torch.zeros(4, 2, c["d"] + 1, device=dev),
                                 action=torch.zeros(4, 1, dtype=torch.int64, device=dev),
                                 reward=torch.zeros(4, 1, device=dev)), 0)
    assert scorer.cur_num_obs.item() == 0  # none of the refused calls trained


def test_world_size_above_one_is_refused(monkeypatch):
    import torch.distributed as dist

    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.linear_regression import LinearRegressionUCB
    from reagent_amd.training import LinUCBTrainer

    scorer = LinearRegressionUCB(4)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="world > 1"):
        LinUCBTrainer(Policy(scorer=scorer, sampler=None))
    with pytest.raises(NotImplementedError, match="world > 1"):
        scorer._calculate_coefs()
