"""DisjointLinUCBTrainer on the three fixtures of the unmodified reference (tests/golden/cb_disjoint/*.npz,
tests/golden_gen/make_disjoint_cb_golden.py): two epochs of three steps, step by step, on the interpreter and, under
`-m gpu`, on the MI355X.  u = 2^-24.

After every step the epoch's sums are held, per arm and entry, to the float64 sum of disjoint_linucb_trainer.py:66-76 with
the bound of tests/test_cb_disjoint_kernels.py carried from step to step (bound' = bound * (1 + 2 u) + (n_a + 2) u
sum|w x_i x_j| + 2 u |value|); the reference's recorded buffers are held to the same bounds.

After every epoch end inv_A, coefs and the held-out scores are held to the reference's within TOL.  TOL is 4 x the
reference's OWN distance (max-abs over the largest entry, the worse of the two epochs) from the float64 inverse of the
float64 A / gamma + lambda I built from its recorded A and b -- 4 x because the LAPACK build and the last bits of A
differ.  Measured (profiles/NOTES_r13.md):
                                inv_A       coefs       scores
    dlinucb_plain               4.247e-07   5.315e-07   4.525e-07
    dlinucb_weighted_ragged     4.586e-07   3.281e-07   3.620e-07
    dlinucb_mean_only           3.106e-07   4.158e-07   2.487e-07
"""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cb_disjoint")
U = 2.0 ** -24
CASES = ["dlinucb_plain", "dlinucb_weighted_ragged", "dlinucb_mean_only"]
KEYS = ("inv_A", "coefs", "scores")
MEASURED = {  # the reference against float64, see the module docstring
    "dlinucb_plain": (4.247e-07, 5.315e-07, 4.525e-07),
    "dlinucb_weighted_ragged": (4.586e-07, 3.281e-07, 3.620e-07),
    "dlinucb_mean_only": (3.106e-07, 4.158e-07, 2.487e-07),
}
TOL = {name: {k: 4.0 * m for k, m in zip(KEYS, row)} for name, row in MEASURED.items()}


def _load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        g = {k: f[k] for k in f.files}
    return g, json.loads(str(g["config_json"]))


def _batch(g, c, e, s, dev):
    from reagent_amd.core.types import CBInput

    out = []
    for a in range(c["arms"]):
        w = g.get(f"e{e}_s{s}_a{a}_weight")
        out.append(CBInput(context_arm_features=torch.from_numpy(g[f"e{e}_s{s}_a{a}_x"]).to(dev),
                           reward=torch.from_numpy(g[f"e{e}_s{s}_a{a}_reward"]).to(dev),
                           weight=None if w is None else torch.from_numpy(w).to(dev)))
    return out


def _trainer(c, dev):
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
    from reagent_amd.training import DisjointLinUCBTrainer

    scorer = DisjointLinearRegressionUCB(c["arms"], c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"],
                                         gamma=c["gamma"]).to(dev)
    return DisjointLinUCBTrainer(Policy(scorer=scorer, sampler=None)), scorer


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _t64(a):
    return torch.from_numpy(np.asarray(a)).double()


class _Statement:
    """the epoch's sums in float64 from the fixture's sub-batches, with the bound carried along"""

    def __init__(self, arms, d):
        self.A, self.b = torch.zeros(arms, d, d, dtype=torch.float64), torch.zeros(arms, d, dtype=torch.float64)
        self.bound_A, self.bound_b = torch.zeros_like(self.A), torch.zeros_like(self.b)
        self.n = torch.zeros(arms, dtype=torch.int64)

    def step(self, g, e, s):
        for a in range(self.A.shape[0]):
            x, y = _t64(g[f"e{e}_s{s}_a{a}_x"]), _t64(g[f"e{e}_s{s}_a{a}_reward"]).reshape(-1)
            n = x.shape[0]
            w = _t64(g[f"e{e}_s{s}_a{a}_weight"]).reshape(-1) if f"e{e}_s{s}_a{a}_weight" in g else torch.ones(n, dtype=torch.float64)
            self.A[a] += x.t() @ (x * w[:, None])
            self.b[a] += x.t() @ (w * y)
            self.n[a] += n
            if n == 0:
                continue  # (an empty sub-batch leaves the arm alone: no rounding either)
            absA, absb = x.abs().t() @ (x.abs() * w[:, None]), x.abs().t() @ (w * y).abs()
            self.bound_A[a] = self.bound_A[a] * (1 + 2 * U) + (n + 2) * U * absA + 2 * U * self.A[a].abs()
            self.bound_b[a] = self.bound_b[a] * (1 + 2 * U) + (n + 2) * U * absb + 2 * U * self.b[a].abs()

    def check(self, who, A, b):
        for name, got, ref, bound in (("cur_A", A, self.A, self.bound_A), ("cur_b", b, self.b, self.bound_b)):
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
    gamma, i, carried = c["gamma"], 0, {"A": 0.0, "b": 0.0}
    for e in range(c["epochs"]):
        st = _Statement(c["arms"], c["d"])
        for s in range(c["steps"]):
            assert tr.training_step(_batch(g, c, e, s, dev), i) is None
            st.step(g, e, s)
            st.check(("ours", e, s), scorer.cur_A, scorer.cur_b)
            st.check(("reference", e, s), g[f"e{e}_s{s}_cur_A"], g[f"e{e}_s{s}_cur_b"])
            assert torch.equal(scorer.cur_num_obs.cpu(), st.n) and torch.equal(st.n, torch.from_numpy(g[f"e{e}_s{s}_cur_num_obs"]))
            assert scorer.cur_num_obs.device == scorer.cur_A.device
            assert torch.equal(scorer.cur_A, scorer.cur_A.transpose(1, 2))
            if c["twin_arms"]:  # the same rows at other positions of the packed batch: the same bits
                assert torch.equal(scorer.cur_A[1], scorer.cur_A[2]) and torch.equal(scorer.cur_b[1], scorer.cur_b[2])
            i += 1
        tr.on_train_epoch_end()
        ref = lambda k: torch.from_numpy(g[f"e{e}_end_{k}"])  # noqa: E731
        # A = (A + cur_A) * gamma on both sides: each side's cur_A is within the epoch's bound of the float64 sums, so the two
        # are within twice it of each other; `+=` and `*= gamma` round once on each side (2 u |value| each); what the earlier
        # epochs left is carried, scaled by gamma like the values themselves
        for k, bound in (("A", st.bound_A), ("b", st.bound_b)):
            got, want = getattr(scorer, k).cpu().double(), ref(k).double()
            carried[k] = gamma * (carried[k] + 2 * bound + 2 * U * (want / gamma).abs()) + 2 * U * want.abs()
            assert ((got - want).abs() <= carried[k]).all(), (e, k)
        for k in ("cur_A", "cur_b"):
            assert not getattr(scorer, k).any() and not ref(k).any()
        assert not scorer.cur_num_obs.any()
        assert torch.equal(scorer.coefs_valid_for_A, scorer.A) and torch.equal(ref("coefs_valid_for_A"), ref("A"))
        if c["twin_arms"]:
            for k in ("A", "b", "inv_A", "coefs"):
                assert torch.equal(getattr(scorer, k)[1], getattr(scorer, k)[2]), k
        scores = scorer(held)
        tol = TOL[name]
        for k, got, want in (("inv_A", scorer.inv_A, ref("inv_A")), ("coefs", scorer.coefs, ref("coefs")),
                             ("scores", scores, g[f"e{e}_heldout_scores"])):
            assert tuple(got.shape) == tuple(want.shape)
            r = _rel(got, want)
            print(name, e, k, f"{r:.3e} of {tol[k]:.3e}")
            assert r <= tol[k], (e, k, r, tol[k])
        want_actions = torch.from_numpy(g[f"e{e}_heldout_actions"])
        assert torch.equal(get_model_actions(scores, presence).cpu(), want_actions)
        both = scorer.forward_with_actions(held, arm_presence=presence)
        assert torch.equal(both["model_actions"].cpu(), want_actions) and torch.equal(both["ucb"], scores)
        assert both["model_actions"].shape == (c["heldout"], 1) and both["model_actions"].dtype == torch.int64
        if c["twin_arms"]:  # an exact tie in every row; where it is the (present) maximum the lower index wins
            assert torch.equal(scores[:, 1].view(torch.int32), scores[:, 2].view(torch.int32))
            top = scores.max(1).values
            rows = (scores[:, 1] == top).cpu()
            assert rows.any() and (both["model_actions"].cpu().reshape(-1)[rows] == 1).all()


@pytest.mark.parametrize("name", CASES)
def test_measured_tolerances_are_the_references_own_error(name):
    """MEASURED is what the committed fixture says: the reference's recorded inverse, coefficients and held-out scores
    against the float64 inverse of the float64 A / gamma + lambda I of its recorded sums"""
    g, c = _load(name)
    worst = dict.fromkeys(KEYS, 0.0)
    eye = torch.eye(c["d"], dtype=torch.float64)
    for e in range(c["epochs"]):
        # (recorded after the discount; the matrix inverted saw the sums before it)
        A, b = _t64(g[f"e{e}_end_A"]) / c["gamma"], _t64(g[f"e{e}_end_b"]) / c["gamma"]
        ext = A + c["l2_reg_lambda"] * eye
        assert all(torch.linalg.cond(ext[a]).item() <= 100 for a in range(c["arms"]))
        inv = torch.linalg.inv(ext)
        coefs = torch.einsum("jkl,jl->jk", inv, b)
        x = _t64(g["heldout_x"])
        scores = x @ coefs.t()
        if c["ucb_alpha"] != 0:
            scores = scores + c["ucb_alpha"] * torch.einsum("ijk,jk->ji", torch.matmul(x, inv), x).sqrt()
        want = dict(zip(KEYS, (inv, coefs, scores)))
        got = dict(zip(KEYS, (g[f"e{e}_end_inv_A"], g[f"e{e}_end_coefs"], g[f"e{e}_heldout_scores"])))
        for k in KEYS:
            worst[k] = max(worst[k], _rel(got[k], want[k]))
    print(name, "  ".join(f"{worst[k]:.3e}" for k in KEYS))
    for k, m in zip(KEYS, MEASURED[name]):
        assert worst[k] == pytest.approx(m, rel=2e-3, abs=0), (k, worst[k], m)


@pytest.mark.parametrize("name", CASES)
def test_reference_state_dict_loads_and_scores_like_the_trained_model(backend, name):
    """the state_dict the reference's scorer had at the end (every buffer and dummy_param, under the reference's names) loads
    strictly and scores the held-out rows like the model trained here from the same sub-batches"""
    dev = backend.device
    g, c = _load(name)
    tr, trained = _trainer(c, dev)
    i = 0
    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            tr.training_step(_batch(g, c, e, s, dev), i)
            i += 1
        tr.on_train_epoch_end()
    _, loaded = _trainer(c, dev)
    last = c["epochs"] - 1
    sd = {k[len(f"e{last}_end_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"e{last}_end_")}
    assert set(sd) == set(loaded.state_dict()) and "cur_num_obs" not in sd
    assert all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in loaded.state_dict().items())
    loaded.load_state_dict(sd, strict=True)
    held = torch.from_numpy(g["heldout_x"]).to(dev)
    want = g[f"e{last}_heldout_scores"]
    for out in (loaded(held), trained(held)):
        assert _rel(out, want) <= TOL[name]["scores"]


def test_a_step_is_one_accumulate_call_and_equal_sizes_upload_nothing(backend, monkeypatch):
    """cb_training_step packs the list and calls rg_dlinucb_accumulate once; the device copy of row_offsets and the
    workspace are made once per tuple of sub-batch sizes"""
    from reagent_amd import ops

    dev = backend.device
    g, c = _load("dlinucb_weighted_ragged")
    tr, scorer = _trainer(c, dev)
    tr.training_step(_batch(g, c, 0, 0, dev), 0)
    calls = []
    real = ops.dlinucb_accumulate

    def counted(x, y, w, offsets, longest, *a):
        calls.append((tuple(x.shape), w is not None, offsets.data_ptr(), offsets.tolist(), longest, a[3].data_ptr()))
        return real(x, y, w, offsets, longest, *a)

    monkeypatch.setattr(ops, "dlinucb_accumulate", counted)
    monkeypatch.setattr(ops, "dlinucb_workspace", lambda *a, **k: pytest.fail("a second workspace for the same sizes"))
    tr.training_step(_batch(g, c, 0, 2, dev), 1)  # the same sizes (arm 0 without weights this time: ones are filled in)
    tr.training_step(_batch(g, c, 1, 0, dev), 2)
    assert len(calls) == 2 and calls[0] == calls[1]
    assert calls[0][0] == (64, c["d"]) and calls[0][1] and calls[0][3] == [0, 37, 48, 59, 64] and calls[0][4] == 37
    assert scorer.cur_num_obs.tolist() == [111, 33, 33, 15]


def test_refusals(backend):
    import torch.nn as nn

    from reagent_amd.core.types import CBInput
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
    from reagent_amd.models.linear_regression import LinearRegressionUCB
    from reagent_amd.training import DisjointLinUCBTrainer, LinUCBTrainer

    dev = backend.device
    g, c = _load("dlinucb_plain")
    tr, scorer = _trainer(c, dev)
    batch = _batch(g, c, 0, 0, dev)
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.attach_eval_module(object())
    tr.eval_module = object()
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.training_step(batch, 0)
    tr.eval_module = None
    policy = Policy(scorer=scorer, sampler=None)
    with pytest.raises(NotImplementedError, match="recmetric_module"):
        DisjointLinUCBTrainer(policy, recmetric_module=object(), log_every_n_steps=5)
    with pytest.raises(AssertionError, match="if and only if"):
        DisjointLinUCBTrainer(policy, log_every_n_steps=5)
    with pytest.raises(AssertionError, match="DisjointLinUCBTrainer requires the policy scorer to be DisjointLinearRegressionUCB"):
        DisjointLinUCBTrainer(Policy(scorer=LinearRegressionUCB(c["d"]), sampler=None))
    with pytest.raises(AssertionError, match="DisjointLinearRegressionUCB"):
        DisjointLinUCBTrainer(Policy(scorer=nn.Linear(c["d"], 1), sampler=None))
    with pytest.raises(NotImplementedError, match="512"):
        DisjointLinearRegressionUCB(2, 513)
    wrong = list(batch)
    wrong[2] = CBInput(context_arm_features=torch.zeros(4, c["d"] + 1, device=dev), reward=torch.zeros(4, 1, device=dev))
    with pytest.raises(ValueError, match="input_dim"):
        tr.training_step(wrong, 0)
    with pytest.raises(ValueError, match="input_dim"):
        tr.update_params(1, torch.zeros(4, c["d"] + 1, device=dev), torch.zeros(4, 1, device=dev))
    with pytest.raises(AssertionError):  # the reference's three assertions
        tr.training_step(batch[:-1], 0)
    with pytest.raises(AssertionError):
        tr.training_step([CBInput(context_arm_features=b.context_arm_features.unsqueeze(1), reward=b.reward) for b in batch], 0)
    with pytest.raises(AssertionError):
        tr.training_step([CBInput(context_arm_features=b.context_arm_features) for b in batch], 0)
    assert not scorer.cur_num_obs.any() and not scorer.cur_A.any()  # none of the refused calls trained
    # a list handed to the joint trainer is still refused
    joint = LinUCBTrainer(Policy(scorer=LinearRegressionUCB(c["d"]).to(dev), sampler=None))
    with pytest.raises(NotImplementedError, match=r"List\[CBInput\]"):
        joint.training_step(batch, 0)
    assert tr.training_step(batch, 0) is None and scorer.cur_num_obs.tolist() == [37] * 4


def test_world_size_above_one_is_refused(monkeypatch):
    import torch.distributed as dist

    from reagent_amd.gym.policies import Policy
    from reagent_amd.models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
    from reagent_amd.training import DisjointLinUCBTrainer

    scorer = DisjointLinearRegressionUCB(3, 4)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="world > 1"):
        DisjointLinUCBTrainer(Policy(scorer=scorer, sampler=None))
    with pytest.raises(NotImplementedError, match="world > 1"):
        scorer._estimate_coefs()
