"""DeepRepresentLinUCBTrainer on the four fixtures of the unmodified reference (tests/golden/cb_deep/*.npz,
tests/golden_gen/make_deep_cb_golden.py): two epochs of three steps, step by step, on the interpreter and, under `-m gpu`,
on the MI355X, in PREC_F32.  Every fixture is replayed twice -- through training_step + backward + step (the Lightning
loop) and through train_step_native -- and the two replays give the same bits.

Bounds (u = 2^-24), those the LinUCB and policy-gradient trainer tests apply to the same kinds of quantity:
  losses                      1e-4 |ref| + 2e-6                                            (tests/test_pg_trainers.py)
  parameters, batch-norm statistics, Adam's moments   2e-5 absolute                        (tests/test_pg_trainers.py)
  the epoch's averages        the any-order bound of tests/test_cb_kernels.py on the step's own z, from the state the
                              reference recorded before the step (exact "given the same z": the z used is OURS)
  counts                      exact
  inv_avg_A, _coefs, held-out outputs    relative to the largest entry, 4 x the reference's own fp32 distance from the
                              float64 inverse of its recorded averages (tests/test_linucb_trainer.py's rule) + 2e-5 for
                              the representation the held-out rows are scored on
New here: the parameters of drlinucb_plain_coefs_weighted (nn_e2e=False) receive their gradient through the LinUCB
coefficients, so through the inverse.  Their bound is derived below (`_float64_replay`) as 4 x the largest distance, over
the six steps, between the reference's recorded fp32 parameters and a float64 replay of the same steps -- 4 x because ours
differs from the reference in summation order and in elimination order, each an error of the reference's own kind and
size.  The spread is 1.09e-7, the bound 4.36e-7 (fifty times tighter than the 2e-5 of the other cases); ours measured
8.9e-8 on the interpreter (profiles/NOTES_r14.md has the values of both machines).
"""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cb_deep")
U = 2.0 ** -24
CASES = ["drlinucb_defaults", "drlinucb_plain_coefs_weighted", "drlinucb_sigmoid_bce_layernorm", "drlinucb_mae_mean_only"]
BATCH_KEYS = ("context_arm_features", "arm_presence", "action", "reward", "weight", "importance_weight")
MODEL_KEYS = ("output_activation", "l2_reg_lambda", "ucb_alpha", "gamma", "use_batch_norm", "normalize_output",
              "use_layer_norm", "use_skip_connections", "nn_e2e")
PARAM_TOL, MARGIN = 2e-5, 4.0


def _load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        g = {k: f[k] for k in f.files}
    return g, json.loads(str(g["config_json"]))


def _batch(g, e, s, dev):
    from reagent_amd.core.types import CBInput

    d = {k: torch.from_numpy(g[f"e{e}_s{s}_batch_{k}"]).to(dev) for k in BATCH_KEYS if f"e{e}_s{s}_batch_{k}" in g}
    return CBInput.from_dict(d)


def _trainer(g, c, dev, **over):
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models import DeepRepresentLinearRegressionUCB
    from reagent_amd.training import DeepRepresentLinUCBTrainer

    scorer = DeepRepresentLinearRegressionUCB(c["F"], list(c["sizes"]), list(c["activations"]),
                                              **dict({k: c[k] for k in MODEL_KEYS}, **over))
    if g is not None:
        scorer.load_state_dict({k[len("init_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init_")},
                               strict=True)
    scorer = scorer.to(dev)
    tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=c["lr"], weight_decay=c["weight_decay"],
                                    loss_type=c["loss_type"])
    return tr, scorer


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _t64(a):
    return torch.from_numpy(np.asarray(a)).double()


LINUCB = ("avg_A", "avg_b", "cur_avg_A", "cur_avg_b", "_coefs", "inv_avg_A", "coefs_valid_for_avg_A", "num_obs",
          "cur_num_obs", "sum_weight", "cur_sum_weight")


def _snapshot(scorer, opt):
    sd = {k: v.detach().cpu().clone() for k, v in scorer.state_dict().items()}
    names = {id(p): n for n, p in scorer.named_parameters()}
    adam = {}
    for p, st in opt.state.items():
        if len(st):
            for k in ("exp_avg", "exp_avg_sq", "step"):
                adam[f"{names[id(p)]}_{k}"] = torch.as_tensor(st[k]).detach().cpu().clone().reshape(-1 if k == "step" else st[k].shape)
    return sd, adam


def _reference_inverse_error(g, c, prefix, discounted):
    """the reference's recorded inverse and coefficients against the float64 inverse of its recorded averages"""
    d = c["sizes"][-1] + 1
    A, b = _t64(g[prefix + "avg_A"]), _t64(g[prefix + "avg_b"])
    sw = _t64(g[prefix + "sum_weight"]) / (c["gamma"] if discounted else 1.0)
    inv = torch.linalg.inv(A + c["l2_reg_lambda"] * torch.eye(d, dtype=torch.float64) / sw)
    return _rel(g[prefix + "inv_avg_A"], inv), _rel(g[prefix + "_coefs"], inv @ b)


def _float64_replay(g, c):
    """drlinucb_plain_coefs_weighted in float64 (plain Linear -> relu stack, mean through the LinUCB coefficients, weighted
    mse, torch's Adam): -> the largest distance of the reference's recorded fp32 parameters from it, over all steps"""
    assert not c["use_batch_norm"] and not c["use_layer_norm"] and not c["nn_e2e"] and c["loss_type"] == "mse"
    n_layers = len(c["sizes"])
    Ws = [_t64(g[f"init_deep_represent_layers.dnn.{i}.0.weight"]).requires_grad_() for i in range(n_layers)]
    bs = [_t64(g[f"init_deep_represent_layers.dnn.{i}.0.bias"]).requires_grad_() for i in range(n_layers)]
    opt = torch.optim.Adam(Ws + bs, lr=c["lr"], weight_decay=c["weight_decay"])
    d = c["sizes"][-1] + 1
    eye = torch.eye(d, dtype=torch.float64)
    A, b, sw = torch.zeros(d, d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64), float(np.float32(1e-5))
    cA, cb, cw = torch.zeros_like(A), torch.zeros_like(b), float(np.float32(1e-5))
    worst = 0.0

    def fold():
        nonlocal A, b, sw, cA, cb, cw
        tot = sw + cw
        A, b, sw = (A * sw + cA * cw) / tot, (b * sw + cb * cw) / tot, tot
        cA, cb, cw = torch.zeros_like(A), torch.zeros_like(b), 0.0
        return torch.linalg.inv(A + c["l2_reg_lambda"] * eye / sw) @ b

    for e in range(c["epochs"]):
        for s in range(c["steps"]):
            x3, action = _t64(g[f"e{e}_s{s}_batch_context_arm_features"]), torch.from_numpy(g[f"e{e}_s{s}_batch_action"])
            B = x3.shape[0]
            x = torch.gather(x3, 1, action.view(B, 1, 1).expand(-1, 1, x3.shape[2])).squeeze(1)
            y = _t64(g[f"e{e}_s{s}_batch_reward"]).reshape(B)
            w = (torch.from_numpy(g[f"e{e}_s{s}_batch_weight"]) * torch.from_numpy(g[f"e{e}_s{s}_batch_importance_weight"]))
            w = w.double().reshape(B)
            coefs = fold() if (s > 0 or e == 0) else coefs  # noqa: F821 (after an epoch end nothing moved: no recalculation)
            hcur = x
            for i in range(n_layers):
                hcur = hcur @ Ws[i].t() + bs[i]
                if c["activations"][i] == "relu":
                    hcur = torch.relu(hcur)
            z = torch.cat([torch.ones(B, 1, dtype=torch.float64), hcur], 1)
            loss = (((z @ coefs.detach()) - y) ** 2 * w).sum() / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            zd, s_w = z.detach(), w.sum()
            cw = cw + s_w
            keep = 1.0 - s_w / cw
            cA, cb = cA * keep + zd.t() @ (zd * w[:, None]) / cw, cb * keep + zd.t() @ (w * y) / cw
            for i in range(n_layers):
                for kind, t in (("weight", Ws[i]), ("bias", bs[i])):
                    ref = _t64(g[f"e{e}_s{s}_sd_deep_represent_layers.dnn.{i}.0.{kind}"])
                    worst = max(worst, (ref - t.detach()).abs().max().item())
        coefs = fold()
        sw = sw * c["gamma"]
    return worst


def _replay(name, dev, native, check):
    """one replay of a fixture -> per step (loss, state_dict, Adam state), per epoch end (state_dict, held-out outputs)"""
    from reagent_amd.training.cb import get_model_actions

    g, c = _load(name)
    tr, scorer = _trainer(g, c, dev)
    opt = tr.native_optimizers()[0] if native else tr.configure_optimizers()
    held = torch.from_numpy(g["heldout_x"]).to(dev)
    presence = torch.from_numpy(g["heldout_presence"]).to(dev) if "heldout_presence" in g else None
    param_tol = PARAM_TOL
    if check and name == "drlinucb_plain_coefs_weighted":
        spread = _float64_replay(g, c)
        param_tol = MARGIN * spread
        print(name, f"reference fp32 against the float64 replay: {spread:.3e}; bound {param_tol:.3e}")
        assert 0 < param_tol <= PARAM_TOL
    d = c["sizes"][-1] + 1
    trace, i, num_obs = [], 0, 0
    for e in range(c["epochs"]):
        scorer.train()
        for s in range(c["steps"]):
            batch = _batch(g, e, s, dev)
            before = {k: scorer.state_dict()[k].detach().cpu().clone() for k in ("cur_avg_A", "cur_avg_b", "cur_sum_weight")}
            solved = scorer._coefs_dirty
            if native:
                loss = tr.train_step_native(batch)
            else:
                opt.zero_grad()
                loss = tr.training_step(batch, i)
                loss.backward()
                opt.step()
            sd, adam = _snapshot(scorer, opt)
            trace.append((loss.detach().cpu().clone().reshape(1), sd, adam))
            i += 1
            if not check:
                continue
            who = (name, e, s)
            ref_loss = float(g[f"e{e}_s{s}_loss"][0])
            loss = loss.detach()
            print(name, e, s, f"loss {float(loss):.7f} reference {ref_loss:.7f}")
            assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss) + 2e-6, who
            z, pred = tr._bufs["z"].cpu(), tr._bufs["pred"].cpu()
            assert torch.equal(z[:, 0], torch.ones(len(z)))
            assert (z - torch.from_numpy(g[f"e{e}_s{s}_mlp_out_with_ones"])).abs().max() <= PARAM_TOL, who
            assert (pred - torch.from_numpy(g[f"e{e}_s{s}_pred_label"])).abs().max() <= PARAM_TOL, who
            worst = {}
            for k, v in sd.items():
                ref = torch.from_numpy(g[f"e{e}_s{s}_sd_{k}"])
                assert v.shape == ref.shape and v.dtype == ref.dtype, (who, k)
                if k in LINUCB or k == "dummy_param":
                    continue
                err = (v.double() - ref.double()).abs().max().item()
                kind = "bn_count" if k.endswith("num_batches_tracked") else ("bn_stat" if "running_" in k else "param")
                worst[kind] = max(worst.get(kind, 0.0), err)
                assert err <= (0 if kind == "bn_count" else PARAM_TOL if kind == "bn_stat" else param_tol), (who, k, err)
            ref_adam = {k[len(f"e{e}_s{s}_adam_"):] for k in g if k.startswith(f"e{e}_s{s}_adam_")}
            assert set(adam) == ref_adam, (who, set(adam) ^ ref_adam)  # (the same parameters are skipped)
            for k, v in adam.items():
                ref = torch.from_numpy(g[f"e{e}_s{s}_adam_{k}"])
                err = (v.double() - ref.double()).abs().max().item()
                worst["adam"] = max(worst.get("adam", 0.0), err)
                assert err <= (0 if k.endswith("_step") else PARAM_TOL), (who, k, err)
            print(name, e, s, " ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())), f"(parameter bound {param_tol:.3e})")
            assert torch.equal(sd["dummy_param"], torch.zeros(1))
            # the epoch's averages from the state before the step and OUR z: the bounds of tests/test_cb_kernels.py
            y = _t64(g[f"e{e}_s{s}_batch_reward"]).reshape(-1)
            B = len(y)
            w = torch.ones(B, dtype=torch.float64)
            if f"e{e}_s{s}_batch_weight" in g:
                w = (torch.from_numpy(g[f"e{e}_s{s}_batch_weight"])
                     * torch.from_numpy(g[f"e{e}_s{s}_batch_importance_weight"])).double().reshape(B)
            z64 = z.double()
            cw0 = 0.0 if solved else before["cur_sum_weight"].double().item()
            cA0 = torch.zeros(d, d, dtype=torch.float64) if solved else before["cur_avg_A"].double()
            cb0 = torch.zeros(d, dtype=torch.float64) if solved else before["cur_avg_b"].double()
            s_w = w.sum()
            cw1 = cw0 + s_w
            keep = 1.0 - s_w / cw1
            for k, want, asum in (("cur_avg_A", cA0 * keep + z64.t() @ (z64 * w[:, None]) / cw1, z64.abs().t() @ (z64.abs() * w[:, None])),
                                  ("cur_avg_b", cb0 * keep + z64.t() @ (w * y) / cw1, z64.abs().t() @ (w * y).abs())):
                bound = (B + 2) * U * asum / cw1 + 8 * U * want.abs()
                assert ((sd[k].double() - want).abs() <= bound).all(), (who, k)
            assert abs(sd["cur_sum_weight"].item() - cw1.item()) <= (B + 2) * U * w.sum().item() + 8 * U * cw1.item(), who
            num_obs_before = num_obs
            assert sd["cur_num_obs"].item() == g[f"e{e}_s{s}_sd_cur_num_obs"].item()
            assert sd["num_obs"].item() == g[f"e{e}_s{s}_sd_num_obs"].item(), who
            assert torch.equal(sd["cur_avg_A"], sd["cur_avg_A"].t())
            if solved and (e > 0 or s > 0):  # the solve at the start of this step against the reference's
                ref_inv, ref_coefs = _reference_inverse_error(g, c, f"e{e}_s{s}_sd_", False)
                for k, m in (("inv_avg_A", ref_inv), ("_coefs", ref_coefs)):
                    r = _rel(sd[k], g[f"e{e}_s{s}_sd_{k}"])
                    assert r <= MARGIN * m + PARAM_TOL, (who, k, r, m)
            del num_obs_before
        tr.on_train_epoch_end()
        assert int(scorer._solve_status.item()) == 0 and not scorer._coefs_dirty
        scorer.eval()
        out = scorer(held)
        end = {k: v.detach().cpu().clone() for k, v in scorer.state_dict().items()}
        trace.append((end, {k: v.cpu().clone() for k, v in out.items()}))
        if not check:
            continue
        assert set(out) == {"pred_label", "pred_sigma", "ucb", "mlp_out_with_ones"}
        for k in ("cur_avg_A", "cur_avg_b", "cur_sum_weight", "cur_num_obs"):
            assert not end[k].any() and not g[f"e{e}_end_{k}"].any()
        assert torch.equal(end["coefs_valid_for_avg_A"], end["avg_A"])
        assert end["num_obs"].item() == g[f"e{e}_end_num_obs"].item()
        ref_inv, ref_coefs = _reference_inverse_error(g, c, f"e{e}_end_", True)
        for k, m in (("inv_avg_A", ref_inv), ("_coefs", ref_coefs), ("avg_A", 0.0), ("avg_b", 0.0), ("sum_weight", 0.0)):
            r = _rel(end[k], g[f"e{e}_end_{k}"])
            print(name, e, "end", k, f"{r:.3e} (reference against float64 {m:.3e})")
            assert r <= MARGIN * m + PARAM_TOL, (e, k, r)
        for k in ("pred_label", "pred_sigma", "ucb", "mlp_out_with_ones"):
            want = g[f"e{e}_heldout_{k}"]
            assert tuple(out[k].shape) == want.shape, k
            r = _rel(out[k], want) if np.abs(want).max() > 0 else out[k].abs().max().item()
            print(name, e, "held-out", k, f"{r:.3e}")
            assert r <= MARGIN * max(ref_inv, ref_coefs) + PARAM_TOL, (e, k, r)
        want_actions = torch.from_numpy(g[f"e{e}_heldout_actions"])
        assert torch.equal(get_model_actions(out["ucb"], presence).cpu(), want_actions)
        both = scorer.forward_with_actions(held, arm_presence=presence)
        assert torch.equal(both["model_actions"].cpu(), want_actions) and torch.equal(both["ucb"], out["ucb"])
        tie = out["ucb"][:, 1] == out["ucb"][:, 2]
        assert tie[0] and tie[3]  # the planted ties are exact here too
    return trace


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_fixture_step_by_step_and_the_two_paths_agree(backend, name):
    lightning = _replay(name, backend.device, native=False, check=True)
    native = _replay(name, backend.device, native=True, check=False)
    assert _same(lightning, native)


def test_state_dict_round_trips_under_the_references_keys(backend):
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_records", "deep_cb_signatures.json")))
    rec = rec["reagent.models.deep_represent_linucb.DeepRepresentLinearRegressionUCB"]
    from reagent_amd.models import DeepRepresentLinearRegressionUCB

    for tag, kw in (("defaults", {}), ("plain", dict(use_batch_norm=False, use_skip_connections=False)),
                    ("layer_norm", dict(use_batch_norm=False, use_skip_connections=False, use_layer_norm=True))):
        m = DeepRepresentLinearRegressionUCB(9, [8, 8, 5], ["relu", "relu", "linear"], **kw)
        sd = m.state_dict()
        assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()} == rec["state_dict"][tag], tag
        assert [n for n, _ in m.named_parameters()] == rec["parameters"][tag], tag
    name = "drlinucb_defaults"
    g, c = _load(name)
    last = c["epochs"] - 1
    sd = {k[len(f"e{last}_end_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"e{last}_end_")}
    _, loaded = _trainer(None, c, "cpu")
    loaded.load_state_dict(sd, strict=True)
    loaded = loaded.to(backend.device).eval()
    assert not loaded._coefs_dirty
    out = loaded(torch.from_numpy(g["heldout_x"]).to(backend.device))
    for k in ("pred_label", "pred_sigma", "ucb", "mlp_out_with_ones"):
        assert _rel(out[k], g[f"e{last}_heldout_{k}"]) <= PARAM_TOL, k
    back = {k: v.cpu() for k, v in loaded.state_dict().items()}
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    inf = loaded.forward_inference(torch.from_numpy(g["heldout_x"]).to(backend.device))
    assert torch.equal(inf["pred_sigma"], out["pred_sigma"]) and torch.equal(inf["mlp_out_with_ones"], out["mlp_out_with_ones"])


def test_dimension_129_takes_the_host_path_and_matches(backend, monkeypatch):
    """sizes[-1] + 1 = 129 is above rg_linucb_solve's range: the parent's host path, against the same model solved through
    the float64 inverse"""
    from reagent_amd import ops
    from reagent_amd.core.types import CBInput

    dev = backend.device
    c = dict(_load("drlinucb_plain_coefs_weighted")[1], sizes=[8, 128], activations=["relu", "linear"], weight_decay=0.0)
    torch.manual_seed(5)
    tr, scorer = _trainer(None, c, dev)
    assert scorer.input_dim == 129
    monkeypatch.setattr(ops, "linucb_solve", lambda *a, **k: pytest.fail("the kernel was called at d = 129"))
    gen = torch.Generator().manual_seed(6)
    B = 600
    for i in range(2):
        x = torch.randn(B, 3, c["F"], generator=gen).to(dev)
        batch = CBInput(context_arm_features=x, action=torch.randint(0, 3, (B, 1), generator=gen).to(dev),
                        reward=torch.randn(B, 1, generator=gen).to(dev))
        tr.train_step_native(batch)
    tr.on_train_epoch_end()
    A, b, sw = scorer.avg_A.cpu().double(), scorer.avg_b.cpu().double(), scorer.sum_weight.cpu().double() / c["gamma"]
    inv = torch.linalg.inv(A + c["l2_reg_lambda"] * torch.eye(129, dtype=torch.float64) / sw)
    e_ref = _rel(torch.linalg.inv((A + c["l2_reg_lambda"] * torch.eye(129, dtype=torch.float64) / sw).float()), inv)
    assert _rel(scorer.inv_avg_A, inv) <= MARGIN * e_ref + 129 * 2 * U
    assert scorer.num_obs.item() == 2 * B and not scorer.cur_avg_A.any()


def test_a_failed_pivot_is_recomputed_on_the_host_once(backend):
    g, c = _load("drlinucb_defaults")
    _, scorer = _trainer(g, dict(c, l2_reg_lambda=0.0), backend.device)
    d = scorer.input_dim
    v = torch.randn(d, generator=torch.Generator().manual_seed(1))
    scorer.cur_avg_A.copy_(torch.outer(v, v))  # rank one, no regularisation: a zero pivot
    scorer.cur_sum_weight.fill_(10.0)
    scorer.mark_dirty()
    scorer._calculate_coefs()
    assert int(scorer._solve_status.item()) == 1
    scorer.check_solve_status()  # the parent's inv / pinv on the host, from the folded avg_A
    assert int(scorer._solve_status.item()) == 0 and not scorer._solve_unchecked
    from reagent_amd.models.linear_regression import matrix_inv_fallback_pinv

    assert torch.equal(scorer.avg_A.cpu(), (torch.outer(v, v) * 10.0) / (torch.tensor(10.0) + torch.tensor(1e-5)))
    want = matrix_inv_fallback_pinv(scorer.avg_A.cpu() + 0.0 * torch.eye(d) / scorer.sum_weight.cpu())
    assert torch.allclose(scorer.inv_avg_A.cpu(), want, rtol=0, atol=0, equal_nan=True)
    assert not scorer.cur_avg_A.any() and scorer.cur_sum_weight.item() == 0.0


def test_refusals(backend):
    import torch.nn as nn

    from reagent_amd.gym.policies import Policy
    from reagent_amd.models import DeepRepresentLinearRegressionUCB, LinearRegressionUCB
    from reagent_amd.training import DeepRepresentLinUCBTrainer

    dev = backend.device
    g, c = _load("drlinucb_defaults")
    tr, scorer = _trainer(g, c, dev)
    batch = _batch(g, 0, 0, dev)
    with pytest.raises(AssertionError, match="DeepRepresentLinearRegressionUCB"):
        DeepRepresentLinUCBTrainer(Policy(scorer=LinearRegressionUCB(4), sampler=None))
    with pytest.raises(AssertionError, match="DeepRepresentLinearRegressionUCB"):
        DeepRepresentLinUCBTrainer(Policy(scorer=nn.Linear(4, 1), sampler=None))
    policy = Policy(scorer=scorer, sampler=None)
    with pytest.raises(NotImplementedError, match="recmetric_module"):
        DeepRepresentLinUCBTrainer(policy, recmetric_module=object(), log_every_n_steps=5)
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.attach_eval_module(object())
    tr.eval_module = object()
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="eval_module"):
        tr.train_step_native(batch)
    tr.eval_module = None
    for step in (lambda b: tr.training_step(b, 0), tr.train_step_native):
        with pytest.raises(NotImplementedError, match=r"List\[CBInput\]"):
            step([batch, batch])
    with pytest.raises(NotImplementedError, match="world > 1"):
        tr.enable_data_parallel()
    with pytest.raises(KeyError, match="loss_type"):
        DeepRepresentLinUCBTrainer(policy, loss_type="huber")
    with pytest.raises(NotImplementedError, match="mlp_layers"):
        DeepRepresentLinearRegressionUCB(9, [8, 5], ["relu", "linear"], mlp_layers=nn.Linear(9, 5))
    with pytest.raises(NotImplementedError, match="output_activation"):
        DeepRepresentLinearRegressionUCB(9, [8, 5], ["relu", "linear"], output_activation="gelu")
    assert scorer.cur_num_obs.item() == 0 and scorer.num_obs.item() == 0  # none of the refused calls trained


def test_world_size_above_one_is_refused(monkeypatch):
    import torch.distributed as dist

    from reagent_amd.gym.policies import Policy
    from reagent_amd.models import DeepRepresentLinearRegressionUCB
    from reagent_amd.training import DeepRepresentLinUCBTrainer

    scorer = DeepRepresentLinearRegressionUCB(9, [8, 5], ["relu", "linear"])
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="world > 1"):
        DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None))
    with pytest.raises(NotImplementedError, match="world > 1"):
        scorer._calculate_coefs()
