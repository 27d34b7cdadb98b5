"""Counterfactual policy evaluation of DQNTrainer / QRDQNTrainer (validation_step -> EvaluationDataPage -> Evaluator ->
CpeDetails) against the three fixtures of the unmodified reference (tests/golden/cpe_eval, made by
tests/golden_gen/make_cpe_eval_golden.py), on the interpreter and, under `-m gpu`, on the MI355X, in PREC_F32.  u = 2^-24.

Pages.  The fields that are copies or exact functions of the batch (mdp_id, sequence_number, logged_propensities, logged_rewards,
action_mask, possible_actions_mask, logged_metrics, eval_action_idxs: the generator's check_inputs keeps every arg-max a gap of
1e-3 clear) are EQUAL to the fixture.  The network-derived fields are within 1e-4 absolute: the fp32 forward tolerance
tests/test_dqn_trainer.py holds these stacks' Q-values to (BASELINE.json north_star).

Gathered page.  From the fixture's OWN per-batch pages, append + sort + compute_values give the fixture's gathered order and
logged_values / logged_metrics_values bit for bit (the reference scans column 0 of logged_metrics only; so does the page).

Estimates.  Evaluator.evaluate_post_training runs on the FIXTURE's gathered page, and each raw and normalized DM / IPS / DR /
sequential-DR estimate is compared with float64 recomputed from that page.  The bound is the any-order fp32 one, stated per
row and averaged:
  a sum of A products:            (A + 1) u sum|terms|
  iw = tp / lp:                   (A + 3) u |iw|
  ips = iw r, dr = iw (r - mrl) + dm:   (A + 6) u (|iw| (|r| + |mrl|) + sum|p mr|)
  the mean of N rows in fp32 (the reference's torch.mean; ours is a double sum):  + (N + 2) u mean|rows|
  sequential DR: the same row bounds pushed through the recurrence step by step (e' = e_sv + e_iw |inner| + |iw| (g e +
  e_q + 3 u (|r| + g |d| + |q|)) + 2 u (|sv| + |iw inner|)), then the mean over episodes (a float64 mean on both sides)
  normalized = raw * normalizer: the relative bound of raw plus that of the logged mean, plus 2 u.
The reference's recorded value is held to the same bound in the same assertion.  The zero-normalizer branch gives exactly 0.0.
Standard errors: within 6 / sqrt(2 (K - 1)) = 13.4 % of sqrt(var64 / sample_size) at K = 1000, and so is the reference's recorded
one (check_inputs guarantees it); normalized_std_error == raw_std_error * normalizer for DM / IPS / DR, raw_std_error /
logged_policy_score for sequential DR (the reference divides there).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from reagent_amd.core import types as rlt
from reagent_amd.core.parameters import EvaluationParameters, RLParameters
from reagent_amd.models import FullyConnectedDQN
from reagent_amd.optimizer import Optimizer__Union
from reagent_amd.training import DQNTrainer, QRDQNTrainer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpe_eval")
CASES = ["cpe_dqn_plain", "cpe_dqn_metrics_masks", "cpe_qrdqn"]
U = 2.0 ** -24
FORWARD_TOL = 1e-4  # tests/test_dqn_trainer.py: Q-values within 1e-4 abs in fp32 mode
STD_TOL = 6.0 / math.sqrt(2.0 * 999.0)
EXACT = ("mdp_id", "sequence_number", "logged_propensities", "logged_rewards", "action_mask", "possible_actions_mask",
         "logged_metrics", "eval_action_idxs")
DERIVED = ("model_propensities", "model_rewards", "model_rewards_for_logged_action", "model_values", "optimal_q_values",
           "model_metrics", "model_metrics_for_logged_action", "model_metrics_values", "model_metrics_values_for_logged_action")
ESTIMATORS = ("direct_method", "inverse_propensity", "doubly_robust", "sequential_doubly_robust")
_CACHE = {}


def _fixture(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            arrays = {k: z[k] for k in z.files}
        _CACHE[name] = (json.loads(str(arrays["config_json"])), arrays)
    return _CACHE[name]


def _trainer(c, arrays, device, cpe=True):
    A, n_out = c["num_actions"], (len(c["cpe_metrics"]) + 1) * c["num_actions"]

    def net(out, which, num_atoms=None):
        m = FullyConnectedDQN(c["state_dim"], out, c["sizes"], c["activations"], num_atoms=num_atoms)
        if which is not None:
            m.load_state_dict({k[len(f"sd_{which}_"):]: torch.from_numpy(v) for k, v in arrays.items()
                               if k.startswith(f"sd_{which}_fc.")})
        return m.to(device)

    q = net(A, "q_network", c["num_atoms"])
    common = dict(actions=[str(i) for i in range(A)], rl=RLParameters(**c["rl"]), double_q_learning=c["double_q"],
                  optimizer=Optimizer__Union.default(lr=c["lr"]), evaluation=EvaluationParameters(calc_cpe_in_training=cpe))
    if cpe:
        reward_net, q_cpe = net(n_out, "reward_network"), net(n_out, "q_network_cpe")
        common.update(reward_network=reward_net, q_network_cpe=q_cpe, q_network_cpe_target=q_cpe.get_target_network(),
                      metrics_to_score=list(c["cpe_metrics"]))
    else:
        common.update(reward_network=None)
    if c["num_atoms"] is None:
        return DQNTrainer(q, q.get_target_network(), **common).to(device)
    return QRDQNTrainer(q, q.get_target_network(), num_atoms=c["num_atoms"], cpe_optimizer=Optimizer__Union.default(lr=c["lr"]),
                        **common).to(device)


def _batch(arrays, i, device):
    pre = f"b{i}_batch_"
    return {k[len(pre):]: torch.from_numpy(v).to(device) for k, v in arrays.items() if k.startswith(pre)}


def _page(arrays, pre, device):
    from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage

    return EvaluationDataPage(**{k[len(pre):]: torch.from_numpy(v).to(device) for k, v in arrays.items() if k.startswith(pre)})


@pytest.mark.parametrize("name", CASES)
def test_validation_step_pages(backend, name):
    c, arrays = _fixture(name)
    tr = _trainer(c, arrays, backend.device)
    flags = [n.training for n in (tr.q_network, tr.reward_network, tr.q_network_cpe)]
    for i in range(3):
        b = _batch(arrays, i, backend.device)
        page = tr.validation_step(b, i) if i else tr.validation_step(rlt.DiscreteDqnInput.from_dict(b), i)  # a dict or the input
        pre = f"b{i}_page_"
        recorded = {k[len(pre):] for k in arrays if k.startswith(pre)}
        mine = {k for k, v in page.__dict__.items() if v is not None}
        assert mine == recorded, (mine ^ recorded)
        for k in recorded:
            got, want = getattr(page, k), torch.from_numpy(arrays[pre + k])
            assert got.device.type == torch.device(backend.device).type, k  # the page stays on the device
            assert got.shape == want.shape and got.dtype == want.dtype, (k, got.shape, want.shape, got.dtype, want.dtype)
            if k in EXACT:
                assert torch.equal(got.cpu(), want), k
            else:
                assert k in DERIVED, k
                err = (got.cpu() - want).abs().max().item() if want.numel() else 0.0
                print(f"CPEERR {name} b{i} {k} err={err:.3e} tol={FORWARD_TOL:.1e}")
                assert err <= FORWARD_TOL, (k, err)
        # the column slices are views of the forward outputs
        assert page.model_values.data_ptr() == page.model_values._base.data_ptr()
        assert page.model_rewards._base is page.model_metrics._base
    assert flags == [n.training for n in (tr.q_network, tr.reward_network, tr.q_network_cpe)]


@pytest.mark.parametrize("name", CASES)
def test_gathered_page_order_and_values(backend, name):
    c, arrays = _fixture(name)
    tr = _trainer(c, arrays, backend.device)
    gathered = tr.gather_eval_data([_page(arrays, f"b{i}_page_", backend.device) for i in range(3)])
    pre = "page_"
    recorded = {k[len(pre):] for k in arrays if k.startswith(pre)}
    assert {k for k, v in gathered.__dict__.items() if v is not None} == recorded
    for k in recorded:  # every field was gathered from the fixture's own pages: all of them are bit-equal
        got, want = getattr(gathered, k).cpu(), torch.from_numpy(arrays[pre + k])
        assert got.dtype == want.dtype and torch.equal(got, want), k
    key = list(zip(arrays["page_mdp_id"].reshape(-1).tolist(), arrays["page_sequence_number"].reshape(-1).tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)
    # validate: a broken-up MDP and a repeated sequence number are named
    import dataclasses

    broken = dataclasses.replace(gathered, mdp_id=torch.roll(gathered.mdp_id, 1, 0))
    with pytest.raises(AssertionError, match="MDPs are broken up|increasing order"):
        broken.validate()
    same = gathered.sequence_number.clone()
    lengths = sorted_lengths(arrays)
    assert lengths == sorted_lengths(dict(page_mdp_id=gathered.mdp_id.cpu().numpy())) and sorted(lengths) == sorted(c["episode_lengths"])
    first_long = int(np.argmax(np.array(lengths) > 1))
    start = int(np.cumsum([0] + lengths)[first_long])
    same[start + 1] = same[start]
    with pytest.raises(AssertionError, match="increasing order"):
        dataclasses.replace(gathered, sequence_number=same).validate()


def sorted_lengths(arrays):
    mdp = arrays["page_mdp_id"].reshape(-1)
    bounds = [0] + (np.nonzero(mdp[1:] != mdp[:-1])[0] + 1).tolist() + [len(mdp)]
    return [b - a for a, b in zip(bounds[:-1], bounds[1:])]


def _float64(arrays, c, t):
    """float64 rows and per-row error bounds (module docstring) of target t from the fixture's gathered page"""
    A = c["num_actions"]
    f = lambda k: arrays["page_" + k].astype(np.float64)
    if t == 0:
        r, mr, mv = f("logged_rewards")[:, 0], f("model_rewards"), f("model_values")
    else:
        i = t - 1
        r, mr, mv = f("logged_metrics")[:, i], f("model_metrics")[:, i * A:(i + 1) * A], f("model_metrics_values")[:, i * A:(i + 1) * A]
    mrl = f("model_rewards_for_logged_action")[:, 0]  # (set_metric_as_reward leaves the reward's: the reference's quirk)
    p, m, lp = f("model_propensities"), f("action_mask"), f("logged_propensities")[:, 0]
    tp = (p * m).sum(1)
    iw = tp / lp
    dm, sv, ql = (p * mr).sum(1), (p * mv).sum(1), (mv * m).sum(1)
    e_dm, e_sv, e_ql = ((A + 1) * U * np.abs(x).sum(1) for x in (p * mr, p * mv, mv * m))
    e_iw = (A + 3) * U * np.abs(iw)
    ips, dr = iw * r, iw * (r - mrl) + dm
    e_row = (A + 6) * U * (np.abs(iw) * (np.abs(r) + np.abs(mrl)) + np.abs(p * mr).sum(1))
    N = len(r)
    rows = dict(direct_method=(dm, e_dm), inverse_propensity=(ips, e_row), doubly_robust=(dr, e_row))
    out = {k: (x.mean(), e.mean() + (N + 2) * U * np.abs(x).mean(), x) for k, (x, e) in rows.items()}
    g = float(np.float32(c["rl"]["gamma"]))
    sdr, ev, e_sdr, e_ev = [], [], [], []
    b = 0
    for n in sorted_lengths(arrays):
        d = v = ed = evv = 0.0
        for j in range(b + n - 1, b - 1, -1):
            inner = r[j] + g * d - ql[j]
            ed = (e_sv[j] + e_iw[j] * abs(inner) + abs(iw[j]) * (g * ed + e_ql[j] + 3 * U * (abs(r[j]) + g * abs(d) + abs(ql[j])))
                  + 2 * U * (abs(sv[j]) + abs(iw[j] * inner)))
            d = sv[j] + iw[j] * inner
            evv = g * evv + 2 * U * (abs(v) * g + abs(r[j]))
            v = v * g + r[j]
        sdr.append(d), ev.append(v), e_sdr.append(ed), e_ev.append(evv)
        b += n
    sdr, ev = np.array(sdr), np.array(ev)
    out["sequential_doubly_robust"] = (sdr.mean(), float(np.mean(e_sdr)) + 4 * 2.0 ** -53 * np.abs(sdr).mean(), sdr)
    logged = dict(mean=r.mean(), e_mean=(N + 2) * U * np.abs(r).mean(), ev_mean=ev.mean(), e_ev_mean=float(np.mean(e_ev)))
    return out, logged


_DETAILS = {}


def _details(name, backend):
    """Evaluator.evaluate_post_training on the fixture's gathered page, once per (fixture, backend)"""
    key = (name, backend.name)
    if key not in _DETAILS:
        from reagent_amd.evaluation.evaluator import Evaluator

        c, arrays = _fixture(name)
        page = _page(arrays, "page_", backend.device)
        ev = Evaluator([str(i) for i in range(c["num_actions"])], c["rl"]["gamma"], None, list(c["cpe_metrics"]) or None)
        torch.manual_seed(123)
        _DETAILS[key] = ev.evaluate_post_training(page)
    return _DETAILS[key]


@pytest.mark.parametrize("name", CASES)
def test_estimates_against_float64_and_the_reference(backend, name):
    c, arrays = _fixture(name)
    details = _details(name, backend)
    sets = {"reward": details.reward_estimates}
    sets.update(details.metric_estimates)
    assert list(sets) == ["reward"] + list(c["cpe_metrics"])
    saw_zero_normalizer = False
    for t, (target, got_set) in enumerate(sets.items()):
        want, logged = _float64(arrays, c, t)
        assert got_set.weighted_doubly_robust == (0.0, 0.0, 0.0, 0.0) and got_set.magic == (0.0, 0.0, 0.0, 0.0)  # filled
        got_set.check_estimates_exist()
        for est in ESTIMATORS:
            mine, ref = getattr(got_set, est), arrays[f"est_{target}_{est}"]
            raw64, bound, rows = want[est]
            sequential = est == "sequential_doubly_robust"
            score, e_score = (logged["ev_mean"], logged["e_ev_mean"]) if sequential else (logged["mean"], logged["e_mean"])
            print(f"CPEERR {name} {target} {est} raw={mine.raw!r} ref={ref[0]!r} f64={raw64!r} bound={bound:.3e}")
            assert abs(mine.raw - raw64) <= bound and abs(ref[0] - raw64) <= bound
            if score < 1e-6:
                saw_zero_normalizer = True
                assert mine.normalized == 0.0 and mine.normalized_std_error == 0.0
                assert ref[1] == 0.0 and ref[3] == 0.0
                normalizer = 0.0
            else:
                normalizer = 1.0 / score
                n64 = raw64 * normalizer
                n_bound = (bound / abs(raw64) + e_score / abs(score) + 2 * U) * abs(n64) if raw64 != 0 else bound * normalizer
                assert abs(mine.normalized - n64) <= n_bound and abs(ref[1] - n64) <= n_bound
            # standard errors
            S = int(0.25 * len(rows))
            se = math.sqrt(rows.var() / S)
            print(f"CPEERR {name} {target} {est} std={mine.raw_std_error!r} ref={ref[2]!r} want={se!r}")
            assert abs(mine.raw_std_error - se) <= STD_TOL * se and abs(ref[2] - se) <= STD_TOL * se
            if score >= 1e-6:
                if sequential:
                    assert mine.normalized_std_error == pytest.approx(mine.raw_std_error / score, rel=1e-5)
                else:
                    own_normalizer = mine.normalized / mine.raw
                    assert mine.normalized_std_error == pytest.approx(mine.raw_std_error * own_normalizer, rel=1e-12)
                    assert mine.normalized_std_error == pytest.approx(mine.raw_std_error * normalizer, rel=1e-5)
    assert saw_zero_normalizer == (name == "cpe_dqn_metrics_masks")
    # per-action numbers
    A = c["num_actions"]
    names = [str(i) for i in range(A)]
    q = arrays["page_optimal_q_values"].astype(np.float64)
    for k, f64 in (("q_value_means", q.mean(0)), ("q_value_stds", q.std(0, ddof=1))):
        got = np.array([getattr(details, k)[a] for a in names])
        tol = (len(q) + 4) * U * (np.abs(q).mean(0) + np.abs(f64))
        assert (np.abs(got - f64) <= tol).all() and (np.abs(arrays[k] - f64) <= tol).all(), k
    dist = np.array([details.action_distribution[a] for a in names])
    assert np.array_equal(dist, arrays["action_distribution"])


@pytest.mark.parametrize("name", ["cpe_dqn_metrics_masks", "cpe_qrdqn"])
def test_validation_epoch_end_hands_the_reporter_one_cpe_details(backend, name):
    from reagent_amd.evaluation.cpe import CpeDetails

    c, arrays = _fixture(name)
    tr = _trainer(c, arrays, backend.device)
    calls = []

    class _Reporter:
        def log(self, **kw):
            calls.append(kw)

    tr.set_reporter(_Reporter())
    outs = [tr.validation_step(_batch(arrays, i, backend.device), i) for i in range(3)]
    tr.validation_epoch_end(outs)
    assert len(calls) == 1 and list(calls[0]) == ["cpe_details"] and isinstance(calls[0]["cpe_details"], CpeDetails)
    d = calls[0]["cpe_details"]
    assert list(d.metric_estimates) == list(c["cpe_metrics"])
    # the trainer's own page differs from the fixture's by the forward tolerance only: its estimates sit near the reference's
    for est in ESTIMATORS[:3]:
        ref = arrays[f"est_reward_{est}"]
        assert abs(getattr(d.reward_estimates, est).raw - ref[0]) <= 1e-3 * max(1.0, abs(ref[0])), est
    assert d.action_distribution == {str(i): float(v) for i, v in enumerate(arrays["action_distribution"])}
    assert tr.evaluator.metrics_to_score == (list(c["cpe_metrics"]) or None) and tr.evaluator.model is tr
    tr.validation_epoch_end([])  # nothing gathered: nothing logged
    assert len(calls) == 1


def test_named_refusals(backend):
    from reagent_amd.evaluation.doubly_robust_estimator import DoublyRobustEstimator, DoublyRobustHP
    from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage
    from reagent_amd.evaluation.sequential_doubly_robust_estimator import SequentialDoublyRobustEstimator

    c, arrays = _fixture("cpe_dqn_plain")
    dev = backend.device
    tr = _trainer(c, arrays, dev)
    b = _batch(arrays, 0, dev)
    # a trainer built without CPE networks names the reason (the reference dies on None.training)
    plain = _trainer(c, arrays, dev, cpe=False)
    with pytest.raises(RuntimeError, match="without CPE networks.*calc_cpe_in_training"):
        plain.validation_step(b, 0)
    # world > 1
    tr._dp_world = 2
    with pytest.raises(NotImplementedError, match="world > 1"):
        tr.validation_step(b, 0)
    tr._dp_world = 1
    # other input types and trainers
    with pytest.raises(NotImplementedError, match="ParametricDqnInput"):
        EvaluationDataPage.create_from_training_batch(
            rlt.ParametricDqnInput(state=None, next_state=None, reward=None, time_diff=None, step=None, not_terminal=None,
                                   action=None, next_action=None, possible_actions=None, possible_actions_mask=None,
                                   possible_next_actions=None, possible_next_actions_mask=None, extras=None), tr)
    with pytest.raises(NotImplementedError, match="training_input type"):
        EvaluationDataPage.create_from_training_batch(object(), tr)
    from reagent_amd.training import C51Trainer, DiscreteCRRTrainer, ParametricDQNTrainer

    for cls in (C51Trainer, DiscreteCRRTrainer, ParametricDQNTrainer):
        stub = cls.__new__(cls)
        torch.nn.Module.__init__(stub)
        with pytest.raises(NotImplementedError, match=cls.__name__):
            stub.validation_step(b, 0)
    # estimator options that are not served, and the reference's RuntimeError where there is no episode
    page = _page(arrays, "page_", dev)
    for kw in (dict(xgb_params={"a": 1}), dict(bope_mode="x"), dict(bope_num_samples=3)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            DoublyRobustEstimator().estimate(page, DoublyRobustHP(**kw))
    empty = EvaluationDataPage(**{k: (v[:0] if torch.is_tensor(v) else v) for k, v in page.__dict__.items()})
    with pytest.raises(RuntimeError, match="No valid doubly robusts data"):
        SequentialDoublyRobustEstimator(0.9).estimate(empty)
    # the bootstrap fields of DoublyRobustHP are honoured
    torch.manual_seed(3)
    few = DoublyRobustEstimator().estimate(page, DoublyRobustHP(bootstrap_num_samples=7, bootstrap_sample_percent=0.5))
    assert all(math.isfinite(e.raw_std_error) for e in few)
