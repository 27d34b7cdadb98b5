"""LinUCBTrainer and DeepRepresentLinUCBTrainer with an attached PolicyEvaluator on the four fixtures of the unmodified
reference (tests/golden/cb_eval/*.npz, tests/golden_gen/make_cb_eval_golden.py): two epochs of four evaluated steps, step by
step, on the interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24.

Per step.  The frozen model's actions are the reference's exactly (the fixtures keep every row's two best arms either
bit-equal or 1e-3 (1 + max|ucb|) apart, so acceptance does not hinge on rounding); importance_weight is the reference's
bit for bit where no exp is involved and within the exp bound of tests/test_cb_eval_kernels.py (min(3 * 2^-23 relative,
4 spacings)) where it is; effective_weight is the fp32 product weight * importance_weight, bit for bit;
num_eval_model_updates is exact.

Sums.  The nine local buffers are held, ours and the reference's recorded ones alike, to the any-order fp32 bound
(B + 2) u sum|terms| + 2 u |buffer| against a float64 statement of policy_evaluator.py:22-68 that is carried from step to
step (the bounds add up; an aggregation resets both).  Each side's statement takes that side's importance weights (they
differ, by the exp bound, in eval_full only).  The totals and the window's averages of _aggregate_across_instances are
propagated through the statement as (value, bound) pairs -- a sum or difference adds the bounds and one rounding, a
quotient a / b gets |a / b| (bound_a / |a| + bound_b / |b|) (1 + that) + 2 u |a / b| -- and every value the logger
received, ours and the reference's, is held to its pair.

The scorer.  cur_avg_A, cur_avg_b, cur_sum_weight after every step: the carried any-order bounds of
tests/test_linucb_trainer.py on the float64 statement with the effective weights; avg_A, avg_b, sum_weight after an epoch
end: that file's rule; inv_avg_A and _coefs: that file's TOL -- relative to the largest entry, 4 x the reference's own
distance from the float64 inverse of its recorded averages, the worse of the two epochs (computed here from the fixture).  The deep case: the bounds of tests/test_deep_represent_linucb_trainer.py (loss
1e-4 |ref| + 2e-6, parameters 2e-5, the epoch's averages on our own z from the state before the step).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cb_eval")
U = 2.0 ** -24
LINUCB_CASES = ["eval_plain", "eval_full", "eval_presence_ties"]
BATCH_KEYS = ("context_arm_features", "arm_presence", "action", "reward", "weight", "action_log_probability")
MODEL_KEYS = ("output_activation", "l2_reg_lambda", "ucb_alpha", "gamma", "use_batch_norm", "normalize_output",
              "use_layer_norm", "use_skip_connections", "nn_e2e")
LOCAL = ("sum_weight_all_data_local", "sum_reward_weighted_all_data_local", "sum_size_weighted_all_data_local",
         "sum_reward_importance_weighted_accepted_local", "sum_reward_weighted_accepted_local", "sum_weight_accepted_local",
         "sum_importance_weight_accepted_local", "sum_size_weighted_accepted_local", "sum_weight_since_update_local")
PREFIX = "[model]Offline_Eval_"
PARAM_TOL, MARGIN = 2e-5, 4.0


def _load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        g = {k: f[k] for k in f.files}
    return g, json.loads(str(g["config_json"]))


def _batch(g, pre, dev):
    from reagent_amd.core.types import CBInput

    return CBInput.from_dict({k: torch.from_numpy(g[f"{pre}batch_{k}"]).to(dev) for k in BATCH_KEYS if f"{pre}batch_{k}" in g})


class Recorder:
    def __init__(self):
        self.calls = []

    def log_metrics(self, metrics, step=None):
        self.calls.append({"step": step, "metrics": dict(metrics)})


def _make(g, c, dev):
    """-> trainer, scorer, evaluator (attached, on the device), recording logger, optimizer (deep) or None"""
    from reagent_amd.evaluation.cb import PolicyEvaluator
    from reagent_amd.gym.policies import Policy

    if c["deep"]:
        from reagent_amd.models import DeepRepresentLinearRegressionUCB
        from reagent_amd.training import DeepRepresentLinUCBTrainer

        scorer = DeepRepresentLinearRegressionUCB(c["d"], list(c["sizes"]), list(c["activations"]), **{k: c[k] for k in MODEL_KEYS})
        scorer.load_state_dict({k[len("init_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init_")}, strict=True)
        scorer = scorer.to(dev)
        tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=c["lr"], weight_decay=c["weight_decay"],
                                        loss_type=c["loss_type"], eval_model_update_critical_weight=c["critical_weight"])
    else:
        from reagent_amd.models.linear_regression import LinearRegressionUCB
        from reagent_amd.training import LinUCBTrainer

        scorer = LinearRegressionUCB(c["d"], l2_reg_lambda=c["l2_reg_lambda"], ucb_alpha=c["ucb_alpha"], gamma=c["gamma"]).to(dev)
        tr = LinUCBTrainer(Policy(scorer=scorer, sampler=None), eval_model_update_critical_weight=c["critical_weight"])
    rec = Recorder()
    ev = PolicyEvaluator(scorer, logger=rec, max_importance_weight=c["max_importance_weight"]).to(dev)
    tr.attach_eval_module(ev)
    return tr, scorer, ev, rec


def _watch(ev):
    """records what every ingest of `ev` saw and gave: model_actions, importance_weight, effective_weight"""
    seen, real = {}, ev._ingest

    def recording(batch, model_actions, count_since_update):
        out = real(batch, model_actions, count_since_update)
        seen.update(model_actions=model_actions.cpu().clone(), importance_weight=out[0].importance_weight.cpu().clone(),
                    effective_weight=out[1].cpu().clone())
        return out

    ev._ingest = recording
    return seen


# ---- (value, bound) arithmetic of the statement ---------------------------------------------------------------------------
class V:
    def __init__(self, val=0.0, err=0.0):
        self.val, self.err = float(val), float(err)

    def __add__(self, o):
        v = self.val + o.val
        return V(v, self.err + o.err + 2 * U * abs(v))

    def __sub__(self, o):
        v = self.val - o.val
        return V(v, self.err + o.err + 2 * U * abs(v))

    def __truediv__(self, o):
        if o.val == 0 or o.err >= abs(o.val):
            return V(float("nan") if self.val == 0 else math.copysign(float("inf"), self.val), float("inf"))
        q = self.val / o.val
        rel = (self.err / abs(self.val) if self.val != 0 else 0.0) + o.err / abs(o.val)
        extra = self.err / abs(o.val) if self.val == 0 else 0.0
        return V(q, abs(q) * rel * (1 + rel) + extra + 2 * U * abs(q))

    def holds(self, x):
        x = float(x)
        if math.isnan(self.val) or math.isinf(self.err):
            return True if math.isinf(self.err) else math.isnan(x)
        return abs(x - self.val) <= self.err


def _same_kind(x, y):
    """both NaN, both the same infinity, or both finite: what the two sides have to agree on even where a statement's bound
    is infinite (a window's 0 / 0 right after an aggregation, a rejected weight of 0) and `holds` can say nothing"""
    x, y = float(x), float(y)
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) and math.isnan(y)
    if math.isinf(x) or math.isinf(y):
        return x == y
    return True


class EvalStatement:
    """policy_evaluator.py in float64 with bounds: the nine local sums, the five totals, the window's averages"""

    def __init__(self):
        self.local = [V() for _ in LOCAL]
        self.total = dict.fromkeys(("sum_weight_accepted", "sum_importance_weight_accepted", "sum_weight_all_data",
                                    "sum_reward_weighted_accepted", "sum_reward_importance_weighted_accepted"))
        self.total = {k: V() for k in self.total}
        self.window = {k: V() for k in ("frac_accepted", "avg_reward_accepted", "avg_reward_rejected", "avg_size_accepted",
                                        "avg_size_rejected", "accepted_rejected_reward_ratio", "avg_reward_all_data")}
        self.updates = 0

    def step(self, g, pre, iw, arms):
        r = torch.from_numpy(g[pre + "batch_reward"]).double()
        B = r.shape[0]
        w = torch.from_numpy(g[pre + "batch_weight"]).double() if pre + "batch_weight" in g else torch.ones_like(r)
        iw = iw.double().reshape(B, 1)
        acc = (iw > 0).double()
        if pre + "batch_arm_presence" in g:
            sizes = torch.from_numpy(g[pre + "batch_arm_presence"]).sum(1).double()
        else:  # the reference's [B, 1] sizes against the squeezed weights: a [B, B] product
            sizes = torch.ones_like(r) * arms
        eff = (w.float() * iw.float()).double()  # (effective_weight is an fp32 product on both sides)
        terms = [w, w * r, w.squeeze(1) * sizes, eff * r, w * acc * r, w * acc, eff, (w * acc).squeeze(1) * sizes, w]
        for k, t in enumerate(terms):
            v = self.local[k].val + t.sum().item()
            self.local[k] = V(v, self.local[k].err + (B + 2) * U * t.abs().sum().item() + 2 * U * abs(v))

    def update(self):  # base_trainer.py:110-113
        self.local[8] = V()
        self.updates += 1
        self.aggregate()

    def aggregate(self):
        L = dict(zip(LOCAL, self.local))
        acc, iwa, all_ = L["sum_weight_accepted_local"], L["sum_importance_weight_accepted_local"], L["sum_weight_all_data_local"]
        rej = all_ - acc
        r_acc, r_iw, r_all = (L["sum_reward_weighted_accepted_local"], L["sum_reward_importance_weighted_accepted_local"],
                              L["sum_reward_weighted_all_data_local"])
        r_rej = r_all - r_acc
        s_acc, s_all = L["sum_size_weighted_accepted_local"], L["sum_size_weighted_all_data_local"]
        s_rej = s_all - s_acc
        T = self.total
        T["sum_reward_weighted_accepted"] = T["sum_reward_weighted_accepted"] + r_acc
        T["sum_reward_importance_weighted_accepted"] = T["sum_reward_importance_weighted_accepted"] + r_iw
        T["sum_weight_accepted"] = T["sum_weight_accepted"] + acc
        T["sum_importance_weight_accepted"] = T["sum_importance_weight_accepted"] + iwa
        T["sum_weight_all_data"] = T["sum_weight_all_data"] + all_
        W = self.window
        W["frac_accepted"], W["avg_reward_accepted"], W["avg_reward_rejected"] = acc / all_, r_acc / acc, r_rej / rej
        W["avg_reward_all_data"] = r_all / all_
        W["accepted_rejected_reward_ratio"] = W["avg_reward_accepted"] / W["avg_reward_rejected"]
        W["avg_size_accepted"], W["avg_size_rejected"] = s_acc / acc, s_rej / rej
        self.local[:8] = [V() for _ in range(8)]

    def avg_reward(self):
        return self.total["sum_reward_importance_weighted_accepted"] / (self.total["sum_importance_weight_accepted"] + V(1e-9))

    def logged(self):
        d = {"avg_reward": self.avg_reward(), "sum_weight_accepted": self.total["sum_weight_accepted"],
             "sum_weight_all_data": self.total["sum_weight_all_data"], "num_eval_model_updates": V(self.updates)}
        d.update(self.window)
        return {PREFIX + k: v for k, v in d.items()}

    def check_local(self, who, values):
        for name, v, x in zip(LOCAL, self.local, values):
            assert v.holds(x), (who, name, float(x), v.val, v.err)


class ScorerStatement:
    """the epoch's averages in float64 from the chosen rows x [B, d] and the effective weights, with the bound carried along
    (tests/test_linucb_trainer.py's)"""

    def __init__(self, d, sum_weight):
        self.A, self.b, self.sw = torch.zeros(d, d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64), sum_weight
        self.bound_A, self.bound_b, self.bound_sw = torch.zeros_like(self.A), torch.zeros_like(self.b), U * sum_weight

    def step(self, x, y, w):
        B = x.shape[0]
        s_w = w.sum()
        self.sw = self.sw + s_w
        keep = 1.0 - s_w / self.sw
        self.A = self.A * keep + x.t() @ (x * w[:, None]) / self.sw
        self.b = self.b * keep + x.t() @ (w * y) / self.sw
        absA, absb = x.abs().t() @ (x.abs() * w[:, None]), x.abs().t() @ (w * y).abs()
        self.bound_A = self.bound_A * keep + (B + 2) * U * absA / self.sw + 8 * U * self.A.abs()
        self.bound_b = self.bound_b * keep + (B + 2) * U * absb / self.sw + 8 * U * self.b.abs()
        self.bound_sw = self.bound_sw + (B + 2) * U * w.abs().sum() + 8 * U * self.sw

    def check(self, who, A, b, sw):
        for name, got, ref, bound in (("cur_avg_A", A, self.A, self.bound_A), ("cur_avg_b", b, self.b, self.bound_b),
                                      ("cur_sum_weight", sw, torch.as_tensor(self.sw).reshape(1), torch.as_tensor(self.bound_sw).reshape(1))):
            err = (torch.as_tensor(got).double().cpu() - ref).abs()
            assert (err <= bound).all(), (who, name, (err / bound.clamp_min(1e-300)).max().item())


def _t64(a):
    return torch.from_numpy(np.asarray(a)).double()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _reference_inverse_error(g, c):
    """tests/test_linucb_trainer.py's measure: the reference's recorded inv_avg_A and _coefs against the float64 inverse of
    the float64 A_extended of its recorded averages, max-abs over the largest entry, the worse of the epochs"""
    worst = {"inv_avg_A": 0.0, "_coefs": 0.0}
    for e in range(c["epochs"]):
        A, b = _t64(g[f"e{e}_end_avg_A"]), _t64(g[f"e{e}_end_avg_b"])
        sw = _t64(g[f"e{e}_end_sum_weight"]) / c["gamma"]  # (recorded after the discount; the matrix inverted saw it before)
        inv = torch.linalg.inv(A + c["l2_reg_lambda"] * torch.eye(c["d"], dtype=torch.float64) / sw)
        worst["inv_avg_A"] = max(worst["inv_avg_A"], _rel(g[f"e{e}_end_inv_avg_A"], inv))
        worst["_coefs"] = max(worst["_coefs"], _rel(g[f"e{e}_end__coefs"], inv @ b))
    return worst


def _chosen(g, pre):
    x3, action = _t64(g[pre + "batch_context_arm_features"]), torch.from_numpy(g[pre + "batch_action"])
    B, _, d = x3.shape
    return torch.gather(x3, 1, action.view(B, 1, 1).expand(-1, 1, d)).squeeze(1), _t64(g[pre + "batch_reward"]).reshape(B)


def _spacing(x):
    x = x.abs().float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _check_step_rows(g, pre, c, seen, who):
    """the frozen model's actions, acceptance, importance and effective weights of one step against the reference's"""
    ref_iw = torch.from_numpy(g[pre + "importance_weight"])
    iw = seen["importance_weight"]
    assert torch.equal(seen["model_actions"], torch.from_numpy(g[pre + "model_actions"])), who
    assert iw.shape == ref_iw.shape and iw.dtype == ref_iw.dtype
    assert torch.equal(iw > 0, ref_iw > 0), who
    if c["logp"]:
        err = (iw.double() - ref_iw.double()).abs()
        bound = torch.minimum(3 * 2.0 ** -23 * ref_iw.double().abs(), 4 * _spacing(ref_iw))
        print(who, "importance_weight: worst error / bound", (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= bound).all(), who
        clip = c["max_importance_weight"]
        assert torch.equal(iw == clip, ref_iw == clip) and (iw == clip).any() and ((iw > 0) & (iw < clip)).any(), who
    else:
        assert torch.equal(iw, ref_iw), who
    w = torch.from_numpy(g[pre + "batch_weight"]) if pre + "batch_weight" in g else torch.ones_like(iw)
    assert torch.equal(seen["effective_weight"], w * iw), who
    return iw, ref_iw


def _check_logs(ours, ref, want_ours, want_ref, who):
    """every call the two loggers received, in order: the same step, the same eleven keys in the same order, every value
    within its side's statement"""
    assert len(ours) == len(ref) == len(want_ours) == len(want_ref), (who, len(ours), len(ref), len(want_ours))
    for i, (a, b, sa, sb) in enumerate(zip(ours, ref, want_ours, want_ref)):
        assert a["step"] == b["step"], (who, i)
        assert list(a["metrics"]) == list(b["metrics"]) == list(sa) and len(sa) == 11, (who, i)
        for side, m, st in (("ours", a["metrics"], sa), ("reference", b["metrics"], sb)):
            for k, v in st.items():
                assert v.holds(m[k]), (who, i, side, k, m[k], v.val, v.err)
        for k in sa:
            assert _same_kind(a["metrics"][k], b["metrics"][k]), (who, i, k, a["metrics"][k], b["metrics"][k])
        assert a["metrics"][PREFIX + "num_eval_model_updates"] == b["metrics"][PREFIX + "num_eval_model_updates"]


def _replay_linucb(name, dev):
    g, c = _load(name)
    tr, scorer, ev, rec = _make(g, c, dev)
    seen = _watch(ev)
    ref_logs = json.loads(str(g["log_json"]))
    st_ours, st_ref, want_logs, want_ref_logs = EvalStatement(), EvalStatement(), [], []
    carried, i, updates = {}, 0, 0
    ref_inverse_error = _reference_inverse_error(g, c)
    for e in range(c["epochs"]):
        sc_ours = ScorerStatement(c["d"], float(np.float32(1e-5)) if e == 0 else 0.0)
        sc_ref = ScorerStatement(c["d"], float(np.float32(1e-5)) if e == 0 else 0.0)
        for s in range(c["steps"]):
            pre, who = f"e{e}_s{s}_", (name, e, s)
            tr.global_step = i
            assert tr.training_step(_batch(g, pre, dev), i) is None
            n_ref = int(g[pre + "ev_num_eval_model_updates"][0])
            assert int(ev.num_eval_model_updates.item()) == n_ref, who
            if n_ref > updates:  # the frozen model was replaced before this step: an aggregation and a log
                assert n_ref == updates + 1
                updates = n_ref
                for st in (st_ours, st_ref):
                    st.update()
                assert len(rec.calls) == len(want_logs) + 1, who
                want_logs.append(st_ours.logged())
                want_ref_logs.append(st_ref.logged())  # (the reference's numbers against the statement of ITS weights)
            iw, ref_iw = _check_step_rows(g, pre, c, seen, who)
            st_ours.step(g, pre, iw, c["arms"])
            st_ref.step(g, pre, ref_iw, c["arms"])
            st_ours.check_local(who + ("ours",), [getattr(ev, n).item() for n in LOCAL])
            st_ref.check_local(who + ("reference",), [g[f"{pre}ev_{n}"][0] for n in LOCAL])
            x, y = _chosen(g, pre)
            w = torch.from_numpy(g[pre + "batch_weight"]) if pre + "batch_weight" in g else torch.ones_like(iw)
            sc_ours.step(x, y, (w * iw).double().reshape(-1))
            sc_ref.step(x, y, (w * ref_iw).double().reshape(-1))
            sc_ours.check(who + ("ours",), scorer.cur_avg_A, scorer.cur_avg_b, scorer.cur_sum_weight)
            sc_ref.check(who + ("reference",), g[pre + "cur_avg_A"], g[pre + "cur_avg_b"], g[pre + "cur_sum_weight"])
            assert scorer.cur_num_obs.item() == g[pre + "cur_num_obs"].item()
            i += 1
        tr.global_step = i
        tr.on_train_epoch_end()
        for st in (st_ours, st_ref):
            st.aggregate()
        want_logs.append(st_ours.logged())
        want_ref_logs.append(st_ref.logged())
        # every buffer of the evaluator after the epoch end, ours and the reference's, against the statement
        for side, st, get in (("ours", st_ours, lambda k: getattr(ev, k).item()), ("reference", st_ref, lambda k: g[f"e{e}_end_ev_{k}"][0])):
            pairs = dict(st.total, **st.window, **dict(zip(LOCAL, st.local)))
            for k, v in pairs.items():
                assert v.holds(get(k)), (name, e, side, k, get(k), v.val, v.err)
            assert get("num_eval_model_updates") == updates
        for k in list(st_ours.total) + list(st_ours.window):
            assert _same_kind(getattr(ev, k).item(), g[f"e{e}_end_ev_{k}"][0]), (name, e, k)
        assert all(getattr(ev, n).item() == 0 for n in LOCAL[:8])
        assert st_ours.avg_reward().holds(ev.get_avg_reward()) and st_ref.avg_reward().holds(g[f"e{e}_end_avg_reward"][0])
        print(name, e, "avg_reward", ev.get_avg_reward(), "reference", g[f"e{e}_end_avg_reward"][0])
        # the scorer after the epoch end: tests/test_linucb_trainer.py's rule
        ref = lambda k: torch.from_numpy(g[f"e{e}_end_{k}"])  # noqa: E731
        for k, bo, br in (("avg_A", sc_ours.bound_A, sc_ref.bound_A), ("avg_b", sc_ours.bound_b, sc_ref.bound_b)):
            got, want = getattr(scorer, k).cpu().double(), ref(k).double()
            # each side within its own statement's bound; the two statements differ where the two sides' importance weights
            # do (eval_full: the exp bound) by an amount that is computed, not estimated -- twice it, for the second-order
            # difference of the weights of the mean the epoch's average enters; zero in the other cases
            apart = 2 * ((sc_ours.A - sc_ref.A).abs() if k == "avg_A" else (sc_ours.b - sc_ref.b).abs())
            assert c["logp"] or not apart.any()
            carried[k] = carried.get(k, 0.0) + bo + br + apart + 8 * U * want.abs()
            assert ((got - want).abs() <= carried[k]).all(), (e, k)
        carried["sw"] = carried.get("sw", 0.0) + float(sc_ours.bound_sw) + float(sc_ref.bound_sw) + 8 * U * abs(ref("sum_weight").item())
        carried["sw"] += 2 * abs(float(sc_ours.sw) - float(sc_ref.sw))
        assert abs(scorer.sum_weight.item() - ref("sum_weight").item()) <= carried["sw"]
        assert scorer.num_obs.item() == ref("num_obs").item()
        for k in ("inv_avg_A", "_coefs"):
            m = ref_inverse_error[k]
            r = _rel(getattr(scorer, k), ref(k))
            print(name, e, k, f"{r:.3e} of {MARGIN * m:.3e}")
            assert r <= MARGIN * m, (e, k, r, m)
    _check_logs(rec.calls, ref_logs[:int(g["n_log_calls_before_x"][0])], want_logs, want_ref_logs, name)
    return tr, scorer, ev


@pytest.mark.parametrize("name", LINUCB_CASES)
def test_linucb_fixture_step_by_step(backend, name):
    _replay_linucb(name, backend.device)


def test_the_planted_ties_go_to_the_lower_index(backend):
    """eval_presence_ties, step e1_s1: rows 0 and 1 have the same features in arms 1 and 3, the frozen model's two best; it
    picks arm 1 in both, so row 0 (logged arm 1) is accepted and row 1 (logged arm 3) rejected -- here as in the reference"""
    g, c = _load("eval_presence_ties")
    ucb, actions, iw = g["e1_s1_ucb"], g["e1_s1_model_actions"], g["e1_s1_importance_weight"]
    present = g["e1_s1_batch_arm_presence"]
    assert (ucb[:2, 1] == ucb[:2, 3]).all() and (ucb[:2, 1] >= np.where(present, ucb, -np.inf)[:2].max(1)).all()
    assert actions[:2, 0].tolist() == [1, 1] and g["e1_s1_batch_action"][:2, 0].tolist() == [1, 3]
    assert iw[0, 0] > 0 and iw[1, 0] == 0
    tr, scorer, ev, rec = _make(g, c, backend.device)
    seen = _watch(ev)
    for i, pre in enumerate(["e0_s0_", "e0_s1_", "e0_s2_", "e0_s3_", None, "e1_s0_", "e1_s1_"]):
        if pre is None:
            tr.on_train_epoch_end()
        else:
            tr.training_step(_batch(g, pre, backend.device), i)
    out = ev.eval_model.forward_with_actions(torch.from_numpy(g["e1_s1_batch_context_arm_features"]).to(backend.device),
                                             arm_presence=torch.from_numpy(g["e1_s1_batch_arm_presence"]).to(backend.device))
    assert torch.equal(out["ucb"][:2, 1], out["ucb"][:2, 3])  # exact here too
    assert seen["model_actions"][:2, 0].tolist() == [1, 1]
    assert seen["importance_weight"][0, 0].item() == iw[0, 0] and seen["importance_weight"][1, 0].item() == 0.0


def test_the_size_quirk_shows_in_the_logged_metrics(backend):
    """eval_plain has no arm_presence: the reference logs avg_size_accepted = B * A = 148, and so does this package;
    eval_presence_ties has one: a size between 1 and A"""
    g, c = _load("eval_plain")
    last = json.loads(str(g["log_json"]))[int(g["n_log_calls_before_x"][0]) - 1]["metrics"]
    assert last[PREFIX + "avg_size_accepted"] == c["batch"] * c["arms"] == 148
    tr, scorer, ev = _replay_linucb("eval_plain", backend.device)
    assert ev.avg_size_accepted.item() == 148 and ev.avg_size_rejected.item() == 148
    g, c = _load("eval_presence_ties")
    last = json.loads(str(g["log_json"]))[int(g["n_log_calls_before_x"][0]) - 1]["metrics"]
    assert 1 <= last[PREFIX + "avg_size_accepted"] <= c["arms"]


def _replay_deep(native, dev, check):
    name = "eval_deep"
    g, c = _load(name)
    tr, scorer, ev, rec = _make(g, c, dev)
    seen = _watch(ev)
    opt = tr.native_optimizers()[0] if native else tr.configure_optimizers()
    ref_logs = json.loads(str(g["log_json"]))
    st, want_logs = EvalStatement(), []
    d = c["sizes"][-1] + 1
    trace, i, updates = [], 0, 0
    for e in range(c["epochs"]):
        scorer.train()
        for s in range(c["steps"]):
            pre, who = f"e{e}_s{s}_", (name, e, s)
            batch = _batch(g, pre, dev)
            before = {k: getattr(scorer, k).detach().cpu().clone() for k in ("cur_avg_A", "cur_avg_b", "cur_sum_weight")}
            solved = scorer._coefs_dirty
            tr.global_step = i
            if native:
                loss = tr.train_step_native(batch)
            else:
                opt.zero_grad()
                loss = tr.training_step(batch, i)
                loss.backward()
                opt.step()
            sd = {k: v.detach().cpu().clone() for k, v in scorer.state_dict().items()}
            evsd = {k: v.detach().cpu().clone() for k, v in ev.state_dict().items()}
            trace.append((loss.detach().cpu().clone().reshape(1), sd, evsd, {k: v.clone() for k, v in seen.items()}))
            i += 1
            if not check:
                continue
            n_ref = int(g[pre + "ev_num_eval_model_updates"][0])
            assert int(ev.num_eval_model_updates.item()) == n_ref, who
            if n_ref > updates:
                updates = n_ref
                st.update()
                want_logs.append(st.logged())
            iw, _ = _check_step_rows(g, pre, c, seen, who)
            st.step(g, pre, iw, c["arms"])  # (no exp in this case: one statement serves both sides)
            st.check_local(who + ("ours",), [getattr(ev, n).item() for n in LOCAL])
            st.check_local(who + ("reference",), [g[f"{pre}ev_{n}"][0] for n in LOCAL])
            ref_loss = float(g[pre + "loss"][0])
            print(name, e, s, f"loss {float(loss.detach()):.7f} reference {ref_loss:.7f}")
            assert abs(float(loss.detach()) - ref_loss) <= 1e-4 * abs(ref_loss) + 2e-6, who
            for k, v in sd.items():
                ref = torch.from_numpy(g[f"{pre}sd_{k}"])
                assert v.shape == ref.shape and v.dtype == ref.dtype, (who, k)
                if "deep_represent_layers" in k or k == "linear_layer.weight":
                    assert (v.double() - ref.double()).abs().max().item() <= PARAM_TOL, (who, k)
            assert sd["cur_num_obs"].item() == g[pre + "cur_num_obs"].item() and sd["num_obs"].item() == g[pre + "sd_num_obs"].item()
            # the epoch's averages from the state before the step and OUR z (tests/test_deep_represent_linucb_trainer.py)
            z64, y = tr._bufs["z"].cpu().double(), _t64(g[pre + "batch_reward"]).reshape(-1)
            B = len(y)
            w = seen["effective_weight"].double().reshape(B)
            cw0 = 0.0 if solved else before["cur_sum_weight"].double().item()
            cA0 = torch.zeros(d, d, dtype=torch.float64) if solved else before["cur_avg_A"].double()
            cb0 = torch.zeros(d, dtype=torch.float64) if solved else before["cur_avg_b"].double()
            cw1 = cw0 + w.sum()
            keep = 1.0 - w.sum() / cw1
            for k, want, asum in (("cur_avg_A", cA0 * keep + z64.t() @ (z64 * w[:, None]) / cw1, z64.abs().t() @ (z64.abs() * w[:, None])),
                                  ("cur_avg_b", cb0 * keep + z64.t() @ (w * y) / cw1, z64.abs().t() @ (w * y).abs())):
                assert ((sd[k].double() - want).abs() <= (B + 2) * U * asum / cw1 + 8 * U * want.abs()).all(), (who, k)
            assert abs(sd["cur_sum_weight"].item() - cw1.item()) <= (B + 2) * U * w.sum().item() + 8 * U * cw1.item(), who
            assert abs(sd["cur_sum_weight"].item() - g[pre + "cur_sum_weight"][0]) <= 2 * ((B + 2) * U * w.sum().item() + 8 * U * cw1.item())
        tr.global_step = i
        tr.on_train_epoch_end()
        trace.append(({k: v.detach().cpu().clone() for k, v in scorer.state_dict().items()},
                      {k: v.detach().cpu().clone() for k, v in ev.state_dict().items()}))
        if not check:
            continue
        st.aggregate()
        want_logs.append(st.logged())
        for side, get in (("ours", lambda k: getattr(ev, k).item()), ("reference", lambda k: g[f"e{e}_end_ev_{k}"][0])):
            for k, v in dict(st.total, **st.window, **dict(zip(LOCAL, st.local))).items():
                assert v.holds(get(k)), (name, e, side, k, get(k), v.val, v.err)
        for k in list(st.total) + list(st.window):
            assert _same_kind(getattr(ev, k).item(), g[f"e{e}_end_ev_{k}"][0]), (name, e, k)
        assert st.avg_reward().holds(ev.get_avg_reward()) and st.avg_reward().holds(g[f"e{e}_end_avg_reward"][0])
        for k in ("avg_A", "avg_b", "sum_weight"):
            assert _rel(getattr(scorer, k), g[f"e{e}_end_{k}"]) <= PARAM_TOL, (e, k)
        assert scorer.num_obs.item() == g[f"e{e}_end_num_obs"].item()
    if check:
        _check_logs(rec.calls, ref_logs[:int(g["n_log_calls_before_x"][0])], want_logs, want_logs, name)
    return trace


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a.is_floating_point():  # (a window right after an aggregation is 0 / 0 on both paths: a NaN is equal to a NaN here)
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
    return torch.equal(a, b)


def test_deep_fixture_step_by_step_and_the_two_paths_agree(backend):
    """eval_deep through training_step + backward + step, checked against the reference, and through train_step_native:
    losses, the scorer's and the evaluator's whole state_dict (the frozen model's included), actions and weights of every
    step are the same bits"""
    lightning = _replay_deep(False, backend.device, check=True)
    native = _replay_deep(True, backend.device, check=False)
    assert _same(lightning, native)


def _recorded_state(g, c, tr, ev):
    """the reference's recorded state after the last epoch under the keys of ev.state_dict() and of tr.state_dict()"""
    last = c["epochs"] - 1
    ev_sd = {k[len("final_ev_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("final_ev_")}
    scorer_sd = {k[len(f"e{last}_end_"):]: torch.from_numpy(v) for k, v in g.items()
                 if k.startswith(f"e{last}_end_") and not k.startswith(f"e{last}_end_ev_") and k != f"e{last}_end_avg_reward"}
    tr_sd = {k: v.clone() for k, v in tr.state_dict().items()}
    assert {k for k in tr_sd if k.startswith("eval_module.")} == {"eval_module." + k for k in ev_sd}
    assert {k for k in tr_sd if k.startswith("scorer.")} == {"scorer." + k for k in scorer_sd}
    tr_sd.update({"eval_module." + k: v for k, v in ev_sd.items()})
    tr_sd.update({"scorer." + k: v for k, v in scorer_sd.items()})
    return ev_sd, scorer_sd, tr_sd


@pytest.mark.parametrize("through", ["evaluator", "trainer"])
@pytest.mark.parametrize("name", LINUCB_CASES + ["eval_deep"])
def test_state_dict_round_trips_and_the_next_step_matches(backend, name, through):
    """keys, shapes and dtypes of the evaluator's state_dict are the signature record's; the state the reference's
    evaluator and scorer had after the last epoch loads strictly -- through the evaluator's and the scorer's own
    load_state_dict, or through the TRAINER's, which holds both as submodules (a checkpoint restore: a nested load, which
    calls no load_state_dict override) -- and the next step from it matches the one the reference took: the frozen model is
    replaced where the reference replaced it, which needs sum_weight_since_update_local as LOADED, not the host mirror of
    the fresh evaluator"""
    dev = backend.device
    g, c = _load(name)
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_records", "cb_eval_signatures.json")))
    rec = rec["reagent.evaluation.cb.policy_evaluator.PolicyEvaluator"]["state_dict"]
    tr, scorer, ev, _ = _make(g, c, dev)
    own = {k: v for k, v in ev.state_dict().items() if not k.startswith("eval_model.")}
    assert set(own) == set(rec)
    for k, (shape, dtype, first) in rec.items():
        assert list(own[k].shape) == shape and str(own[k].dtype) == dtype and float(own[k].reshape(-1)[0]) == first, k
    sd, scorer_sd, tr_sd = _recorded_state(g, c, tr, ev)
    assert set(sd) == set(ev.state_dict())
    assert all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in ev.state_dict().items())
    assert ev._since_update_mirror == 0.0
    ev.eval_model.mark_dirty()
    scorer.mark_dirty()
    if through == "trainer":
        tr.load_state_dict(tr_sd, strict=True)
    else:
        ev.load_state_dict(sd, strict=True)
        scorer.load_state_dict(scorer_sd, strict=True)
    # what the host holds beside the buffers follows the load: the mirror is forgotten, the scorers' flags re-derived
    assert ev._since_update_mirror is None and not ev.eval_model._coefs_dirty and not scorer._coefs_dirty
    since0 = float(g["final_ev_sum_weight_since_update_local"][0])
    assert ev.weight_since_update() == since0 > 0
    for k, v in ev.state_dict().items():  # and back: what this package saves is what the reference saved
        assert torch.equal(v.cpu(), sd[k]), k
    seen = _watch(ev)
    n0 = int(ev.num_eval_model_updates.item())
    updated = int(g["x_ev_num_eval_model_updates"][0]) > n0
    if c["critical_weight"] is not None and name != "eval_full":  # (eval_full's next step falls between two replacements)
        assert updated and since0 >= c["critical_weight"]
    tr.global_step = c["epochs"] * c["steps"]
    if c["deep"]:
        scorer.train()
        tr.train_step_native(_batch(g, "x_", dev))
    else:
        tr.training_step(_batch(g, "x_", dev), tr.global_step)
    iw, ref_iw = _check_step_rows(g, "x_", c, seen, (name, "x"))
    assert int(ev.num_eval_model_updates.item()) == int(g["x_ev_num_eval_model_updates"][0])
    st_ours, st_ref = EvalStatement(), EvalStatement()
    for st, w in ((st_ours, iw), (st_ref, ref_iw)):
        st.local[8] = V(0.0 if updated else since0, 0.0)
        st.step(g, "x_", w, c["arms"])
    st_ours.check_local((name, "x", "ours"), [getattr(ev, n).item() for n in LOCAL])
    st_ref.check_local((name, "x", "reference"), [g[f"x_ev_{n}"][0] for n in LOCAL])
    assert scorer.cur_num_obs.item() == g["x_cur_num_obs"].item()
    if c["deep"]:
        ref_loss = float(g["x_loss"][0])
        assert abs(tr._bufs["loss"].item() - ref_loss) <= 1e-4 * abs(ref_loss) + 2e-6
        return
    x, y = _chosen(g, "x_")
    w = torch.from_numpy(g["x_batch_weight"]) if "x_batch_weight" in g else torch.ones_like(iw)
    for side, weights, got in (("ours", iw, [getattr(scorer, k) for k in ("cur_avg_A", "cur_avg_b", "cur_sum_weight")]),
                               ("reference", ref_iw, [g["x_cur_avg_A"], g["x_cur_avg_b"], g["x_cur_sum_weight"]])):
        sc = ScorerStatement(c["d"], 0.0)
        sc.step(x, y, (w * weights).double().reshape(-1))
        sc.check((name, "x", side), *got)
