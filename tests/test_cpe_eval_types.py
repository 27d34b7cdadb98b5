"""The public surface of counterfactual policy evaluation (reagent_amd.evaluation: evaluation_data_page, cpe,
doubly_robust_estimator, sequential_doubly_robust_estimator, evaluator; the DQN trainers' validation methods) against the
record of the unmodified reference (tests/golden/reference_records/cpe_eval_signatures.json, written by
tests/golden_gen/make_cpe_eval_golden.py): module paths, names, signatures and field order, so a caller switches by import."""
import dataclasses
import importlib
import inspect
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "reference_records", "cpe_eval_signatures.json")


def _params(fn):
    out = []
    for n, p in inspect.signature(fn).parameters.items():
        if n == "self":
            continue
        default = ["required"] if p.default is inspect.Parameter.empty else ["value", repr(p.default)]
        out.append([n, p.kind.name, default])
    return out


def _own(path):
    """the reference's dotted path -> this package's object at the same path under reagent_amd"""
    mod, name = ("reagent_amd" + path[len("reagent"):]).rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


def test_signatures_and_field_order_are_the_references():
    rec = json.load(open(RECORD))
    fields = rec.pop("fields")
    checked = 0
    for path, methods in rec.items():
        obj = _own(path)
        for method, want in methods.items():
            got = _params(obj if method == "__call__" else getattr(obj, method))
            # a trailing parameter with a default may be added (bootstrapped_std_error_of_mean's `seed`), nothing else moves
            assert got[:len(want)] == want and all(p[2] != ["required"] for p in got[len(want):]), (path, method, got, want)
            checked += 1
    assert checked >= 30
    from reagent_amd.evaluation.cpe import bootstrapped_std_error_of_mean, CpeEstimate, CpeEstimateSet
    from reagent_amd.evaluation.doubly_robust_estimator import DoublyRobustHP
    from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage

    assert [f.name for f in dataclasses.fields(EvaluationDataPage)] == fields["EvaluationDataPage"]
    assert len(fields["EvaluationDataPage"]) == 21
    assert list(CpeEstimate._fields) == fields["CpeEstimate"] and list(CpeEstimateSet._fields) == fields["CpeEstimateSet"]
    assert list(DoublyRobustHP._fields) == fields["DoublyRobustHP"]
    assert {k: repr(v) for k, v in DoublyRobustHP._field_defaults.items()} == fields["DoublyRobustHP_defaults"]
    assert [p[0] for p in _params(bootstrapped_std_error_of_mean)] == ["data", "sample_percent", "num_samples", "seed"]
    from reagent_amd.core import types as rlt

    assert issubclass(EvaluationDataPage, rlt.TensorDataClass)


def test_abi_21_is_bound():
    import reagent_amd._lib as L

    assert L.ABI_VERSION >= 21
    for name in ("rg_cpe_page_rows", "rg_cpe_episode_values", "rg_cpe_dr_partials", "rg_cpe_dr_rows", "rg_cpe_sdr",
                 "rg_cpe_bootstrap"):
        assert name in L.SIGNATURES, name


def test_estimate_set_helpers():
    from reagent_amd.evaluation.cpe import CpeDetails, CpeEstimate, CpeEstimateSet

    s = CpeEstimateSet(direct_method=CpeEstimate(1.0, 2.0, 3.0, 4.0))
    filled = s.fill_empty_with_zero()
    assert filled.direct_method == (1.0, 2.0, 3.0, 4.0) and filled.magic == (0.0, 0.0, 0.0, 0.0) and filled.switch_dr is not None
    try:
        s.check_estimates_exist()
        raise RuntimeError("an empty estimate passed check_estimates_exist")
    except AssertionError:
        pass
    filled.check_estimates_exist()
    filled.log()
    d = CpeDetails()
    assert d.metric_estimates == {} and d.q_value_means is None and d.action_distribution is None
    d.reward_estimates = filled
    d.log()
