"""Drop-in detail of SURVEY §8 a8: inside a ReAgent installation the trainers must be annotated with the
reference's OWN batch classes, because `make_trainer_preprocessor` looks the input maker up by class object
(reagent/gym/preprocessors/trainer_preprocessor.py:39-48).  Runs in a subprocess so that `reagent` is importable BEFORE
reagent_amd is imported: the reference tree through oracle/stubs.py where it is present, elsewhere a stand-in `reagent`
package whose `reagent.core.types` holds classes of its own (this package's restatements, loaded as a separate module)."""
import os
import subprocess
import sys
import textwrap

from oracle import stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


STAND_IN = textwrap.dedent("""
    # stand-in for the reference's reagent.core.types: this package's restatements executed as a module of their own, so
    # that its classes are distinct objects from the ones reagent_amd defines
    import importlib.util, os
    _keep = os.environ.get("REAGENT_AMD_OWN_TYPES")
    os.environ["REAGENT_AMD_OWN_TYPES"] = "1"
    try:
        _spec = importlib.util.spec_from_file_location("reagent.core._restated", %r)
        _m = importlib.util.module_from_spec(_spec)
        _spec.loader.exec_module(_m)
    finally:
        os.environ.pop("REAGENT_AMD_OWN_TYPES")
        if _keep is not None:
            os.environ["REAGENT_AMD_OWN_TYPES"] = _keep
    globals().update({k: v for k, v in vars(_m).items() if not k.startswith("__")})
""") % os.path.join(ROOT, "reagent_amd", "core", "types.py")


def test_reference_batch_classes_are_used_when_reagent_is_importable(tmp_path):
    if os.path.isdir(os.path.join(stubs.REFERENCE_ROOT, "reagent")):
        setup = "from oracle import stubs\nstubs.install()\n"  # the reference on sys.path with fakes for uninstalled deps
    else:
        core = tmp_path / "reagent" / "core"
        core.mkdir(parents=True)
        (tmp_path / "reagent" / "__init__.py").write_text("")
        (core / "__init__.py").write_text("")
        (core / "types.py").write_text(STAND_IN)
        setup = "sys.path.insert(0, %r)\n" % str(tmp_path)
    code = textwrap.dedent("""
        import inspect, sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
    """) % (ROOT, os.path.join(ROOT, "tests")) + setup + textwrap.dedent("""
        import reagent.core.types as ref
        assert ref.DiscreteDqnInput.__module__ != "reagent_amd.core.types"
        import reagent_amd.core.types as rlt
        assert rlt.USING_REFERENCE_TYPES and rlt.DiscreteDqnInput is ref.DiscreteDqnInput
        assert rlt.PolicyNetworkInput is ref.PolicyNetworkInput and rlt.FeatureData is ref.FeatureData
        from reagent_amd.training import DQNTrainer, SACTrainer
        ann = inspect.signature(DQNTrainer.train_step_gen).parameters["training_batch"].annotation
        assert ann is ref.DiscreteDqnInput, ann     # what make_trainer_preprocessor keys its maker map with
        ann = inspect.signature(SACTrainer.train_step_gen).parameters["training_batch"].annotation
        assert ann is ref.PolicyNetworkInput, ann
        # and a native step runs on a batch of the reference's class (SIMT interpreter backend)
        sys.path.insert(0, %r)
        import emu_backend, torch
        class MP:
            def setattr(self, obj, name, value, raising=True): setattr(obj, name, value)
        emu_backend.install(MP())
        from reagent_amd import synthetic
        from reagent_amd.core.parameters import EvaluationParameters, RLParameters
        from reagent_amd.models import FullyConnectedDQN
        from reagent_amd.optimizer import Optimizer__Union
        q = FullyConnectedDQN(12, 4, [32, 16], ["relu", "relu"])
        tr = DQNTrainer(q, q.get_target_network(), None, actions=list("abcd"), rl=RLParameters(gamma=0.9),
                        optimizer=Optimizer__Union.default(lr=0.01),
                        evaluation=EvaluationParameters(calc_cpe_in_training=False))
        batch = synthetic.to_dqn_input(synthetic.dqn_batch(32, 12, 4, seed=1), "cpu")
        assert type(batch) is ref.DiscreteDqnInput
        loss = tr.train_step_native(batch)
        assert torch.isfinite(loss).all()
        print("ok")
    """) % (os.path.join(ROOT, "tests"),)
    env = {k: v for k, v in os.environ.items() if k != "REAGENT_AMD_OWN_TYPES"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-1500:] + out.stderr[-3000:]


def test_own_types_by_default_outside_a_reagent_installation():
    import reagent_amd.core.types as rlt

    assert rlt.DiscreteDqnInput.__module__ in ("reagent_amd.core.types", "reagent.core.types")
