"""the Python surface is the reference's — constructor parameter NAMES, ORDER and DEFAULT VALUES of every
class on the path equal the reference's own (`inspect.signature`), so a config / call site written for ReAgent binds
the same way here.  The reference's side is recorded in tests/golden/reference_records/reference_signatures.json (read where the reference
tree is present, in a subprocess so that `reagent` is importable through oracle/stubs.py).  Allowed additions: keyword parameters this package adds AFTER the
reference's (listed in EXTRA below, e.g. `device=` of the replay buffers)."""
import json
import os
import subprocess
import sys
import textwrap

from oracle import stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (reference class, this package's class, extra trailing keyword parameters allowed here)
PAIRS = [
    ("reagent.training.dqn_trainer.DQNTrainer", "reagent_amd.training.DQNTrainer", ()),                    # dqn_trainer.py:50-74
    ("reagent.training.qrdqn_trainer.QRDQNTrainer", "reagent_amd.training.QRDQNTrainer", ()),              # qrdqn_trainer.py:28-52
    ("reagent.training.sac_trainer.SACTrainer", "reagent_amd.training.SACTrainer", ()),                    # sac_trainer.py:57-88
    ("reagent.training.td3_trainer.TD3Trainer", "reagent_amd.training.TD3Trainer", ()),
    ("reagent.training.c51_trainer.C51Trainer", "reagent_amd.training.C51Trainer", ()),
    ("reagent.training.discrete_crr_trainer.DiscreteCRRTrainer", "reagent_amd.training.DiscreteCRRTrainer", ()),
    ("reagent.replay_memory.circular_replay_buffer.ReplayBuffer", "reagent_amd.replay_memory.ReplayBuffer", ("device",)),  # :323-332
    ("reagent.replay_memory.prioritized_replay_buffer.PrioritizedReplayBuffer",
     "reagent_amd.replay_memory.PrioritizedReplayBuffer", ("device",)),
    ("reagent.preprocessing.preprocessor.Preprocessor", "reagent_amd.preprocessing.Preprocessor", ()),
    ("reagent.models.dqn.FullyConnectedDQN", "reagent_amd.models.FullyConnectedDQN", ()),
    ("reagent.models.critic.FullyConnectedCritic", "reagent_amd.models.FullyConnectedCritic", ()),
    ("reagent.models.actor.GaussianFullyConnectedActor", "reagent_amd.models.GaussianFullyConnectedActor", ()),
    ("reagent.models.actor.FullyConnectedActor", "reagent_amd.models.FullyConnectedActor", ()),
    ("reagent.models.dueling_q_network.DuelingQNetwork", "reagent_amd.models.DuelingQNetwork", ()),
    ("reagent.models.categorical_dqn.CategoricalDQN", "reagent_amd.models.CategoricalDQN", ()),
    ("reagent.models.fully_connected_network.FullyConnectedNetwork", "reagent_amd.models.fully_connected_network.FullyConnectedNetwork", ()),
    ("reagent.models.fully_connected_network.FloatFeatureFullyConnected",
     "reagent_amd.models.fully_connected_network.FloatFeatureFullyConnected", ()),
    ("reagent.optimizer.soft_update.SoftUpdate", "reagent_amd.optimizer.SoftUpdate", ()),
    ("reagent.gym.preprocessors.trainer_preprocessor.DiscreteDqnInputMaker", "reagent_amd.preprocessing.DiscreteDqnInputMaker", ()),
    ("reagent.gym.preprocessors.trainer_preprocessor.PolicyNetworkInputMaker", "reagent_amd.preprocessing.PolicyNetworkInputMaker", ()),
    ("reagent.gym.datasets.replay_buffer_dataset.ReplayBufferDataset", "reagent_amd.gym.datasets.ReplayBufferDataset", ()),  # :22-48
    ("reagent.gym.datasets.replay_buffer_dataset.OfflineReplayBufferDataset", "reagent_amd.gym.datasets.OfflineReplayBufferDataset", ()),
    ("reagent.gym.types.Transition", "reagent_amd.gym.types.Transition", ()),                             # gym/types.py:19-29
    ("reagent.gym.types.Trajectory", "reagent_amd.gym.types.Trajectory", ()),
]
# methods whose parameter lists are part of the contract as well
METHODS = [
    ("reagent.replay_memory.circular_replay_buffer.ReplayBuffer", "reagent_amd.replay_memory.ReplayBuffer",
     ("add", "sample_transition_batch", "sample_index_batch", "save", "load")),
    ("reagent.training.dqn_trainer.DQNTrainer", "reagent_amd.training.DQNTrainer", ("train_step_gen", "configure_optimizers")),
    ("reagent.training.sac_trainer.SACTrainer", "reagent_amd.training.SACTrainer", ("train_step_gen", "configure_optimizers")),
    ("reagent.training.qrdqn_trainer.QRDQNTrainer", "reagent_amd.training.QRDQNTrainer", ("train_step_gen", "configure_optimizers")),
    ("reagent.preprocessing.preprocessor.Preprocessor", "reagent_amd.preprocessing.Preprocessor", ("forward",)),
    ("reagent.gym.datasets.replay_buffer_dataset.ReplayBufferDataset", "reagent_amd.gym.datasets.ReplayBufferDataset", ("create_for_trainer",)),
    ("reagent.gym.datasets.replay_buffer_dataset.OfflineReplayBufferDataset", "reagent_amd.gym.datasets.OfflineReplayBufferDataset",
     ("create_for_trainer",)),
    ("reagent.gym.preprocessors.trainer_preprocessor.DiscreteDqnInputMaker", "reagent_amd.preprocessing.DiscreteDqnInputMaker",
     ("create_for_env", "__call__")),
    ("reagent.gym.preprocessors.trainer_preprocessor.PolicyNetworkInputMaker", "reagent_amd.preprocessing.PolicyNetworkInputMaker",
     ("create_for_env", "__call__")),
    ("reagent.gym.types.Trajectory", "reagent_amd.gym.types.Trajectory", ("add_transition", "calculate_cumulative_reward", "to_dict")),
]


GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_records", "reference_signatures.json")

# what a signature is reduced to (name, kind, default), the same on both sides
_PARAMS = textwrap.dedent("""
    import dataclasses, importlib, inspect

    def resolve(path):
        mod, name = path.rsplit(".", 1)
        return getattr(importlib.import_module(mod), name)

    def default_of(p):
        d = p.default
        if isinstance(d, dataclasses.Field):            # resolve_defaults' field(default_factory=...): compare the factory
            f = d.default_factory
            return ["factory", getattr(f, "__qualname__", repr(f)).split(".")[-1]]
        if d is inspect.Parameter.empty:
            return ["required"]
        if repr(d) == "<factory>":                      # the __init__ a @dataclass generates for field(default_factory=...)
            return ["factory", "dataclass"]
        if dataclasses.is_dataclass(d) or callable(d):
            return ["object", type(d).__name__ if not callable(d) else getattr(d, "__name__", repr(d))]
        return ["value", repr(d)]

    def params(fn):
        return [[n, p.kind.name, default_of(p)] for n, p in inspect.signature(fn).parameters.items() if n != "self"]

    def surface(paths_methods):
        return {path: {m: params(getattr(resolve(path), m)) for m in methods} for path, methods in paths_methods}
""")


def _wanted(ref):
    """(class path, the methods recorded for it) of one side: `__init__` of every pair plus the METHODS"""
    out = {}
    for r, o, _ in PAIRS:
        out.setdefault(r if ref else o, ["__init__"])
    for r, o, names in METHODS:
        out.setdefault(r if ref else o, ["__init__"]).extend(n for n in names if n not in out[r if ref else o])
    return sorted(out.items())


def _surface(ref):
    """{class path: {method: [[name, kind, default], ...]}} of the reference (through oracle/stubs.py) or of this package,
    in a fresh interpreter so that `reagent` is importable only where it is asked for"""
    pre = "import sys; sys.path.insert(0, %r)\n" % ROOT
    if ref:
        pre += "from oracle import stubs\nstubs.install()\nstubs.install_gym()\n"  # the input makers live under reagent.gym
    code = pre + _PARAMS + "import json\nprint(json.dumps(surface(%r)))\n" % (_wanted(ref),)
    env = {k: v for k, v in os.environ.items() if k != "REAGENT_AMD_OWN_TYPES"} if ref else dict(os.environ)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _same(ref, own):
    # the reference writes mutable defaults as field(default_factory=F) under @resolve_defaults
    # (reagent/core/configuration.py); here such a parameter defaults to None and the constructor calls the same F
    if len(ref) != len(own):
        return False
    for (rn, rk, rd), (on, ok, od) in zip(ref, own):
        if (rn, rk) != (on, ok):
            return False
        # (SACTrainer.alpha_optimizer: None means "fixed temperature" in both, so the stand-in for the factory there
        # is the sentinel "default")
        if rd != od and not (rd[0] == "factory" and od in (["value", "None"], ["value", "'default'"])):
            return False
    return True


def test_constructor_and_method_signatures_equal_the_reference():
    """against the reference's signatures as recorded in tests/golden/reference_records/reference_signatures.json; where the reference tree
    is present the record is checked against it first (RG_WRITE_GOLDEN=1 rewrites it from there)"""
    if os.path.isdir(os.path.join(stubs.REFERENCE_ROOT, "reagent")):
        live = _surface(ref=True)
        if os.environ.get("RG_WRITE_GOLDEN") == "1":
            with open(GOLDEN, "w") as f:
                json.dump(live, f, indent=1, sort_keys=True)
        assert live == json.load(open(GOLDEN)), "tests/golden/reference_records/reference_signatures.json is not what the reference has"
    recorded, here = json.load(open(GOLDEN)), _surface(ref=False)
    bad = []
    for ref_path, own_path, extra in PAIRS:
        ref, own = recorded[ref_path]["__init__"], here[own_path]["__init__"]
        tail = own[len(ref):]
        if not _same(ref, own[:len(ref)]) or [t[0] for t in tail] != list(extra) or any(t[2] == ["required"] for t in tail):
            bad.append((own_path, "reference: %r" % (ref,), "here: %r" % (own,)))
    for ref_path, own_path, names in METHODS:
        for m in names:
            ref, own = recorded[ref_path][m], here[own_path][m]
            if [(n, k) for n, k, _ in own[:len(ref)]] != [(n, k) for n, k, _ in ref] or any(t[2] == ["required"] for t in own[len(ref):]):
                bad.append((own_path + "." + m, "reference: %r" % (ref,), "here: %r" % (own,)))
    assert not bad, "\n".join("MISMATCH " + "\n   ".join(b) for b in bad)
