"""TEST INFRASTRUCTURE.  Generates tests/golden/pdqn/pdqn_*.npz by running the UNMODIFIED reference ParametricDQNTrainer
(through oracle/reference_harness.py: its stubs, its Lightning-1.6 loop emulation) on seeded synthetic batches.  Run where
the reference tree is present:   python tests/golden_gen/make_parametric_golden.py
Layout (golden_util.Golden): config_json, init_q_<i> / init_reward_<i>, per step the batch, td_loss / reward_loss, every
parameter of the q network, its target and the reward network, and the tensors handed to the reporter.

`generate(name)` returns the arrays without writing them (tests/test_pdqn_trainer.py regenerates each fixture in memory
and compares it with the committed file).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
# a directory of their own: `python -m oracle.make_golden --check` holds every .npz directly under tests/golden to be one of ITS fixtures
OUT = os.path.join(GOLDEN, "pdqn")

_NET = dict(state_dim=6, action_dim=3, sizes=[24, 16], activations=["relu", "relu"], lr=0.003, batch=16, steps=4)
CASES = {
    # (i) maxq, double-q, mse, M = 5, a random mask; two fully masked (terminal) states per batch
    "pdqn_maxq_double": dict(_NET, max_num_actions=5, double_q=True, p_impossible=0.35, n_fully_masked=2,
                             rl=dict(gamma=0.9, target_update_rate=0.1, maxq_learning=True, q_network_loss="mse")),
    # (ii) maxq, single-q, huber, the discount's exponent from time_diff
    "pdqn_maxq_single_timediff": dict(_NET, max_num_actions=4, double_q=False, p_impossible=0.25, n_fully_masked=1,
                                      with_steps=True,
                                      rl=dict(gamma=0.95, target_update_rate=0.2, maxq_learning=True, q_network_loss="huber",
                                              use_seq_num_diff_as_time_diff=True)),
    # (iii) SARSA, multi_steps, with a reward network
    "pdqn_sarsa_multistep_reward": dict(_NET, max_num_actions=3, double_q=True, with_steps=True, reward_network=True,
                                        rl=dict(gamma=0.9, target_update_rate=0.05, maxq_learning=False,
                                                q_network_loss="mse", multi_steps=3)),
    # (iv) gamma = 0, bce_with_logits, rewards in [0, 1]
    "pdqn_bce": dict(_NET, max_num_actions=3, double_q=True,
                     rl=dict(gamma=0.0, target_update_rate=0.1, maxq_learning=True, q_network_loss="bce_with_logits")),
}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _batch(c, s):
    from reagent_amd import synthetic

    return synthetic.parametric_batch(c["batch"], c["state_dim"], c["action_dim"], c["max_num_actions"], seed=900 + s,
                                      p_impossible=c.get("p_impossible", 0.0), n_fully_masked=c.get("n_fully_masked", 0),
                                      with_steps=c.get("with_steps", False))


def generate(name):
    from oracle import reference_harness as rh

    rh._install()
    import reagent.core.types as rlt
    from reagent.models.critic import FullyConnectedCritic
    from reagent.training.parametric_dqn_trainer import ParametricDQNTrainer

    c = CASES[name]
    torch.manual_seed(0)
    q = FullyConnectedCritic(c["state_dim"], c["action_dim"], c["sizes"], c["activations"])
    reward = FullyConnectedCritic(c["state_dim"], c["action_dim"], c["sizes"], c["activations"]) if c.get("reward_network") else None
    tr = ParametricDQNTrainer(q, q.get_target_network(), reward, rl=rh.make_rl_parameters(**c["rl"]),
                              double_q_learning=c["double_q"], optimizer=rh.make_adam(c["lr"]))
    nets = dict(q=tr.q_network, target=tr.q_network_target)
    if reward is not None:
        nets["reward"] = tr.reward_network
    arrays = {}
    for n in ("q", "reward"):
        if n in nets:
            for i, p in enumerate(nets[n].parameters()):
                arrays[f"init_{n}_{i}"] = _np(p)
    reported = {}

    class _Reporter:
        def log(self, **kw):
            reported.update({k: v.detach().clone() for k, v in kw.items() if isinstance(v, torch.Tensor)})

    tr.set_reporter(_Reporter())
    loop = rh.PLLoop(tr)
    for s in range(c["steps"]):
        b = _batch(c, s)
        for k, v in b.items():
            arrays[f"step{s}_batch_{k}"] = _np(v)
        fd = lambda k: rlt.FeatureData(b[k])  # noqa: E731
        losses = loop.step(rlt.ParametricDqnInput(
            state=fd("state"), next_state=fd("next_state"), reward=b["reward"], time_diff=b["time_diff"], step=b["step"],
            not_terminal=b["not_terminal"], action=fd("action"), next_action=fd("next_action"),
            possible_actions=fd("possible_actions"), possible_actions_mask=b["possible_actions_mask"],
            possible_next_actions=fd("possible_next_actions"),
            possible_next_actions_mask=b["possible_next_actions_mask"], extras=rlt.ExtraData()))
        arrays[f"step{s}_td_loss"] = _np(losses[0])
        if reward is not None:
            arrays[f"step{s}_reward_loss"] = _np(losses[1])
        for k, v in reported.items():
            arrays[f"step{s}_report_{k}"] = _np(v)
        reported.clear()
        for n, net in nets.items():
            for i, p in enumerate(net.parameters()):
                arrays[f"step{s}_{n}_{i}"] = _np(p)
    arrays["config_json"] = np.array(json.dumps(c))
    return arrays


def signatures():
    """the reference's ParametricDQNTrainer / ParametricDqnInputMaker signatures as tests/test_reference_signatures.py
    reduces them (name, kind, default)"""
    from oracle import reference_harness as rh, stubs

    rh._install()
    stubs.install_gym()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    return ns["surface"]([
        ("reagent.training.parametric_dqn_trainer.ParametricDQNTrainer",
         ["__init__", "train_step_gen", "configure_optimizers", "_check_input", "get_detached_model_outputs"]),
        ("reagent.gym.preprocessors.trainer_preprocessor.ParametricDqnInputMaker", ["__init__", "create_for_env", "__call__"]),
    ])


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        arrays = generate(name)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print("wrote", name, sum(a.nbytes for a in arrays.values()) // 1024, "KiB")
    with open(os.path.join(GOLDEN, "reference_records", "parametric_dqn_signatures.json"), "w") as f:
        json.dump(signatures(), f, indent=1, sort_keys=True)
    print("wrote parametric_dqn_signatures.json")


if __name__ == "__main__":
    main()
