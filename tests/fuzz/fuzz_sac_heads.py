import os, sys, random, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import emu_backend
emu_backend.install()
from conftest import Backend
import test_sac_head_statements as T

# the Gaussian policy head (forward, log-prob of a given action, backward with its KLD branch) on random (batch, action_dim)
# — rows of one element, widths around the wavefront and beyond one workgroup — through the staged checks of
# tests/test_sac_head_statements.py: inputs planted per stratum, stage A to 4 ulp, stage B and the backward to the pool's
# per-stratum tables (float64 statements of tests/sac_refs.py, actor.py:166-261)
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
cases = int(sys.argv[2]) if len(sys.argv) > 2 else 30
random.seed(seed)
bad = 0
run = T.KernelRunner("cpu")
for case in range(cases):
    B = random.choice([1, 2, 3, 63, 64, 65, 257, 1000])
    A = random.choice([1, 2, 3, 16, 31, 32, 33, 64, 65, 128, 255, 256, 257, 300])
    try:
        worst = {}
        for c in T.shape_cases(B, A, seed=seed * 100000 + case * 100):
            for k, r in T.check_head(run, c).items():
                worst[k] = max(worst.get(k, 0.0), r)
        print("OK ", B, A, "worst ratio %.3f (%s)" % max((r, k) for k, r in worst.items()))
    except Exception:
        bad += 1
        print("BAD", B, A)
        traceback.print_exc(limit=2)

# the SAC loss heads (critic targets / losses / gradients under every (q2, q2_target) combination and both gamma branches, the
# actor loss with its tie split, CRR weights and detached log-prob, per-partial loss and entropy sums) at batch sizes around the
# workgroup and partial-sum boundaries — sac_trainer.py:23-47, 205-340 in float64
for case in range(cases):
    B = random.choice([1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
    try:
        T.test_critic_head(Backend("emu", "cpu"), B, seed=seed * 100000 + case * 100)
        T.test_actor_head(Backend("emu", "cpu"), B, seed=seed * 100000 + case * 100)
        print("OK ", "loss heads", dict(B=B))
    except Exception:
        bad += 1
        print("BAD", "loss heads", dict(B=B))
        traceback.print_exc(limit=2)
print("bad cases:", bad)
sys.exit(1 if bad else 0)
