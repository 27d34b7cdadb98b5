"""The parametric DQN step's tiled critic forward on the GPU box: 8 192 states x M = 8 candidates (65 536 tiled rows),
S = 256, A = 32, 512-512 hidden, bf16 and split-bf16.   python profiles/microbench/pdqn_step.py [--step-only]

  (a) the tiled fused forward: forward(next_state, out, x2=candidates, x_tile=M) — the tiled state is never written
  (b) next_state.repeat_interleave(M, 0) + the existing two-panel forward: what the step would cost without x_tile
  (b') (b) again: the run-to-run spread of the same work, measured in the same call

timed with device events after warm-up, in one process, alternating a / b / b' inside every round; then the full native
step's ms/step.  --step-only runs the native steps alone (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import reagent_amd._lib as L  # noqa: E402
from reagent_amd import synthetic  # noqa: E402
from reagent_amd.core.parameters import RLParameters  # noqa: E402
from reagent_amd.models import FullyConnectedCritic, set_default_precision  # noqa: E402
from reagent_amd.optimizer import Optimizer__Union  # noqa: E402
from reagent_amd.training import ParametricDQNTrainer  # noqa: E402

dev = torch.device("cuda")
B, M, S, A, H = 8192, 8, 256, 32, [512, 512]
ROUNDS, INNER = 12, 10


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(INNER):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / INNER * 1e3  # us per call


def trainer(prec):
    torch.manual_seed(0)
    set_default_precision(prec)
    try:
        q = FullyConnectedCritic(S, A, H, ["relu"] * len(H)).to(dev)
    finally:
        set_default_precision(L.PREC_F32)
    return ParametricDQNTrainer(q, q.get_target_network(), rl=RLParameters(gamma=0.99, maxq_learning=True),
                                optimizer=Optimizer__Union.default(lr=1e-3)).to(dev)


step_only = "--step-only" in sys.argv
for name, prec in (("bf16", L.PREC_BF16), ("bf16x3", L.PREC_BF16X3)):
    tr = trainer(prec)
    batch = synthetic.to_parametric_input(synthetic.parametric_batch(B, S, A, M, seed=1, p_impossible=0.2), dev)
    for _ in range(3):
        tr.train_step_native(batch)
    torch.cuda.synchronize()
    if not step_only:
        st = tr.q_network_target.fc.stack()
        ns, pna = batch.next_state.float_features, batch.possible_next_actions.float_features
        out_a, out_b = torch.empty(B * M, 1, device=dev), torch.empty(B * M, 1, device=dev)
        fa = lambda: st.forward(ns, out_a, x2=pna, x_tile=M)  # noqa: E731
        fb = lambda: st.forward(ns.repeat_interleave(M, 0), out_b, x2=pna)  # noqa: E731
        for f in (fa, fb):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        assert torch.equal(out_a, out_b)
        ta, tb, tb2 = [], [], []
        for _ in range(ROUNDS):
            ta.append(timed(fa))
            tb.append(timed(fb))
            tb2.append(timed(fb))
        med = statistics.median
        spread = max(abs(x - y) for x, y in zip(tb, tb2))
        print(f"[{name}] (a) tiled forward {med(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f})   (b) repeat_interleave + "
              f"two-panel forward {med(tb):.1f} us (min {min(tb):.1f}, max {max(tb):.1f})   (b') {med(tb2):.1f} us   "
              f"spread max|b - b'| {spread:.1f} us, |median b - median b'| {abs(med(tb) - med(tb2)):.1f} us   "
              f"(b) - (a) = {med(tb) - med(ta):.1f} us")
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    s.record()
    for _ in range(n):
        tr.train_step_native(batch)
    e.record()
    e.synchronize()
    print(f"[{name}] native step: {s.elapsed_time(e) / n:.3f} ms/step ({B} states x {M} candidates)")
    del tr, batch
    torch.cuda.empty_cache()
