"""The disjoint LinUCB kernels on the GPU box: B = 65 536 rows over 8 arms (8 192 rows an arm), d = 256 features.
python profiles/microbench/dcb_step.py

  (a)  rg_dlinucb_accumulate (its main and finishing launch) on the packed batch
  (b)  the reference's step on the same rows: the Python loop of DisjointLinUCBTrainer.update_params over the arms, two
       matmuls and two `+=` an arm (disjoint_linucb_trainer.py:66-76, 94-101)
  (b') (b) again: the run-to-run spread of the same work, measured in the same call
and the same three for rg_dlinucb_score with the arg-max against matmul, batch_quadratic_form_multi_arms, sqrt and argmax
on [B, d] (disjoint_linucb_predictor.py:165-174).

timed with device events after warm-up, in one process, alternating a / b / b' inside every round: (a) and (b) are read
against (b'), not against a fixed ratio."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from reagent_amd import ops  # noqa: E402

dev = torch.device("cuda")
B, D, A = 65536, 256, 8
ROUNDS, INNER = 12, 10


def timed(fn, inner=INNER):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def report(what, fa, fb):
    for fn in (fa, fb):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ta, tb, tb2 = [], [], []
    for _ in range(ROUNDS):
        ta.append(timed(fa))
        tb.append(timed(fb))
        tb2.append(timed(fb))
    med = statistics.median
    spread = max(abs(x - y) for x, y in zip(tb, tb2))
    print(f"{what}: (a) kernels {med(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f})   (b) torch ops {med(tb):.1f} us "
          f"(min {min(tb):.1f}, max {max(tb):.1f})   (b') {med(tb2):.1f} us   spread max|b - b'| {spread:.1f} us   "
          f"(b) - (a) = {med(tb) - med(ta):.1f} us", flush=True)


g = torch.Generator().manual_seed(3)
n = B // A
x = torch.randn(B, D, generator=g).to(dev)
y = torch.randn(B, 1, generator=g).to(dev)
w = (0.5 + torch.rand(B, 1, generator=g)).to(dev)
offsets = torch.arange(0, B + 1, n, dtype=torch.int64).to(dev)
state = [torch.zeros(A, D, D, device=dev), torch.zeros(A, D, device=dev), torch.zeros(A, dtype=torch.int64, device=dev)]
ref = [t.clone() for t in state]
ws = ops.dlinucb_workspace(n, A, D, dev)
subs = [(x[a * n:(a + 1) * n], y[a * n:(a + 1) * n], w[a * n:(a + 1) * n]) for a in range(A)]  # (views: the arms' sub-batches)


def acc_a():
    ops.dlinucb_accumulate(x, y.view(-1), w.view(-1), offsets, n, state[0], state[1], state[2], ws)


def acc_b():
    for a, (xa, ya, wa) in enumerate(subs):
        ref[2][a] += ya.shape[0]
        ref[0][a] += torch.matmul(xa.t(), xa * wa)
        ref[1][a] += torch.matmul(xa.t(), ya * wa).squeeze()


report("accumulate", acc_a, acc_b)
# ((b) ran twice as often as (a): the sums are compared per observation)
mean_a, mean_b = state[0] / state[2].view(A, 1, 1), ref[0] / ref[2].view(A, 1, 1)
assert (mean_a - mean_b).abs().max() <= 1e-4 * mean_b.abs().max()

G = torch.randn(A, D, D, generator=g)
M = (G @ G.transpose(1, 2) / D + torch.eye(D)).to(dev)
coefs = torch.randn(A, D, generator=g).to(dev)
ucb = torch.empty(B, A, device=dev)
best = torch.empty(B, dtype=torch.int64, device=dev)
keep = {}


def score_a():
    ops.dlinucb_score(x, coefs, M, 1.0, ucb, best_arm=best)


def score_b():  # disjoint_linucb_predictor.py:165-174 and cb/utils.py:128
    results = torch.matmul(x, coefs.t())
    results += 1.0 * torch.sqrt(torch.einsum("ijk, jk -> ji", torch.matmul(x, M), x))
    keep["ucb"] = results
    keep["best"] = torch.argmax(results, dim=1)


report("score", score_a, score_b)
assert (ucb - keep["ucb"]).abs().max() <= 1e-3
assert (best != keep["best"]).sum().item() <= B // 1000  # (near-ties may fall either way between two fp32 orders)
