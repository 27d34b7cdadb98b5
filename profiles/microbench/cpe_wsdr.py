"""rg_cpe_wsdr (csrc/cpe_wsdr.hip) on the GPU box at a page of N = 2^20 rows, A = 16 actions, mean episode length 20 with one
episode of 500 steps, J = 25 j-steps (MAGIC) and J = 1 (weighted DR):
python profiles/microbench/cpe_wsdr.py

  (a) the seven launches of rg_cpe_wsdr (workspace and outputs allocated per call, as the estimator does), device events,
      medians of 12 rounds;
  (e) WeightedSequentialDoublyRobustEstimator.estimate end to end (offsets, launches, one read-back, the host quadratic
      programs: 1 for the point estimate and 50 for the bootstrap), wall clock, medians of 12 rounds;
  (q) the host quadratic programs alone: solve_simplex_qp on the page's covariance and bias, 1 + 50 solves, wall clock;
  (h) the reference's dense computation restated in float64 numpy on the host (tests/cpe_wsdr_statement.py: padded
      [episodes, T, A] cubes by itertools.zip_longest, 25 subsets recomputed), one wall-clock run, on a page of 2^16 ROWS drawn the
      same way (the 500-step episode included): the full page's four cubes are 4 x 3.4 GB and its zip_longest runs for minutes.
No speed is promised for any of these: the numbers go to profiles/NOTES_r20.md."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
from reagent_amd import ops  # noqa: E402
from reagent_amd.evaluation.evaluation_data_page import EvaluationDataPage  # noqa: E402
from reagent_amd.evaluation.weighted_sequential_doubly_robust_estimator import (  # noqa: E402
    reference_j_steps, solve_simplex_qp, subset_offsets, WeightedSequentialDoublyRobustEstimator)

dev = torch.device("cuda")
N, A, MEAN_LEN, LONG, J, GAMMA = 1 << 20, 16, 20, 500, 25, 0.9
ROUNDS = 12
med = statistics.median


def make_page(n_rows, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = [LONG]
    while sum(lengths) < n_rows:
        lengths.append(min(int(torch.randint(1, 2 * MEAN_LEN, (1,), generator=g)), n_rows - sum(lengths)))
    lengths = lengths[1:3] + lengths[:1] + lengths[3:]  # the long episode is not the first
    n = sum(lengths)
    logged = torch.randint(A, (n,), generator=g)
    page = dict(mdp_id=torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths)).reshape(n, 1),
                sequence_number=torch.cat([torch.arange(k) for k in lengths]).reshape(n, 1),
                logged_propensities=(0.2 + 0.8 * torch.rand(n, 1, generator=g)),
                logged_rewards=torch.rand(n, 1, generator=g), action_mask=torch.nn.functional.one_hot(logged, A).float(),
                model_propensities=torch.softmax(torch.randn(n, A, generator=g), 1), model_values=torch.randn(n, A, generator=g))
    return page, lengths


def device_page(page):
    t = {k: v.to(dev) for k, v in page.items()}
    n = t["mdp_id"].shape[0]
    return EvaluationDataPage(model_rewards=torch.zeros_like(t["model_values"]),
                              model_rewards_for_logged_action=torch.zeros(n, 1, device=dev), **t)


def timed_device(fn, inner=3):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)  # ms


def main():
    from reagent_amd.evaluation.evaluation_data_page import episode_offsets

    page, lengths = make_page(N, 1)
    edp = device_page(page)
    E, T = len(lengths), max(lengths)
    offsets = episode_offsets(edp.mdp_id)
    est = WeightedSequentialDoublyRobustEstimator(GAMMA)
    print(f"page: N = {sum(lengths)} rows, E = {E} episodes, T = {T}, A = {A}", flush=True)
    for j in (J, 1):
        js = [int(min(x, T - 1)) for x in reference_j_steps(T, j)]
        subsets = subset_offsets(E, 25) if j > 1 else None
        run = lambda: ops.cpe_wsdr(edp.model_propensities, edp.action_mask, edp.model_values, edp.logged_propensities.reshape(-1),
                                   edp.logged_rewards, offsets, T, GAMMA, True, js, subsets)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        a = [timed_device(run) for _ in range(ROUNDS)]
        print(f"J = {j}: (a) rg_cpe_wsdr {med(a):.1f} us (min {min(a):.1f}, max {max(a):.1f})", flush=True)
        torch.manual_seed(0)
        est.estimate(edp, j, True)
        e = [wall(lambda: est.estimate(edp, j, True)) for _ in range(ROUNDS)]
        print(f"J = {j}: (e) estimate end to end {med(e):.2f} ms (min {min(e):.2f}, max {max(e):.2f})", flush=True)
    q = est.device_quantities(edp, J, True)
    bias = est.j_step_bias(q["j_step_returns"], q["infinite_step_returns"])

    def programs():
        solve_simplex_qp(q["covariance"], bias * bias)
        for k in range(50):
            idx = np.sort(torch.randperm(J)[:12].numpy())
            solve_simplex_qp(q["covariance"][np.ix_(idx, idx)], (bias * bias)[idx])

    t = [wall(programs) for _ in range(ROUNDS)]
    print(f"(q) 1 + 50 host quadratic programs {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})", flush=True)
    from cpe_wsdr_statement import dense_statement

    small, small_lengths = make_page(1 << 16, 1)
    Ts, Es = max(small_lengths), len(small_lengths)
    t0 = time.perf_counter()
    dense_statement(small_lengths, small["action_mask"].numpy(), small["logged_rewards"].numpy(),
                    small["logged_propensities"].numpy(), small["model_propensities"].numpy(), small["model_values"].numpy(),
                    GAMMA, True, reference_j_steps(Ts, J), subset_offsets(Es, 25))
    print(f"(h) the dense float64 statement on the host, {sum(small_lengths)} rows, {Es} episodes, T = {Ts}: "
          f"{time.perf_counter() - t0:.2f} s, one run", flush=True)
    sdev = device_page(small)
    s = [wall(lambda: est.device_quantities(sdev, J, True)) for _ in range(ROUNDS)]
    print(f"    the same page through rg_cpe_wsdr and its read-back: {med(s):.2f} ms", flush=True)


if __name__ == "__main__":
    main()
