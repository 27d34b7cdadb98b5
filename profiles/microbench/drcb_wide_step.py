"""The deep-represent LinUCB step where the LinUCB layer is wide, on the GPU box: B = 65 536 rows, F = 256 raw features, MLPs
of 512-512-256 (d = 257) and 512-512-511 (d = 512), relu, relu, linear; plain stack, PREC_F32.
python profiles/microbench/drcb_wide_step.py

  solve : (a) rg_linucb_solve_blocked (d / 32 + 3 launches on the device-resident buffers and the model's workspace)
          (b) LinearRegressionUCB._calculate_coefs, the parent class's host path (six downloads, torch.linalg.inv on the
              host, seven uploads) on the same buffers: what the step ran at these widths before
          (c) torch.linalg.inv on the device plus the fold as torch operations
  step  : train_step_native (solve, saving forward, head, accumulate, backward, Adam), wall clock over a synchronise, and
          the solve's share of it

timed with device events after warm-up, in one process, the candidates alternating inside every round, medians of 12
rounds; (b) is run twice a round and read against its own repeat (b')."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reagent_amd import ops  # noqa: E402
from reagent_amd.core.types import CBInput  # noqa: E402
from reagent_amd.gym.policies import Policy  # noqa: E402
from reagent_amd.models import DeepRepresentLinearRegressionUCB, LinearRegressionUCB  # noqa: E402
from reagent_amd.training import DeepRepresentLinUCBTrainer  # noqa: E402

dev = torch.device("cuda")
B, F, ARMS = 65536, 256, 2
ROUNDS, INNER = 12, 10
med = statistics.median


def timed(fn, inner=INNER):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def report(what, fns):
    """fns: name -> callable; every one warmed up, then alternated inside each round"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)
    return {k: med(v) for k, v in t.items()}


def run(sizes):
    torch.manual_seed(0)
    scorer = DeepRepresentLinearRegressionUCB(F, sizes, ["relu", "relu", "linear"], use_batch_norm=False,
                                              use_skip_connections=False).to(dev)
    d = scorer.input_dim
    g = torch.Generator().manual_seed(3)
    zrows = torch.randn(4096, d, generator=g)
    zrows[:, 0] = 1.0
    A0 = (zrows.t() @ zrows / 4096).to(dev)
    b0 = torch.randn(d, generator=g).to(dev)

    def refill(m):
        """an epoch's averages in the buffers, so that every solve folds and inverts the same problem"""
        m.cur_avg_A.copy_(A0)
        m.cur_avg_b.copy_(b0)
        m.cur_sum_weight.fill_(4096.0)
        m.sum_weight.fill_(1e-5)
        m.avg_A.zero_()
        m.avg_b.zero_()

    host = LinearRegressionUCB(d).to(dev)
    inv_out = {}

    def solve_kernel():
        refill(scorer)
        scorer._calculate_coefs()

    def solve_host():
        refill(host)
        host._calculate_coefs()

    def solve_torch_device():
        refill(host)
        total = host.cur_sum_weight + host.sum_weight
        avg_A = (host.avg_A * host.sum_weight + host.cur_avg_A * host.cur_sum_weight) / total
        avg_b = (host.avg_b * host.sum_weight + host.cur_avg_b * host.cur_sum_weight) / total
        inv = torch.linalg.inv(avg_A + host.l2_reg_lambda * torch.eye(d, device=dev) / total)
        inv_out["inv"], inv_out["coefs"] = inv, inv @ avg_b

    def refill_only():
        refill(host)

    t = report(f"solve d={d}", {"(a) rg_linucb_solve_blocked + refill": solve_kernel,
                                "(b) host _calculate_coefs + refill": solve_host, "(b') again": solve_host,
                                "(c) torch.linalg.inv on the device + refill": solve_torch_device,
                                "refill alone": refill_only})
    solve_kernel()
    solve_torch_device()
    scale = inv_out["inv"].abs().max()
    print(f"  kernel inverse against torch's on the device: "
          f"{((scorer.inv_avg_A - inv_out['inv']).abs().max() / scale).item():.3e} of the largest entry; status "
          f"{scorer._solve_status.item()}", flush=True)
    with ops.profile() as prof:
        for _ in range(INNER):
            solve_kernel()
    for rec in prof.summary()[:4]:
        print(f"  {rec['name']:28s} {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // INNER}", flush=True)

    tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=1e-3)
    x3 = torch.randn(B, ARMS, F, generator=g).to(dev)
    action = torch.randint(0, ARMS, (B, 1), generator=g).to(dev)
    chosen = torch.gather(x3, 1, action.unsqueeze(-1).expand(-1, 1, F)).squeeze(1).contiguous()
    y = torch.randn(B, generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g)).to(dev)
    batch = CBInput(context_arm_features=x3, features_of_chosen_arm=chosen, action=action, reward=y.reshape(B, 1).clone(),
                    weight=w.reshape(B, 1).clone())
    refill(scorer)
    scorer._calculate_coefs()
    for _ in range(5):
        tr.train_step_native(batch)
    torch.cuda.synchronize()
    walls = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(INNER):
            tr.train_step_native(batch)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / INNER * 1e6)
    solve_us = t["(a) rg_linucb_solve_blocked + refill"] - t["refill alone"]
    print(f"native step B={B} F={F} {'-'.join(map(str, sizes))} (PREC_F32): {med(walls):.1f} us a step (min {min(walls):.1f}, "
          f"max {max(walls):.1f}), wall clock over a synchronise; the solve less its refill {solve_us:.1f} us = "
          f"{100 * solve_us / med(walls):.1f} % of it; the host path less its refill "
          f"{t['(b) host _calculate_coefs + refill'] - t['refill alone']:.1f} us", flush=True)
    with ops.profile() as prof:
        for _ in range(INNER):
            tr.train_step_native(batch)
    for rec in prof.summary()[:12]:
        print(f"  {rec['name']:28s} {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // INNER} a step", flush=True)
    tr.on_train_epoch_end()
    print(f"  status after the epoch end: {scorer._solve_status.item()}, loss {tr._bufs['loss'].item():.5f}", flush=True)


for last in (256, 511):
    run([512, 512, last])
