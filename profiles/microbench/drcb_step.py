"""The deep-represent LinUCB step on the GPU box: B = 65 536 rows, F = 256 raw features, an MLP of 512-512-64 (relu, relu,
linear; plain stack, PREC_F32), so the LinUCB dimension is d = 65.
python profiles/microbench/drcb_step.py

  solve : (a) rg_linucb_solve (one launch on the device-resident buffers)
          (b) LinearRegressionUCB._calculate_coefs, the parent class's host path (six downloads, torch.linalg.inv on the
              host, seven uploads) on the same buffers; (c) torch.linalg.inv on the device plus the fold as torch operations
  head  : (a) rg_drlinucb_head (its main and finishing launch: z, pred_label, loss, d loss / d mlp_out, d loss / d v)
          (b) the torch operations it replaces: cat, linear, mse_loss, the weighted mean, and autograd's backward of them
  step  : train_step_native (solve, saving forward, head, accumulate, backward, Adam), wall clock over a synchronise

timed with device events after warm-up, in one process, the candidates alternating inside every round, medians of 12
rounds; every (b) is run twice a round and read against its own repeat (b')."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import reagent_amd._lib as L  # noqa: E402
from reagent_amd import ops  # noqa: E402
from reagent_amd.core.types import CBInput  # noqa: E402
from reagent_amd.gym.policies import Policy  # noqa: E402
from reagent_amd.models import DeepRepresentLinearRegressionUCB, LinearRegressionUCB  # noqa: E402
from reagent_amd.training import DeepRepresentLinUCBTrainer  # noqa: E402

dev = torch.device("cuda")
B, F, SIZES, ARMS = 65536, 256, [512, 512, 64], 2
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


torch.manual_seed(0)
scorer = DeepRepresentLinearRegressionUCB(F, SIZES, ["relu", "relu", "linear"], use_batch_norm=False,
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


report(f"solve d={d}", {"(a) rg_linucb_solve + refill": solve_kernel, "(b) host _calculate_coefs + refill": solve_host,
                        "(b') again": solve_host, "(c) torch.linalg.inv on the device + refill": solve_torch_device,
                        "refill alone": refill_only})
solve_kernel()
solve_torch_device()
scale = inv_out["inv"].abs().max()
print(f"  kernel inverse against torch's on the device: {((scorer.inv_avg_A - inv_out['inv']).abs().max() / scale).item():.3e} "
      f"of the largest entry; status {scorer._solve_status.item()}", flush=True)

h = SIZES[-1]
mlp = torch.randn(B, h, generator=g).to(dev)
y = torch.randn(B, generator=g).to(dev)
w = (0.5 + torch.rand(B, generator=g)).to(dev)
v = (torch.randn(h + 1, generator=g) / (h + 1) ** 0.5).to(dev)
P = ops.drlinucb_head_partials(B, h)
e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
o = dict(z=e(B, h + 1), lin=e(B), pred=e(B), rows=e(B), dm=e(B, h), lp=e(P), dvp=e(P * (h + 1)), loss=e(1), dv=e(h + 1))
keep = {}


def head_kernel():
    ops.drlinucb_head(mlp, v, L.ACT["linear"], o["z"], o["lin"], o["pred"], label=y, weight=w, loss_type=L.CB_LOSS["mse"],
                      row_loss=o["rows"], dmlp_out=o["dm"], loss_partials=o["lp"], dv_partials=o["dvp"], loss=o["loss"],
                      dv=o["dv"])


def head_torch():
    m = mlp.detach().requires_grad_()
    lin_w = v.detach().reshape(1, -1).requires_grad_()
    z = torch.cat((torch.ones(B, 1, device=dev), m), -1)
    pred = torch.nn.functional.linear(z, lin_w).squeeze(-1)
    losses = torch.nn.functional.mse_loss(pred, y, reduction="none")
    loss = (losses * w).sum() / B
    loss.backward()
    keep.update(loss=loss.detach(), dm=m.grad, dv=lin_w.grad.reshape(-1))


report(f"head B={B} h={h}", {"(a) rg_drlinucb_head": head_kernel, "(b) torch forward + autograd backward": head_torch,
                             "(b') again": head_torch})
head_kernel()
head_torch()
print(f"  loss {o['loss'].item():.6f} / {keep['loss'].item():.6f}   max|d mlp_out| {(o['dm'] - keep['dm']).abs().max().item():.2e}   "
      f"max|dv| {(o['dv'] - keep['dv']).abs().max().item():.2e}", flush=True)

tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=1e-3)
x3 = torch.randn(B, ARMS, F, generator=g).to(dev)
action = torch.randint(0, ARMS, (B, 1), generator=g).to(dev)
chosen = torch.gather(x3, 1, action.unsqueeze(-1).expand(-1, 1, F)).squeeze(1).contiguous()
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
print(f"native step B={B} F={F} {'-'.join(map(str, SIZES))} (PREC_F32): {med(walls):.1f} us a step (min {min(walls):.1f}, "
      f"max {max(walls):.1f}), wall clock over a synchronise", flush=True)
with ops.profile() as prof:
    for _ in range(INNER):
        tr.train_step_native(batch)
for rec in prof.summary()[:12]:
    print(f"  {rec['name']:28s} {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // INNER} a step", flush=True)
tr.on_train_epoch_end()
print(f"  status after the epoch end: {scorer._solve_status.item()}, loss {tr._bufs['loss'].item():.5f}", flush=True)
