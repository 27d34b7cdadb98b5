"""Offline evaluation inside the LinUCB step on the GPU box: B = 65 536 rows, A = 8 arms, d = 256 features, weights +
arm_presence + action_log_probability, max_importance_weight = 4.
python profiles/microbench/cb_eval_step.py             (the timings)
python profiles/microbench/cb_eval_step.py --profile   (events around every entry point of the evaluated step, a run of its own)

  ingest : (a) rg_cb_eval_ingest (its main and finishing launch: importance and effective weights, the nine running sums)
           (b) the torch operations of the reference's ingest_batch on the device (_process_all_data, add_importance_weights,
               _process_used_data and the trainer's since-update sum: about 25 operations), written as the reference does
  step   : (a) LinUCBTrainer.training_step with a PolicyEvaluator attached (frozen model's scores and arg-max, ingest,
               accumulate with the effective weights)
           (b) the same trainer's step without an evaluator (the parent commit's step: accumulate alone)
           (c) the frozen model's forward_with_actions alone (what (a) adds beside the ingest)

timed with device events after warm-up, in one process, the candidates alternating inside every round, medians of 12
rounds.  A window is INNER_INGEST = 1000 calls of the ingest (30 ms of the kernel, 180 ms of the torch operations) or INNER =
50 steps (13 ms unevaluated, 125 ms evaluated): a window of a few calls of a 30 us kernel measures the scheduler; every (b) is run twice a round and read against its own repeat (b').  The step's (a) and (b) are also timed by the
wall clock over a synchronise."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reagent_amd import ops  # noqa: E402
from reagent_amd.core.types import CBInput  # noqa: E402
from reagent_amd.evaluation.cb import PolicyEvaluator  # noqa: E402
from reagent_amd.gym.policies import Policy  # noqa: E402
from reagent_amd.models.linear_regression import LinearRegressionUCB  # noqa: E402
from reagent_amd.training import LinUCBTrainer  # noqa: E402

dev = torch.device("cuda")
B, A, D, CLIP = 65536, 8, 256, 4.0
ROUNDS, INNER, INNER_INGEST = 12, 50, 1000
PROFILE = "--profile" in sys.argv[1:]
med = statistics.median


def timed(fn, inner=INNER):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def report(what, fns, inner=INNER):
    """fns: name -> callable; every one warmed up, then alternated inside each round"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn, inner))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)
    return {k: med(v) for k, v in t.items()}


g = torch.Generator().manual_seed(7)
x = torch.randn(B, A, D, generator=g).to(dev)
action = torch.randint(0, A, (B, 1), generator=g)
presence = torch.rand(B, A, generator=g) < 0.7
presence[torch.arange(B), action.reshape(-1)] = True
batch = CBInput(context_arm_features=x, arm_presence=presence.to(dev), action=action.to(dev),
                reward=torch.randn(B, 1, generator=g).to(dev), weight=(0.5 + torch.rand(B, 1, generator=g)).to(dev),
                action_log_probability=torch.log(0.05 + 0.95 * torch.rand(B, 1, generator=g)).to(dev))
model_actions = torch.randint(0, A, (B, 1), generator=g).to(dev)

# ---- ingest ------------------------------------------------------------------------------------------------------------------
state = torch.zeros(9, device=dev)
out = torch.empty(2, B, 1, device=dev)
partials = ops.cb_eval_partials(B, dev)
flat = dict(action=batch.action.reshape(-1), model=model_actions.reshape(-1), reward=batch.reward.reshape(-1),
            weight=batch.weight.reshape(-1), logp=batch.action_log_probability.reshape(-1))


def ingest_kernel():
    ops.cb_eval_ingest(flat["action"], flat["model"], flat["reward"], flat["weight"], flat["logp"], batch.arm_presence, A, CLIP,
                       out[0], out[1], partials, [state[k:k + 1] for k in range(8)], state[8:])


tstate = {k: torch.zeros(1, device=dev) for k in range(9)}
keep = {}


def ingest_torch():
    # _process_all_data
    weights = batch.weight
    tstate[0] += weights.sum()
    tstate[1] += (weights * batch.reward).sum()
    sizes = batch.arm_presence.sum(1)
    tstate[2] += (weights.squeeze() * sizes).sum()
    # add_importance_weights
    prob = torch.exp(batch.action_log_probability)
    iw = torch.ones_like(prob) / prob
    iw = torch.clamp(iw, max=CLIP)
    iw = (batch.action == model_actions) * iw
    # _process_used_data
    eff = weights * iw
    tstate[3] += (eff * batch.reward).sum()
    acc = (iw > 0).float()
    tstate[4] += (weights * acc * batch.reward).sum()
    tstate[5] += (weights * acc).sum()
    tstate[6] += eff.sum()
    sizes = batch.arm_presence.sum(1)
    tstate[7] += ((weights * acc).squeeze() * sizes).sum()
    tstate[8] += batch.weight.sum()
    keep.update(iw=iw, eff=eff)


if not PROFILE:
    report(f"ingest B={B} A={A}", {"(a) rg_cb_eval_ingest": ingest_kernel, "(b) torch ingest_batch": ingest_torch,
                                   "(b') again": ingest_torch}, INNER_INGEST)
state.zero_()
for t in tstate.values():
    t.zero_()
ingest_kernel()
ingest_torch()
ts = torch.cat([tstate[k] for k in range(9)])
print(f"  max|iw - torch| {(out[0] - keep['iw']).abs().max().item():.2e}  max|eff - torch| {(out[1] - keep['eff']).abs().max().item():.2e}"
      f"  sums: worst relative difference {((state - ts).abs() / ts.abs()).max().item():.2e}", flush=True)
moved = B * (8 + 8 + 4 + 4 + 4 + A + 4 + 4)
print(f"  bytes the kernel has to move: {moved / 1e6:.2f} MB", flush=True)


# ---- the step ----------------------------------------------------------------------------------------------------------------
def trainer(evaluated):
    scorer = LinearRegressionUCB(D).to(dev)
    tr = LinUCBTrainer(Policy(scorer=scorer, sampler=None))
    # a model that has seen data, so that the frozen copy scores with a real inverse
    tr.training_step(batch, 0)
    tr.on_train_epoch_end()
    ev = None
    if evaluated:
        ev = PolicyEvaluator(scorer, max_importance_weight=CLIP).to(dev)
        tr.attach_eval_module(ev)
    return tr, ev


tr_eval, ev = trainer(True)
tr_plain, _ = trainer(False)
frozen = ev.eval_model


def step_eval():
    tr_eval.training_step(batch, 0)


def step_plain():
    tr_plain.training_step(batch, 0)


def frozen_forward():
    frozen.forward_with_actions(batch.context_arm_features, arm_presence=batch.arm_presence)


if PROFILE:
    for _ in range(5):
        step_eval()
    torch.cuda.synchronize()
    with ops.profile() as prof:
        for _ in range(INNER):
            step_eval()
    for rec in prof.summary()[:8]:
        print(f"  {rec['name']:28s} {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // INNER} a step", flush=True)
    sys.exit(0)
report(f"step B={B} A={A} d={D}", {"(a) evaluated step": step_eval, "(b) unevaluated step": step_plain, "(b') again": step_plain,
                                  "(c) frozen model's forward_with_actions": frozen_forward})
for name, fn in (("(a) evaluated step", step_eval), ("(b) unevaluated step", step_plain)):
    walls = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(INNER):
            fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / INNER * 1e6)
    print(f"  {name}: {med(walls):.1f} us a step (min {min(walls):.1f}, max {max(walls):.1f}), wall clock over a synchronise", flush=True)
tr_eval.on_train_epoch_end()
print(f"  after the epoch end: avg_reward {ev.get_avg_reward():.5f}, frac_accepted {ev.frac_accepted.item():.4f}, "
      f"avg_size_accepted {ev.avg_size_accepted.item():.3f}", flush=True)
