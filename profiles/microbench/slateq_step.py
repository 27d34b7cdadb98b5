"""The SlateQ step's own kernels on the GPU box: 8 192 states x C = 32 candidates, K = 8, S = 256, D = 32, 512-512 hidden.
python profiles/microbench/slateq_step.py [--step-only]

  (a) the three kernels of a maxq single-selection step on given critic outputs: rg_slate_topk, rg_slate_gather twice (the
      next slate's weights; the logged slate's panel with the reward_mask count), rg_slateq_head + rg_reduce_sum
  (b) the torch operations they replace, on the same inputs: softmax + topk, advanced indexing (select_slate) with
      value * mask, the softmax-weighted sum, the masked mse_loss with autograd
  (b') (b) again: the run-to-run spread of the same work, measured in the same call

timed with device events after warm-up, in one process, alternating a / b / b' inside every round: (a) and (b) are read
against (b'), not against a fixed ratio.  Then the full native step's ms/step (bf16 and split-bf16).  --step-only runs the
native steps alone (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import reagent_amd._lib as L  # noqa: E402
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.core.parameters import RLParameters, SlateOptParameters  # noqa: E402
from reagent_amd.models import FullyConnectedCritic, set_default_precision  # noqa: E402
from reagent_amd.optimizer import Optimizer__Union  # noqa: E402
from reagent_amd.training import SlateQTrainer  # noqa: E402

dev = torch.device("cuda")
B, C, K, S, D, H = 8192, 32, 8, 256, 32, [512, 512]
ROUNDS, INNER = 12, 10
GAMMA = 0.9


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
        q = FullyConnectedCritic(S, D, H, ["relu"] * len(H)).to(dev)
    finally:
        set_default_precision(L.PREC_F32)
    return SlateQTrainer(q, q.get_target_network(), K, rl=RLParameters(gamma=GAMMA, maxq_learning=True),
                         optimizer=Optimizer__Union.default(lr=1e-3), slate_opt_parameters=SlateOptParameters()).to(dev)


def kernels_vs_torch():
    d = {k: v.to(dev) for k, v in synthetic.slateq_batch(B, S, D, C, K, seed=1).items()}
    g = torch.Generator().manual_seed(2)
    q_all = torch.randn(B, C, generator=g).to(dev)   # the target critic on every candidate of the next state
    q = torch.randn(B, K, generator=g).to(dev)       # the online critic on the logged slate
    nt = d["not_terminal"].reshape(-1).contiguous()
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    idx, q_sel, wn, w, panel = torch.empty(B, K, dtype=torch.int64, device=dev), f(B, K), f(B, K), f(B, K), f(B * K, D)
    n, y, dq, nq = torch.zeros(1, dtype=torch.int32, device=dev), f(B, K), f(B, K), f(B)
    parts, loss = f(ops.slateq_head_partials(B)), f(1)

    def fa():
        ops.slate_topk(q_all, d["next_item_probability"], d["next_item_mask"], True, idx, q_sel)
        ops.slate_gather(d["next_candidate_features"], d["next_item_mask"], d["next_item_probability"], idx, None, wn,
                         not_terminal=nt)
        ops.slate_gather(d["candidate_features"], d["item_mask"], d["item_probability"], d["action"], panel, w,
                         count_mask=d["reward_mask"], count_out=n)
        ops.slateq_head(q, q_sel, wn, d["position_reward"], d["reward_mask"], nt, GAMMA, None, None, True, None, K, n, y, dq,
                        parts, nq)
        ops.reduce_sum(parts, parts.numel(), 1.0, loss)

    rows = torch.arange(B, device=dev).unsqueeze(1).expand(B, K)
    out_b = {}

    def fb():
        value = d["next_item_probability"] * d["next_item_mask"]
        _, next_action = torch.topk(q_all * F.softmax(value, dim=1), K, dim=1)
        next_action = torch.where(nt.bool().unsqueeze(1), next_action, torch.zeros_like(next_action))
        qn, wn_ = q_all[rows, next_action], F.softmax(value[rows, next_action], dim=1)
        next_q = torch.sum(qn * wn_, dim=1, keepdim=True) * nt.unsqueeze(1)
        target = d["position_reward"] + GAMMA * next_q
        feats = d["candidate_features"][rows, d["action"]]  # select_slate of the logged slate: the online critic's panel
        qg = q.detach().requires_grad_(True)
        lv = F.mse_loss(qg[d["reward_mask"]], target[d["reward_mask"]])
        lv.backward()
        out_b.update(loss=lv.detach(), dq=qg.grad, feats=feats, idx=next_action)

    for fn in (fa, fb):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(panel.view(B, K, D), out_b["feats"]) and abs(loss.item() - out_b["loss"].item()) <= 1e-4 * abs(loss.item())
    ta, tb, tb2 = [], [], []
    for _ in range(ROUNDS):
        ta.append(timed(fa))
        tb.append(timed(fb))
        tb2.append(timed(fb))
    med = statistics.median
    spread = max(abs(x - y) for x, y in zip(tb, tb2))
    print(f"(a) slate kernels {med(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f})   (b) torch ops {med(tb):.1f} us "
          f"(min {min(tb):.1f}, max {max(tb):.1f})   (b') {med(tb2):.1f} us   spread max|b - b'| {spread:.1f} us, "
          f"|median b - median b'| {abs(med(tb) - med(tb2)):.1f} us   (b) - (a) = {med(tb) - med(ta):.1f} us")


if "--step-only" not in sys.argv:
    kernels_vs_torch()
for name, prec in (("bf16", L.PREC_BF16), ("bf16x3", L.PREC_BF16X3)):
    tr = trainer(prec)
    batch = synthetic.to_slateq_input(synthetic.slateq_batch(B, S, D, C, K, seed=1), dev)
    for _ in range(3):
        tr.train_step_native(batch)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n_steps = 20
    s.record()
    for _ in range(n_steps):
        tr.train_step_native(batch)
    e.record()
    e.synchronize()
    print(f"[{name}] native step: {s.elapsed_time(e) / n_steps:.3f} ms/step ({B} states x {C} candidates, slates of {K})")
    del tr, batch
    torch.cuda.empty_cache()
