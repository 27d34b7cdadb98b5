"""The policy-gradient step's own kernels on the GPU box: 64 trajectories of 256 steps (N = 16 384), A = 16, S = 128,
512-512 hidden.
python profiles/microbench/pg_step.py [--step-only]

  (a)  rg_pg_returns + rg_pg_head + the two rg_reduce_sum on given scores and values (PPO with a value net)
  (b)  the torch operations they replace on the same inputs: a VECTORISED reverse discounted scan per trajectory (the
       trajectories have one length here, so it is one [T, 256] cumulative form), the temperature log-softmax, gather,
       ratio, clip, minimum, entropy, the summed MSE, with autograd for d loss / d scores and d loss / d values
  (b') (b) again: the run-to-run spread of the same work, measured in the same call
  (c)  the reference's scan as it is written — one 0-dim tensor operation per time step, once per trajectory — timed
       separately on 4 of the 64 trajectories and scaled, so that (b) is not a straw man

timed with device events after warm-up, in one process, alternating a / b / b' inside every round: (a) and (b) are read
against (b'), not against a fixed ratio.  Then the native PPO update's ms per update (bf16 and split-bf16).  --step-only
runs the native updates alone (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import reagent_amd._lib as L  # noqa: E402
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.gym.policies import Policy, SoftmaxActionSampler  # noqa: E402
from reagent_amd.models import FloatFeatureFullyConnected, FullyConnectedDQN, set_default_precision  # noqa: E402
from reagent_amd.optimizer import Optimizer__Union  # noqa: E402
from reagent_amd.training import PPOTrainer  # noqa: E402

dev = torch.device("cuda")
T, LEN, A, S, H = 64, 256, 16, 128, [512, 512]
N = T * LEN
ROUNDS, INNER = 12, 10
GAMMA, EPS, W, TEMP = 0.9, 0.2, 0.01, 1.0


def timed(fn, inner=INNER):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def kernels_vs_torch():
    g = torch.Generator().manual_seed(2)
    scores = (torch.randn(N, A, generator=g) * 2).to(dev)
    values = torch.randn(N, generator=g).to(dev)
    reward = torch.randn(N, generator=g).to(dev)
    a = torch.randint(A, (N,), generator=g).to(dev)
    action = torch.nn.functional.one_hot(a, A)
    old = (torch.log_softmax(scores / TEMP, dim=1)[torch.arange(N, device=dev), a] + (torch.rand(N, generator=g).to(dev) - 0.5))
    offsets = torch.arange(0, N + 1, LEN, dtype=torch.int32, device=dev)
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    P = ops.pg_head_partials(N, A)
    ret, dsc, dv, lp, ratio, adv, pp, vp, pl, vl = f(N), f(N, A), f(N), f(N), f(N), f(N), f(P), f(P), f(1), f(1)

    def fa():
        ops.pg_returns(reward, offsets, GAMMA, 1e6, False, False, False, ret)
        ops.pg_head(scores, action, ret, values, old, TEMP, L.PG_PPO, EPS, W, 1.0, dsc, dv, lp, ratio, adv, pp, vp)
        ops.reduce_sum(pp, P, 1.0, pl)
        ops.reduce_sum(vp, P, 1.0, vl)

    # discounted sum over a trajectory as one matrix product with the [LEN, LEN] upper-triangular discount table
    k = torch.arange(LEN, device=dev)
    table = torch.triu(GAMMA ** (k.unsqueeze(0) - k.unsqueeze(1)).clamp(min=0).float())
    out_b = {}

    def fb():
        r = torch.clamp(reward, max=1e6).view(T, LEN)
        returns = (r @ table.t()).reshape(N)
        sg, vg = scores.detach().requires_grad_(True), values.detach().requires_grad_(True)
        m = torch.distributions.Categorical(logits=sg / TEMP)
        l = m.log_prob(action.argmax(dim=1))
        advantage = (returns - vg).detach()
        rho = torch.exp(l - old)
        loss = -torch.min(advantage * rho, advantage * torch.clamp(rho, 1 - EPS, 1 + EPS)).sum() - W * m.entropy().sum()
        vloss = ((vg - returns) ** 2).sum()
        loss.backward()
        vloss.backward()
        out_b.update(loss=loss.detach(), vloss=vloss.detach(), dsc=sg.grad, dv=vg.grad)

    def fc():  # training/utils.py:42-54 as written, on 4 trajectories
        for t in range(4):
            r = reward[t * LEN:(t + 1) * LEN]
            returns = torch.empty_like(r)
            running = torch.zeros((), device=dev)
            for i in range(LEN - 1, -1, -1):
                running = r[i] + GAMMA * running
                returns[i] = running

    for fn in (fa, fb):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert abs(pl.item() - out_b["loss"].item()) <= 1e-4 * abs(pl.item()) and (dsc - out_b["dsc"]).abs().max() <= 1e-4
    ta, tb, tb2 = [], [], []
    for _ in range(ROUNDS):
        ta.append(timed(fa))
        tb.append(timed(fb))
        tb2.append(timed(fb))
    med = statistics.median
    spread = max(abs(x - y) for x, y in zip(tb, tb2))
    print(f"(a) pg kernels {med(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f})   (b) torch ops {med(tb):.1f} us "
          f"(min {min(tb):.1f}, max {max(tb):.1f})   (b') {med(tb2):.1f} us   spread max|b - b'| {spread:.1f} us, "
          f"|median b - median b'| {abs(med(tb) - med(tb2)):.1f} us   (b) - (a) = {med(tb) - med(ta):.1f} us")
    fc()
    tc = [timed(fc, inner=1) * (T / 4) for _ in range(3)]
    print(f"(c) the reference's per-step scan, 4 trajectories timed and scaled to {T}: {med(tc) / 1e3:.1f} ms "
          f"(min {min(tc) / 1e3:.1f}, max {max(tc) / 1e3:.1f})")


def trainer(prec):
    torch.manual_seed(0)
    set_default_precision(prec)
    try:
        scorer = FullyConnectedDQN(S, A, H, ["relu"] * len(H)).to(dev)
        value = FloatFeatureFullyConnected(S, 1, H, ["relu"] * len(H)).to(dev)
    finally:
        set_default_precision(L.PREC_F32)
    return PPOTrainer(Policy(scorer, SoftmaxActionSampler(temperature=TEMP)), gamma=GAMMA, optimizer=Optimizer__Union.default(lr=1e-3),
                      optimizer_value_net=Optimizer__Union.default(lr=1e-3), normalize=False, update_freq=T, ppo_batch_size=T,
                      ppo_epsilon=EPS, entropy_weight=W, value_net=value).to(dev)


if "--step-only" not in sys.argv:
    kernels_vs_torch()
trajs = [synthetic.to_pg_input(synthetic.pg_trajectory(LEN, S, A, seed=10 + t), dev) for t in range(T)]
for name, prec in (("bf16", L.PREC_BF16), ("bf16x3", L.PREC_BF16X3)):
    tr = trainer(prec)
    for _ in range(3):
        tr._update_model(trajs)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n_updates = 20
    s.record()
    for _ in range(n_updates):
        tr._update_model(trajs)
    e.record()
    e.synchronize()
    print(f"[{name}] native PPO update: {s.elapsed_time(e) / n_updates:.3f} ms/update ({T} trajectories x {LEN} steps packed, "
          f"A = {A}, the torch.cat of the minibatch included)")
    del tr
    torch.cuda.empty_cache()
