"""The counterfactual-evaluation steps on the GPU box: Bayes by backprop at B = 4 096 with layers 160-512-512-1 (A = 32 action
columns first, S = 128 state columns), the bandit head at B = 65 536 with A = 16.
python profiles/microbench/bbb_step.py          (--device cpu rehearses the script on the interpreter backend of tests/)

  sample : (a) rg_bbb_sample on the net's six segments, explicit noise (its two launches; the noise is NOT produced in it)
           (a') the same drawing its noise: the like-for-like partner of (b), which draws with torch.randn
           (b) the reference's lines per layer (probabilistic_fully_connected_network.py:87-105 without the linear) on the device
  grad   : (a) rg_bbb_grad on the same table
           (b) the draw's forward AND autograd's backward of (log_post - log_prior + sum(dW * w)): not like for like (the
               backward alone is not timed)
  elbo   : (a) rg_bbb_elbo_head at B = 4 096   (b) Normal(out, noise_tol).log_prob(target).sum(), the loss and its backward
  bandit : (a) rg_bandit_reward_head at B = 65 536, A = 16, SmoothL1 with propensities and a threshold (its two launches)
           (b) argmax, gather, the loss wrapper, the unweighted loss, with autograd's backward into q
  step   : (a) BayesByBackpropTrainer.train_step_native / BanditRewardNetTrainer.train_step_native (128-512-512-16), wall clock
           (b) the same step as torch modules on the device: the reference's layers, backward, torch.optim.Adam

timed with device events after warm-up (the steps: wall clock over a synchronise), in one process, the candidates
alternating inside every round, medians of 12 rounds; every (b) is run twice a round and read against its own repeat (b')."""
import contextlib
import statistics
import sys
import time

import torch
import torch.nn as nn
from torch.distributions import Normal

sys.path.insert(0, ".")
CPU = "--device" in sys.argv and sys.argv[sys.argv.index("--device") + 1] == "cpu"
if CPU:  # a rehearsal of the script alone: the kernels on the SIMT interpreter, tiny shapes, no number means anything
    sys.path.insert(0, "tests")
    import emu_backend

    emu_backend.install()
from reagent_amd import _lib as L  # noqa: E402
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.models import FullyConnectedDQN  # noqa: E402
from reagent_amd.models.probabilistic_fully_connected_network import FullyConnectedProbabilisticNetwork  # noqa: E402
from reagent_amd.optimizer import Optimizer__Union  # noqa: E402
from reagent_amd.training import BanditRewardNetTrainer, LossFunction  # noqa: E402
from reagent_amd.training.cfeval.bayes_by_backprop_trainer import BayesByBackpropTrainer  # noqa: E402

dev = torch.device("cpu" if CPU else "cuda")
B, S, A, LAYERS, BH, AH = (64, 12, 4, [16, 32, 32, 1], 512, 16) if CPU else (4096, 128, 32, [160, 512, 512, 1], 65536, 16)
ROUNDS, INNER = (2, 1) if CPU else (12, 10)
PRIOR, TOL = 1.0, 0.1
med = statistics.median
sync = (lambda: None) if CPU else torch.cuda.synchronize


def timed(fn):
    if CPU:
        return wall(fn)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(INNER):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / INNER * 1e3  # us per call


def wall(fn):
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    sync()
    return (time.perf_counter() - t0) / INNER * 1e6


def report(what, fns, clock=timed):
    for fn in fns.values():
        for _ in range(1 if CPU else 3):
            fn()
    sync()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(clock(fn))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)


class TorchBBB(nn.Module):
    """the reference's network as torch runs it (:87-105, :190-213)"""

    def __init__(self, layers):
        super().__init__()
        self.mu = nn.ParameterList([nn.Parameter(0.1 * torch.randn(o, i)) for i, o in zip(layers, layers[1:])])
        self.rho = nn.ParameterList([nn.Parameter(0.1 * torch.randn(o, i)) for i, o in zip(layers, layers[1:])])
        self.bmu = nn.ParameterList([nn.Parameter(torch.zeros(o)) for o in layers[1:]])
        self.brho = nn.ParameterList([nn.Parameter(torch.zeros(o)) for o in layers[1:]])
        self.prior = Normal(0, PRIOR)

    def draw(self):
        """every layer's (w, b) and the two log-densities"""
        ws, prior, post = [], 0, 0
        for mu, rho in list(zip(self.mu, self.rho)) + list(zip(self.bmu, self.brho)):
            eps = torch.randn(mu.shape, device=mu.device)  # (drawn on the device: the reference's Normal(0, 1).sample is on the host)
            w = mu + torch.log(1 + torch.exp(rho)) * eps
            prior = prior + torch.sum(self.prior.log_prob(w))
            post = post + Normal(mu.data, torch.log(1 + torch.exp(rho))).log_prob(w).sum()
            ws.append(w)
        return ws, prior, post

    def loss(self, x, y):
        ws, prior, post = self.draw()
        n = len(self.mu)
        for i in range(n):
            x = nn.functional.linear(x, ws[i], ws[n + i])
            if i < n - 1:
                x = torch.relu(x)
        like = Normal(x.reshape(-1), TOL).log_prob(y.reshape(-1)).sum()
        return post - prior - like


def bandit_lines(q, action, reward, prob, threshold):
    idx = torch.argmax(action, dim=1, keepdim=True)
    pred = q.gather(1, idx)
    loss = nn.SmoothL1Loss(reduction="none")(pred, reward)
    keep = reward <= threshold
    with torch.no_grad():
        unweighted = torch.mean(loss[keep])
    return torch.mean((loss * (1.0 / prob))[keep]), unweighted


def main():
    f = dict(dtype=torch.float32, device=dev)
    torch.manual_seed(0)
    net = FullyConnectedProbabilisticNetwork(LAYERS, ["relu", "relu", "linear"], PRIOR, noise_tol=TOL).to(dev)
    net.noise_source = lambda shape: torch.randn(shape)
    ws = net._draw()
    net.noise_source = None
    grads = [(torch.empty_like(w), torch.empty_like(w)) for w in ws["w"]]
    for dw in ws["dw"]:
        dw.normal_()
    table = net._table(grads)
    n_elems = sum(w.numel() for w in ws["w"])
    ref = TorchBBB(LAYERS).to(dev)

    def torch_sample():
        return ref.draw()

    def torch_grad():
        w, prior, post = ref.draw()
        for p in ref.parameters():
            p.grad = None
        (post - prior + sum((d.view_as(x) * x).sum() for d, x in zip(ws["dw"][0::2] + ws["dw"][1::2], w))).backward()

    report(f"sample {n_elems} elements in 6 segments", {
        "(a) rg_bbb_sample": lambda: ops.bbb_sample(table, PRIOR, ws["log_prior"], ws["log_post"], ws["terms"], ws["ws"]),
        "(a') rg_bbb_sample drawing": lambda: ops.bbb_sample(table, PRIOR, ws["log_prior"], ws["log_post"], ws["terms"], ws["ws"], seed=7),
        "(b) torch draw + log-densities": torch_sample, "(b') again": torch_sample})
    report("grad (the torch side includes its forward)", {
        "(a) rg_bbb_grad": lambda: ops.bbb_grad(table, PRIOR), "(b) torch forward + autograd backward": torch_grad, "(b') again": torch_grad})

    out, target = torch.randn(B, 1, **f), torch.randn(B, **f)
    acc, result = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(4, **f)
    hws, dout = torch.empty(ops.bbb_elbo_head_partials(B), dtype=torch.float64, device=dev), torch.empty(B, 1, **f)
    o = out.clone().requires_grad_()

    def torch_elbo():
        o.grad = None
        (ws["log_post"] - ws["log_prior"] - Normal(o.reshape(-1), TOL).log_prob(target).sum()).sum().backward()

    report(f"elbo head B={B}", {
        "(a) rg_bbb_elbo_head": lambda: ops.bbb_elbo_head(out, target, TOL, ws["terms"], acc, result, hws, dout=dout),
        "(b) torch forward + autograd backward": torch_elbo, "(b') again": torch_elbo})

    bh = synthetic.bandit_reward_batch(BH, 8, AH, seed=1, with_propensities=True, device=dev)
    q = torch.randn(BH, AH, **f)
    pred, loss, unweighted = torch.empty(BH, **f), torch.empty(1, **f), torch.empty(1, **f)
    n_kept, dq = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(BH, AH, **f)
    bws = torch.empty(ops.bandit_reward_head_workspace(BH), dtype=torch.float64, device=dev)
    qa = q.clone().requires_grad_()

    def torch_bandit():
        qa.grad = None
        bandit_lines(qa, bh.action, bh.reward, bh.action_prob, 0.5)[0].backward()

    report(f"bandit head B={BH} A={AH}", {
        "(a) rg_bandit_reward_head": lambda: ops.bandit_reward_head(
            q, bh.action, bh.reward.view(-1), pred, loss, n_kept, bws, action_prob=bh.action_prob.view(-1),
            loss_type=L.SRW_LOSS["SmoothL1_Loss"], threshold=0.5, unweighted_loss=unweighted, dq=dq),
        "(b) torch forward + autograd backward": torch_bandit, "(b') again": torch_bandit})

    # ---- the whole steps ---------------------------------------------------------------------------------------------------
    batch = synthetic.bandit_reward_batch(B, S, A, seed=2, with_propensities=True, device=dev)
    tr = BayesByBackpropTrainer(net, optimizer=Optimizer__Union.default(lr=1e-3)).to(dev)
    x, y = torch.cat([batch.action, batch.state.float_features], 1), batch.reward
    topt = torch.optim.Adam(ref.parameters(), lr=1e-3)

    def torch_bbb_step():
        topt.zero_grad()
        ref.loss(x, y).backward()
        topt.step()

    report(f"Bayes-by-backprop step B={B} {LAYERS}", {"(a) train_step_native": lambda: tr.train_step_native(batch),
                                                       "(b) torch modules": torch_bbb_step, "(b') again": torch_bbb_step}, clock=wall)
    with ops.profile() if not CPU else contextlib.nullcontext() as prof:
        tr.train_step_native(batch)
    for r in prof.summary() if prof is not None else []:
        print(f"  {r['name']:<22} {str(r['meta']):<50} {r['ms'] / r['calls'] * 1e3:7.1f} us a call  x{r['calls']} a step")

    dqn = FullyConnectedDQN(S, AH, LAYERS[1:-1], ["relu"] * (len(LAYERS) - 2)).to(dev)
    bb = synthetic.bandit_reward_batch(B, S, AH, seed=3, with_propensities=True, device=dev)
    btr = BanditRewardNetTrainer(dqn, optimizer=Optimizer__Union.default(lr=1e-3), loss_type=LossFunction.SmoothL1Loss,
                                 reward_ignore_threshold=0.5, weighted_by_inverse_propensity=True).to(dev)
    dims = [S] + LAYERS[1:-1]
    tnet = nn.Sequential(*[m for i, o in zip(dims, dims[1:]) for m in (nn.Linear(i, o), nn.ReLU())], nn.Linear(dims[-1], AH)).to(dev)
    bopt = torch.optim.Adam(tnet.parameters(), lr=1e-3)

    def torch_bandit_step():
        bopt.zero_grad()
        bandit_lines(tnet(bb.state.float_features), bb.action, bb.reward, bb.action_prob, 0.5)[0].backward()
        bopt.step()

    report(f"bandit reward step B={B} {dims + [AH]}", {"(a) train_step_native": lambda: btr.train_step_native(bb),
                                                        "(b) torch modules": torch_bandit_step, "(b') again": torch_bandit_step}, clock=wall)
    with ops.profile() if not CPU else contextlib.nullcontext() as prof:
        btr.train_step_native(bb)
    for r in prof.summary() if prof is not None else []:
        print(f"  {r['name']:<22} {str(r['meta']):<50} {r['ms'] / r['calls'] * 1e3:7.1f} us a call  x{r['calls']} a step")


if __name__ == "__main__":
    main()
