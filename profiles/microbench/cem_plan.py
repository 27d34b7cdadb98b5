"""One CEMPlannerNetwork.forward (continuous planning) on the GPU box at two shapes.    python profiles/microbench/cem_plan.py

  cartpole : the reference's CartPole configuration: P = 100, E = 1, horizon 10, hidden 100 x 2 layers, G = 5, S = 4, A = 1,
             10 iterations, 15 elites, one world model
  pets     : a PETS-like shape: P = 500, E = 20, horizon 30, hidden 200 x 2 layers, G = 5, S = 17, A = 6, 5 iterations, 50 elites,
             five world models (baselines (a) and (b) run with E = 1: the reference's formula has no E > 1)

  (k) this package's planner: per iteration rg_cem_sample, rg_cem_group, rg_cem_rollout, rg_cem_refit; one readback
  (a) a batched torch statement on the device: per step one MemoryNetwork.forward of this package over [1, N, .] rows plus
      torch's samplers (Categorical, Normal, Bernoulli), then topk, mean and var per iteration; the trajectories of a model
      are its contiguous share of N
  (b) the reference's per-trajectory loop restated with this package's modules on the device (one mem_net call per
      trajectory and step, three torch.distributions samples, two .item() calls), timed on FEW solutions of one iteration
      and SCALED to P solutions and all iterations: labelled as scaled

wall clock over a synchronise, after warm-up in one process, the candidates alternating inside every round, medians of 12
rounds with min and max."""
import statistics
import sys
import time

import numpy as np
import torch
from torch.distributions.bernoulli import Bernoulli
from torch.distributions.categorical import Categorical
from torch.distributions.normal import Normal

sys.path.insert(0, ".")
from reagent_amd.core import types as rlt  # noqa: E402
from reagent_amd.models.cem_planner import CEMPlannerNetwork  # noqa: E402
from reagent_amd.models.world_model import MemoryNetwork  # noqa: E402

dev = torch.device("cuda")
ROUNDS, FEW = 12, 4
SHAPES = {
    "cartpole": dict(P=100, E=1, T=10, H=100, L=2, G=5, S=4, A=1, iters=10, elites=15, M=1),
    "pets": dict(P=500, E=20, T=30, H=200, L=2, G=5, S=17, A=6, iters=5, elites=50, M=5),
}


def fd(x):
    return rlt.FeatureData(x)


@torch.no_grad()
def torch_batched(nets, c, state, E):
    """(a): continuous_planning with every iteration's trajectories as one batch of torch calls"""
    P, T, A, S, N = c["P"], c["T"], c["A"], c["S"], c["P"] * E
    D = T * A
    mean, var = torch.zeros(D, device=dev, dtype=torch.float64), torch.full((D,), 0.25, device=dev, dtype=torch.float64)
    share = [(m * N // len(nets), (m + 1) * N // len(nets)) for m in range(len(nets))]
    for _ in range(c["iters"]):
        cv = torch.minimum(torch.minimum(((mean + 1) / 2) ** 2, ((1 - mean) / 2) ** 2), var)
        tn = torch.fmod(torch.randn(P, D, device=dev, dtype=torch.float64), 2.0)
        sol = tn * cv.sqrt() + mean
        act = sol.float().view(P, T, A).repeat_interleave(E, dim=0)
        st = state.expand(N, S).contiguous()
        acc, alive = torch.zeros(N, device=dev, dtype=torch.float64), torch.ones(N, device=dev, dtype=torch.bool)
        for j in range(T):
            nxt = torch.empty_like(st)
            for net, (lo, hi) in zip(nets, share):
                if hi == lo:
                    continue
                o = net(fd(st[None, lo:hi]), fd(act[None, lo:hi, j]))
                k = Categorical(torch.exp(o.logpi[0])).sample()
                rows = torch.arange(hi - lo, device=dev)
                nxt[lo:hi] = Normal(o.mus[0, rows, k], o.sigmas[0, rows, k]).sample()
                nt = Bernoulli(torch.sigmoid(o.not_terminal[0])).sample().bool()
                acc[lo:hi] += torch.where(alive[lo:hi], o.reward[0].double() * (0.99 ** j), 0.0)
                alive[lo:hi] &= nt
            st = nxt
        rewards = acc.view(P, E).mean(dim=1)
        el = sol[torch.topk(rewards, c["elites"]).indices]
        mean = 0.25 * mean + 0.75 * el.mean(dim=0)
        var = 0.25 * var + 0.75 * el.var(dim=0, unbiased=False)
    return mean[:A].cpu()


@torch.no_grad()
def reference_loop(nets, c, state, few):
    """(b): cem_planner.py:121-215 for `few` solutions of one iteration, with this package's MemoryNetwork on the device"""
    T, A, S = c["T"], c["A"], c["S"]
    sol = torch.rand(few, T, A, device=dev) * 2 - 1
    out = np.zeros(few)
    for i in range(few):
        st = state.view(S)
        net = nets[np.random.randint(0, len(nets))]
        for j in range(T):
            o = net(fd(st.reshape(1, 1, S)), fd(sol[i, j].reshape(1, 1, A)))
            k = Categorical(torch.exp(o.logpi.view(-1))).sample().long().item()
            st = Normal(o.mus[0, 0, k], o.sigmas[0, 0, k]).sample()
            out[i] += float(o.reward[0, 0]) * (0.99 ** j)
            if not Bernoulli(torch.sigmoid(o.not_terminal[0, 0])).sample().long().item():
                break
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    for name, c in SHAPES.items():
        torch.manual_seed(0)
        nets = [MemoryNetwork(c["S"], c["A"], c["H"], c["L"], c["G"]).to(dev) for _ in range(c["M"])]
        with torch.no_grad():
            for n in nets:
                n.mdnrnn.gmm_linear.bias[-1] = 3.0  # most trajectories run the whole horizon
        bounds = dict(action_upper_bounds=np.ones(c["A"]), action_lower_bounds=-np.ones(c["A"]))
        pl = CEMPlannerNetwork(nets, c["iters"], c["P"], c["E"], c["elites"], c["T"], c["S"], c["A"], False, True, 0.99,
                               epsilon=0.0, **bounds)
        state = torch.randn(1, c["S"], device=dev)
        cands = {
            "(k) planner": lambda: pl(fd(state)),
            "(a) torch batched, E = 1": lambda: torch_batched(nets, c, state, 1),
            f"(b) reference loop, {FEW} solutions of one iteration": lambda: reference_loop(nets, c, state, FEW),
        }
        for fn in cands.values():
            fn(), fn()
        times = {k: [] for k in cands}
        for _ in range(ROUNDS):
            for k, fn in cands.items():
                times[k].append(wall(fn))
        print(f"{name}: {c}")
        for k, v in times.items():
            print(f"  {k:55s} median {statistics.median(v):10.3f} ms   min {min(v):10.3f}   max {max(v):10.3f}")
        b = statistics.median(times[f"(b) reference loop, {FEW} solutions of one iteration"])
        print(f"  (b) SCALED to {c['P']} solutions x {c['iters']} iterations (E = 1): {b / FEW * c['P'] * c['iters']:.1f} ms")


if __name__ == "__main__":
    main()
