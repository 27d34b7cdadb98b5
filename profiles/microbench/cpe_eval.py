"""The five entry points of csrc/cpe_eval.hip on the GPU box at a page of N = 2^20 rows, A = 16 actions, M = 2 (one extra
metric), mean episode length 20, K = 1 000 resamples of 25 %:
python profiles/microbench/cpe_eval.py

  page rows      (a) rg_cpe_page_rows          (b) the torch operations of create_from_tensors_dqn on the device
  episode values (a) rg_cpe_episode_values     (b) a torch segmented statement on the device (a loop over the longest
                                                   episode's steps, every episode advanced at once)   (h) the reference's
                                                   Python loop over rows, on numpy scalars on the host
  dr rows        (a) rg_cpe_dr_rows            (b) the torch operations of the two estimators' row quantities and means
  sequential dr  (a) rg_cpe_sdr                (b) the same segmented torch loop   (h) the reference's Python loop, numpy scalars
  bootstrap      (a) rg_cpe_bootstrap, C = 3   (b) torch.randint + gather + mean on the device, 3 columns from one index set,
                                                   in chunks of 50 resamples   (h) the reference's 1 000 np.random.choice calls
                                                   for ONE column

(a) and (b) are timed with device events after warm-up, in one process, alternating inside every round, medians of 12
rounds; (h) is one wall-clock run each (they take seconds).  The (b) and (h) statements are yardsticks, not the product."""
import math
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from reagent_amd import ops  # noqa: E402
from reagent_amd.core.torch_utils import masked_softmax  # noqa: E402

dev = torch.device("cuda")
N, A, M, MEAN_LEN, K, GAMMA, T = 1 << 20, 16, 2, 20, 1000, 0.9, 0.7
ROUNDS = 12
med = statistics.median


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3  # us per call


def report(what, fns, inner):
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn, inner))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)


def host(what, fn):
    t = time.perf_counter()
    fn()
    print(f"{what}: (h) {1e3 * (time.perf_counter() - t):.0f} ms on the host, one run", flush=True)


g = torch.Generator().manual_seed(3)
lengths = torch.randint(1, 2 * MEAN_LEN, (N // MEAN_LEN + 1000,), generator=g)
lengths = lengths[: int(torch.searchsorted(torch.cumsum(lengths, 0), N)) + 1]
lengths[-1] -= int(lengths.sum()) - N
assert int(lengths.sum()) == N and int(lengths.min()) >= 1
E, LMAX = lengths.numel(), int(lengths.max())
mdp = torch.repeat_interleave(torch.arange(E), lengths)
seq = torch.cumsum(torch.randint(1, 4, (N,), generator=g), 0)
offsets = torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0))).to(torch.int32).to(dev)
q, q_cpe, reward_est = (torch.randn(N, w, generator=g).to(dev) for w in (A, M * A, M * A))
logged = torch.randint(A, (N,), generator=g)
action = torch.nn.functional.one_hot(logged, A).float().to(dev)
mask = (torch.rand(N, A, generator=g) < 0.8).float()
mask[torch.arange(N), logged] = 1.0
mask = mask.to(dev)
reward = torch.rand(N, generator=g).to(dev)
boosts = torch.randn(A, generator=g).to(dev)
lp = (0.2 + 0.8 * torch.rand(N, generator=g)).to(dev)
seq_d, mdp_d = seq.to(dev), mdp.to(dev)
print(f"N={N} A={A} M={M} episodes={E} longest={LMAX} K={K}", flush=True)


# ---- page rows -----------------------------------------------------------------------------------------------------------------
def page_kernel():
    return ops.cpe_page_rows(q, q_cpe, reward_est, action, mask, reward, boosts, T, M)


def page_torch():
    lr = reward.reshape(N, 1) + (action * boosts.reshape(1, A)).sum(1, keepdim=True)
    idx = torch.max(q + -1e9 * (1 - mask), dim=1, keepdim=True)[1]
    prop = masked_softmax(q, mask, T)
    mr = (reward_est[:, :A] * action).sum(1, keepdim=True)
    mm = (reward_est[:, A:] * action).sum(1, keepdim=True)
    mmv = (q_cpe[:, A:] * action).sum(1, keepdim=True)
    return lr, prop, idx, mr, mm, mmv


report("page rows", {"(a) rg_cpe_page_rows": page_kernel, "(b) torch": page_torch}, 50)
lr, prop, idx, mr, mm, mmv = page_kernel()

# ---- episode values -------------------------------------------------------------------------------------------------------------
starts, ends = offsets[:-1].long(), offsets[1:].long()
values_out = torch.empty(N, 1, device=dev)


def values_kernel():
    ops.cpe_episode_values(lr, seq_d, offsets, GAMMA, values_out)


def values_torch():
    v = lr.reshape(-1).clone()
    for step in range(2, LMAX + 1):  # row end - step of every episode that is at least `step` long
        x = ends - step
        live = x >= starts
        x = x[live]
        f = torch.pow(torch.tensor(GAMMA, dtype=torch.float64, device=dev), (seq_d[x + 1] - seq_d[x]).double()).float()
        v[x] = v[x] + v[x + 1] * f
    return v


def values_host():
    c, s, m = lr.reshape(-1).cpu().numpy(), seq.numpy(), mdp.numpy()
    v = c.copy()
    for x in range(N - 2, -1, -1):
        if m[x] != m[x + 1]:
            continue
        v[x] += v[x + 1] * np.float32(math.pow(GAMMA, float(s[x + 1] - s[x])))
    return v


report("episode values", {"(a) rg_cpe_episode_values": values_kernel, "(b) torch, segmented": values_torch}, 10)
host("episode values", values_host)

# ---- dr rows ---------------------------------------------------------------------------------------------------------------------
mv, mrew = q_cpe[:, :A], reward_est[:, :A]


def dr_kernel():
    return ops.cpe_dr_rows(prop, action, mrew, mv, lp, lr, mr)


def dr_torch():
    tp = (prop * action).sum(1)
    iw = tp / lp
    dm = (prop * mrew).sum(1)
    r, mrl = lr.reshape(-1), mr.reshape(-1)
    ips, dr = iw * r, iw * (r - mrl) + dm
    sv, ql = (prop * mv).sum(1), (mv * action).sum(1)
    return iw, torch.stack((dm, ips, dr)), sv, ql, torch.stack((r.mean(), dm.mean(), mrl.mean(), ips.mean(), dr.mean()))


report("dr rows", {"(a) rg_cpe_dr_rows": dr_kernel, "(b) torch": dr_torch}, 50)
rows = dr_kernel()
sv, iw, ql = rows["state_value"], rows["importance_weight"], rows["q_logged"]


# ---- sequential dr -----------------------------------------------------------------------------------------------------------------
def sdr_kernel():
    return ops.cpe_sdr(sv, iw, lr, ql, offsets, GAMMA)


def sdr_torch():
    d, e = torch.zeros(E, device=dev), torch.zeros(E, device=dev)
    r = lr.reshape(-1)
    for step in range(1, LMAX + 1):
        x = ends - step
        live = x >= starts
        x = x[live]
        d[live] = sv[x] + iw[x] * (r[x] + GAMMA * d[live] - ql[x])
        e[live] = e[live] * GAMMA + r[x]
    return d, e


def sdr_host():
    s_, i_, r_, q_, m = (t.reshape(-1).cpu().numpy() for t in (sv, iw, lr, ql, mdp))
    g32 = np.float32(GAMMA)
    out, last, i = [], -1, 0
    while i < N:
        if i == N - 1 or m[i] != m[i + 1]:
            d = e = np.float32(0)
            for j in range(i, last, -1):
                d = s_[j] + i_[j] * (r_[j] + g32 * d - q_[j])
                e = e * g32 + r_[j]
            out.append((float(d), float(e)))
            last = i
        i += 1
    return out


report("sequential dr", {"(a) rg_cpe_sdr": sdr_kernel, "(b) torch, segmented": sdr_torch}, 10)
host("sequential dr", sdr_host)

# ---- bootstrap ----------------------------------------------------------------------------------------------------------------------
est = rows["dm_ips_dr"]
S = int(0.25 * N)


def boot_kernel():
    return ops.cpe_bootstrap(est, S, K, 12345)


def boot_torch():
    means = torch.empty(3, K, dtype=torch.float64, device=dev)
    for k0 in range(0, K, 50):
        idx = torch.randint(N, (50, S), device=dev)
        means[:, k0:k0 + 50] = est[:, idx].double().mean(2)
    return means.std(1, unbiased=False)


def boot_host():
    data = est[2].cpu().numpy()
    return np.std([np.mean(np.random.choice(data, size=S, replace=True)) for _ in range(K)])


report("bootstrap (3 columns)", {"(a) rg_cpe_bootstrap": boot_kernel, "(b) torch": boot_torch}, 2)
host("bootstrap (1 column)", boot_host)
print("std errors", boot_kernel()[1].tolist(), "torch", boot_torch().tolist(),
      "sqrt(var / S)", (est.double().var(1, unbiased=False) / S).sqrt().tolist())
