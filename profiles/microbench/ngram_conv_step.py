"""The n-gram conv reward net on the GPU box: B = 4 096, T = 10, S = 128, A = 32 (S + A = 160), n = 3, the reference's default
tower (conv_dims [256, 128], kh [1, 1]) and FC sizes [256, 128].
python profiles/microbench/ngram_conv_step.py

  entry points : each of rg_seqconv_forward (both layers), rg_ngram_window, rg_ngram_window_backward, rg_seqconv_dgrad and
                 rg_seqconv_wgrad (both layers) against the torch operations that state the same thing on the device:
                 ngram + conv2d + relu per window, and autograd through them
  step         : (a) RewardNetTrainer.train_step_native of NGramConvolutionalNetwork, wall clock
                 (b) the same net as torch modules on the device: forward, backward, torch.optim.Adam

timed with device events after warm-up (the steps: wall clock over a synchronise), in one process, the candidates alternating
inside every round, medians of 12 rounds with min and max; the torch side is run twice a round and read against its own repeat (')."""
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, ".")
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.core.parameters import ConvNetParameters  # noqa: E402
from reagent_amd.models import NGramConvolutionalNetwork, SyntheticRewardNet  # noqa: E402
from reagent_amd.models.synthetic_reward import ngram  # noqa: E402
from reagent_amd.training import LossFunction, RewardNetTrainer  # noqa: E402

dev = torch.device("cuda")
B, T, S, A, N_CTX, DIMS, KH, SIZES = 4096, 10, 128, 32, 3, [256, 128], [1, 1], [256, 128]
ROUNDS, INNER = 12, 10
med = statistics.median


def timed(fn):
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
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / INNER * 1e6


def report(what, fns, clock=timed):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(clock(fn))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)


class TorchNet(nn.Module):
    """NGramConvolutionalNetwork's statement as torch runs it"""

    def __init__(self):
        super().__init__()
        dims = [1] + DIMS
        self.convs = nn.ModuleList([nn.Conv2d(dims[i], dims[i + 1], kernel_size=(KH[i], S + A if i == 0 else 1)) for i in range(len(KH))])
        h = N_CTX - sum(k - 1 for k in KH)
        fc = [DIMS[-1] * h] + SIZES + [1]
        self.fc = nn.ModuleList([nn.Linear(fc[i], fc[i + 1]) for i in range(len(fc) - 1)])
        self.register_buffer("pad", torch.zeros(1, 1, S + A))

    def tower(self, state, action):
        x = ngram(torch.cat((state, action), dim=-1), N_CTX, self.pad).reshape(-1, 1, N_CTX, S + A)
        for conv in self.convs:
            x = torch.relu(conv(x))
        return x.flatten(1)

    def loss(self, b):
        x = self.tower(b["state"], b["action"])
        for i, lin in enumerate(self.fc):
            x = torch.relu(lin(x)) if i + 1 < len(self.fc) else F.leaky_relu(lin(x))
        output = x.reshape(T, B).transpose(0, 1)
        mask = (torch.arange(T, device=x.device).repeat(B, 1) >= (T - b["valid_step"])).float()
        return torch.mean(nn.MSELoss(reduction="none")((output * mask).sum(dim=1, keepdim=True), b["reward"]))


def main():
    f = dict(dtype=torch.float32, device=dev)
    b = {k: x.to(dev) for k, x in synthetic.synthetic_reward_batch(T, B, S, A, seed=1).items()}
    batch = synthetic.to_synthetic_reward_input(b)
    p = ConvNetParameters(conv_dims=DIMS, conv_height_kernels=KH, pool_types=["max"] * len(KH), pool_kernel_sizes=[1] * len(KH))
    net = NGramConvolutionalNetwork(S, A, SIZES, ["relu"] * len(SIZES), "leaky_relu", N_CTX, p)
    tr = RewardNetTrainer(SyntheticRewardNet(net).to(dev), loss_type=LossFunction.MSE).to(dev)
    tm = TorchNet().to(dev)
    with torch.no_grad():
        for mine, theirs in zip(net.conv_net.conv_layers, tm.convs):
            theirs.weight.copy_(mine.weight)
            theirs.bias.copy_(mine.bias)

    # ---- the entry points, on the tape of one pass
    tape = net._run(b["state"], b["action"], save=True)
    g, feat, H, half = tape["g"], tape["x"], net.heights[-1], N_CTX // 2
    N = T * B
    st, ac = b["state"].view(N, S), b["action"].view(N, A)
    convs = [(c.weight.detach(), c.bias.detach()) for c in net.conv_net.conv_layers]
    dfeat = torch.randn(N, feat.shape[1], **f)
    y0, y1, ft = torch.empty_like(g[0]), torch.empty_like(g[1]), torch.empty_like(feat)
    dz1, dz0 = torch.empty_like(g[1]), torch.empty_like(g[0])
    dws = [torch.empty_like(w) for w, _ in convs]
    dbs = [torch.empty_like(bb) for _, bb in convs]
    P1 = g[0].shape[0] // B
    ws = [torch.empty(ops.seqconv_wgrad_workspace_bytes(P1, B, 1, S + A, DIMS[0]) // 4, **f),
          torch.empty(ops.seqconv_wgrad_workspace_bytes(P1, B, 1, DIMS[0], DIMS[1]) // 4, **f)]

    def tower_kernels():
        ops.seqconv_forward(st, ac, T, half, B, *convs[0], y0)
        ops.seqconv_forward(y0, None, P1, 0, B, *convs[1], y1)
        ops.ngram_window(y1, T, B, H, ft)

    def tower_backward_kernels():
        ops.ngram_window_backward(dfeat, T, B, H, dz1, g=g[1])
        ops.seqconv_wgrad(dz1, g[0], None, P1, 0, B, dws[1], dbs[1], ws[1])
        ops.seqconv_dgrad(dz1, P1, B, convs[1][0], dz0, below=g[0])
        ops.seqconv_wgrad(dz0, st, ac, T, half, B, dws[0], dbs[0], ws[0])

    def torch_tower():
        return tm.tower(b["state"], b["action"])

    def torch_tower_both():
        for c in tm.convs:
            c.zero_grad(set_to_none=True)
        tm.tower(b["state"], b["action"]).backward(dfeat)

    report("tower forward", {"(a) rg_seqconv_forward x2 + rg_ngram_window": tower_kernels, "(b) ngram + conv2d + relu": torch_tower,
                             "(b') again": torch_tower})
    report("tower forward + backward", {"(a) the five entry points": lambda: (tower_kernels(), tower_backward_kernels()),
                                        "(b) torch + autograd": torch_tower_both, "(b') again": torch_tower_both})
    for name, fn in {
        "rg_seqconv_forward layer 0": lambda: ops.seqconv_forward(st, ac, T, half, B, *convs[0], y0),
        "rg_seqconv_forward layer 1": lambda: ops.seqconv_forward(y0, None, P1, 0, B, *convs[1], y1),
        "rg_ngram_window": lambda: ops.ngram_window(y1, T, B, H, ft),
        "rg_ngram_window_backward": lambda: ops.ngram_window_backward(dfeat, T, B, H, dz1, g=g[1]),
        "rg_seqconv_wgrad layer 1": lambda: ops.seqconv_wgrad(dz1, g[0], None, P1, 0, B, dws[1], dbs[1], ws[1]),
        "rg_seqconv_dgrad layer 1": lambda: ops.seqconv_dgrad(dz1, P1, B, convs[1][0], dz0, below=g[0]),
        "rg_seqconv_wgrad layer 0": lambda: ops.seqconv_wgrad(dz0, st, ac, T, half, B, dws[0], dbs[0], ws[0]),
    }.items():
        report(name, {"(a)": fn})
    tower_kernels()
    tower_backward_kernels()
    torch_tower_both()
    assert (ft - torch_tower()).abs().max().item() < 1e-4
    for dw, c in zip(dws, tm.convs):
        err = (dw - c.weight.grad).abs().max().item()
        assert err < 1e-3 * max(1.0, c.weight.grad.abs().max().item()), err

    # ---- the step
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3)

    def torch_step():
        opt.zero_grad()
        tm.loss(b).backward()
        opt.step()

    report("step", {"(a) train_step_native": lambda: tr.train_step_native(batch), "(b) torch modules on the device": torch_step,
                    "(b') again": torch_step}, clock=wall)
    with ops.profile() as prof:
        for _ in range(INNER):
            tr.train_step_native(batch)
    total = sum(rec["ms"] for rec in prof.summary())
    print(f"  launches of a step by entry point ({total / INNER * 1e3:.0f} us of device time a step):")
    by_name = {}
    for rec in prof.summary():
        d = by_name.setdefault(rec["name"], [0.0, 0])
        d[0] += rec["ms"]
        d[1] += rec["calls"]
    for name, (ms, calls) in sorted(by_name.items(), key=lambda kv: -kv[1][0]):
        print(f"  {name:28s} {ms / INNER * 1e3:9.1f} us a step  x{calls // INNER} a step", flush=True)


main()
