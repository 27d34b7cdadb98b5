"""The synthetic-reward step on the GPU box: B = 4 096, T = 10, S = 128, A = 32 (S + A = 160), hidden [256, 128], H = 128.
python profiles/microbench/synthetic_reward_step.py

  ngram : (a) rg_ngram_concat, context_size 3 and 5
          (b) the reference's ngram() statement (shifted copies, tiles of the padding, two cats) on the device
  head  : (a) rg_step_reward_head on the trunk's output [T, B, 128] (its three launches), MSE and BCE
          (b) the torch operations it replaces — Linear(128, 1), the activation, _gen_mask, the masked sum, the loss wrapper —
              with autograd's backward
  step  : (a) RewardNetTrainer.train_step_native of the single-step, n-gram (3) and sequence (one layer) nets, wall clock
          (b) the same step as torch modules on the device: the reference's layers, backward, torch.optim.Adam

timed with device events after warm-up (the steps: wall clock over a synchronise), in one process, the candidates
alternating inside every round, medians of 12 rounds; every (b) is run twice a round and read against its own repeat (b')."""
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, ".")
from reagent_amd import _lib as L  # noqa: E402
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.models import synthetic_reward as M  # noqa: E402
from reagent_amd.training import LossFunction, RewardNetTrainer  # noqa: E402

dev = torch.device("cuda")
B, T, S, A, SIZES, H = 4096, 10, 128, 32, [256, 128], 128
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


def head_lines(h, fc, act, valid_step, target, bce):
    """synthetic_reward.py:245-266 behind the last linear, reward_network_trainer.py:43-64"""
    output = act(fc(h)).squeeze(2).transpose(0, 1)
    mask = (torch.arange(T, device=h.device).repeat(B, 1) >= (T - valid_step)).float()
    pred = (output * mask).sum(dim=1, keepdim=True)
    if bce:
        return torch.mean(nn.BCELoss(reduction="none")(pred / valid_step, target / valid_step))
    return torch.mean(nn.MSELoss(reduction="none")(pred, target))


class TorchNet(nn.Module):
    """the reference's three nets as torch runs them"""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        F = (S + A) * (3 if kind == "ngram" else 1)
        if kind == "sequence":
            self.lstm, self.fc_out = nn.LSTM(S + A, H), nn.Linear(H, 1)
        else:
            dims = [F] + SIZES
            self.trunk = nn.Sequential(*[m for i, o in zip(dims, dims[1:]) for m in (nn.Linear(i, o), nn.ReLU())])
            self.fc_out = nn.Linear(SIZES[-1], 1)
        self.pad = torch.zeros(1, 1, S + A, device=dev)

    def loss(self, b):
        x = torch.cat((b["state"], b["action"]), dim=-1)
        if self.kind == "ngram":
            x = M.ngram(x, 3, self.pad)
        h = self.lstm(x)[0] if self.kind == "sequence" else self.trunk(x)
        return head_lines(h, self.fc_out, nn.LeakyReLU(), b["valid_step"], b["reward"], False)


def main():
    f = dict(dtype=torch.float32, device=dev)
    b = {k: v.to(dev) for k, v in synthetic.synthetic_reward_batch(T, B, S, A, seed=1).items()}
    batch = synthetic.to_synthetic_reward_input(b)
    pad = torch.zeros(1, 1, S + A, **f)
    for n in (3, 5):
        out = torch.empty(T, B, (S + A) * n, **f)
        ref = lambda: M.ngram(torch.cat((b["state"], b["action"]), dim=-1), n, pad)  # noqa: E731
        report(f"ngram n={n} ({out.numel() * 4 / 1e6:.0f} MB written)",
               {"(a) rg_ngram_concat": lambda: ops.ngram_concat(b["state"], b["action"], n, out), "(b) torch ngram": ref,
                "(b') again": ref})
        assert torch.equal(out, ref())
    # the head
    P = SIZES[-1]
    g = torch.Generator().manual_seed(2)
    h = torch.tanh(torch.randn(T, B, P, generator=g)).abs().to(dev)
    fc = nn.Linear(P, 1).to(dev)
    with torch.no_grad():
        fc.weight.copy_(torch.rand(1, P, generator=g) * (0.45 / P))
        fc.bias.fill_(0.03)
    w, bias = fc.weight.detach().view(-1), fc.bias.detach()
    v = b["valid_step"].flatten().contiguous()
    binary = (torch.rand(B, 1, generator=g).to(dev) < 0.5).float() * b["valid_step"]
    output, mask, pred, loss = torch.empty(B, T, **f), torch.empty(B, T, **f), torch.empty(B, **f), torch.empty(1, **f)
    n_kept = torch.empty(1, dtype=torch.int32, device=dev)
    dh, dw, db = torch.empty(T, B, P, **f), torch.empty(P, **f), torch.empty(1, **f)
    ws = torch.empty(ops.step_reward_head_workspace(T, B, P), dtype=torch.float64, device=dev)
    for name, act, target, module in (("MSE_Loss", "leaky_relu", b["reward"], nn.LeakyReLU()), ("BCE_Loss", "sigmoid", binary, nn.Sigmoid())):
        tgt = target.view(B).contiguous()

        def kernel():
            ops.step_reward_head(h, w, bias, L.ACT[act], v, output, mask, pred, target=tgt, loss_type=L.SRW_LOSS[name], loss=loss,
                                 n_kept=n_kept, dh=dh, dw=dw, dbias=db, workspace=ws)

        def lines():
            hh = h.detach().requires_grad_()
            fc.zero_grad()
            head_lines(hh, fc, module, b["valid_step"], target, name == "BCE_Loss").backward()

        report(f"head {name} T*B={T * B} P={P}", {"(a) rg_step_reward_head": kernel, "(b) torch forward + autograd backward": lines,
                                                   "(b') again": lines})
    # the steps
    nets = {
        "single": M.SingleStepSyntheticRewardNet(S, A, SIZES, ["relu", "relu"], "leaky_relu"),
        "ngram": M.NGramFullyConnectedNetwork(S, A, SIZES, ["relu", "relu"], "leaky_relu", 3),
        "sequence": M.SequenceSyntheticRewardNet(S, A, H, 1, False, "leaky_relu"),
    }
    for kind, net in nets.items():
        tr = RewardNetTrainer(M.SyntheticRewardNet(net).to(dev), loss_type=LossFunction.MSE).to(dev)
        tm = TorchNet(kind).to(dev)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-3)

        def torch_step():
            opt.zero_grad()
            tm.loss(b).backward()
            opt.step()

        report(f"step {kind}", {"(a) train_step_native": lambda: tr.train_step_native(batch), "(b) torch modules on the device": torch_step,
                                "(b') again": torch_step}, clock=wall)
        with ops.profile() as prof:
            for _ in range(INNER):
                tr.train_step_native(batch)
        for rec in prof.summary()[:8]:
            print(f"  {rec['name']:22s} {rec['meta']}  {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // INNER} a step",
                  flush=True)


main()
