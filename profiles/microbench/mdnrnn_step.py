"""The world-model (MDN-RNN) step on the GPU box: T = 8, S = 128, A = 32, H = 128, L = 2, G = 5 at B = 65 536 and B = 1 024.
python profiles/microbench/mdnrnn_step.py

  lstm  : (a) rg_lstm_forward (saving) and rg_lstm_backward of one layer on xproj [T, B, 4H]
          (b) torch.nn.LSTM on the same device with W_ih read as given: forward, and forward + autograd backward
  head  : (a) rg_mdn_head (its main and finishing launch)
          (b) the torch operations of MDNRNN.forward's split and MDNRNNTrainer.get_loss with autograd's backward
  step  : (a) MDNRNNTrainer.train_step_native, wall clock over a synchronise
          (b) the same step as torch modules on the device: nn.LSTM, nn.Linear, get_loss's lines, backward, torch.optim.Adam
          (c) (b) on the host's cores, fp32 (what the reference runs), at B = 1 024 only

timed with device events after warm-up, in one process, the candidates alternating inside every round, medians of 12
rounds; every (b) is run twice a round and read against its own repeat (b')."""
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, ".")
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.core.parameters import MDNRNNTrainerParameters  # noqa: E402
from reagent_amd.models.world_model import MemoryNetwork  # noqa: E402
from reagent_amd.training.world_model import MDNRNNTrainer  # noqa: E402

dev = torch.device("cuda")
T, S, A, H, NL, G = 8, 128, 32, 128, 2, 5
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
    """fns: name -> callable; every one warmed up, then alternated inside each round"""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn, inner))
    print(what + ": " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)


class TorchModel(nn.Module):
    """the reference's MDNRNN and get_loss as torch runs them"""

    def __init__(self):
        super().__init__()
        self.rnn = nn.LSTM(input_size=S + A, hidden_size=H, num_layers=NL)
        self.gmm_linear = nn.Linear(H, (2 * S + 1) * G + 2)

    def loss(self, b):
        z = self.gmm_linear(self.rnn(torch.cat([b["action"], b["state"]], dim=-1))[0])
        return head_lines(z, b)


def head_lines(z, b):
    st, lead = G * S, z.shape[:-1]
    mus, sigmas = z[..., :st].reshape(*lead, G, S), torch.exp(z[..., st:2 * st].reshape(*lead, G, S))
    logpi = F.log_softmax(z[..., 2 * st:2 * st + G], dim=-1)
    lp = logpi + torch.distributions.Normal(mus, sigmas).log_prob(b["next_state"].unsqueeze(-2)).sum(-1)
    m = lp.max(dim=-1, keepdim=True)[0]
    gmm = -(m.squeeze(-1) + torch.log(torch.exp(lp - m).sum(-1))).mean()
    bce = F.binary_cross_entropy_with_logits(z[..., -1], b["not_terminal"])
    mse = F.mse_loss(z[..., -2], b["reward"])
    return gmm / (S + 2) + bce + mse


def run(B):
    inner = 3 if B > 4096 else 10
    N = T * B
    print(f"---- B = {B}: {(B + 31) // 32} row tiles of 32 for the 256 CUs ----", flush=True)
    g = torch.Generator().manual_seed(B)
    f = dict(dtype=torch.float32, device=dev)
    # one layer
    xproj = torch.randn(T, B, 4 * H, generator=g).to(dev)
    w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(dev)
    b_hh = ((torch.rand(4 * H, generator=g) * 2 - 1) / H ** 0.5).to(dev)
    dh = torch.randn(T, B, H, generator=g).to(dev)
    h_all, c_all, gates, dgates = torch.empty(T, B, H, **f), torch.empty(T, B, H, **f), torch.empty(T, B, 4 * H, **f), \
        torch.empty(T, B, 4 * H, **f)
    layer = nn.LSTM(input_size=4 * H, hidden_size=H).to(dev)
    with torch.no_grad():
        layer.weight_hh_l0.copy_(w_hh)
        layer.bias_hh_l0.copy_(b_hh)

    def lstm_fwd():
        ops.lstm_forward(xproj, w_hh, b_hh, None, None, h_all, c_all, gates)

    def lstm_bwd():
        ops.lstm_backward(dh, gates, c_all, None, w_hh, dgates)

    def torch_fwd():
        with torch.no_grad():
            layer(xproj)

    def torch_fwd_bwd():
        x = xproj.detach().requires_grad_()
        (layer(x)[0] * dh).sum().backward()

    lstm_fwd()
    report(f"lstm layer B={B}", {"(a) rg_lstm_forward": lstm_fwd, "(a) rg_lstm_backward": lstm_bwd,
                                 "(b) nn.LSTM forward (incl. its 4H x 4H input product)": torch_fwd, "(b') again": torch_fwd,
                                 "(b) nn.LSTM forward + backward": torch_fwd_bwd, "(b') again ": torch_fwd_bwd}, inner)
    del xproj, dh, h_all, c_all, gates, dgates
    # the head
    W = (2 * S + 1) * G + 2
    z = torch.randn(N, W, generator=g).to(dev)
    b = {k: (v.to(dev) if v is not None else None) for k, v in synthetic.memory_network_batch(T, B, S, A, seed=1).items()}
    flat = dict(next_state=b["next_state"].reshape(N, S), reward=b["reward"].reshape(N), not_terminal=b["not_terminal"].reshape(N))
    dz, losses = torch.empty(N, W, **f), torch.empty(4, **f)
    partials = torch.empty(3 * ops.mdn_head_partials(N), dtype=torch.float64, device=dev)

    def head_kernel():
        ops.mdn_head(z, flat["next_state"], flat["reward"], flat["not_terminal"], G, (1.0, 1.0, 1.0), True, 0, dz, partials, losses)

    def head_torch():
        zz = z.detach().requires_grad_()
        head_lines(zz, flat).backward()

    report(f"head N={N}", {"(a) rg_mdn_head": head_kernel, "(b) torch forward + autograd backward": head_torch,
                           "(b') again": head_torch}, inner)
    del z, dz
    # the step
    torch.manual_seed(0)
    net = MemoryNetwork(state_dim=S, action_dim=A, num_hiddens=H, num_hidden_layers=NL, num_gaussians=G).to(dev)
    tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=NL, num_gaussians=G, action_dim=A))
    batch = synthetic.to_memory_network_input(synthetic.memory_network_batch(T, B, S, A, seed=1), dev)
    tm = TorchModel().to(dev)
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3)

    def torch_step():
        opt.zero_grad()
        tm.loss(b).backward()
        opt.step()

    for _ in range(3):
        tr.train_step_native(batch)
        torch_step()
    torch.cuda.synchronize()
    walls = {"(a) train_step_native": [], "(b) torch modules on the device": [], "(b') again": []}
    fns = [lambda: tr.train_step_native(batch), torch_step, torch_step]
    for _ in range(ROUNDS):
        for k, fn in zip(walls, fns):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            walls[k].append((time.perf_counter() - t0) / inner * 1e6)
    print(f"step B={B}: " + "   ".join(f"{k} {med(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})" for k, v in walls.items()),
          flush=True)
    with ops.profile() as prof:
        for _ in range(inner):
            tr.train_step_native(batch)
    for rec in prof.summary()[:10]:
        print(f"  {rec['name']:20s} {rec['meta']}  {rec['ms'] / rec['calls'] * 1e3:9.1f} us a call  x{rec['calls'] // inner} a step",
              flush=True)
    if B <= 1024:
        cm = TorchModel()
        copt = torch.optim.Adam(cm.parameters(), lr=1e-3)
        cb = {k: (v.cpu() if v is not None else None) for k, v in b.items()}
        ts = []
        for i in range(5):
            t0 = time.perf_counter()
            copt.zero_grad()
            cm.loss(cb).backward()
            copt.step()
            ts.append((time.perf_counter() - t0) * 1e6)
        print(f"step B={B}: (c) torch modules on the host's cores ({torch.get_num_threads()} threads) {med(ts[1:]):.1f} us "
              f"(min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f})", flush=True)


for B in (1024, 65536):
    run(B)
