"""One SHA-256 per case over the raw bytes of what the recurrent kernels and the world-model trainers write, from seeded inputs
generated on the host: run at two commits, equal digests pair by pair say that the second computes the first's bits.

    python profiles/microbench/recurrent_bits.py                      (the HIP library, on the GPU)
    python profiles/microbench/recurrent_bits.py --emu --max-hidden 65 (the kernel sources on the tests' SIMT interpreter)

  lstm     rg_lstm_forward (saving) then rg_lstm_backward: H in {1, 31, 33, 65, 256}, B in {1, 33}, T in {1, 3}, with and
           without h0 / c0 -> h_all, c_all, gates, dgates, dh0, dc0
  fanout   rg_lstm_fanout_step on tests/test_seq2reward_kernels.py's (H, parents, fanout) grid, from a table and from rows
           -> h, c
  cem      rg_cem_rollout with explicit noise on tests/test_cem_kernels.py's SHAPES -> out and the trace
  mdnrnn   two train_step_native of MDNRNNTrainer, L = 2 -> every parameter and both Adam moments
  s2r      two train_step_native of Seq2RewardTrainer, then get_Q, L = 2, A = 2, multi_steps = 3 -> every parameter, both Adam
           moments and the Q values
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--emu", action="store_true", help="run the kernels on the SIMT interpreter of tests/emu (no GPU)")
ap.add_argument("--max-hidden", type=int, default=256, help="leave out the kernel cases with a larger H")
args = ap.parse_args()
if args.emu:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu_backend

    emu_backend.install()
dev = torch.device("cpu" if args.emu else "cuda")

from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.core.parameters import MDNRNNTrainerParameters, Seq2RewardTrainerParameters  # noqa: E402
from reagent_amd.models.cem_planner import CEMPlannerNetwork  # noqa: E402
from reagent_amd.models.seq2reward_model import Seq2RewardNetwork  # noqa: E402
from reagent_amd.models.world_model import MemoryNetwork  # noqa: E402
from reagent_amd.training.utils import gen_permutations  # noqa: E402
from reagent_amd.training.world_model import MDNRNNTrainer, Seq2RewardTrainer  # noqa: E402
from reagent_amd.training.world_model.seq2reward_trainer import get_Q  # noqa: E402

F32, F64 = torch.float32, torch.float64


def digest(name, tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=dev)


def lstm_cases():
    for H in (1, 31, 33, 65, 256):
        if H > args.max_hidden:
            continue
        for B in (1, 33):
            for T in (1, 3):
                for state in (False, True):
                    g = torch.Generator().manual_seed(1000 * H + 10 * B + T)
                    k = 1.0 / H ** 0.5
                    w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(dev)
                    b_hh = ((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(dev)
                    xproj = torch.randn(T, B, 4 * H, generator=g).to(dev)
                    dh = torch.randn(T, B, H, generator=g).to(dev)
                    h0 = (torch.randn(B, H, generator=g) * 0.5).to(dev) if state else None
                    c0 = torch.randn(B, H, generator=g).to(dev) if state else None
                    h_all, c_all, gates, dgates = nan(T, B, H), nan(T, B, H), nan(T, B, 4 * H), nan(T, B, 4 * H)
                    dh0, dc0 = nan(B, H), nan(B, H)
                    ops.lstm_forward(xproj, w_hh, b_hh, h0, c0, h_all, c_all, gates)
                    ops.lstm_backward(dh, gates, c_all, c0, w_hh, dgates, dh0, dc0)
                    digest(f"lstm H={H} B={B} T={T} state={int(state)}", [h_all, c_all, gates, dgates, dh0, dc0])


def fanout_cases():
    grid = [(H, p, f) for H in (1, 31, 33, 65) for p in (1, 33) for f in (1, 2, 3)] + [(256, 1, 2)]
    for H, parents, fanout in grid:
        if H > args.max_hidden:
            continue
        g = torch.Generator().manual_seed(7000 + 100 * H + 10 * parents + fanout)
        k = 1.0 / H ** 0.5
        n = parents * fanout
        w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(dev)
        b_hh = ((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(dev)
        h_prev = (torch.randn(parents, H, generator=g) * 0.5).to(dev)
        c_prev = torch.randn(parents, H, generator=g).to(dev)
        table = torch.randn(fanout, 4 * H, generator=g).to(dev)
        dense = torch.randn(n, 4 * H, generator=g).to(dev)
        for from_table in (True, False):
            h, c = nan(n, H), nan(n, H)
            ops.lstm_fanout_step(h_prev, c_prev, table if from_table else dense, from_table, w_hh, b_hh, fanout, h, c)
            digest(f"fanout H={H} parents={parents} fanout={fanout} table={int(from_table)}", [h, c])


CEM_SHAPES = {
    "h1_one_row": dict(H=1, L=2, S=1, A=1, G=1, P=1, T=1, te=False),
    "h31_n31": dict(H=31, L=2, S=4, A=3, G=3, P=31, T=5, te=True, nt_bias=1.5),
    "h33_n33_g32_s33": dict(H=33, L=2, S=33, A=1, G=32, P=33, T=5, te=True, nt_bias=1.5),
    "h100_l4_two_models": dict(H=100, L=4, S=4, A=3, G=3, P=33, T=2, M=2, te=True, nt_bias=1.5),
    "h256_l1": dict(H=256, L=1, S=4, A=1, G=1, P=33, T=1, te=False),
    "h8_n65": dict(H=8, L=2, S=4, A=3, G=3, P=65, T=5, te=True, nt_bias=1.5),
}


def cem_cases():
    for name, cfg in CEM_SHAPES.items():
        H, L, S, A, G, P, T = (cfg[k] for k in "HLSAGPT")
        if H > args.max_hidden:
            continue
        M = cfg.get("M", 1)
        torch.manual_seed(0)
        nets = [MemoryNetwork(S, A, H, L, G) for _ in range(M)]
        for net in nets:
            if cfg.get("nt_bias") is not None:
                with torch.no_grad():
                    net.mdnrnn.gmm_linear.bias[-1] = cfg["nt_bias"]
            net.to(dev)
        pl = CEMPlannerNetwork(nets, 2, P, 1, 1, T, S, A, False, cfg["te"], 0.9, action_upper_bounds=np.ones(A),
                               action_lower_bounds=-np.ones(A))
        g = torch.Generator().manual_seed(11)
        init = torch.randn(S, generator=g).to(dev)
        sol = (torch.rand(P, T, A, generator=g) * 2 - 1).to(dev).contiguous()
        noise = dict(u_model=torch.rand(P, generator=g).to(dev), u_mix=torch.rand(T, P, generator=g).to(dev),
                     eps=torch.randn(T, P, S, generator=g).to(dev), u_term=torch.rand(T, P, generator=g).to(dev))
        out = torch.full((P,), -7.0, dtype=F64, device=dev)
        trace = pl._rollout(init, sol, None, out, seed=11, iteration=0, noise=noise, trace=True)
        digest(f"cem {name}", [out, trace])


def moments(opt, params):
    return [opt.state[p][k] for k in ("exp_avg", "exp_avg_sq") for p in params]


def mdnrnn_case():
    T, B, S, A, H, L, G = 3, 33, 5, 3, 33, 2, 3
    torch.manual_seed(0)
    net = MemoryNetwork(state_dim=S, action_dim=A, num_hiddens=H, num_hidden_layers=L, num_gaussians=G).to(dev)
    tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=L, num_gaussians=G, action_dim=A))
    batch = synthetic.to_memory_network_input(synthetic.memory_network_batch(T, B, S, A, seed=1), dev)
    for _ in range(2):
        tr.train_step_native(batch)
    params = list(net.mdnrnn.parameters())
    digest(f"mdnrnn T={T} B={B} S={S} A={A} H={H} L={L} G={G}", params + moments(tr._native_opt, params))


def s2r_case():
    K, B, S, A, H, L = 3, 33, 5, 2, 33, 2
    torch.manual_seed(0)
    net = Seq2RewardNetwork(state_dim=S, action_dim=A, num_hiddens=H, num_hidden_layers=L).to(dev)
    tr = Seq2RewardTrainer(net, Seq2RewardTrainerParameters(multi_steps=K, action_names=[str(i) for i in range(A)],
                                                            step_predict_net_size=16)).to(dev)
    b = synthetic.seq2reward_batch(K, B, S, A, seed=2)
    batch = synthetic.to_seq2reward_input(b, dev)
    for _ in range(2):
        tr.train_step_native(batch)
    q = get_Q(net, b["state"][0].to(dev).contiguous(), gen_permutations(K, A))
    params = list(net.parameters())
    digest(f"s2r K={K} B={B} S={S} A={A} H={H} L={L}", params + moments(tr.native_optimizers()[0], params) + [q])


with torch.no_grad():
    lstm_cases()
    fanout_cases()
    cem_cases()
    mdnrnn_case()
    s2r_case()
if not args.emu:
    torch.cuda.synchronize()
