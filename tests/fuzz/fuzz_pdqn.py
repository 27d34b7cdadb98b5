# python tests/fuzz/fuzz_pdqn.py [seed] [cases]   (FUZZ_ON_GPU=1: the same cases on the real library, tensors built on cuda:0)
# prints one line per case and `bad cases: 0` at the end
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT + "/tests/fuzz")
import torch
import torch.nn.functional as F
import gpu_ops  # FUZZ_ON_GPU=1: the real library on cuda:0 instead of the interpreter
gpu_ops.select()
import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.engine import FusedMLP, make_stack

# the parametric DQN step's three kernels on random shapes: rg_tile_concat against torch.cat (random widths, pitches, base
# offsets: bits), the tiled two-panel fused forward against the two-panel forward on the materialised tiled state (bf16 and
# split-bf16, 256 / 512 wide, M from 1 to beyond a tile: bits), rg_pdqn_head against dqn_trainer_base.py:33-77 +
# parametric_dqn_trainer.py:112-171 under torch autograd (index and next value exact, target 1e-6, dq 1e-8, loss 1e-5
# relative to max(1, loss); fully masked rows are terminal)
dev = "cuda:0" if gpu_ops.ON_GPU else "cpu"
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
cases = int(sys.argv[2]) if len(sys.argv) > 2 else 24
random.seed(seed)
bad = 0
for case in range(cases):
    gen = torch.Generator().manual_seed(seed * 1000 + case)
    # ---- rg_tile_concat
    R, M = random.choice([1, 7, 64, 129, 500]), random.choice([1, 2, 3, 8, 130])
    S, A = random.choice([1, 4, 7, 32, 100]), random.choice([1, 3, 4, 16, 33])
    off = random.choice([0, 0, 1, 4])
    n = (R + M - 1) // M

    def view(rows, cols, pad):
        flat = torch.randn(rows * (cols + pad) + off, generator=gen).to(dev)
        return flat[off:].view(rows, cols + pad)[:, :cols]

    pads = [random.choice([0, 0, 1, 4]) for _ in range(3)]
    x, x2, out = view(n, S, pads[0]), view(R, A, pads[1]), view(R, S + A, pads[2])
    before = out._base.clone()
    ops.tile_concat(x, x2, out, x_tile=M)
    ok_c = torch.equal(out.cpu().view(torch.int32), torch.cat((x.repeat_interleave(M, 0)[:R], x2), 1).cpu().view(torch.int32))
    if pads[2]:
        ok_c &= torch.equal(out._base[off:].view(R, -1)[:, S + A:].cpu(), before[off:].view(R, -1)[:, S + A:].cpu())
    # ---- tiled fused forward
    H, x3 = random.choice([256, 512]), random.random() < 0.5
    Sf, Af, Mf = random.choice([32, 64, 96]), random.choice([1, 5, 8, 32]), random.choice([1, 2, 3, 8, 130])
    Rf = random.choice([1, 63, 64, 65, 128, 200, 257])
    dims = [Sf + Af, H, H, 1]
    ws = [torch.nn.Parameter((torch.randn(o, i, generator=gen) * (1.5 / i ** 0.5)).to(dev)) for i, o in zip(dims, dims[1:])]
    bs = [torch.nn.Parameter((torch.randn(o, generator=gen) * 0.1).to(dev)) for o in dims[1:]]
    st = make_stack(ws, bs, [L.ACT["relu"], L.ACT["relu"], L.ACT["linear"]], L.PREC_BF16X3 if x3 else L.PREC_BF16)
    assert isinstance(st, FusedMLP)
    st.stage_weights(need_transposed=False)
    sdt = random.choice([torch.float32, torch.bfloat16])
    state = torch.randn((Rf + Mf - 1) // Mf, Sf, generator=gen).to(sdt).to(dev)
    cand = torch.randn(Rf, Af, generator=gen).to(dev)
    want, got = torch.zeros(Rf, 1, device=dev), torch.full((Rf, 1), float("nan"), device=dev)
    st.forward(state.repeat_interleave(Mf, 0)[:Rf].contiguous(), want, x2=cand)
    st.forward(state, got, x2=cand, x_tile=Mf)
    ok_f = torch.equal(got.cpu().view(torch.int32), want.cpu().view(torch.int32))
    # ---- rg_pdqn_head
    B, Mh = random.choice([1, 2, 63, 64, 65, 256, 257, 1000]), random.choice([1, 2, 3, 5, 16, 64, 130])
    loss, double_q, maxq = random.choice(["mse", "huber", "bce"]), random.random() < 0.5, random.random() < 0.75
    gamma = 0.0 if loss == "bce" else random.choice([0.0, 0.9, 1.0])
    scale = random.choice([0.3, 3.0, 15.0])
    perm = lambda: torch.stack([torch.randperm(Mh, generator=gen) for _ in range(B)]).float()  # noqa: E731
    qo = ((perm() + torch.rand(B, Mh, generator=gen) * 0.5) / Mh - 0.5) * 2 * scale
    qt = ((perm() + torch.rand(B, Mh, generator=gen) * 0.5) / Mh - 0.5) * 2 * scale
    mask = (torch.rand(B, Mh, generator=gen) > random.choice([0.0, 0.4, 0.9])).float()
    nt = (torch.rand(B, generator=gen) > 0.2).float()
    nt[mask.sum(1) == 0] = 0.0
    ge = torch.randint(1, 5, (B,), generator=gen).float() if random.random() < 0.5 else None
    q, reward = torch.randn(B, generator=gen) * scale, torch.rand(B, generator=gen)
    disc = torch.full((B, 1), gamma) if ge is None else torch.pow(gamma, ge.reshape(B, 1))
    if maxq:
        pen = -1e9 * (1 - mask)
        if double_q:
            idx = torch.max(qo + pen, dim=1, keepdim=True)[1]
            nq = torch.gather(qt + pen, 1, idx)
        else:
            nq, idx = torch.max(qt + pen, dim=1, keepdim=True)
        qt_in = qt.reshape(-1)
    else:
        nq, idx, qt_in = qt[:, :1].clone(), torch.zeros(B, 1, dtype=torch.int64), qt[:, 0].contiguous()
    target = reward.reshape(B, 1) + nt.reshape(B, 1) * disc * nq
    qg = q.reshape(B, 1).clone().requires_grad_(True)
    lv = {"mse": F.mse_loss, "huber": F.smooth_l1_loss, "bce": F.binary_cross_entropy_with_logits}[loss](qg, target)
    lv.backward()
    t = lambda v: None if v is None else v.to(dev)  # noqa: E731
    f = lambda *s: torch.full(s, float("nan")).to(dev)  # noqa: E731
    tg, dq, nqo, parts, lo = f(B), f(B), f(B), f(ops.pdqn_head_partials(B)), f(1)
    io = torch.full((B,), -1, dtype=torch.int64).to(dev)
    ops.pdqn_head(t(q), t(qo.reshape(-1)) if maxq else None, t(qt_in), t(mask) if maxq else None, t(reward), t(nt), gamma, t(ge),
                  double_q, dict(L.LOSS, bce=L.LOSS_BCE_LOGITS)[loss], tg, dq, parts, nqo, io)
    ops.reduce_sum(parts, parts.numel(), 1.0 / B, lo)
    errs = ((tg.cpu() - target.reshape(-1)).abs().max().item(), (dq.cpu() - qg.grad.reshape(-1)).abs().max().item(),
            abs(lo.item() - lv.item()) / max(1.0, abs(lv.item())))
    ok_h = torch.equal(io.cpu(), idx.reshape(-1)) and torch.equal(nqo.cpu(), nq.reshape(-1)) and errs[0] <= 1e-6 \
        and errs[1] <= 1e-8 and errs[2] <= 1e-5
    ok = ok_c and ok_f and ok_h
    bad += not ok
    print(f"case {case}: concat R={R} M={M} S={S} A={A} pads={pads} off={off} {'ok' if ok_c else 'BAD'} | tiled H={H} "
          f"x3={int(x3)} R={Rf} M={Mf} S={Sf} A={Af} {'ok' if ok_f else 'BAD'} | head B={B} M={Mh} {loss} dq={int(double_q)} "
          f"maxq={int(maxq)} g={gamma} errs=({errs[0]:.1e}, {errs[1]:.1e}, {errs[2]:.1e}) {'ok' if ok_h else 'BAD'}")
print("bad cases:", bad)
