"""rg_fi_sweep (csrc/feature_importance.hip) on the GPU box at 128 features (one normalized column each), the stack
128-512-512-512-16 (relu), B = 4096, pred = max_a Q:
python profiles/microbench/feature_importance.py

  (n) the native sweep: the layer-0 rg_fc_forward (RG_ACT_LINEAR), the base forward, rg_fi_sweep over the 128 variants,
      rg_fi_finish; and rg_fi_sweep alone;
  (a) F + 1 calls of the existing per-layer PREC_F32 forward on materialised perturbed batches (clone, one permuted column,
      four rg_fc_forward launches, max, mean |delta| as torch ops on the device);
  (b) the same statement as torch modules on the device (nn.Linear + ReLU in fp32).
Device events, medians of 12 rounds after a warm-up of each; the permutations are drawn once and shared.  The three results
are compared before anything is timed.  No speed is promised: the numbers go to profiles/NOTES_r36.md."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import reagent_amd._lib as L  # noqa: E402
from reagent_amd import ops  # noqa: E402

dev = torch.device("cuda")
DIMS, B, ROUNDS = [128, 512, 512, 512, 16], 4096, 12
ACTS = ["relu", "relu", "relu", "linear"]
med = statistics.median


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)  # ms


def main():
    g = torch.Generator().manual_seed(0)
    F, A = DIMS[0], DIMS[-1]
    Ws = [(torch.randn(o, i, generator=g) * i ** -0.5).to(dev) for i, o in zip(DIMS, DIMS[1:])]
    bs = [(0.1 * torch.randn(o, generator=g)).to(dev) for o in DIMS[1:]]
    x = torch.randn(B, F, generator=g).to(dev)
    perm = torch.stack([torch.randperm(B, generator=g) for _ in range(F)]).to(dev)
    perm32 = perm.to(torch.int32)
    blocks = torch.tensor([(c, c + 1) for c in range(F)], dtype=torch.int32, device=dev)
    acts = [L.ACT[a] for a in ACTS]
    partials = torch.empty(ops.fi_partials(B, F, A, 0), dtype=torch.float64, device=dev)
    z0, imp = torch.empty(B, DIMS[1], device=dev), torch.empty(F, 1, device=dev)

    def layers(h):
        for W, b, a in zip(Ws, bs, acts):
            y = torch.empty(h.shape[0], W.shape[0], device=dev)
            ops.fc_forward(h, W, b, a, L.PREC_F32, y32=y)
            h = y
        return h

    state = {}

    def front():
        ops.fc_forward(x, Ws[0], bs[0], L.ACT["linear"], L.PREC_F32, y32=z0)
        state["q"] = layers(x)

    def sweep():
        ops.fi_sweep(x, z0, perm32, blocks, Ws, bs, acts, state["q"], None, 0, 1, partials)

    def native():
        front()
        sweep()
        ops.fi_finish(partials, B, imp)
        return imp[:, 0]

    def loop(forward):
        base = forward(x).max(dim=1)[0]
        out = []
        for c in range(F):
            xv = x.clone()
            xv[:, c] = x[perm[c], c]
            out.append((forward(xv).max(dim=1)[0] - base).abs().mean())
        return torch.stack(out)

    mods = []
    for W, b, a in zip(Ws, bs, ACTS):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dev)
        with torch.no_grad():
            lin.weight.copy_(W), lin.bias.copy_(b)
        mods += [lin] + ([torch.nn.ReLU()] if a == "relu" else [])
    seq = torch.nn.Sequential(*mods)

    with torch.no_grad():
        rn, ra, rb = native().clone(), loop(layers), loop(seq)
        print(f"agreement: max |native - (a)| {(rn - ra).abs().max().item():.3e}, max |native - (b)| "
              f"{(rn - rb).abs().max().item():.3e}, importances {rn.min().item():.3e} .. {rn.max().item():.3e}", flush=True)
        flop = 2.0 * F * B * sum(i * o for i, o in zip(DIMS[1:], DIMS[2:]))
        for name, fn in (("(n) native: front + rg_fi_sweep + rg_fi_finish", native), ("    rg_fi_sweep alone", sweep),
                         ("(a) F + 1 per-layer PREC_F32 forwards on materialised batches", lambda: loop(layers)),
                         ("(b) the same statement as torch modules", lambda: loop(seq))):
            fn()
            torch.cuda.synchronize()
            t = [timed(fn) for _ in range(ROUNDS)]
            extra = f", {flop / med(t) / 1e9:.1f} TFLOP/s of the tail's {flop:.3g} FLOP" if "alone" in name else ""
            print(f"{name}: {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f}){extra}", flush=True)


if __name__ == "__main__":
    main()
