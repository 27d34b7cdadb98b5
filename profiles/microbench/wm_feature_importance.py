"""The feature-importance sweep on the GPU box.
python profiles/microbench/wm_feature_importance.py

  (a) FeatureImportanceEvaluator.evaluate: rg_wm_feature_fill, one base projection, rg_lstm_forward_ablate and the layers
      above over V x B virtual rows in chunks, rg_wm_mdn_losses, one read
  (b) the route before the sweep existed (the reference's evaluate on this package's get_loss): F + 1 get_loss calls on
      cloned, overwritten batches with a host read after each, the replacement values by torch on the device

B = 4 096, T = 10, S + A = 160 (S = 120 in 30 blocks of 4, A = 40 in 10 blocks of 4: F = 40), H = 128, G = 5, one and two
layers.  Wall clock over a call that ends in a host read, after warm-up, the two alternating inside every round, medians of 7
rounds with min and max; (a) is checked against (b) before it is timed."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.core import types as rlt  # noqa: E402
from reagent_amd.core.parameters import MDNRNNTrainerParameters  # noqa: E402
from reagent_amd.evaluation.world_model_evaluator import FeatureImportanceEvaluator  # noqa: E402
from reagent_amd.models.world_model import MemoryNetwork  # noqa: E402
from reagent_amd.training.world_model import MDNRNNTrainer  # noqa: E402

dev = torch.device("cuda")
B, T, S, A, H, G, WIDTH, ROUNDS = 4096, 10, 120, 40, 128, 5, 4, 7
S_STARTS, A_STARTS = list(range(0, S, WIDTH)), list(range(0, A, WIDTH))


def materialised(tr, batch):
    """the reference's evaluate (world_model_evaluator.py:63-157) on get_loss: a pass and a host read per feature"""
    def value(cols):
        counts = cols.sum(dim=0)
        first = int((counts == torch.median(counts)).nonzero()[0])
        return (torch.arange(cols.shape[1], device=cols.device) == first).float()

    with torch.no_grad():
        base = tr.get_loss(batch, state_dim=S)["loss"].cpu().item()
        out = []
        for key, dim, starts in (("action", A, A_STARTS), ("state", S, S_STARTS)):
            for s, e in zip(starts, starts[1:] + [dim]):
                rows = getattr(batch, key).float_features.reshape(T * B, dim).clone()
                rows[:, s:e] = value(rows[:, s:e])
                new = rlt.MemoryNetworkInput(**{**{f: getattr(batch, f) for f in ("state", "action", "next_state", "reward",
                                                                                  "time_diff", "not_terminal", "step")},
                                                key: rlt.FeatureData(float_features=rows.view(T, B, dim))})
                out.append(tr.get_loss(new, state_dim=S)["loss"].cpu().item() - base)
    return torch.tensor(out)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # (ends in a host read)
    return (time.perf_counter() - t0) * 1e3


def main():
    for layers in (1, 2):
        torch.manual_seed(0)
        net = MemoryNetwork(state_dim=S, action_dim=A, num_hiddens=H, num_hidden_layers=layers, num_gaussians=G).to(dev)
        tr = MDNRNNTrainer(net, MDNRNNTrainerParameters(hidden_size=H, num_hidden_layers=layers, num_gaussians=G, action_dim=A))
        b = synthetic.memory_network_batch(T, B, S, A, seed=1)
        for key, dim in (("state", S), ("action", A)):  # every block a one-hot enum of WIDTH columns
            pick = torch.randint(0, WIDTH, (T, B, dim // WIDTH, 1), generator=torch.Generator().manual_seed(dim))
            b[key] = (pick == torch.arange(WIDTH)).float().view(T, B, dim)
        batch = synthetic.to_memory_network_input(b, dev)
        ev = FeatureImportanceEvaluator(tr, False, len(S_STARTS), len(A_STARTS), A_STARTS, S_STARTS)
        fns = {"(a) sweep": lambda: ev.evaluate(batch), "(b) F + 1 get_loss": lambda: materialised(tr, batch)}
        got, ref = torch.as_tensor(fns["(a) sweep"]()["feature_loss_increase"]), fns["(b) F + 1 get_loss"]()
        err = (got - ref).abs().max().item()
        print(f"layers={layers}: largest |sweep - materialised| {err:.2e} (largest increase {ref.abs().max().item():.3e})", flush=True)
        assert err <= 1e-5 * max(1.0, ref.abs().max().item())
        t = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t[k].append(wall(fn))
        print(f"layers={layers} B={B} T={T} S+A={S + A} H={H} F={len(S_STARTS) + len(A_STARTS)}: " + "   ".join(
            f"{k} {statistics.median(v):.1f} ms (min {min(v):.1f}, max {max(v):.1f})" for k, v in t.items()), flush=True)
        with ops.profile() as prof:
            ev.evaluate(batch)
        for rec in prof.summary()[:5]:
            print(f"    {rec['name']:26s} {rec['ms']:9.2f} ms  x{rec['calls']}  {rec['meta']}", flush=True)


main()
