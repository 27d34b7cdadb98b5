"""The row-major weight gradient on the GPU box.
python profiles/microbench/fc_wgrad_rows.py

  call : (a) rg_fc_wgrad_rows on the row-major operands
         (b) the path it replaces: two rg_transpose_cast, rg_fc_wgrad, its reduces (lstm_stack.wgrad_rows below its threshold)
         (c) x.t() @ dz and dz.sum(0) in torch
         rows 40 960 at (out, in) = (128, 128), (512, 160), (512, 128), (384, 128); rows 32 to 16 384 in powers of two at
         (128, 128), where lstm_stack.WGRAD_ROWS_MIN is read from
  step : RewardNetTrainer.train_step_native of the two-layer TransformerSyntheticRewardNet (B = 4 096, T = 10, d_model 128, 2
         heads), (a) with wgrad_rows' threshold as committed, (b) with the threshold out of reach: the launches of the commit
         before, in the same process

device events after warm-up (the step: wall clock over a synchronise), the candidates alternating inside every round, medians
of 12 rounds with min and max; (a) is checked against (c) before it is timed."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from reagent_amd import ops, synthetic  # noqa: E402
from reagent_amd.models import SyntheticRewardNet, TransformerSyntheticRewardNet, lstm_stack  # noqa: E402
from reagent_amd.training import LossFunction, RewardNetTrainer  # noqa: E402

dev = torch.device("cuda")
ROUNDS, INNER = 12, 10
SHAPES = [(40960, 128, 128), (40960, 512, 160), (40960, 512, 128), (40960, 384, 128)] + [(32 << k, 128, 128) for k in range(10)]
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


def with_threshold(rows_min, fn):
    def run():
        keep, lstm_stack.WGRAD_ROWS_MIN = lstm_stack.WGRAD_ROWS_MIN, rows_min
        try:
            fn()
        finally:
            lstm_stack.WGRAD_ROWS_MIN = keep
    return run


def main():
    f = dict(dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(1)
    for rows, out_f, in_f in SHAPES:
        dz, x = torch.randn(rows, out_f, generator=g).to(dev), torch.randn(rows, in_f, generator=g).to(dev)
        dw, db, dw_old, db_old = torch.empty(out_f, in_f, **f), torch.empty(out_f, **f), torch.empty(out_f, in_f, **f), torch.empty(out_f, **f)
        nbytes = ops.fc_wgrad_rows_workspace_bytes(out_f, in_f, rows)
        ws = torch.empty(max(nbytes // 4, 1), **f)
        new = lambda: ops.fc_wgrad_rows(dz, x, dw, db, ws)  # noqa: E731
        old = with_threshold(1 << 30, lambda: lstm_stack.wgrad_rows(dz, x, dw_old, db_old))
        new(), old()
        ref, S = dz.double().t() @ x.double(), dz.double().abs().t() @ x.double().abs()
        bound = (2 * rows + 4) * 2.0 ** -24 * S
        assert bool(((dw.double() - ref).abs() <= bound).all()) and bool(((dw_old.double() - ref).abs() <= bound).all())
        assert bool(((db.double() - dz.double().sum(0)).abs() <= (2 * rows + 4) * 2.0 ** -24 * dz.double().abs().sum(0)).all())
        moved = (rows * (out_f + in_f) + out_f * in_f) * 4
        report(f"rows={rows} out={out_f} in={in_f} ({moved / 1e6:.1f} MB of operands and dw, {nbytes / 1e6:.1f} MB of partials)",
               {"(a) rg_fc_wgrad_rows": new, "(b) 2 rg_transpose_cast + rg_fc_wgrad": old,
                "(c) torch dz.t() @ x, dz.sum(0)": lambda: (dz.t() @ x, dz.sum(0))})
    # the step
    B, T, S_, A, E, NH, FD, LAYERS = 4096, 10, 128, 32, 128, 2, 128, 2
    batch = synthetic.to_synthetic_reward_input({k: v.to(dev) for k, v in synthetic.synthetic_reward_batch(T, B, S_, A, seed=1).items()})
    net = TransformerSyntheticRewardNet(S_, A, E, nhead=NH, num_encoder_layers=LAYERS, dim_feedforward=FD, max_len=T)
    tr = RewardNetTrainer(SyntheticRewardNet(net).to(dev), loss_type=LossFunction.MSE).to(dev)
    step = lambda: tr.train_step_native(batch)  # noqa: E731
    report(f"transformer reward step B={B} T={T} d_model={E} nhead={NH} (WGRAD_ROWS_MIN = {lstm_stack.WGRAD_ROWS_MIN})",
           {"(a) as committed": step, "(b) threshold out of reach": with_threshold(1 << 30, step), "(a') again": step}, clock=wall)
    for name, fn in (("as committed", step), ("threshold out of reach", with_threshold(1 << 30, step))):
        with ops.profile() as prof:
            for _ in range(INNER):
                fn()
        by_name = {}
        for rec in prof.summary():
            d = by_name.setdefault(rec["name"], [0.0, 0])
            d[0] += rec["ms"]
            d[1] += rec["calls"]
        print(f"  {name}: {sum(v[0] for v in by_name.values()) / INNER * 1e3:.0f} us of device time a step")
        for k, (ms, calls) in sorted(by_name.items(), key=lambda kv: -kv[1][0])[:6]:
            print(f"    {k:28s} {ms / INNER * 1e3:9.1f} us a step  x{calls // INNER} a step", flush=True)


main()
