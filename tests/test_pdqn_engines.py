"""ParametricDQNTrainer beyond the fp32 fixtures: the fused tiled path end to end against the same trainer on the
rg_tile_concat path, data parallel on two ranks, and the register / scratch budget of the new kernels."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _trainer(dev, precision, S=64, A=8, H=256, reward=False, **rl):
    import reagent_amd._lib as L
    from reagent_amd.core.parameters import RLParameters
    from reagent_amd.models import FullyConnectedCritic, set_default_precision
    from reagent_amd.optimizer import Optimizer__Union
    from reagent_amd.training import ParametricDQNTrainer

    torch.manual_seed(0)
    set_default_precision(precision)
    try:
        q = FullyConnectedCritic(S, A, [H, H], ["relu", "relu"])
        r = FullyConnectedCritic(S, A, [H, H], ["relu", "relu"]) if reward else None
    finally:
        set_default_precision(L.PREC_F32)
    rl = dict(dict(gamma=0.9, target_update_rate=0.1, maxq_learning=True, q_network_loss="huber"), **rl)
    return ParametricDQNTrainer(q.to(dev), q.get_target_network().to(dev), r.to(dev) if r is not None else None,
                                rl=RLParameters(**rl), optimizer=Optimizer__Union.default(lr=0.001)).to(dev)


def _run(tr, batches, dev):
    from reagent_amd import synthetic

    out = []
    for d in batches:
        r = tr.train_step_native(synthetic.to_parametric_input(d, dev))
        out.append((r["td_loss"].detach().cpu().clone(), tr._next_idx.cpu().clone()))
    return out, [p.detach().cpu().clone() for p in tr.parameters()]


def test_fused_tiled_path_against_the_tile_concat_path(backend, monkeypatch):
    """a 256-wide split-bf16 critic with state_dim = 64, three native steps: the step that reads the tiled next state in
    place (rg_mlp_desc.x_tile) against the same trainer forced onto rg_tile_concat + the one-panel forward.  The selected
    candidates are identical; loss and parameters are held to the bound of split-bf16 critics' gradients in
    tests/test_full_size.py (STEP_BOUND[("c4", "bf16x3")]["grad"], (max-abs over the largest entry, norm-relative), the
    bound tests/test_full_size_bounds.py shows to flag a wrong tile) with that file's comparison.  (Both paths hand the
    kernels the same fp32 values, so the expected difference is none at all.)  Two runs of the same steps are bit-identical."""
    import reagent_amd._lib as L
    import test_full_size as FS
    from reagent_amd import synthetic
    from reagent_amd.engine import FusedMLP
    from reagent_amd.training import ParametricDQNTrainer

    dev = backend.device
    S, A, M, B = 64, 8, 5, 96
    batches = [synthetic.parametric_batch(B, S, A, M, seed=20 + s, p_impossible=0.3, n_fully_masked=2) for s in range(3)]
    tr = _trainer(dev, L.PREC_BF16X3)
    assert isinstance(tr.q_network.fc.stack(), FusedMLP) and tr.q_network.fc.stack().x3
    calls = []
    real = FusedMLP.forward

    def spy(self, xc, out32, save=False, x2=None, rowmap=None, x_tile=1):
        calls.append((x2 is not None, x_tile))
        return real(self, xc, out32, save=save, x2=x2, rowmap=rowmap, x_tile=x_tile)

    monkeypatch.setattr(FusedMLP, "forward", spy)
    fused, p_fused = _run(tr, batches, dev)
    assert calls[:3] == [(True, M), (True, M), (True, 1)]  # online + target on the tiled rows, then q(s, a): all in place
    again, p_again = _run(_trainer(dev, L.PREC_BF16X3), batches, dev)
    for (l0, i0), (l1, i1) in zip(fused, again):
        assert torch.equal(l0, l1) and torch.equal(i0, i1)
    assert all(torch.equal(a, b) for a, b in zip(p_fused, p_again))
    calls.clear()
    monkeypatch.setattr(ParametricDQNTrainer, "_reads_panels", staticmethod(lambda stack, state_dim: False))
    cat, p_cat = _run(_trainer(dev, L.PREC_BF16X3), batches, dev)
    assert calls and all(c == (False, 1) for c in calls)
    bound = FS.STEP_BOUND[("c4", "bf16x3")]["grad"]
    for (l0, i0), (l1, i1) in zip(fused, cat):
        assert torch.equal(i0, i1)
        assert abs(l0.item() - l1.item()) <= bound[0] * abs(l1.item())
    assert not FS.flagged(p_fused, p_cat, bound), FS.worst(p_fused, p_cat)


@pytest.mark.parametrize("precision,S", [("bf16", 64), ("bf16", 40), ("bf16x3", 40)])
def test_fused_critics_train_on_either_input_path(backend, precision, S):
    """bf16 / split-bf16 critics with a reward network: a state width that is a multiple of 32 reads panels, another one
    goes through rg_tile_concat; the loss falls over a few steps on a repeated batch"""
    import reagent_amd._lib as L
    from reagent_amd import synthetic

    dev = backend.device
    tr = _trainer(dev, dict(bf16=L.PREC_BF16, bf16x3=L.PREC_BF16X3)[precision], S=S, reward=True, maxq_learning=False,
                  q_network_loss="mse")
    b = synthetic.to_parametric_input(synthetic.parametric_batch(64, S, 8, 3, seed=1), dev)
    first = {k: v.item() for k, v in tr.train_step_native(b).items()}
    for _ in range(4):
        last = {k: v.item() for k, v in tr.train_step_native(b).items()}
    assert last["td_loss"] < first["td_loss"] and last["reward_loss"] < first["reward_loss"]


def _dp_build():
    import reagent_amd._lib as L

    return _trainer("cpu", L.PREC_F32, S=6, A=3, H=16, reward=True)


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu_backend

    emu_backend.install()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from reagent_amd import synthetic

    B, M = 64, 4
    full = synthetic.parametric_batch(B, 6, 3, M, seed=5, p_impossible=0.2)
    per = B // world
    half = {k: v[rank * per * (M if v.shape[0] == B * M else 1):(rank + 1) * per * (M if v.shape[0] == B * M else 1)].contiguous()
            for k, v in full.items()}
    tr = _dp_build().enable_data_parallel()
    for _ in range(2):
        tr.train_step_native(synthetic.to_parametric_input(half))
    torch.save([p.detach().clone() for p in tr.parameters()], os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_equal_single_process_on_concatenated_batch(tmp_path, emu_lib):
    """two gloo ranks on disjoint halves of one batch (the candidate rows shard with their states): replicas bit-identical,
    and equal to one process on the whole batch within tests/test_data_parallel.py's 2e-6"""
    from reagent_amd import synthetic

    port = free_port()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for a, b in zip(r0, r1):
        assert torch.equal(a, b)
    tr = _dp_build()
    full = synthetic.parametric_batch(64, 6, 3, 4, seed=5, p_impossible=0.2)
    for _ in range(2):
        tr.train_step_native(synthetic.to_parametric_input(full))
    n = 0
    for a, p in zip(r0, tr.parameters()):
        assert (a.double() - p.detach().double()).abs().max() <= 2e-6
        n += 1
    assert n == 3 * 6  # q, its target and the reward network


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pdqn_kernels_do_not_spill(tmp_path):
    """pdqn.hip compiled for gfx950 with the resource remarks on: no spilled register and no scratch in any of its kernels.
    (The tiled forward is a path of the existing fused instantiations, which tests/test_kernel_resources.py holds.)"""
    csrc = os.path.join(ROOT, "reagent_amd", "csrc")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", f"-I{ROOT}/include",
                          "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "pdqn.hip"),
                          "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                kernels[name].setdefault(key, int(m.group(1)))
    for n in ("tile_concat_kernel", "pdqn_head_kernel"):
        assert any(n in k for k in kernels), (n, list(kernels))
    assert len(kernels) >= 3  # the concat kernel in both index widths, and the head
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
