"""SlateQTrainer beyond the fp32 fixtures: the fused path that reads the candidate panels in place end to end against the
same trainer on the rg_tile_concat path, a bf16 critic on the concat path, and the register / scratch budget of
slateq.hip's kernels."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _trainer(dev, precision, S=64, D=8, K=3, H=256, maxq=True, single=True):
    import reagent_amd._lib as L
    from reagent_amd.core.parameters import RLParameters, SlateOptParameters
    from reagent_amd.models import FullyConnectedCritic, set_default_precision
    from reagent_amd.optimizer import Optimizer__Union
    from reagent_amd.training import SlateQTrainer

    torch.manual_seed(0)
    set_default_precision(precision)
    try:
        q = FullyConnectedCritic(S, D, [H, H], ["relu", "relu"])
    finally:
        set_default_precision(L.PREC_F32)
    return SlateQTrainer(q.to(dev), q.get_target_network().to(dev), K,
                         rl=RLParameters(gamma=0.9, target_update_rate=0.1, maxq_learning=maxq),
                         optimizer=Optimizer__Union.default(lr=0.001), slate_opt_parameters=SlateOptParameters(),
                         single_selection=single).to(dev)


def _run(tr, batches, dev):
    from reagent_amd import synthetic

    out = []
    for d in batches:
        r = tr.train_step_native(synthetic.to_slateq_input(d, dev))
        out.append((r["td_loss"].detach().cpu().clone(), tr._next_idx.cpu().clone()))
    return out, [p.detach().cpu().clone() for p in tr.parameters()]


def test_fused_panel_path_against_the_tile_concat_path(backend, monkeypatch):
    """a 256-wide split-bf16 critic, S = 64, D = 8, C = 6, K = 3, B = 96, maxq, three native steps: the step whose target
    forward reads cat(next_state[r / C], candidates[r]) in place (rg_mlp_desc.x_tile = C) against the same trainer forced
    onto rg_tile_concat + the one-panel forward.  The online critic's SAVING forward on the K tiled rows takes assembled
    rows on both paths: the fused kernels' tiled two-panel forward is forward-only (rg_mlp_forward_fused returns
    RG_EUNSUPPORTED for x_tile > 1 with save), so what the spy sees there is the one-panel form.  The selected slates are
    identical; loss and parameters are held to the bound of split-bf16 critics' gradients in tests/test_full_size.py
    (STEP_BOUND[("c4", "bf16x3")]["grad"]) with that file's comparison, as test_fused_tiled_path_against_the_tile_concat_path
    does.  Two runs of the same steps are bit-identical."""
    import reagent_amd._lib as L
    import test_full_size as FS
    from reagent_amd import synthetic
    from reagent_amd.engine import FusedMLP
    from reagent_amd.training import SlateQTrainer

    dev = backend.device
    S, D, C, K, B = 64, 8, 6, 3, 96
    batches = [synthetic.slateq_batch(B, S, D, C, K, seed=40 + s) for s in range(3)]
    tr = _trainer(dev, L.PREC_BF16X3)
    assert isinstance(tr.q_network.fc.stack(), FusedMLP) and tr.q_network.fc.stack().x3
    calls = []
    real = FusedMLP.forward

    def spy(self, xc, out32, save=False, x2=None, rowmap=None, x_tile=1):
        calls.append((x2 is not None, x_tile, bool(save), out32.shape[0]))
        return real(self, xc, out32, save=save, x2=x2, rowmap=rowmap, x_tile=x_tile)

    monkeypatch.setattr(FusedMLP, "forward", spy)
    fused, p_fused = _run(tr, batches, dev)
    # per step: the target critic on all B * C candidate rows in place, then the online critic's saving forward on B * K rows
    assert calls == [(True, C, False, B * C), (False, 1, True, B * K)] * 3
    again, p_again = _run(_trainer(dev, L.PREC_BF16X3), batches, dev)
    for (l0, i0), (l1, i1) in zip(fused, again):
        assert torch.equal(l0, l1) and torch.equal(i0, i1)
    assert all(torch.equal(a, b) for a, b in zip(p_fused, p_again))
    calls.clear()
    monkeypatch.setattr(SlateQTrainer, "_reads_panels", staticmethod(lambda stack, state_dim: False))
    cat, p_cat = _run(_trainer(dev, L.PREC_BF16X3), batches, dev)
    assert calls and all(c[:2] == (False, 1) for c in calls)
    bound = FS.STEP_BOUND[("c4", "bf16x3")]["grad"]
    for (l0, i0), (l1, i1) in zip(fused, cat):
        assert torch.equal(i0, i1)
        assert abs(l0.item() - l1.item()) <= bound[0] * abs(l1.item())
    assert not FS.flagged(p_fused, p_cat, bound), FS.worst(p_fused, p_cat)


def test_sarsa_target_reads_the_gathered_panel_in_place(backend, monkeypatch):
    """SARSA on the same critic: the target forward runs on the rg_slate_gather panel with x_tile = K"""
    import reagent_amd._lib as L
    from reagent_amd import synthetic
    from reagent_amd.engine import FusedMLP

    dev = backend.device
    S, D, C, K, B = 64, 8, 6, 3, 96
    tr = _trainer(dev, L.PREC_BF16X3, maxq=False, single=False)
    calls = []
    real = FusedMLP.forward

    def spy(self, xc, out32, save=False, x2=None, rowmap=None, x_tile=1):
        calls.append((x2 is not None, x_tile, bool(save), out32.shape[0]))
        return real(self, xc, out32, save=save, x2=x2, rowmap=rowmap, x_tile=x_tile)

    monkeypatch.setattr(FusedMLP, "forward", spy)
    out = tr.train_step_native(synthetic.to_slateq_input(synthetic.slateq_batch(B, S, D, C, K, seed=7), dev))
    assert torch.isfinite(out["td_loss"]).all()
    assert calls == [(True, K, False, B * K), (False, 1, True, B * K)]


def test_bf16_critic_trains_on_the_concat_path(backend, monkeypatch):
    """a bf16 critic with a state width that is no multiple of 32 (S = 40) takes rg_tile_concat for every forward; the loss
    falls over five steps on a repeated batch"""
    import reagent_amd._lib as L
    from reagent_amd import synthetic
    from reagent_amd.engine import FusedMLP

    dev = backend.device
    tr = _trainer(dev, L.PREC_BF16, S=40)
    calls = []
    real = FusedMLP.forward

    def spy(self, xc, out32, save=False, x2=None, rowmap=None, x_tile=1):
        calls.append((x2 is not None, x_tile))
        return real(self, xc, out32, save=save, x2=x2, rowmap=rowmap, x_tile=x_tile)

    monkeypatch.setattr(FusedMLP, "forward", spy)
    b = synthetic.to_slateq_input(synthetic.slateq_batch(64, 40, 8, 6, 3, seed=1), dev)
    losses = [tr.train_step_native(b)["td_loss"].item() for _ in range(5)]
    assert calls and all(c == (False, 1) for c in calls)
    assert losses[-1] < losses[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_slateq_kernels_do_not_spill(tmp_path):
    """slateq.hip compiled for gfx950 with the resource remarks on: no spilled register and no scratch in any of its
    kernels (the top-k keeps up to 16 scores per lane in registers: every index into them is a compile-time one)"""
    csrc = os.path.join(ROOT, "reagent_amd", "csrc")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", f"-I{ROOT}/include",
                          "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "slateq.hip"),
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
    for n in ("slate_gather_kernel", "slate_topk_kernel", "slateq_head_kernel"):
        assert any(n in k for k in kernels), (n, list(kernels))
    assert len(kernels) == 8  # the gather in both index widths, the top-k with 1, 2, 4, 8 and 16 scores per lane, the head
    for k, v in kernels.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
