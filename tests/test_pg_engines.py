"""PPOTrainer beyond the fp32 fixtures: native packed updates on 256-wide split-bf16 stacks against the same trainer on
fp32 stacks, their determinism and launch counts, and the register / scratch budget of pg.hip's kernels."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
S, A, H = 64, 16, 256
ACTS = ["tanh", "tanh"]  # smooth hidden layers: see test_split_bf16_updates_against_fp32_stacks
LENGTHS = [20, 70, 33, 64, 65, 41]
LR = 1e-3  # as tests/test_slateq_engines.py


def _trainer(dev, precision):
    import reagent_amd._lib as L
    from reagent_amd.gym.policies import Policy, SoftmaxActionSampler
    from reagent_amd.models import FloatFeatureFullyConnected, FullyConnectedDQN, set_default_precision
    from reagent_amd.optimizer import Optimizer__Union
    from reagent_amd.training import PPOTrainer

    torch.manual_seed(0)
    set_default_precision(precision)
    try:
        scorer = FullyConnectedDQN(S, A, [H, H], ACTS)
        value = FloatFeatureFullyConnected(S, 1, [H, H], ACTS)
    finally:
        set_default_precision(L.PREC_F32)
    tr = PPOTrainer(Policy(scorer.to(dev), SoftmaxActionSampler(temperature=0.8)), gamma=0.9,
                    optimizer=Optimizer__Union.default(lr=LR), optimizer_value_net=Optimizer__Union.default(lr=LR),
                    normalize=False, update_freq=len(LENGTHS), ppo_batch_size=len(LENGTHS), ppo_epsilon=0.2,
                    entropy_weight=0.01, value_net=value.to(dev)).to(dev)
    tr._minibatch_order = lambda n: torch.arange(n)
    return tr


def _run(tr, trajs, updates=3):
    """-> per update (ppo loss, value loss, the gradient of every parameter of both nets), and the parameters at the end"""
    out = []
    for _ in range(updates):
        for j, t in enumerate(trajs):
            tr.training_step(t, j)
        assert tr.traj_buffer == []
        out.append((tr._ploss.detach().cpu().clone(), tr._vloss.detach().cpu().clone(),
                    [p.grad.detach().cpu().clone() for p in tr.parameters()]))
    return out, [p.detach().cpu().clone() for p in tr.parameters()]


def test_split_bf16_updates_against_fp32_stacks(backend, monkeypatch):
    """a 256-wide split-bf16 policy net and value net, S = 64, A = 16, six trajectories of 20 to 70 steps with masks, three
    native PPO updates (one packed minibatch each) against the same trainer on fp32 stacks, with the bound of split-bf16
    gradients in tests/test_full_size.py (STEP_BOUND[("c4", "bf16x3")]["grad"]) and that file's comparison (max|d| / max|ref|
    and ||d|| / ||ref|| per tensor).  Held to it: both losses and the gradient of every parameter of both nets in every
    update — updates 2 and 3 start from the parameters the earlier backwards and Adam steps left — and every parameter
    after the third.
    The hidden layers are tanh.  That bound was measured at 65 536 rows; at the 293 rows of six such trajectories ONE ReLU
    unit whose pre-activation the two engines round to different sides of 0 moves a gradient row by 1 / 293 of a coherent
    sum (measured with ReLU layers here: 8.5e-3 / 2.0e-3 on the value net's hidden layers in an update with such a unit,
    1.7e-5 / 1.4e-5 on the policy net in one without), so whether a ReLU net meets it at this size is a property of the
    draw, not of the engines.  A smooth activation has no such unit: gradients agree to about 2e-5 in all three updates.
    ReLU stacks are held to their gradients at full size in tests/test_full_size.py and, through the policy-gradient step,
    to the reference's fixtures in tests/test_pg_trainers.py.
    Two runs are bit-identical, and an update launches rg_pg_returns and rg_pg_head ONCE each, however many trajectories
    the minibatch has."""
    import reagent_amd._lib as L
    import test_full_size as FS
    from reagent_amd import ops, synthetic
    from reagent_amd.engine import FusedMLP

    dev = backend.device
    trajs = [synthetic.to_pg_input(synthetic.pg_trajectory(n, S, A, seed=300 + n, with_mask=True), dev) for n in LENGTHS]
    calls = []
    for name in ("pg_returns", "pg_head"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    tr = _trainer(dev, L.PREC_BF16X3)
    for net in (tr.scorer, tr.value_net):
        assert isinstance(net.fc.stack(), FusedMLP) and net.fc.stack().x3
    init = [p.detach().cpu().clone() for p in tr.parameters()]
    x3, p_x3 = _run(tr, trajs)
    assert calls == ["pg_returns", "pg_head"] * 3
    again, p_again = _run(_trainer(dev, L.PREC_BF16X3), trajs)
    for (a0, a1, ag), (b0, b1, bg) in zip(x3, again):
        assert torch.equal(a0, b0) and torch.equal(a1, b1) and all(torch.equal(x, y) for x, y in zip(ag, bg))
    assert all(torch.equal(a, b) for a, b in zip(p_x3, p_again))
    f32, p_f32 = _run(_trainer(dev, L.PREC_F32), trajs)
    bound = FS.STEP_BOUND[("c4", "bf16x3")]["grad"]
    for u, ((a0, a1, ag), (b0, b1, bg)) in enumerate(zip(x3, f32)):
        print(f"update {u}: rel. loss differences {abs(a0.item() - b0.item()) / abs(b0.item()):.2e} "
              f"{abs(a1.item() - b1.item()) / abs(b1.item()):.2e}; gradients (max_rel, norm_rel) {FS.worst(ag, bg)}")
        assert abs(a0.item() - b0.item()) <= bound[0] * abs(b0.item()), (u, a0, b0)
        assert abs(a1.item() - b1.item()) <= bound[0] * abs(b1.item()), (u, a1, b1)
        assert all(g.abs().max() > 0 for g in bg)
        assert not FS.flagged(ag, bg, bound), (u, FS.flagged(ag, bg, bound), FS.worst(ag, bg))
    print(f"parameters after three updates (max_rel, norm_rel) {FS.worst(p_x3, p_f32)}")
    assert not FS.flagged(p_x3, p_f32, bound), FS.worst(p_x3, p_f32)
    assert min((a - b).abs().max().item() for a, b in zip(p_f32, init)) > LR  # (every tensor moved)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pg_kernels_do_not_spill(tmp_path):
    """pg.hip compiled for gfx950 with the resource remarks on: every kernel instance has no scratch, no spilled register
    and at most 64 VGPRs (8 waves per SIMD); the head keeps its four actions per lane in registers behind compile-time
    indices, the scan 16 broadcast values at a time"""
    csrc = os.path.join(ROOT, "reagent_amd", "csrc")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", f"-I{ROOT}/include",
                          "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "pg.hip"),
                          "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs", "Occupancy [waves/SIMD]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                kernels[name].setdefault(key, int(m.group(1)))
    assert sum("pg_returns_kernel" in k for k in kernels) == 1 and sum("pg_head_kernel" in k for k in kernels) == 4
    assert len(kernels) == 5  # the scan, the head with 1, 4, 16 and 64 lanes per row
    for k, v in kernels.items():
        print(k, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
        assert 0 < v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] == 8, (k, v)
