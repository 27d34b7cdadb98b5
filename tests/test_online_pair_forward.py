"""The paired online forward (rg_dqn_online_pair_forward: the online network's forwards on next_state and state and
the TD head in one launch) against the three launches it replaces — rg_mlp_forward_fused x 2 + rg_dqn_head + the loss
sum — BIT FOR BIT: q, qn_online, dq, next_q, next_idx, q_sel, the loss scalar after the reduce, and every saved
activation fragment and sign plane.  C2's layer shapes; batch sizes with odd tile counts and a partial last tile; both
workgroup orders run whenever B >= 256 (alternate 128-row tiles take alternate orders)."""
import itertools

import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops, synthetic
from reagent_amd.engine import FusedMLP, make_stack

DIMS, ACTS = [128, 512, 512, 512, 16], ["relu", "relu", "relu", "linear"]
A = 16


def _backend(where, monkeypatch):
    if where == "emu":
        import emu_backend

        emu_backend.install(monkeypatch)
        return "cpu"
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    L.lib()
    return "cuda"


def _stack(seed, dev):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.nn.Parameter((torch.randn(o, i, generator=g) * (1.5 / i ** 0.5)).to(dev)) for i, o in zip(DIMS, DIMS[1:])]
    bs = [torch.nn.Parameter((torch.randn(o, generator=g) * 0.1).to(dev)) for o in DIMS[1:]]
    st = make_stack(ws, bs, [L.ACT[a] for a in ACTS], L.PREC_BF16)
    assert isinstance(st, FusedMLP)
    return st


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.uint8 if t.dtype == torch.uint8 else
                               torch.int64 if t.dtype == torch.int64 else torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {(_bits(a) != _bits(b)).sum().item()} of {a.numel()} elements differ"


def _saved(st):
    ws = st._ws
    return [t for t in ws["act_frag"]] + [t for t in ws["act_sign"] if t is not None]


def _poison(st):
    for t in _saved(st):
        t.view(torch.uint8).fill_(0x5A)


# every option both ways for every B; B = 4096 on the interpreter runs the two complementary combinations (each option once
# on, once off: a forward of 4096 rows takes the interpreter minutes), on the GPU all eight
_COMBOS = list(itertools.product(["huber", "mse"], [False, True], [True, False]))
_CASES = []
for _where in ("emu", "hip"):
    for _B in (128, 384, 1000, 4096):
        for _loss, _extras, _dq in _COMBOS:
            if _where == "emu" and _B == 4096 and (_loss, _extras, _dq) not in (("huber", True, True), ("mse", False, False)):
                continue
            _CASES.append(pytest.param(_where, _B, _loss, _extras, _dq, id=f"{_where}-B{_B}-{_loss}-{'x' if _extras else 'p'}-"
                                       f"{'dq' if _dq else 'sq'}", marks=[pytest.mark.gpu] if _where == "hip" else []))


@pytest.mark.parametrize("where,B,loss,extras,double_q", _CASES)
def test_pair_equals_three_launches_bit_for_bit(where, B, loss, extras, double_q, monkeypatch):
    dev = _backend(where, monkeypatch)
    qs, ts = _stack(1, dev), _stack(2, dev)
    qs.stage_weights(need_transposed=True)
    ts.stage_weights(need_transposed=False)
    g = torch.Generator().manual_seed(100 + B)
    state = torch.randn(B, DIMS[0], generator=g)
    next_state = torch.randn(B, DIMS[0], generator=g)
    if B in (384, 4096):  # network-ready bf16 rows (what the sampler hands the step), else fp32 rows cast in flight
        state, next_state = state.bfloat16(), next_state.bfloat16()
    state, next_state = state.to(dev), next_state.to(dev)
    action = torch.nn.functional.one_hot(torch.randint(A, (B,), generator=g), A).float().to(dev)
    mask = (torch.rand(B, A, generator=g) > 0.3).float()
    single = torch.nn.functional.one_hot(torch.randint(A, (B,), generator=g), A).float()
    mask[::3] = single[::3]  # every third row leaves a single action
    mask = mask.to(dev)
    reward = torch.randn(B, generator=g).to(dev)
    not_terminal = (torch.rand(B, generator=g) > 0.1).float().to(dev)
    gamma_exp = torch.randint(1, 6, (B,), generator=g).float().to(dev) if extras else None
    boosts = torch.randn(A, generator=g).to(dev) if extras else None
    loss_type, gamma = L.LOSS[loss], 0.97
    f32 = dict(dtype=torch.float32, device=dev)

    def outs():
        return dict(q=torch.zeros(B, A, **f32), qn_online=torch.zeros(B, A, **f32), dq=torch.zeros(B, A, **f32),
                    next_q=torch.zeros(B, **f32), next_idx=torch.zeros(B, dtype=torch.int64, device=dev),
                    q_sel=torch.zeros(B, **f32), loss=torch.zeros(1, **f32))

    qn_target = torch.zeros(B, A, **f32)
    ts.forward(next_state, qn_target, save=False)

    # the three launches + the loss sum
    r = outs()
    qs._ensure_ws(B, state.device, training=True)
    _poison(qs)
    qs.forward(next_state, r["qn_online"], save=False)
    qs.forward(state, r["q"], save=True)
    partials = torch.zeros(ops.dqn_head_partials(B), **f32)
    ops.dqn_head(r["q"], r["qn_online"], qn_target, action, mask, reward, boosts, not_terminal, gamma, gamma_exp, double_q,
                 loss_type, r["dq"], partials, r["next_q"], r["next_idx"], r["q_sel"])
    ops.reduce_sum(partials, partials.numel(), 1.0 / B, r["loss"])
    r_saved = [t.clone() for t in _saved(qs)]

    # the pair
    p = outs()
    _poison(qs)
    assert qs.dqn_pair_supported(A)
    waves = torch.full((ops.dqn_pair_wave_sums(B),), float("nan"), **f32)
    qs.dqn_pair_forward(state, next_state, p["q"], p["qn_online"], qn_target, action, mask, reward, boosts, not_terminal,
                        gamma, gamma_exp, double_q, loss_type, p["dq"], waves, p["next_q"], p["next_idx"], p["q_sel"])
    ops.reduce_sum_runs(waves, waves.numel(), ops.DQN_PAIR_RUN, 1.0 / B, p["loss"])
    if dev == "cuda":
        torch.cuda.synchronize()
    assert torch.isfinite(r["q"]).all() and r["q"].abs().max() > 0 and r["dq"].abs().max() > 0 and r["loss"].item() > 0
    for k in r:
        _same(p[k], r[k], k)
    for i, (a, b) in enumerate(zip(_saved(qs), r_saved)):
        _same(a, b, f"saved buffer {i}")
    assert (r_saved[1].view(torch.uint8) != 0x5A).any()  # (the saving forward did write over the poison)


@pytest.mark.parametrize("where", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_native_steps_on_the_paired_path_equal_the_three_launch_sequence(where, monkeypatch):
    """3 native C2-shaped steps: the default trainer takes the paired launch, a twin is held to forward x 3 + dqn_head;
    every loss, parameter, Adam moment and target weight ends bit-identical."""
    from reagent_amd.core.parameters import EvaluationParameters, RLParameters
    from reagent_amd.models import FullyConnectedDQN, set_default_precision
    from reagent_amd.optimizer import Optimizer__Union
    from reagent_amd.training import DQNTrainer

    dev = _backend(where, monkeypatch)

    def make():
        set_default_precision(L.PREC_BF16)
        try:
            torch.manual_seed(7)
            q = FullyConnectedDQN(DIMS[0], A, DIMS[1:-1], ACTS[:-1]).to(dev)
        finally:
            set_default_precision(L.PREC_F32)
        return DQNTrainer(q, q.get_target_network(), None, actions=[str(i) for i in range(A)],
                          rl=RLParameters(gamma=0.9, target_update_rate=0.05, q_network_loss="huber"),
                          optimizer=Optimizer__Union.default(lr=0.003),
                          evaluation=EvaluationParameters(calc_cpe_in_training=False)).to(dev)

    paired, three = make(), make()
    three._pair_wanted = lambda qs, ts: False
    calls = []
    real = ops._run
    monkeypatch.setattr(ops, "_run", lambda name, meta, call: (calls.append((name, dict(meta))), real(name, meta, call))[1])
    B = 384
    for s in range(3):
        batch = synthetic.to_dqn_input(synthetic.dqn_batch(B, DIMS[0], A, seed=70 + s, p_impossible=0.2), dev)
        del calls[:]
        la = paired.train_step_native(batch)
        names = [n for n, _ in calls]
        assert "rg_dqn_head" not in names and "rg_reduce_sum" not in names
        fwd = [m for n, m in calls if n == "rg_mlp_forward_fused"]
        assert len(fwd) == 2 and [m for m in fwd if m.get("pair")] == [dict(B=2 * B, save=1, dims=tuple(DIMS), pair=1)]
        del calls[:]
        lb = three.train_step_native(batch)
        names = [n for n, _ in calls]
        assert names.count("rg_mlp_forward_fused") == 3 and "rg_dqn_head" in names
        _same(la, lb, f"loss of step {s}")
        for k in ("_q", "_qn_online", "_dq", "_next_q", "_next_idx", "_q_sel"):
            _same(getattr(paired, k), getattr(three, k), f"{k} of step {s}")
    for a, b in zip(paired.q_network.parameters(), three.q_network.parameters()):
        _same(a.detach(), b.detach(), "parameter")
    for a, b in zip(paired.q_network_target.parameters(), three.q_network_target.parameters()):
        _same(a.detach(), b.detach(), "target weight")
    oa, ob = paired.native_optimizers()[0], three.native_optimizers()[0]
    for pa, pb in zip(paired.q_network.parameters(), three.q_network.parameters()):
        _same(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"], "exp_avg")
        _same(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"], "exp_avg_sq")


def test_pair_kernel_uses_no_scratch():
    """the paired kernel carries two copies of the forward body at the edge of the register file: no scratch, <= 256 registers"""
    import os
    import re
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    csrc = os.path.join(root, "reagent_amd", "csrc")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", f"-I{root}/include",
                              "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(csrc, "mlp_fused.hip"), "-o", os.path.join(tmp, "o.o")],
                             capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("VGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                kernels[name].setdefault(key, int(m.group(1)))
    pair = {k: v for k, v in kernels.items() if "mlp_fwd_pair_kernel" in k}
    assert len(pair) == 3, list(kernels)  # the three (hidden width, pitch) instantiations
    for k, v in pair.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] <= 256, (k, v)
