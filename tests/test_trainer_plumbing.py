"""The shared step plumbing (reagent_amd/training/plumbing.py) through two trainers that use all of it: a HIP backward
overwrites the gradient slab, so PyTorch's accumulation rule (a second backward without zero_grad() adds; a foreign .grad
tensor is added into, not replaced) and the data-parallel 1/world convention (mean on the generator path, folded into the
Adam launch inside a native step) are host logic of TrainableNet.backward / dp_reduce.  Every statement is bit for bit:
x + x and 0.5 * x are exact in fp32.  Shapes: 128-row tile + a two-row tail, state and action width 32; the fp32
per-layer engine on hidden [64, 64] and a fused bf16 stack on hidden [256, 256] (the fused kernels take no narrower
one: rg_mlp_fused_supported)."""
import os

import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import synthetic
from reagent_amd.core.parameters import RLParameters
from reagent_amd.engine import FusedMLP
from reagent_amd.models import FullyConnectedActor, FullyConnectedCritic, set_default_precision
from reagent_amd.optimizer import FusedAdam, Optimizer__Union

S, A, ACTS, B, M = 32, 32, ["relu", "relu"], 130, 3
HIDDEN = {L.PREC_F32: [64, 64], L.PREC_BF16: [256, 256]}
ENGINES = [pytest.param(L.PREC_F32, id="fp32_per_layer"), pytest.param(L.PREC_BF16, id="bf16_fused")]


def _noise():
    return torch.randn(B, A, generator=torch.Generator().manual_seed(3))


def _td3(device, precision):
    from reagent_amd.training import TD3Trainer

    torch.manual_seed(0)
    set_default_precision(precision)
    try:
        hidden = HIDDEN[precision]
        nets = [FullyConnectedActor(S, A, hidden, ACTS)] + [FullyConnectedCritic(S, A, hidden, ACTS) for _ in range(2)]
    finally:
        set_default_precision(L.PREC_F32)
    adam = lambda: Optimizer__Union.default(lr=1e-3)  # noqa: E731
    tr = TD3Trainer(*[n.to(device) for n in nets], rl=RLParameters(gamma=0.9, target_update_rate=0.1),
                    q_network_optimizer=adam(), actor_network_optimizer=adam(), delayed_policy_update=2).to(device)
    batch = synthetic.to_policy_input(synthetic.policy_batch(B, S, A, seed=11), device)
    return tr, batch


def _pdqn(device, precision):
    from reagent_amd.training import ParametricDQNTrainer

    torch.manual_seed(0)
    set_default_precision(precision)
    try:
        q, qt = FullyConnectedCritic(S, A, HIDDEN[precision], ACTS), FullyConnectedCritic(S, A, HIDDEN[precision], ACTS)
    finally:
        set_default_precision(L.PREC_F32)
    qt.load_state_dict(q.state_dict())
    tr = ParametricDQNTrainer(q.to(device), qt.to(device), rl=RLParameters(gamma=0.9, target_update_rate=0.1),
                              optimizer=Optimizer__Union.default(lr=1e-3)).to(device)
    batch = synthetic.to_parametric_input(synthetic.parametric_batch(B, S, A, M, seed=12, p_impossible=0.2), device)
    return tr, batch


class Segment:
    """the first segment of the generator path (TD3: critic q1, parametric DQN: q): forward + loss.backward()"""

    def __init__(self, kind, device, precision):
        self.kind = kind
        self.tr, self.batch = (_td3 if kind == "td3" else _pdqn)(device, precision)
        self.module = self.tr.q1_network if kind == "td3" else self.tr.q_network
        self.params = list(self.module.parameters())
        self.precision = precision

    def backward(self):
        if self.kind == "td3":
            self.tr.set_noise(_noise())
        next(self.tr.train_step_gen(self.batch, 0)).backward()
        net = self.net()
        assert isinstance(net.stack, FusedMLP) == (self.precision == L.PREC_BF16)
        return [p.grad.detach().cpu().clone() for p in self.params]

    def net(self):
        return self.tr._e["q1" if self.kind == "td3" else "q"]

    def aliases_slab(self, i):
        slab = self.net().slab
        return self.params[i].grad.data_ptr() == slab.grad.data_ptr() + 4 * slab.offsets[i]


@pytest.mark.parametrize("precision", ENGINES)
@pytest.mark.parametrize("kind", ["td3", "pdqn"])
def test_second_backward_without_zero_grad_adds(backend, kind, precision):
    seg = Segment(kind, backend.device, precision)
    single = seg.backward()
    assert all(g.abs().max() > 0 for g in single)
    twice = seg.backward()  # no zero_grad() in between
    for g, gg in zip(single, twice):
        assert torch.equal(gg, g + g)
    seg.module.zero_grad(set_to_none=False)  # zeroed in place: p.grad still aliases the slab
    assert all(seg.aliases_slab(i) and not seg.params[i].grad.any() for i in range(len(seg.params)))
    for g, again in zip(single, seg.backward()):
        assert torch.equal(again, g)
    seg.module.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in seg.params)
    for g, again in zip(single, seg.backward()):
        assert torch.equal(again, g)
    assert all(seg.aliases_slab(i) for i in range(len(seg.params)))


@pytest.mark.parametrize("precision", ENGINES)
@pytest.mark.parametrize("kind", ["td3", "pdqn"])
def test_foreign_grad_tensor_is_added_into(backend, kind, precision):
    seg = Segment(kind, backend.device, precision)
    single = seg.backward()
    seg.module.zero_grad(set_to_none=True)
    foreign = {i: torch.full_like(seg.params[i], 0.25) for i in (0, len(seg.params) - 1)}  # first weight, last bias
    for i, f in foreign.items():
        seg.params[i].grad = f
    got = seg.backward()
    for i, g in enumerate(single):
        if i in foreign:
            assert seg.params[i].grad is foreign[i] and not seg.aliases_slab(i)
            assert torch.equal(got[i], torch.full_like(g, 0.25) + g)
        else:
            assert seg.aliases_slab(i) and torch.equal(got[i], g)


@pytest.fixture
def one_rank_group(backend):
    """a process group of one rank: gloo for the interpreter's CPU tensors, RCCL for the device's"""
    import torch.distributed as dist

    from conftest import free_port

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(free_port())
    if backend.device == "cpu":
        dist.init_process_group("gloo", rank=0, world_size=1)
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("precision", ENGINES)
def test_one_over_world_is_applied_once(backend, one_rank_group, monkeypatch, precision):
    """the sum over a one-rank group is the rank's own gradient, so with _dp_world forced to 2: the generator path
    publishes half the single-process gradient (its caller steps the optimizers); a native step leaves the sum in the
    slab and hands 1/world to the Adam launch"""
    seg = Segment("td3", backend.device, precision)
    single = seg.backward()
    seg.module.zero_grad(set_to_none=True)
    seg.tr.enable_data_parallel(one_rank_group)
    seg.tr._dp_world = 2
    for g, got in zip(single, seg.backward()):
        assert torch.equal(got, g * 0.5)
    seen = []
    real_step = FusedAdam.step

    def spy(opt, *a, **k):
        if opt is seg.tr.native_optimizers()[0]:  # q1's Adam
            seen.append((opt.grad_scale, [v.detach().cpu().clone() for v in seg.net().slab.grad_views()]))
        return real_step(opt, *a, **k)

    monkeypatch.setattr(FusedAdam, "step", spy)
    seg.tr.train_step_native(seg.batch, _noise())
    assert len(seen) == 1 and seen[0][0] == 0.5
    for g, got in zip(single, seen[0][1]):
        assert torch.equal(got, g)
