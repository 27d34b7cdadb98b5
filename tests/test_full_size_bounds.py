"""The bounds of tests/test_full_size.py's oracle checks can fail (CPU).

A gradient check passes a kernel whose error its bound does not see.  Here the comparison helpers of the full-size tests are
fed the oracle's own C2 gradients (128-512-512-512-16, B = 2048) perturbed the way a kernel goes wrong — one tensor scaled,
one 32 x 32 tile of a dW scaled (a wrong MFMA tile), one 1/32 row slab of a dW doubled, one bias gradient offset — and the
unperturbed reference must pass.  The accurate-mode bounds (f32, split-bf16) flag every such perturbation at the sizes the
full-size tests are meant to catch, in every tensor / tile / slab; for the bf16 bounds the smallest size caught everywhere is
stated below.
"""
import pytest
import torch

import test_full_size as F
from oracle import restated as R
from reagent_amd import synthetic

GRID = (1.01, 1.02, 1.05, 1.1, 1.2, 1.5, 2.0, 3.0, 5.0, 10.0)  # scale factors; bias offsets: (f - 1) x max|db|


@pytest.fixture(scope="module")
def c2_grads():
    S, A, H = F.S, F.A, [F.H] * 3
    acts = ["relu"] * 3 + ["linear"]
    init = synthetic.fc_init([S] + H + [A], acts, seed=40)
    o = R.DQNOracle(init, init, acts, gamma=0.99, tau=1e-3, loss="huber", lr=1e-3)
    return o.step(synthetic.dqn_batch(2048, S, A, seed=5, p_impossible=0.3))["grads"]


def _tiles(w):
    return [(r, c) for r in range(0, w.shape[0] - 31, 32) for c in range(0, w.shape[1] - 31, 32)]


def _slabs(w):
    n = w.shape[0] // 32
    return [r for r in range(0, w.shape[0] - n + 1, n)] if n else []


def perturbations(grads, f):
    """(kind, tensor index, perturbed tensor) for every place a perturbation of size f can go"""
    for i, g in enumerate(grads):
        yield "scale", i, g * f
        if g.dim() == 1:
            yield "bias offset", i, g + (f - 1.0) * g.abs().max()
            continue
        for r, c in _tiles(g):
            t = g.clone()
            t[r:r + 32, c:c + 32] *= f
            yield "tile", i, t
        n = g.shape[0] // 32
        for r in _slabs(g):
            t = g.clone()
            t[r:r + n] *= f
            yield "row slab", i, t


def caught_everywhere(grads, bound, f):
    """per perturbation kind: whether every placement of size f is flagged by `bound` — in the gradient and in the moments
    it leaves after one Adam step (exp_avg = 0.1 g: the gradient's relative errors; exp_avg_sq = 1e-3 g^2: twice them)"""
    ok = {}
    vb = (2 * bound[0], 2 * bound[1])
    for kind, i, p in perturbations(grads, f):
        g = grads[i]
        hit = bool(F.flagged([p], [g], bound)) and bool(F.flagged([0.1 * p], [0.1 * g], bound)) \
            and bool(F.flagged([1e-3 * p * p], [1e-3 * g * g], vb))
        ok[kind] = ok.get(kind, True) and hit
    return ok


def smallest_caught(grads, bound):
    out = {}
    for f in GRID:
        for kind, hit in caught_everywhere(grads, bound, f).items():
            if hit and kind not in out:
                out[kind] = f
        if len(out) == 4:
            break
    return out


ACCURATE = {"c2 f32": F.STEP_BOUND[("c2", "f32")]["grad"], "c2 bf16x3": F.STEP_BOUND[("c2", "bf16x3")]["grad"],
            "c3 bf16x3": F.STEP_BOUND[("c3", "bf16x3")]["grad"], "c4 critics bf16x3": F.STEP_BOUND[("c4", "bf16x3")]["grad"],
            "stack bf16x3": F.STACK_BOUND["bf16x3"]["grad"]}


@pytest.mark.parametrize("name", sorted(ACCURATE))
def test_accurate_bounds_flag_every_kernel_shaped_perturbation(c2_grads, name):
    bound = ACCURATE[name]
    assert not F.flagged(c2_grads, c2_grads, bound)
    assert not F.flagged([g.clone() for g in c2_grads], c2_grads, bound)
    for f, kinds in ((1.01, ("scale", "bias offset")), (1.1, ("tile",)), (2.0, ("row slab",))):
        ok = caught_everywhere(c2_grads, bound, f)
        assert all(ok[k] for k in kinds), (name, f, ok)


# the smallest factor of GRID caught at EVERY placement (tensor / tile / slab / bias) by the looser bounds: a doubled 32 x 32
# tile of a dW is what the bf16 step bounds are sure to see (max-abs 2e-2 of the largest entry is bf16's own error there)
LOOSE = {
    "c2 bf16": (F.STEP_BOUND[("c2", "bf16")]["grad"], {"scale": 1.05, "bias offset": 1.02, "row slab": 1.5, "tile": 2.0}),
    "c3 bf16": (F.STEP_BOUND[("c3", "bf16")]["grad"], {"scale": 1.02, "bias offset": 1.01, "row slab": 1.2, "tile": 2.0}),
    "c4 critics bf16": (F.STEP_BOUND[("c4", "bf16")]["grad"], {"scale": 1.02, "bias offset": 1.02, "row slab": 1.5, "tile": 2.0}),
    "c4 actor bf16x3": (F.STEP_BOUND[("c4", "bf16x3")]["actor"], {"scale": 1.01, "bias offset": 1.01, "row slab": 1.05, "tile": 1.1}),
    "c4 actor bf16": (F.STEP_BOUND[("c4", "bf16")]["actor"], {"scale": 1.05, "bias offset": 1.02, "row slab": 1.5, "tile": 2.0}),
    "stack bf16": (F.STACK_BOUND["bf16"]["grad"], {"scale": 1.01, "bias offset": 1.01, "row slab": 1.1, "tile": 1.5}),
}


@pytest.mark.parametrize("name", sorted(LOOSE))
def test_loose_bounds_state_the_smallest_perturbation_they_catch(c2_grads, name):
    bound, stated = LOOSE[name]
    assert not F.flagged(c2_grads, c2_grads, bound)
    got = smallest_caught(c2_grads, bound)
    print(f"\n[{name} bound {bound}] smallest factor caught everywhere: {got}")
    assert got == stated, (name, got)
