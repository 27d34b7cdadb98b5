"""The bf16 mirror of the replay store's observation column (rg_replay_mirror_build) and the sampler that copies its rows
(rg_replay_dqn_batch_mirror), against the sampler that normalizes fp32 rows at every draw (rg_replay_dqn_batch /
rg_replay_dqn_batch_pooled with state_dtype bf16) — BIT FOR BIT: every mirror row, every output of the launch, the rows an
add rewrote, another preprocessor table, and three native C2-shaped steps of a loop on either sampler."""
import os

import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops, synthetic
from reagent_amd.core.parameters import NormalizationParameters as NP
from reagent_amd.preprocessing import Preprocessor
from reagent_amd.replay_memory import ReplayBuffer

WHERE = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
C = 257  # capacity: no multiple of the 64 rows a workgroup converts, more than one workgroup


def _backend(where, monkeypatch):
    if where == "emu":
        import emu_backend

        emu_backend.install(monkeypatch)
        return "cpu"
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    L.lib()
    return "cuda"


def _table(F, dev, seed=1):
    """a 1:1 table that mixes CONTINUOUS, BOXCOX (the op with four parameters), QUANTILE and BINARY columns"""
    g = torch.Generator().manual_seed(seed)
    norm = {}
    for i in range(F):
        m = torch.randn(1, generator=g).item()
        if i % 4 == 0:
            norm[i] = NP(feature_type="CONTINUOUS", mean=m, stddev=1.3 + 0.01 * i)
        elif i % 4 == 1:
            norm[i] = NP(feature_type="BOXCOX", boxcox_lambda=0.5, boxcox_shift=3.5, mean=1.0 + 0.1 * m, stddev=0.7)
        elif i % 4 == 2:
            norm[i] = NP(feature_type="QUANTILE", quantiles=[-1.0, 0.0, 0.5 + 0.01 * i, 2.0])
        else:
            norm[i] = NP(feature_type="BINARY")
    order = Preprocessor(norm, device=dev).sorted_features  # the gather applies descriptor j to column j
    pre = Preprocessor({k: norm[f] for k, f in enumerate(order)}, device=dev)
    assert pre.elementwise
    return pre


def _continuous(F, dev, seed=7):
    mean, std = synthetic.normalization_table(F, seed)
    return Preprocessor({i: NP(feature_type="CONTINUOUS", mean=mean[i].item(), stddev=std[i].item()) for i in range(F)}, device=dev)


def _contents(n, F, A, seed):
    cols = synthetic.replay_contents(n, F, A, seed=seed, p_terminal=0.2)
    g = torch.Generator().manual_seed(seed + 1)
    cols["observation"][::7, ::5] = 0.0  # BINARY's other value
    cols["possible_actions_mask"] = (torch.rand(n, A, generator=g) > 0.3).float()
    cols["log_prob"] = -torch.rand(n, generator=g)
    return cols


def _buffer(dev, F, A=5, horizon=1, n=C, seed=3):
    rb = ReplayBuffer(replay_capacity=C, batch_size=64, update_horizon=horizon, gamma=0.9, device=dev)
    rb.load_columns({k: v.to(dev) for k, v in _contents(n, F, A, seed).items()}, mark_all_valid=True)
    return rb


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


def _fields(inp):
    return dict(state=inp.state.float_features, next_state=inp.next_state.float_features, action=inp.action,
                next_action=inp.next_action, reward=inp.reward, not_terminal=inp.not_terminal,
                possible_actions_mask=inp.possible_actions_mask, possible_next_actions_mask=inp.possible_next_actions_mask,
                action_probability=inp.extras.action_probability)


def _sample(rb, pre, idx, A, mirror):
    """sample_dqn_input (bf16) on the mirror or, with the buffer's mirror switched off, on the fp32 rows"""
    rb._use_mirror = mirror
    try:
        inp = rb.sample_dqn_input(A, len(idx), indices=idx, state_preprocessor=pre, state_dtype=torch.bfloat16)
    finally:
        rb._use_mirror = True
    assert inp is not None
    return _fields(inp)


def _assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what} {k}: {(_bits(a[k]) != _bits(b[k])).sum().item()} elements differ"


@pytest.fixture
def builds(monkeypatch):
    """the (row_begin, row_end) of every rg_replay_mirror_build, and whether each sampler launch read a mirror"""
    seen = dict(build=[], sampler=[])
    build, sample = ops.replay_mirror_build, ops.replay_dqn_batch

    def spy_build(obs, cols, q, mirror, r0, r1):
        seen["build"].append((r0, r1))
        return build(obs, cols, q, mirror, r0, r1)

    def spy_sample(view, indices, cols, q, out, mirror=None):
        seen["sampler"].append(mirror is not None)
        return sample(view, indices, cols, q, out, mirror=mirror)

    monkeypatch.setattr(ops, "replay_mirror_build", spy_build)
    monkeypatch.setattr(ops, "replay_dqn_batch", spy_sample)
    return seen


@pytest.mark.parametrize("F", [128, 12])
@pytest.mark.parametrize("where", WHERE)
def test_mirror_rows_are_the_sampler_rows(where, F, monkeypatch, builds):
    """every row of the mirror == the `state` row rg_replay_dqn_batch writes for that index (mixed-op table, capacity 257)"""
    dev = _backend(where, monkeypatch)
    rb, pre = _buffer(dev, F), _table(F, dev)
    idx = torch.arange(C, device=dev)
    want = _sample(rb, pre, idx, 5, mirror=False)
    assert rb._mirror is None and builds["build"] == []
    mirror = rb._bf16_mirror(pre)
    assert builds["build"] == [(0, C)]  # the whole store in one launch
    assert mirror.dtype == torch.bfloat16 and tuple(mirror.shape) == (C, F)
    assert torch.equal(_bits(mirror), _bits(want["state"]))
    assert len({int(x) for x in _bits(mirror).flatten()[:4 * F].tolist()}) > 8  # (not a constant)
    # a partial build writes its rows and no others
    part = torch.full_like(mirror, 7.0)
    assert ops.replay_mirror_build(rb._store["observation"], pre._col_table, pre._quantiles, part, 63, 130)
    assert torch.equal(_bits(part[63:130]), _bits(mirror[63:130]))
    assert (part[:63] == 7.0).all() and (part[130:] == 7.0).all()


def _direct(dev, cols, horizon, A, extras, pre, mirror, indices, sched=None):
    """the entry points themselves on hand-built views: every field of rg_dqn_batch_out, nullable columns absent or given"""
    st = {k: v.to(dev) for k, v in cols.items()}
    F = st["observation"].shape[1]
    B = indices.numel()
    decays = (0.9 ** torch.arange(horizon)).float().to(dev)
    ids = (torch.arange(C) // 9).to(dev)
    view = L.ReplayView()
    view.observation, view.action, view.reward = st["observation"].data_ptr(), st["action"].data_ptr(), st["reward"].data_ptr()
    term = st["terminal"].to(torch.uint8)
    view.terminal, view.decays = term.data_ptr(), decays.data_ptr()
    view.log_prob = st["log_prob"].data_ptr() if extras else None
    view.possible_actions_mask = st["possible_actions_mask"].data_ptr() if extras else None
    view.mdp_id = ids.data_ptr() if extras else None
    view.sequence_number = ids.data_ptr() if extras else None
    view.capacity, view.n_features, view.n_actions, view.update_horizon = C, F, A, horizon
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(state=torch.zeros(B, F, dtype=torch.bfloat16, device=dev), next_state=torch.zeros(B, F, dtype=torch.bfloat16, device=dev),
               action=torch.zeros(B, A, **f32), next_action=torch.zeros(B, A, **f32), reward=torch.zeros(B, **f32),
               time_diff=torch.zeros(B, **f32), step=torch.zeros(B, **f32), not_terminal=torch.zeros(B, **f32),
               possible_next_actions_mask=torch.zeros(B, A, **f32), action_probability=torch.zeros(B, **f32),
               mdp_id=torch.zeros(B, dtype=torch.int64, device=dev), sequence_number=torch.zeros(B, dtype=torch.int64, device=dev))
    if extras:
        out["possible_actions_mask"] = torch.zeros(B, A, **f32)
    buf = None
    if mirror:
        buf = torch.zeros(C, F, dtype=torch.bfloat16, device=dev)
        assert ops.replay_mirror_build(st["observation"], pre._col_table, pre._quantiles, buf, 0, C)
    assert ops.replay_dqn_batch(view, indices, pre._col_table, pre._quantiles, out, mirror=buf)
    return out


@pytest.mark.parametrize("extras", [True, False], ids=["mask+log_prob", "bare"])
@pytest.mark.parametrize("horizon", [1, 3])
@pytest.mark.parametrize("B,F", [(100, 128), (64, 12)])
@pytest.mark.parametrize("where", WHERE)
def test_mirror_sampler_equals_the_normalizing_sampler(where, B, F, horizon, extras, monkeypatch):
    """rg_replay_dqn_batch_mirror == rg_replay_dqn_batch / _pooled on every output: a batch that is no multiple of 64 and one
    that is, 16-byte (F = 128) and 8-byte (F = 12) row pieces, n-step windows with terminals inside, indices whose window and
    next index wrap past capacity - 1, nullable columns present and absent, the pooled form at two cursor values"""
    dev, A = _backend(where, monkeypatch), 5
    cols, pre = _contents(C, F, A, seed=5), _table(F, dev)
    g = torch.Generator().manual_seed(B)
    pool = torch.randint(C, (2, B), generator=g)
    pool[:, :4] = torch.tensor([C - 1, C - 2, C - 3, 0])
    pool = pool.to(dev)
    term = cols["terminal"]
    assert horizon == 1 or any(term[(int(i) + k) % C] for i in pool[0].tolist() for k in range(horizon - 1))
    for row in (0, 1):
        idx = pool[row].contiguous()
        want = _direct(dev, cols, horizon, A, extras, pre, False, idx)
        got = _direct(dev, cols, horizon, A, extras, pre, True, idx)
        _assert_same(got, want, f"plain row {row}")
        sched = {m: torch.zeros(4, dtype=torch.float64, device=dev) for m in (False, True)}
        cursor = torch.tensor([row], dtype=torch.int64, device=dev)
        for m in (False, True):
            pooled = _direct(dev, cols, horizon, A, extras, pre, m, ops.PooledIndices(pool, cursor, sched[m]))
            _assert_same(pooled, want, f"pooled, cursor {row}, mirror {m}")
            assert sched[m].tolist() == [1.0, 0.0, 0.0, 0.0]  # the launch counted the step
        assert int(cursor.item()) == row


@pytest.mark.parametrize("where", WHERE)
def test_rows_an_add_rewrote_are_rebuilt_before_the_next_sample(where, monkeypatch, builds):
    dev, F, A = _backend(where, monkeypatch), 128, 5
    pre = _continuous(F, dev)
    rb = _buffer(dev, F, A, n=240)
    everything = torch.arange(C, device=dev)
    _assert_same(_sample(rb, pre, everything, A, True), _sample(rb, pre, everything, A, False), "before")
    assert builds["build"] == [(0, C)]
    before = rb._mirror["buf"].clone()
    new = {k: v[:40] for k, v in _contents(64, F, A, seed=9).items()}
    rb.add_many(**new)  # slots 240 .. 256 and 0 .. 22: across the wrap point
    got = _sample(rb, pre, everything, A, True)
    assert builds["build"] == [(0, C), (240, C), (0, 23)]  # exactly the rows written
    _assert_same(got, _sample(rb, pre, everything, A, False), "after add_many")
    now = rb._mirror["buf"]
    assert torch.equal(_bits(now[23:240]), _bits(before[23:240]))
    assert not torch.equal(_bits(now[:23]), _bits(before[:23])) and not torch.equal(_bits(now[240:]), _bits(before[240:]))
    one = _contents(4, F, A, seed=10)
    rb.add(observation=one["observation"][0].numpy(), action=np.int64(1), reward=np.float32(0.5), terminal=False,
           log_prob=np.float32(-0.1), possible_actions_mask=np.ones(A, np.float32))  # slot 23
    _assert_same(_sample(rb, pre, everything, A, True), _sample(rb, pre, everything, A, False), "after add")
    assert builds["build"][3:] == [(23, 24)]
    rb._store["observation"][100] += 1.0  # a write that went round the class: noticed, everything rebuilt
    _assert_same(_sample(rb, pre, everything, A, True), _sample(rb, pre, everything, A, False), "after a direct write")
    assert builds["build"][4:] == [(0, C)]
    assert builds["sampler"].count(True) == 4


@pytest.mark.parametrize("where", WHERE)
def test_another_preprocessor_table_replaces_the_mirror(where, monkeypatch, builds):
    dev, F, A = _backend(where, monkeypatch), 12, 5
    rb = _buffer(dev, F, A, horizon=3)
    a, b = _continuous(F, dev), _table(F, dev)
    idx = torch.arange(C - 100, C, device=dev)
    for pre in (a, b, b, a):
        got = _sample(rb, pre, idx, A, True)
        assert rb._mirror["cols"] is pre._col_table and rb._mirror["quantiles"] is pre._quantiles
        _assert_same(got, _sample(rb, pre, idx, A, False), "table")
    assert builds["build"] == [(0, C)] * 3  # the second draw with b found its mirror
    assert not torch.equal(_bits(_sample(rb, a, idx, A, True)["state"]), _bits(_sample(rb, b, idx, A, True)["state"]))
    # fp32 states are never served from the mirror; a buffer without room for one samples as before
    n = len(builds["sampler"])
    rb.sample_dqn_input(A, len(idx), indices=idx, state_preprocessor=a, state_dtype=torch.float32)
    assert builds["sampler"][n:] == [False]
    def no_room(*args, **kwargs):
        raise torch.OutOfMemoryError("no room")

    monkeypatch.setattr(torch, "empty", no_room)
    rb._mirror = None
    assert rb._bf16_mirror(a) is None and rb._use_mirror is False


def _c2_loop(dev, capacity, batch):
    from reagent_amd.core.parameters import EvaluationParameters, RLParameters
    from reagent_amd.models import FullyConnectedDQN, set_default_precision
    from reagent_amd.optimizer import Optimizer__Union
    from reagent_amd.runtime import OfflineDqnLoop
    from reagent_amd.training import DQNTrainer

    S, A, H = 128, 16, [512, 512, 512]
    set_default_precision(L.PREC_BF16)
    try:
        torch.manual_seed(7)
        q = FullyConnectedDQN(S, A, H, ["relu"] * 3).to(dev)
    finally:
        set_default_precision(L.PREC_F32)
    tr = DQNTrainer(q, q.get_target_network(), None, actions=[str(i) for i in range(A)],
                    rl=RLParameters(gamma=0.99, target_update_rate=0.05, q_network_loss="huber"),
                    optimizer=Optimizer__Union.default(lr=1e-3),
                    evaluation=EvaluationParameters(calc_cpe_in_training=False)).to(dev)
    rb = ReplayBuffer(replay_capacity=capacity, batch_size=batch, device=dev)
    rb.load_columns({k: v.to(dev) for k, v in synthetic.replay_contents(capacity, S, A, seed=100).items()}, mark_all_valid=True)
    return OfflineDqnLoop(rb, tr, batch, _continuous(S, dev), state_dtype=torch.bfloat16), tr


def _state(tr):
    _, exp_avg, exp_avg_sq = tr.native_optimizers()[0].moments_for(0)  # the optimizer's flat moment buffers
    return ([p.detach().clone() for p in list(tr.q_network.parameters()) + list(tr.q_network_target.parameters())]
            + [exp_avg.clone(), exp_avg_sq.clone()])


@pytest.mark.parametrize("where", WHERE)
def test_native_steps_on_the_mirror_equal_steps_on_the_normalizing_sampler(where, monkeypatch, builds):
    """3 native C2-shaped steps (B = 384, 128-512-512-512-16, bf16): the default loop samples from the mirror, its twin is held
    to the fp32 rows; losses, parameters, target weights and Adam moments end bit-identical"""
    dev, B, cap = _backend(where, monkeypatch), 384, 2048
    res = {}
    for mirror in (True, False):
        loop, tr = _c2_loop(dev, cap, B)
        loop.rb._use_mirror = mirror
        del builds["sampler"][:]
        losses = [loop.step(torch.randint(cap, (B,), generator=torch.Generator().manual_seed(60 + s)).to(dev)).clone()
                  for s in range(3)]
        loop.flush()
        assert builds["sampler"] == [mirror] * 3
        res[mirror] = losses + _state(tr)
    assert builds["build"] == [(0, cap)]
    assert len(res[True]) == len(res[False]) > 3
    for i, (x, y) in enumerate(zip(res[True], res[False])):
        assert torch.equal(x, y), i


@pytest.mark.gpu
def test_graph_replay_with_the_mirror_equals_eager(builds):
    """the captured step (device-side index cursor, the default) reads the mirror the warm-up steps built; six replays equal
    six eager steps bit for bit, and no build became a node of the graph"""
    dev = torch.device("cuda")
    L.lib()
    N, W, cap, B = 6, 2, 8192, 1024
    res = {}
    for mode in ("eager", "graph"):
        loop, tr = _c2_loop(dev, cap, B)
        torch.cuda.manual_seed(77)
        del builds["build"][:], builds["sampler"][:]
        if mode == "eager":
            out = [loop.step().clone() for _ in range(W + N)][W:]
        else:
            step = loop.capture(warmup=W)
            assert loop._graph["cursor"] is not None
            out = [step().clone() for _ in range(N)]
        loop.flush()
        torch.cuda.synchronize()
        assert builds["build"] == [(0, cap)] and all(builds["sampler"]) and loop.rb._mirror is not None
        res[mode] = out + _state(tr)
        assert tr.all_batches_processed == N + W
    for i, (x, y) in enumerate(zip(res["eager"], res["graph"])):
        assert torch.equal(x, y), i


def test_mirror_kernels_use_no_scratch(tmp_path):
    import kernel_remarks

    if not os.path.exists(kernel_remarks.HIPCC):
        pytest.skip("needs hipcc")
    kernels = kernel_remarks.kernel_resources("replay.hip", tmp_path)
    new = {n: r for n, r in kernels.items() if "replay_dqn_batch_kernelILb1E" in n or "replay_mirror_build_kernel" in n}
    assert len(new) == 2, sorted(kernels)
    for name, r in new.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    sampler = next(r for n, r in new.items() if "replay_dqn_batch_kernel" in n)
    assert sampler["LDS Size [bytes/block]"] < 2048  # no image of the column descriptors
