"""The Seq2Reward kernels (reagent_amd/csrc/seq2reward.hip): rg_lstm_fanout_step, rg_seq2reward_plan_max, the prefix-tree
rollout of get_Q they make, rg_seq2reward_head and rg_step_ce_head.

The planning kernels are held to exact statements: a fan-out child has the bits of rg_lstm_forward(seq_len = 1) on the
materialised rows; the tree rollout has the bits of the flat route (Seq2RewardNetwork.forward on the reference's materialised
repeat_interleave / repeat tensors, seq2reward_trainer.py:43-62); plan_max equals a float64 dot in index order, rounded once,
and torch.max.  The two heads are held to the reference's lines in float64 under autograd with the self-calibrating bound of
tests/test_lstm_kernels.py: the larger of 4 x torch's own fp32 error against float64 on those inputs and 4 ulp (fp32) of the
quantity's largest magnitude."""
import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.core import types as rlt
from reagent_amd.models.seq2reward_model import Seq2RewardNetwork
from reagent_amd.training.utils import gen_permutations
from reagent_amd.training.world_model import seq2reward_trainer as S

from test_lstm_kernels import _bits, _close


# ---- the fan-out step ------------------------------------------------------------------------------------------------------
def _fanout_inputs(H, parents, fanout, seed=0):
    g = torch.Generator().manual_seed(7000 + 100 * H + 10 * parents + fanout + seed)
    k = 1.0 / H ** 0.5
    n = parents * fanout
    return dict(w_hh=(torch.rand(4 * H, H, generator=g) * 2 - 1) * k, b_hh=(torch.rand(4 * H, generator=g) * 2 - 1) * k,
                h_prev=torch.randn(parents, H, generator=g) * 0.5, c_prev=torch.randn(parents, H, generator=g),
                table=torch.randn(fanout, 4 * H, generator=g), dense=torch.randn(n, 4 * H, generator=g))


def _fanout(dev, inp, fanout, from_table, with_c=True):
    d = {k: v.to(dev).contiguous() for k, v in inp.items()}
    parents, H = inp["h_prev"].shape
    n = parents * fanout
    h, c = torch.full((n, H), float("nan"), device=dev), torch.full((n, H), float("nan"), device=dev)
    ops.lstm_fanout_step(d["h_prev"], d["c_prev"] if with_c else None, d["table"] if from_table else d["dense"], from_table,
                         d["w_hh"], d["b_hh"], fanout, h, c)
    return h.cpu(), c.cpu()


def _materialised(dev, inp, fanout, from_table, with_c=True):
    """rg_lstm_forward with seq_len = 1 on the rows the children stand for"""
    parents, H = inp["h_prev"].shape
    n = parents * fanout
    h0 = inp["h_prev"].repeat_interleave(fanout, dim=0).contiguous().to(dev)
    c0 = inp["c_prev"].repeat_interleave(fanout, dim=0).contiguous().to(dev) if with_c else None
    xproj = (inp["table"][torch.arange(n) % fanout] if from_table else inp["dense"]).contiguous().view(1, n, 4 * H).to(dev)
    h, c = torch.empty(1, n, H, device=dev), torch.empty(1, n, H, device=dev)
    ops.lstm_forward(xproj, inp["w_hh"].to(dev), inp["b_hh"].to(dev), h0, c0, h, c)
    return h[0].cpu(), c[0].cpu()


@pytest.mark.parametrize("H,parents,fanout", [(H, p, f) for H in (1, 31, 33, 65) for p in (1, 33) for f in (1, 2, 3)]
                         + [(256, 1, 2)])
def test_fanout_step_has_the_bits_of_the_sequence_kernel(backend, H, parents, fanout):
    inp = _fanout_inputs(H, parents, fanout)
    for from_table in (True, False):
        got, want = _fanout(backend.device, inp, fanout, from_table), _materialised(backend.device, inp, fanout, from_table)
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), from_table


def test_fanout_step_without_a_cell_is_a_zero_cell(backend):
    inp = _fanout_inputs(33, 33, 2)
    got = _fanout(backend.device, inp, 2, True, with_c=False)
    want = _fanout(backend.device, dict(inp, c_prev=torch.zeros_like(inp["c_prev"])), 2, True)
    flat = _materialised(backend.device, inp, 2, True, with_c=False)
    for a, b, c in zip(got, want, flat):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


def test_a_child_depends_on_its_parent_row_and_projection_row_alone(backend):
    H, parents, fanout, r = 33, 33, 3, 50
    inp = _fanout_inputs(H, parents, fanout)
    for from_table in (True, False):
        whole = _fanout(backend.device, inp, fanout, from_table)
        proj = inp["table"][r % fanout:r % fanout + 1] if from_table else inp["dense"][r:r + 1]
        one = dict(inp, h_prev=inp["h_prev"][r // fanout:r // fanout + 1], c_prev=inp["c_prev"][r // fanout:r // fanout + 1],
                   table=proj, dense=proj)
        alone = _fanout(backend.device, one, 1, from_table)
        assert torch.equal(_bits(whole[0][r]), _bits(alone[0][0])) and torch.equal(_bits(whole[1][r]), _bits(alone[1][0]))
        other = dict(inp, h_prev=inp["h_prev"].clone(), c_prev=inp["c_prev"].clone())
        other["h_prev"][r // fanout + 1] += 1.0  # another parent's state changes: this child does not
        other["c_prev"][r // fanout - 1] -= 1.0
        changed = _fanout(backend.device, other, fanout, from_table)
        assert torch.equal(_bits(whole[0][r]), _bits(changed[0][r])) and not torch.equal(_bits(whole[0]), _bits(changed[0]))


def test_two_runs_give_the_same_bits(backend):
    inp = _fanout_inputs(65, 33, 3)
    a, b = _fanout(backend.device, inp, 3, False), _fanout(backend.device, inp, 3, False)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


# ---- get_Q: the tree against the flat route ------------------------------------------------------------------------------
def _network(S_, A, H, layers, dev, seed=5):
    torch.manual_seed(seed)
    return Seq2RewardNetwork(state_dim=S_, action_dim=A, num_hiddens=H, num_hidden_layers=layers).to(dev)


def _flat_q(net, cur_state, all_permut):
    """the reference's get_Q statement on this package's forward: every sequence materialised"""
    batch_size = cur_state.shape[0]
    _, num_permut, num_action = all_permut.shape
    state = cur_state.unsqueeze(0).repeat_interleave(num_permut, dim=1)
    action = all_permut.to(cur_state.device).repeat(1, batch_size, 1)
    acc = net(rlt.FeatureData(state), rlt.FeatureData(action)).acc_reward.reshape(batch_size, num_action, num_permut // num_action)
    return torch.max(acc, dim=2).values


TREE = [(A, steps, B, layers, H) for A in (2, 3) for steps in (1, 2, 3) for B in (1, 33) for layers in (1, 2) for H in (31, 33)]


def _tree_cost(A, steps, B, layers, H):
    """MFMA steps of the flat route on the interpreter, as _emu_cost of tests/test_lstm_kernels.py counts them"""
    hp = (H + 31) // 32 * 32
    return layers * steps * hp * ((B * A ** steps + 31) // 32)


TREE_SMALL = [c for c in TREE if _tree_cost(*c) <= 2000]
TREE_LARGE = [c for c in TREE if _tree_cost(*c) > 2000]
assert {c[0] for c in TREE_SMALL} == {2, 3} and {c[1] for c in TREE_SMALL} == {1, 2, 3} and {c[2] for c in TREE_SMALL} == {1, 33}


def _check_tree(dev, A, steps, B, layers, H):
    net = _network(4, A, H, layers, dev)
    g = torch.Generator().manual_seed(100 * A + 10 * steps + B)
    cur_state = torch.randn(B, 4, generator=g).to(dev)
    all_permut = gen_permutations(steps, A)
    tree = S.get_Q(net, cur_state, all_permut)
    flat = _flat_q(net, cur_state, all_permut)
    assert tree.shape == flat.shape == (B, A)
    assert torch.equal(_bits(tree), _bits(flat)), (tree - flat).abs().max().item()


@pytest.mark.parametrize("A,steps,B,layers,H", TREE_SMALL)
def test_tree_rollout_has_the_bits_of_the_flat_route(backend, A, steps, B, layers, H):
    _check_tree(backend.device, A, steps, B, layers, H)


@pytest.mark.gpu
@pytest.mark.parametrize("A,steps,B,layers,H", TREE_LARGE)
def test_tree_rollout_has_the_bits_of_the_flat_route_large(A, steps, B, layers, H):
    _check_tree("cuda", A, steps, B, layers, H)


def test_the_projection_table_is_the_projection_of_one_hot_rows(backend):
    """layer 0's input projection of a one-hot row is the identity's row, bit for bit, and that row is W_ih's column plus
    the bias in float64, rounded once"""
    dev = backend.device
    net = _network(4, 3, 33, 1, dev)
    w, b = net.rnn.weight_ih_l0.detach(), net.rnn.bias_ih_l0.detach()
    table = torch.empty(3, 4 * 33, device=dev)
    ops.fc_forward(torch.eye(3, device=dev), w, b, L.ACT["linear"], L.PREC_F32, y32=table)
    x = gen_permutations(2, 3).reshape(-1, 3).to(dev).contiguous()
    rows = torch.empty(x.shape[0], 4 * 33, device=dev)
    ops.fc_forward(x, w, b, L.ACT["linear"], L.PREC_F32, y32=rows)
    assert torch.equal(_bits(rows), _bits(table[x.argmax(1)]))
    assert torch.equal(_bits(table), _bits((w.double().t() + b.double()).float()))


def test_two_batch_chunkings_give_the_same_bits(backend, monkeypatch):
    dev = backend.device
    net = _network(4, 2, 33, 2, dev)
    cur_state = torch.randn(7, 4, generator=torch.Generator().manual_seed(3)).to(dev)
    all_permut = gen_permutations(3, 2)
    whole = S.get_Q(net, cur_state, all_permut)
    per_row = 4 * net.tree_rollout_floats_per_row(3, 2)
    for rows in (1, 3):
        monkeypatch.setattr(S, "GET_Q_WORKSPACE_BYTES", rows * per_row)
        assert torch.equal(_bits(S.get_Q(net, cur_state, all_permut)), _bits(whole)), rows
    assert S.GET_Q_WORKSPACE_BYTES == 3 * per_row


# ---- plan_max ------------------------------------------------------------------------------------------------------------
def _ordered_dot(h, w, b):
    """h . w + b in float64 in index order, rounded once"""
    return torch.from_numpy((np.cumsum(h.double().numpy() * w.double().numpy(), axis=1)[:, -1] + float(b)).astype(np.float32))


@pytest.mark.parametrize("size", [1, 3, 300])
def test_plan_max_is_the_ordered_dot_and_torch_max(backend, size):
    dev, H, groups = backend.device, 33, 7
    g = torch.Generator().manual_seed(size)
    h = torch.randn(groups * size, H, generator=g)
    w, b = torch.randn(H, generator=g).abs() + 0.1, torch.randn(1, generator=g)
    if size > 1:
        h[size + 1] = h[size]  # a tie inside group 1
        h[2 * size:3 * size, 0] = float("-inf")  # all of group 2 (w > 0)
        h[3 * size + 1, 5] = float("-inf")  # one leaf of group 3
        h[4 * size + size // 2, 2] = float("nan")  # a NaN inside group 4
        h[5 * size + size - 1] = 100.0  # the max is the last leaf
    else:
        h[2, 0], h[4, 2] = float("-inf"), float("nan")
    with np.errstate(invalid="ignore"):
        acc = _ordered_dot(h, w, b)
    want = torch.max(acc.view(groups, size), dim=1).values
    q = torch.full((groups,), 7.0, device=dev)
    ops.seq2reward_plan_max(h.to(dev), w.to(dev), b.to(dev), size, q)
    q = q.cpu()
    assert torch.isnan(want[4]) and want[2] == float("-inf") and torch.isfinite(want[[0, 1, 3, 5, 6]]).all()
    assert torch.equal(torch.isnan(q), torch.isnan(want))
    assert torch.equal(_bits(torch.nan_to_num(q, nan=0.0)), _bits(torch.nan_to_num(want, nan=0.0)))


# ---- the two heads -------------------------------------------------------------------------------------------------------
def _head_statement(dtype, h_all, valid_step, reward, gamma, w, b):
    """seq2reward_model.py:65-68 and seq2reward_trainer.py:225-245 in dtype -> (acc_reward, loss, dh_all, dw, db)"""
    T, B, _ = h_all.shape
    h = h_all.to(dtype).requires_grad_(True)
    w_, b_ = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    v = valid_step.clamp(1, T)
    acc = torch.nn.functional.linear(h[v - 1, torch.arange(B)], w_.view(1, -1), b_)
    gamma_mask = torch.Tensor([[gamma ** i for i in range(T)] for _ in range(B)]).transpose(0, 1).to(dtype)
    target = torch.cumsum(reward.to(dtype) * gamma_mask, dim=0)[v - 1, torch.arange(B)].unsqueeze(1)
    loss = torch.nn.MSELoss(reduction="mean")(acc, target)
    loss.backward()
    return acc.detach().view(B), loss.detach(), h.grad, w_.grad, b_.grad


def _run_head(dev, h_all, valid_step, reward, gamma, w, b):
    T, B, H = h_all.shape
    f = dict(dtype=torch.float32, device=dev)
    acc, loss = torch.full((B,), float("nan"), **f), torch.full((1,), float("nan"), **f)
    dh, dw, db = torch.full((T, B, H), float("nan"), **f), torch.full((H,), float("nan"), **f), torch.full((1,), float("nan"), **f)
    partials = torch.empty((H + 2) * ops.seq2reward_head_partials(B), dtype=torch.float64, device=dev)
    gamma_pow = torch.Tensor([gamma ** i for i in range(T)]).to(dev)
    ops.seq2reward_head(h_all.to(dev), valid_step.to(dev), reward.to(dev), gamma_pow, w.to(dev), b.to(dev), acc, dh, dw, db,
                        partials, loss)
    return acc.cpu(), loss.cpu()[0], dh.cpu(), dw.cpu(), db.cpu()


def _head_inputs(T, B, H, steps):
    g = torch.Generator().manual_seed(1000 * T + 10 * B + H)
    h_all = torch.tanh(torch.randn(T, B, H, generator=g))
    reward = torch.randn(T, B, generator=g)
    w, b = (torch.rand(H, generator=g) * 2 - 1) / H ** 0.5, torch.randn(1, generator=g)
    if steps == "ends":
        v = torch.where(torch.arange(B) % 2 == 0, torch.tensor(1), torch.tensor(T))
    elif steps == "outside":
        v = torch.tensor([0, -5, T + 1, T + 40, 2])[torch.arange(B) % 5]
    else:
        v = torch.randint(1, T + 1, (B,), generator=g)
    return h_all, v.long(), reward, w, b


@pytest.mark.parametrize("T,B,H,gamma,steps", [(1, 1, 8, 1.0, "mixed"), (4, 33, 33, 0.9, "mixed"), (3, 65, 31, 1.0, "ends"),
                                               (6, 33, 65, 0.5, "outside"), (5, 300, 8, 0.99, "mixed")])
def test_seq2reward_head_against_float64(backend, T, B, H, gamma, steps):
    h_all, v, reward, w, b = _head_inputs(T, B, H, steps)
    r64 = _head_statement(torch.float64, h_all, v, reward, gamma, w, b)
    r32 = _head_statement(torch.float32, h_all, v, reward, gamma, w, b)
    got = _run_head(backend.device, h_all, v, reward, gamma, w, b)
    tag = f"T={T} B={B} H={H} {steps}"
    for name, a, x, y in zip(("acc_reward", "loss", "dh_all", "dw", "dbias"), got, r64, r32):
        _close(a, x, y, f"{name} {tag}")
    off = torch.ones(T, B, dtype=torch.bool)
    off[v.clamp(1, T) - 1, torch.arange(B)] = False
    assert torch.equal(_bits(got[2][off]), torch.zeros(int(off.sum()), H, dtype=torch.int32))  # exactly +0 off the valid step
    if steps == "outside":  # the clamp: the same bits as the clamped steps
        again = _run_head(backend.device, h_all, v.clamp(1, T), reward, gamma, w, b)
        for a, c in zip(got, again):
            assert torch.equal(_bits(a), _bits(c))
    # the forward alone: the same acc_reward bits; without steps, the last step's
    dev = backend.device
    acc = torch.empty(B, device=dev)
    ops.seq2reward_head(h_all.to(dev), v.to(dev), None, None, w.to(dev), b.to(dev), acc)
    assert torch.equal(_bits(acc), _bits(got[0]))
    ops.seq2reward_head(h_all.to(dev), None, None, None, w.to(dev), b.to(dev), acc)
    last = _run_head(dev, h_all, torch.full((B,), T), reward, gamma, w, b)
    assert torch.equal(_bits(acc), _bits(last[0]))
    again = _run_head(dev, h_all, v, reward, gamma, w, b)
    assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(got, again))  # two runs, the same bits


def _ce_statement(dtype, logits, valid_step):
    K = logits.shape[1]
    z = logits.to(dtype).requires_grad_(True)
    loss = torch.nn.CrossEntropyLoss(reduction="mean")(z, valid_step.clamp(1, K) - 1)
    loss.backward()
    return loss.detach(), z.grad, torch.nn.functional.softmax(logits.to(dtype), dim=1)


@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("K", [1, 2, 32])
def test_step_ce_head_against_float64(backend, B, K):
    dev = backend.device
    g = torch.Generator().manual_seed(100 * B + K)
    logits = torch.randn(B, K, generator=g) * 3
    v = torch.randint(1, K + 1, (B,), generator=g)
    v[0], v[-1] = 1, K
    if B > 2:
        v[1], v[2] = -3, K + 7  # the clamp
    r64, r32 = _ce_statement(torch.float64, logits, v), _ce_statement(torch.float32, logits, v)
    f = dict(dtype=torch.float32, device=dev)
    d, p, loss = torch.full((B, K), float("nan"), **f), torch.full((B, K), float("nan"), **f), torch.full((1,), float("nan"), **f)
    partials = torch.empty(ops.step_ce_head_partials(B), dtype=torch.float64, device=dev)
    ops.step_ce_head(logits.to(dev), v.to(dev), d, p, partials, loss)
    tag = f"B={B} K={K}"
    _close(loss[0], r64[0], r32[0], f"step loss {tag}")
    _close(d, r64[1], r32[1], f"dlogits {tag}")
    _close(p, r64[2], r32[2], f"softmax {tag}")
    alone = torch.full((B, K), float("nan"), **f)
    ops.step_ce_head(logits.to(dev), None, softmax=alone)  # get_step_prediction's call: the same bits
    assert torch.equal(_bits(alone), _bits(p))


def test_get_step_prediction_is_the_heads_softmax(backend):
    from reagent_amd import synthetic
    from reagent_amd.models.fully_connected_network import FullyConnectedNetwork

    dev = backend.device
    torch.manual_seed(2)
    net = FullyConnectedNetwork([4, 8, 8, 3], ["relu", "relu", "linear"], use_layer_norm=False)
    net.precision = L.PREC_F32
    net = net.to(dev)
    batch = synthetic.to_seq2reward_input(synthetic.seq2reward_batch(3, 5, 4, 2, seed=1), dev)
    got = S.get_step_prediction(net, batch)
    logits = net(batch.state.float_features[0])
    want = torch.empty_like(logits)
    ops.step_ce_head(logits, None, softmax=want)
    assert got.shape == (5, 3) and torch.equal(_bits(got), _bits(want))
    assert (got.cpu().double() - torch.softmax(logits.cpu().double(), 1)).abs().max() < 1e-6


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    i = torch.ones(8, dtype=torch.int64, device=dev)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    p, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()
    EINVAL = -1

    def fan(parents=1, fanout=1, H=1, table=0, h_prev=p, c_prev=p, proj=p, w=p, b=p, h=p, c=p):
        return lib.rg_lstm_fanout_step(h_prev, c_prev, proj, table, w, b, parents, fanout, H, h, c, s)

    assert fan() == 0 and fan(c_prev=None, b=None) == 0 and fan(table=1) == 0
    assert fan(H=257) == L.EUNSUPPORTED and fan(parents=1 << 15, fanout=1 << 14) == L.EUNSUPPORTED
    assert fan(parents=1 << 20, fanout=1 << 20) == L.EUNSUPPORTED
    for k in ("parents", "fanout", "H"):
        assert fan(**{k: 0}) == EINVAL
    assert fan(table=-1) == EINVAL
    for k in ("h_prev", "proj", "w", "h", "c"):
        assert fan(**{k: None}) == EINVAL

    def plan(groups=1, size=1, H=1, h=p, w=p, b=p, q=p):
        return lib.rg_seq2reward_plan_max(h, w, b, groups, size, H, q, s)

    assert plan() == 0 and plan(groups=1 << 15, size=1 << 14) == L.EUNSUPPORTED
    for k in ("groups", "size", "H"):
        assert plan(**{k: 0}) == EINVAL
    for k in ("h", "w", "b", "q"):
        assert plan(**{k: None}) == EINVAL

    def head(T=1, B=1, H=1, h=p, v=i.data_ptr(), r=p, gp=p, w=p, b=p, acc=p, dh=p, dw=p, db=p, part=d.data_ptr(), loss=p):
        return lib.rg_seq2reward_head(h, v, r, gp, w, b, T, B, H, acc, dh, dw, db, part, loss, s)

    assert head() == 0 and head(v=None) == 0 and head(r=None, gp=None, dh=None, dw=None, db=None, part=None, loss=None) == 0
    assert head(T=1 << 15, B=1 << 14) == L.EUNSUPPORTED
    for k in ("T", "B", "H"):
        assert head(**{k: 0}) == EINVAL
    for k in ("h", "w", "b", "acc", "r", "gp", "dw", "db", "part", "loss"):
        assert head(**{k: None}) == EINVAL
    assert lib.rg_seq2reward_head_partials(0) == 0 and lib.rg_seq2reward_head_partials(257) == 2

    def ce(B=1, K=1, z=p, v=i.data_ptr(), dz=p, sm=p, part=d.data_ptr(), loss=p):
        return lib.rg_step_ce_head(z, v, B, K, dz, sm, part, loss, s)

    assert ce() == 0 and ce(sm=None) == 0 and ce(v=None, dz=None, part=None, loss=None) == 0
    assert ce(K=33) == L.EUNSUPPORTED and ce(B=0) == EINVAL and ce(K=0) == EINVAL
    for k in ("z", "dz", "part", "loss"):
        assert ce(**{k: None}) == EINVAL
    assert ce(v=None, sm=None) == EINVAL
    assert lib.rg_step_ce_head_partials(0) == 0 and lib.rg_step_ce_head_partials(9) == 2


def test_refusals_by_name(backend):
    dev = backend.device
    f = dict(dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="hidden size 257"):
        ops.lstm_fanout_step(torch.zeros(1, 257, **f), None, torch.zeros(1, 4 * 257, **f), True, torch.zeros(4 * 257, 257, **f),
                             None, 1, torch.zeros(1, 257, **f), torch.zeros(1, 257, **f))
    with pytest.raises(NotImplementedError, match="33 classes"):
        ops.step_ce_head(torch.zeros(1, 33, **f), None, softmax=torch.zeros(1, 33, **f))
    net = _network(4, 2, 8, 1, dev)
    state = torch.zeros(3, 4, **f)
    with pytest.raises(NotImplementedError, match="reagent_amd Seq2RewardNetwork"):
        S.get_Q(torch.nn.Linear(2, 2), state, gen_permutations(2, 2))
    with pytest.raises(NotImplementedError, match="not gen_permutations' lexical"):
        S.get_Q(net, state, gen_permutations(2, 2).flip(1))
    with pytest.raises(NotImplementedError, match="not gen_permutations'"):
        S.get_Q(net, state, gen_permutations(2, 2)[:, :3])
    with pytest.raises(NotImplementedError, match="not gen_permutations'"):
        S.get_Q(net, state, gen_permutations(2, 2)[0])
    with pytest.raises(NotImplementedError, match="33 actions"):
        S.get_Q(net, state, torch.zeros(1, 33, 33))
    with pytest.raises(NotImplementedError, match=r"2 \*\* 21 action sequences"):
        S.get_Q(net, state, torch.zeros(21, 1, 2).expand(21, 1 << 21, 2))
    permut = gen_permutations(2, 2)
    S.get_Q(net, state, permut)
    assert permut._rg_lexical == permut._version  # the content is checked once per tensor object
    permut[0, 0, 0] = 0.0  # ... and again after the tensor was written to
    with pytest.raises(NotImplementedError, match="lexical"):
        S.get_Q(net, state, permut)
