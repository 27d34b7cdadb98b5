"""Seq2RewardNetwork with the surface of reagent/models/seq2reward_model.py:14-95, executed on the HIP kernels: an
nn.LSTM(action_dim, num_hiddens, num_hidden_layers), sequence first, over the actions alone, whose initial hidden state of
every layer is map_linear(state[0]) and whose initial cell is zero; lstm_linear on the hidden state of the last (or each
row's valid) step gives the accumulated reward.  fp32 throughout (PREC_F32), as in MDNRNN.

  forward : rg_fc_forward (map_linear), per layer rg_fc_forward (x W_ih^T + b_ih, all steps) and rg_lstm_forward, then
            rg_seq2reward_head (lstm_linear at the chosen step)
  backward: per layer rg_lstm_backward, rg_fc_wgrad / rg_fc_dgrad; d loss / d embedding = the sum over the layers of dh0, in
            layer order; map_linear's rg_fc_wgrad
  planning: tree_rollout_max — get_Q's enumeration as a prefix tree, a level at a time (rg_lstm_fanout_step,
            rg_seq2reward_plan_max)

The parameters are torch Parameters under torch's own names (rnn.weight_ih_l0, ..., lstm_linear.bias, map_linear.bias),
initialised by constructing nn.LSTM and the two nn.Linear once on the host under the current seed, in the reference's order:
a state_dict moves either way, and the same seed gives the reference's initial weights.  As with MDNRNN, forward carries no
autograd graph: training goes through Seq2RewardTrainer.
"""
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..engine import ensure_slab
from . import lstm_stack
from .base import ModelBase
from .lstm_stack import _f32c, _Parameters

F32 = torch.float32
LINEAR = L.ACT["linear"]


class Seq2RewardNetwork(ModelBase):
    def __init__(self, state_dim, action_dim, num_hiddens, num_hidden_layers) -> None:
        super().__init__()
        if not 1 <= num_hiddens <= L.LSTM_MAX_HIDDEN:
            raise NotImplementedError(f"Seq2RewardNetwork: num_hiddens {num_hiddens} is not supported (1 .. {L.LSTM_MAX_HIDDEN})")
        if not 1 <= num_hidden_layers <= L.LSTM_MAX_LAYERS:
            raise NotImplementedError(f"Seq2RewardNetwork: num_hidden_layers {num_hidden_layers} is not supported "
                                      f"(1 .. {L.LSTM_MAX_LAYERS})")
        assert state_dim >= 1 and action_dim >= 1, (state_dim, action_dim)
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.num_hiddens = num_hiddens
        self.num_hidden_layers = num_hidden_layers
        self.rnn = _Parameters(nn.LSTM(input_size=action_dim, hidden_size=num_hiddens, num_layers=num_hidden_layers))
        self.lstm_linear = _Parameters(nn.Linear(num_hiddens, 1))
        self.map_linear = _Parameters(nn.Linear(state_dim, self.num_hiddens))
        self._wt = lstm_stack.TransposedWeights()

    def input_prototype(self):
        return (
            rlt.FeatureData(torch.randn(1, 1, self.state_dim)),
            rlt.FeatureData(torch.randn(1, 1, self.action_dim)),
        )

    # ---- the recurrence ----------------------------------------------------------------------------------------------
    def _embed(self, state0):
        """map_linear on [B, S] rows -> [B, H]: the initial hidden state of every layer"""
        emb = torch.empty(state0.shape[0], self.num_hiddens, dtype=F32, device=state0.device)
        ops.fc_forward(state0, self.map_linear.weight.detach(), self.map_linear.bias.detach(), LINEAR, L.PREC_F32, y32=emb)
        return emb

    def _run(self, states, actions, save=False):
        """-> the tape of one pass: the first step's state rows, their embedding, per layer the input rows, h_all, c_all and
        (save) the gates"""
        dev = self.lstm_linear.weight.device
        states, actions = states.to(dev), actions.to(dev)
        L.require_cuda(actions, "action")
        assert actions.ndim == 3 and states.ndim == 3 and actions.shape[1] == states.shape[1], (actions.shape, states.shape)
        assert actions.shape[2] == self.action_dim and states.shape[2] == self.state_dim
        T, B = actions.shape[0], actions.shape[1]
        state0 = _f32c(states[0])
        emb = self._embed(state0)
        x = _f32c(actions).view(T * B, -1)
        return dict(T=T, B=B, state0=state0, emb=emb,
                    **lstm_stack.forward(self.rnn, x, T, B, self.num_hiddens, self.num_hidden_layers, emb, None, save))

    def _head_params(self):
        return self.lstm_linear.weight.detach().view(-1), self.lstm_linear.bias.detach()

    @staticmethod
    def _steps(valid_reward_len, B, dev):
        v = valid_reward_len.to(dev).flatten()
        v = v if v.dtype == torch.int64 else v.long()
        assert v.numel() == B, (v.shape, B)
        return v if v.is_contiguous() else v.contiguous()

    def forward(self, state: rlt.FeatureData, action: rlt.FeatureData, valid_reward_len: Optional[torch.Tensor] = None):
        """:35-70 — Seq2RewardOutput(acc_reward [B, 1]): lstm_linear on the last step's hidden state, or on step
        valid_reward_len - 1 of each row (clamped into the sequence, where the reference would index outside it).  No
        gradient flows through it."""
        tape = self._run(state.float_features, action.float_features, save=False)
        B, dev = tape["B"], tape["emb"].device
        acc = torch.empty(B, dtype=F32, device=dev)
        w, b = self._head_params()
        ops.seq2reward_head(tape["h"][-1], None if valid_reward_len is None else self._steps(valid_reward_len, B, dev), None,
                            None, w, b, acc)
        return rlt.Seq2RewardOutput(acc_reward=acc.view(B, 1))

    def get_initial_hidden_state(self, state, batch_size: int = 1):
        """:72-95 — (h0, c0) [num_hidden_layers, B, H] from state [1, B, S]: every layer's h0 is map_linear(state[0]), c0 is
        zero"""
        dev = self.lstm_linear.weight.device
        emb = self._embed(_f32c(state.to(dev)[0]))
        hidden = emb.unsqueeze(0).repeat(self.num_hidden_layers, 1, 1)
        return hidden, torch.zeros(self.num_hidden_layers, batch_size, self.num_hiddens, device=dev)

    # ---- planning ----------------------------------------------------------------------------------------------------
    def tree_rollout_max(self, cur_state, multi_steps: int, num_action: int):
        """get_Q's value [B, A] for cur_state [B, S] without the enumeration: the A^multi_steps action sequences in lexical
        order are the leaves of a tree whose depth-t level has B * A^t distinct rows; row r of a level continues row r // A
        of the level above with action r % A.  Per depth and layer one rg_lstm_fanout_step (layer 0 reads its input
        projection from the A rows of the projected identity; a layer above runs rg_fc_forward on the child rows of the
        layer below first).  Two levels of (h, c) per layer are kept, written alternately; then lstm_linear and the max over
        the leaves of each first action (rg_seq2reward_plan_max)."""
        A, H, nl = int(num_action), self.num_hiddens, self.num_hidden_layers
        assert A == self.action_dim and multi_steps >= 1
        B, dev = cur_state.shape[0], cur_state.device
        f = dict(dtype=F32, device=dev)
        emb = self._embed(_f32c(cur_state))
        layers = [tuple(p.detach() for p in lstm_stack.layer_params(self.rnn, k)) for k in range(nl)]
        table = torch.empty(A, 4 * H, **f)
        ops.fc_forward(torch.eye(A, **f), layers[0][0], layers[0][2], LINEAR, L.PREC_F32, y32=table)
        rows = [B * A ** t for t in range(multi_steps + 1)]
        # level t lives in slot t % 2; the root level is the embedding itself (and a zero cell: no buffer)
        size = [max([rows[t] for t in range(1, multi_steps + 1) if t % 2 == s], default=0) for s in (0, 1)]
        hc = [[(torch.empty(size[s] * H, **f), torch.empty(size[s] * H, **f)) for s in (0, 1)] for _ in range(nl)]
        xproj = torch.empty(rows[-1] * 4 * H, **f) if nl > 1 else None
        for t in range(1, multi_steps + 1):
            n = rows[t]
            for k in range(nl):
                w_ih, w_hh, b_ih, b_hh = layers[k]
                h_prev = emb if t == 1 else hc[k][(t - 1) % 2][0][:rows[t - 1] * H].view(rows[t - 1], H)
                c_prev = None if t == 1 else hc[k][(t - 1) % 2][1][:rows[t - 1] * H].view(rows[t - 1], H)
                h, c = (b[:n * H].view(n, H) for b in hc[k][t % 2])
                if k == 0:
                    ops.lstm_fanout_step(h_prev, c_prev, table, True, w_hh, b_hh, A, h, c)
                else:
                    xp = xproj[:n * 4 * H].view(n, 4 * H)
                    ops.fc_forward(below, w_ih, b_ih, LINEAR, L.PREC_F32, y32=xp)
                    ops.lstm_fanout_step(h_prev, c_prev, xp, False, w_hh, b_hh, A, h, c)
                below = h
        q = torch.empty(B * A, **f)
        w, b = self._head_params()
        ops.seq2reward_plan_max(below, w, b, A ** (multi_steps - 1), q)
        return q.view(B, A)

    def tree_rollout_floats_per_row(self, multi_steps: int, num_action: int) -> int:
        """fp32 values of workspace tree_rollout_max allocates per row of cur_state"""
        A, H, nl = int(num_action), self.num_hiddens, self.num_hidden_layers
        per = 2 * nl * H * (A ** multi_steps + (A ** (multi_steps - 1) if multi_steps > 1 else 0))
        return per + (4 * H * A ** multi_steps if nl > 1 else 0) + H + A

    # ---- the backward ------------------------------------------------------------------------------------------------
    def backward(self, tape, dh_top, dw_head, db_head):
        """d loss / d every parameter from a saving pass and the head's outputs (dh_top [T, B, H] = d loss / d the top layer's
        h_all, dw_head [H] and db_head [1] = lstm_linear's gradients), written into the parameters' gradient slab (the caller
        publishes it).  Per layer, from the top: rg_lstm_backward with dh0, then dW_ih and db_ih = rg_fc_wgrad(dgates, x),
        dW_hh and db_hh = rg_fc_wgrad(dgates, [embedding; h_all[:-1]]), dx = rg_fc_dgrad(dgates, W_ih).  Every layer starts
        from the same embedding: its gradient is dh0 of layer 0 + layer 1 + ..., and map_linear's gradients are
        rg_fc_wgrad(that, state[0])."""
        params = list(self.parameters())
        slab = ensure_slab(params)
        grad = {id(p): slab.view(slab.grad, i) for i, p in enumerate(params)}
        grad[id(self.lstm_linear.weight)].view(-1).copy_(dw_head)
        grad[id(self.lstm_linear.bias)].copy_(db_head)
        dh0 = lstm_stack.backward(self.rnn, tape, dh_top, grad, tape["emb"], None, self._wt, want_dh0=True)
        demb = dh0[0]
        for k in range(1, self.num_hidden_layers):
            demb = demb + dh0[k]
        gw, gb = self.map_linear.weight, self.map_linear.bias
        lstm_stack.wgrad(lstm_stack.transposed(demb), lstm_stack.transposed(tape["state0"]), grad[id(gw)], grad[id(gb)],
                         tape["B"])
        return slab
