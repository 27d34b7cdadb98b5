"""MDNRNN with the surface of reagent/models/mdn_rnn.py, executed on the HIP kernels: an nn.LSTM(num_layers = L), sequence
first, over cat([actions, states], -1) (rg_fc_forward for x W_ih^T + b_ih of all steps at once, rg_lstm_forward for the
recurrence, a launch per layer), gmm_linear (rg_fc_forward) and the mixture-density split (rg_mdn_outputs).  fp32 throughout.

The parameters are torch Parameters under torch's own names (rnn.weight_ih_l0, ..., gmm_linear.bias), initialised by
constructing nn.LSTM and nn.Linear once on the host under the current seed, in the reference's order: a state_dict moves
either way between this class and the reference's, and the same seed gives the reference's initial weights.

Also here, restated: gmm_loss (the reference's signature, on rg_mdn_gmm_nll), MDNRNNMemoryPool, MDNRNNMemorySample, transpose.
"""
from collections import deque
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..engine import ensure_slab
from . import lstm_stack
from .lstm_stack import _f32c, _Parameters

F32 = torch.float32
LINEAR = L.ACT["linear"]


class MDNRNN(nn.Module):
    """Mixture Density Network - Recurrent Neural Network"""

    def __init__(self, state_dim, action_dim, num_hiddens, num_hidden_layers, num_gaussians, *, dropout=0.0,
                 bidirectional=False, proj_size=0):
        super().__init__()
        for name, value in (("dropout", dropout), ("bidirectional", bidirectional), ("proj_size", proj_size)):
            if value:
                raise NotImplementedError(f"MDNRNN: an LSTM with {name} is not supported (the reference's has none)")
        if not 1 <= num_hiddens <= L.LSTM_MAX_HIDDEN:
            raise NotImplementedError(f"MDNRNN: num_hiddens {num_hiddens} is not supported (1 .. {L.LSTM_MAX_HIDDEN})")
        if not 1 <= num_hidden_layers <= L.LSTM_MAX_LAYERS:
            raise NotImplementedError(f"MDNRNN: num_hidden_layers {num_hidden_layers} is not supported (1 .. {L.LSTM_MAX_LAYERS})")
        if not 1 <= num_gaussians <= L.MDN_MAX_GAUSSIANS:
            raise NotImplementedError(f"MDNRNN: num_gaussians {num_gaussians} is not supported (1 .. {L.MDN_MAX_GAUSSIANS})")
        if state_dim < 1 or action_dim < 1 or state_dim + action_dim > L.MDN_MAX_STATE_DIM:
            raise NotImplementedError(f"MDNRNN: state_dim + action_dim = {state_dim + action_dim} is not supported "
                                      f"(both at least 1, together at most {L.MDN_MAX_STATE_DIM})")
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.num_hiddens = num_hiddens
        self.num_hidden_layers = num_hidden_layers
        self.num_gaussians = num_gaussians
        self.rnn = _Parameters(nn.LSTM(input_size=state_dim + action_dim, hidden_size=num_hiddens, num_layers=num_hidden_layers))
        self.gmm_linear = _Parameters(nn.Linear(num_hiddens, (2 * state_dim + 1) * num_gaussians + 2))
        self._wt = lstm_stack.TransposedWeights()

    # ---- the recurrence ----------------------------------------------------------------------------------------------
    def _run(self, actions, states, hidden=None, save=False):
        """-> the tape of one pass: z [T * B, W] = gmm_linear's output, per layer the input rows, h_all, c_all and (save) the
        gates, and the initial state"""
        dev = self.gmm_linear.weight.device
        actions, states = actions.to(dev), states.to(dev)
        L.require_cuda(actions, "actions")
        assert actions.ndim == 3 and states.ndim == 3 and actions.shape[:2] == states.shape[:2], (actions.shape, states.shape)
        assert actions.shape[2] == self.action_dim and states.shape[2] == self.state_dim
        T, B = actions.shape[0], actions.shape[1]
        N, H = T * B, self.num_hiddens
        f = dict(dtype=F32, device=dev)
        h0 = c0 = None
        if hidden is not None:
            h0, c0 = _f32c(hidden[0].to(dev)), _f32c(hidden[1].to(dev))
            assert h0.shape == c0.shape == (self.num_hidden_layers, B, H), (h0.shape, c0.shape)
        x = _f32c(torch.cat([actions.float(), states.float()], dim=-1)).view(N, -1)
        tape = dict(T=T, B=B, h0=h0, c0=c0, **lstm_stack.forward(self.rnn, x, T, B, H, self.num_hidden_layers, h0, c0, save))
        z = torch.empty(N, self.gmm_linear.weight.shape[0], **f)
        top = tape["h"][-1].view(N, H)
        ops.fc_forward(top, self.gmm_linear.weight.detach(), self.gmm_linear.bias.detach(), LINEAR, L.PREC_F32, y32=z)
        tape["z"] = z
        return tape

    def _split(self, tape, sigmas, logpi):
        """the reference's seven values from a tape and the head's (or rg_mdn_outputs') sigmas and logpi"""
        T, B, G, S = tape["T"], tape["B"], self.num_gaussians, self.state_dim
        z = tape["z"].view(T, B, -1)
        stride = G * S
        mus = z[:, :, :stride].view(T, B, G, S)
        h_n = torch.stack([h[-1] for h in tape["h"]])
        c_n = torch.stack([c[-1] for c in tape["c"]])
        return (mus, sigmas.view(T, B, G, S), logpi.view(T, B, G), z[:, :, -2], z[:, :, -1], tape["h"][-1], (h_n, c_n))

    def forward(self, actions: torch.Tensor, states: torch.Tensor, hidden=None):
        """:47-102 — (mus, sigmas, logpi, reward, not_terminal, all_steps_hidden, (h_n, c_n)); no gradient flows through it:
        training goes through MDNRNNTrainer, whose backward is the kernels'"""
        tape = self._run(actions, states, hidden, save=False)
        N, G, S = tape["T"] * tape["B"], self.num_gaussians, self.state_dim
        f = dict(dtype=F32, device=tape["z"].device)
        sigmas, logpi = torch.empty(N, G, S, **f), torch.empty(N, G, **f)
        ops.mdn_outputs(tape["z"], G, S, sigmas, logpi)
        return self._split(tape, sigmas, logpi)

    def get_initial_hidden_state(self, batch_size=1):
        return (torch.zeros(self.num_hidden_layers, batch_size, self.num_hiddens),
                torch.zeros(self.num_hidden_layers, batch_size, self.num_hiddens))

    # ---- the backward ------------------------------------------------------------------------------------------------
    def backward(self, tape, dz):
        """d loss / d every parameter from dz = d loss / d gmm_linear's output of a saving pass, written into the parameters'
        gradient slab (the caller publishes it).  Per layer, from the top: rg_lstm_backward, then dW_ih and db_ih =
        rg_fc_wgrad(dgates, x), dW_hh and db_hh = rg_fc_wgrad(dgates, [h0; h_all[:-1]]), dx = rg_fc_dgrad(dgates, W_ih)."""
        params = list(self.parameters())
        slab = ensure_slab(params)
        grad = {id(p): slab.view(slab.grad, i) for i, p in enumerate(params)}
        T, B, H = tape["T"], tape["B"], self.num_hiddens
        N, dev = T * B, dz.device
        f = dict(dtype=F32, device=dev)
        transposed = lstm_stack.transposed
        gw, gb = self.gmm_linear.weight, self.gmm_linear.bias
        lstm_stack.wgrad(transposed(dz), transposed(tape["h"][-1].view(N, H)), grad[id(gw)], grad[id(gb)], N)
        dh = torch.empty(N, H, **f)
        ops.fc_dgrad(dz, self._wt("gmm", gw), None, LINEAR, L.PREC_F32, dx32=dh)
        lstm_stack.backward(self.rnn, tape, dh, grad, tape["h0"], tape["c0"], self._wt, want_dh0=False)
        return slab


class MDNRNNMemorySample(NamedTuple):
    state: np.ndarray
    action: np.ndarray
    next_state: np.ndarray
    reward: float
    not_terminal: float


class MDNRNNMemoryPool:
    """:121-178 — a deque of whole sequences; sample_memories draws with np.random.randint as the reference does, so a
    seeded run samples the same indices"""

    def __init__(self, max_replay_memory_size):
        self.replay_memory = deque(maxlen=max_replay_memory_size)
        self.max_replay_memory_size = max_replay_memory_size
        self.accu_memory_num = 0

    def deque_sample(self, indices):
        for i in indices:
            s = self.replay_memory[i]
            yield s.state, s.action, s.next_state, s.reward, s.not_terminal

    def sample_memories(self, batch_size, use_gpu=False) -> rlt.MemoryNetworkInput:
        """state / next_state [seq_len, batch_size, state_dim], action [seq_len, batch_size, action_dim], reward /
        not_terminal [seq_len, batch_size]"""
        sample_indices = np.random.randint(self.memory_size, size=batch_size)
        device = torch.device("cuda") if use_gpu else torch.device("cpu")
        columns = zip(*self.deque_sample(sample_indices))
        state, action, next_state, reward, not_terminal = transpose(
            *(torch.stack([torch.as_tensor(np.asarray(v)) for v in col]).float().to(device) for col in columns))
        return rlt.MemoryNetworkInput(
            state=rlt.FeatureData(float_features=state),
            reward=reward,
            time_diff=torch.ones_like(reward).float(),
            action=rlt.FeatureData(float_features=action),
            next_state=rlt.FeatureData(float_features=next_state),
            not_terminal=not_terminal,
            step=None,
        )

    def insert_into_memory(self, state, action, next_state, reward, not_terminal):
        self.replay_memory.append(MDNRNNMemorySample(state=state, action=action, next_state=next_state, reward=reward,
                                                     not_terminal=not_terminal))
        self.accu_memory_num += 1

    @property
    def memory_size(self):
        return min(self.accu_memory_num, self.max_replay_memory_size)


def transpose(*args):
    return [arg.transpose(1, 0) for arg in args]


def gmm_loss(batch, mus, sigmas, logpi, reduce=True):
    """:188-233 — minus the log probability of batch [*, fs] under the mixture mus / sigmas [*, gs, fs], logpi [*, gs]: its
    mean over the leading dimensions, or with reduce=False one value per leading index.  rg_mdn_gmm_nll, then rg_reduce_sum."""
    lead = batch.shape[:-1]
    G, S = mus.shape[-2], mus.shape[-1]
    assert mus.shape == sigmas.shape == (*lead, G, S) and logpi.shape == (*lead, G), (batch.shape, mus.shape, logpi.shape)
    n = 1
    for d in lead:
        n *= d
    nll = torch.empty(n, dtype=F32, device=batch.device)
    ops.mdn_gmm_nll(_f32c(batch).view(n, S), _f32c(mus).view(n, G, S), _f32c(sigmas).view(n, G, S), _f32c(logpi).view(n, G), nll)
    if not reduce:
        return nll.view(lead)
    out = torch.empty(1, dtype=F32, device=batch.device)
    ops.reduce_sum(nll, n, 1.0 / n, out)
    return out.view(())
