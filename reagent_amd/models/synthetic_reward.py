"""The synthetic-reward nets with the surface of reagent/models/synthetic_reward.py, executed on the HIP kernels: a per-step
reward learnt from a reward observed at the end of a sequence.  SyntheticRewardNet wraps one of

  SingleStepSyntheticRewardNet  (:275-308)  an MLP on cat(state, action) of each step
  NGramFullyConnectedNetwork    (:373-405)  an MLP on the step's window of context_size steps (zero padded)
  SequenceSyntheticRewardNet    (:408-453)  an LSTM over cat(state, action) and a Linear on its top layer's hidden states

and masks the steps before the last valid_step, sums, and returns SyntheticRewardNetworkOutput (:245-266).

  input   : rg_ngram_concat — cat(state, action) (n = 1) or the n-gram windows, one launch, no shifted copies
  trunk   : the FC stack over all but the last linear in fp32 (engine.FCStack: rg_fc_forward, rg_layer_norm_*), or
            models/lstm_stack.py (rg_fc_forward, rg_lstm_forward per layer); with sizes == [] the head reads the input rows
  head    : rg_step_reward_head — the last Linear(P, 1), its activation, _gen_mask, the masked sum and, in a trainer, the loss
            and the gradients into the trunk's output and the last linear
  backward: the stack's backward from d loss / d (trunk output), or lstm_stack.backward

The parameters sit under the reference's names (net.dnn.1.weight ..., net.fc.dnn.0.0.weight ..., net.lstm.weight_ih_l0 ...,
net.fc_out.weight): a state_dict moves either way.  The single-step and sequence nets are initialised by constructing torch's
modules in the reference's order, so the same seed gives the reference's initial weights; the n-gram net is this package's
FullyConnectedNetwork (the reference's Gaussian law, its own draw).  forward carries no autograd graph (training goes through
RewardNetTrainer); under grad mode its outputs raise on backward.  valid_step is clamped into [1, seq_len] by the kernel where
_gen_mask asserts on the host.

Refused by name: lstm_bidirectional, lstm_hidden_size > 256, lstm_num_layers > 4 (the LSTM kernels' limits), an even
context_size, an activation outside the six HIP epilogues, use_batch_norm on the single-step net (its BatchNorm1d would see
3-D input).  TransformerSyntheticRewardNet is its own module, models/synthetic_reward_transformer.py (re-exported from
reagent_amd.models, not from here).  Not built: NGramConvolutionalNetwork.

ngram and _gen_mask are plain torch statements of the reference's functions: the tests compare the kernels against them.
"""
from typing import List

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..engine import FCStack, ensure_slab
from . import lstm_stack
from .base import ModelBase
from .fully_connected_network import FullyConnectedNetwork, _Activation, no_autograd_guard
from .lstm_stack import _f32c, _Parameters

F32 = torch.float32


def ngram(input: torch.Tensor, context_size: int, ngram_padding: torch.Tensor):
    """:177-205 as one torch statement — input [seq_len, batch, feature] -> [seq_len, batch, feature * context_size]: window slot
    i holds the step at offset i - context_size // 2, ngram_padding [1, 1, feature] where that step lies outside the sequence.
    Like the reference it raises (from narrow) once context_size // 2 exceeds seq_len; rg_ngram_concat does not."""
    seq_len, batch_size, _ = input.shape
    half = context_size // 2
    slots = []
    for i in range(context_size):
        offset = i - half
        pad = ngram_padding.tile((abs(offset), batch_size, 1))
        kept = input.narrow(0, max(offset, 0), seq_len - abs(offset))
        slots.append(input if offset == 0 else torch.cat((pad, kept) if offset < 0 else (kept, pad), dim=0))
    return torch.cat(slots, dim=-1)


def _gen_mask(valid_step: torch.Tensor, batch_size: int, seq_len: int):
    """:208-226 — mask [batch, seq_len] of a [batch, 1] valid_step in 1 .. seq_len (asserted, on the host): 1.0 on the last
    valid_step steps of each row.  valid_step = [[1], [3]] at seq_len 4 gives [[0, 0, 0, 1], [0, 1, 1, 1]]."""
    assert valid_step.shape == (batch_size, 1)
    assert (1 <= valid_step).all()
    assert (valid_step <= seq_len).all()
    steps = torch.arange(seq_len, device=valid_step.device).repeat(batch_size, 1)
    return (steps >= (seq_len - valid_step)).float()


def _act_code(name: str, who: str) -> int:
    if name not in L.ACT:
        raise NotImplementedError(f"{who}: activation {name} has no HIP epilogue (one of {sorted(L.ACT)})")
    return L.ACT[name]


class _Concat(nn.Module):
    """:29-31 (index 0 of the single-step net's Sequential; the copy is rg_ngram_concat's)"""


class _RewardTrunk(nn.Module):
    """What the three nets share: the input rows (rg_ngram_concat), an FC trunk over all but the last linear and the
    gradient slab.  A subclass names its linears, layer norms and activations; SequenceSyntheticRewardNet overrides the trunk."""

    context_size = 1

    def _device(self):
        return next(self.parameters()).device

    def _input_rows(self, state, action):
        dev = self._device()
        state, action = _f32c(state.to(dev)), _f32c(action.to(dev))
        L.require_cuda(state, "state")
        assert state.ndim == 3 and action.ndim == 3 and state.shape[:2] == action.shape[:2], (state.shape, action.shape)
        assert state.shape[2] == self.state_dim and action.shape[2] == self.action_dim, (state.shape, action.shape)
        T, B = state.shape[:2]
        x = torch.empty(T, B, (self.state_dim + self.action_dim) * self.context_size, dtype=F32, device=dev)
        ops.ngram_concat(state, action, self.context_size, x)
        return x

    # ---- the FC trunk -------------------------------------------------------------------------------------------------
    def _stack(self):
        """the FC stack over all but the last linear (None when there is no hidden layer), in fp32"""
        lin, lns = self._linears()[:-1], self._layer_norms()[:-1]
        if not lin:
            return None
        if getattr(self, "_trunk", None) is None:
            self._trunk = FCStack([l.weight for l in lin], [l.bias for l in lin], self._act_codes[:-1], L.PREC_F32, layer_norms=lns)
        return self._trunk

    def _run(self, state, action, save=False):
        """-> the tape of one pass: T, B, the input rows x [T * B, In], the trunk's output h [T, B, P] and (save) the
        transposed staged input"""
        x = self._input_rows(state, action)
        T, B, In = x.shape
        st = self._stack()
        if st is None:
            return dict(T=T, B=B, x=x.view(T * B, In), h=x, xt=None)
        st.stage_weights(need_transposed=True)
        xc, xt = st.stage_input(x.view(T * B, In), need_transposed=save)
        h = torch.empty(T * B, st.dims[-1], dtype=F32, device=x.device)
        st.forward(xc, h, save=save)
        return dict(T=T, B=B, x=xc, h=h.view(T, B, -1), xt=xt)

    def head_params(self):
        """(weight [P], bias [1], activation code) of the last Linear(P, 1): handed to rg_step_reward_head"""
        last = self._linears()[-1]
        return last.weight.detach().view(-1), last.bias.detach(), self._act_codes[-1]

    def _grad_views(self):
        params = list(self.parameters())
        slab = ensure_slab(params)
        return slab, {id(p): slab.view(slab.grad, i) for i, p in enumerate(params)}

    def backward(self, tape, dh, dw, db):
        """d loss / d every parameter from a saving pass and the head's outputs (dh [T, B, P] = d loss / d the trunk's
        output, dw [P] and db [1] = the last linear's gradients), written into the parameters' gradient slab (the caller
        publishes it)"""
        slab, grad = self._grad_views()
        lin, lns = self._linears(), self._layer_norms()
        grad[id(lin[-1].weight)].view(-1).copy_(dw)
        grad[id(lin[-1].bias)].copy_(db)
        st = self._stack()
        if st is not None:
            st.bind_ln_grads([(grad[id(ln.weight)], grad[id(ln.bias)]) if ln is not None else None for ln in lns[:-1]])
            N = tape["T"] * tape["B"]
            st.backward(dh.view(N, -1), tape["xt"], [grad[id(l.weight)] for l in lin[:-1]], [grad[id(l.bias)] for l in lin[:-1]],
                        out32=tape["h"].view(N, -1))
        return slab

    def forward(self, state: torch.Tensor, action: torch.Tensor):
        """the net alone, as the reference's nn.Module: output [batch, seq_len] (no mask, no sum; no autograd graph)"""
        tape = self._run(state, action, save=False)
        T, B = tape["T"], tape["B"]
        f = dict(dtype=F32, device=tape["h"].device)
        output, mask, pred = torch.empty(B, T, **f), torch.empty(B, T, **f), torch.empty(B, **f)
        w, b, act = self.head_params()
        ops.step_reward_head(tape["h"], w, b, act, torch.full((B,), T, dtype=torch.int64, device=output.device), output, mask, pred)
        return no_autograd_guard(output, self, type(self).__name__)


class SingleStepSyntheticRewardNet(_RewardTrunk):
    def __init__(
        self,
        state_dim: int,
        action_dim: int,
        sizes: List[int],
        activations: List[str],
        last_layer_activation: str,
        use_batch_norm: bool = False,
        use_layer_norm: bool = False,
    ):
        """:276-303 — an MLP on cat(state, action) of every step; the last layer has one output"""
        super().__init__()
        if use_batch_norm:
            raise NotImplementedError("SingleStepSyntheticRewardNet: use_batch_norm=True is not supported: its BatchNorm1d "
                                      "would see [seq_len, batch, features] input, which the FC stack has no statement for")
        names = list(activations) + [last_layer_activation]
        self._act_codes = [_act_code(a, "SingleStepSyntheticRewardNet") for a in names]
        self.state_dim, self.action_dim = state_dim, action_dim
        modules: List[nn.Module] = [_Concat()]
        prev_layer_size = state_dim + action_dim
        for size, activation in zip(sizes, activations):
            modules.append(nn.Linear(prev_layer_size, size))
            if use_layer_norm:
                modules.append(nn.LayerNorm(size))
            modules.append(_Activation(activation))
            prev_layer_size = size
        modules.append(nn.Linear(prev_layer_size, 1))
        modules.append(_Activation(last_layer_activation))
        assert len(self._act_codes) == sum(isinstance(m, nn.Linear) for m in modules), (sizes, activations)
        self.dnn = nn.Sequential(*modules)  # (parameter holders under the reference's indices: nothing runs torch's forward)

    def _linears(self):
        return [m for m in self.dnn if isinstance(m, nn.Linear)]

    def _layer_norms(self):
        mods = list(self.dnn)
        return [mods[i + 1] if isinstance(mods[i + 1], nn.LayerNorm) else None for i, m in enumerate(mods) if isinstance(m, nn.Linear)]


class NGramFullyConnectedNetwork(_RewardTrunk):
    def __init__(
        self,
        state_dim: int,
        action_dim: int,
        sizes: List[int],
        activations: List[str],
        last_layer_activation: str,
        context_size: int,
        use_layer_norm: bool = False,
    ) -> None:
        if context_size % 2 != 1 or context_size < 1:
            raise NotImplementedError(f"NGramFullyConnectedNetwork: context_size {context_size} is not supported (odd, at least 1)")
        super().__init__()
        names = list(activations) + [last_layer_activation]
        self._act_codes = [_act_code(a, "NGramFullyConnectedNetwork") for a in names]
        self.state_dim, self.action_dim = state_dim, action_dim
        self.context_size = context_size
        self.ngram_padding = torch.zeros(1, 1, state_dim + action_dim)  # (as in the reference: not a parameter, not a buffer)
        self.fc = FullyConnectedNetwork(
            [(state_dim + action_dim) * context_size] + list(sizes) + [1],
            names,
            use_layer_norm=use_layer_norm,
        )
        self.fc.precision = L.PREC_F32

    def _linears(self):
        return self.fc.linears()

    def _layer_norms(self):
        return self.fc.layer_norms()


class SequenceSyntheticRewardNet(_RewardTrunk):
    def __init__(
        self,
        state_dim: int,
        action_dim: int,
        lstm_hidden_size: int,
        lstm_num_layers: int,
        lstm_bidirectional: bool,
        last_layer_activation: str,
    ):
        """:409-442 — an LSTM over cat(state, action) and Linear(lstm_hidden_size, 1) on every step's top hidden state"""
        super().__init__()
        if lstm_bidirectional:
            raise NotImplementedError("SequenceSyntheticRewardNet: lstm_bidirectional=True is not supported (the LSTM kernels run "
                                      "one direction)")
        if not 1 <= lstm_hidden_size <= L.LSTM_MAX_HIDDEN:
            raise NotImplementedError(f"SequenceSyntheticRewardNet: lstm_hidden_size {lstm_hidden_size} is not supported "
                                      f"(1 .. {L.LSTM_MAX_HIDDEN})")
        if not 1 <= lstm_num_layers <= L.LSTM_MAX_LAYERS:
            raise NotImplementedError(f"SequenceSyntheticRewardNet: lstm_num_layers {lstm_num_layers} is not supported "
                                      f"(1 .. {L.LSTM_MAX_LAYERS})")
        self._act_codes = [_act_code(last_layer_activation, "SequenceSyntheticRewardNet")]
        self.state_dim = state_dim
        self.action_dim = action_dim

        self.lstm_hidden_size = lstm_hidden_size
        self.lstm_num_layers = lstm_num_layers
        self.lstm_bidirectional = lstm_bidirectional

        self.lstm = _Parameters(nn.LSTM(input_size=self.state_dim + self.action_dim, hidden_size=self.lstm_hidden_size,
                                        num_layers=self.lstm_num_layers, bidirectional=False))
        self.fc_out = _Parameters(nn.Linear(self.lstm_hidden_size, 1))
        self.output_activation = _Activation(last_layer_activation)
        self._wt = lstm_stack.TransposedWeights()

    def _linears(self):
        return [self.fc_out]

    def _layer_norms(self):
        return [None]

    def _run(self, state, action, save=False):
        x = self._input_rows(state, action)
        T, B, In = x.shape
        tape = lstm_stack.forward(self.lstm, x.view(T * B, In), T, B, self.lstm_hidden_size, self.lstm_num_layers, None, None, save)
        return dict(T=T, B=B, lstm=tape, h=tape["h"][-1])

    def backward(self, tape, dh, dw, db):
        slab, grad = self._grad_views()
        grad[id(self.fc_out.weight)].view(-1).copy_(dw)
        grad[id(self.fc_out.bias)].copy_(db)
        lstm_stack.backward(self.lstm, tape["lstm"], dh, grad, None, None, self._wt, want_dh0=False)
        return slab


class SyntheticRewardNet(ModelBase):
    """:229-272 — reads state [seq_len, batch, state_dim], action [seq_len, batch, action_dim] and valid_step [batch, 1] out of a
    MemoryNetworkInput, runs self.net (one of the three nets above: a reward per step, [batch, seq_len]), masks the steps before
    each row's last valid_step and sums"""

    def __init__(self, net: nn.Module):
        super().__init__()
        if not isinstance(net, _RewardTrunk):
            raise NotImplementedError("SyntheticRewardNet: net must be a reagent_amd SingleStepSyntheticRewardNet, "
                                      f"NGramFullyConnectedNetwork or SequenceSyntheticRewardNet (got {type(net).__name__}): the "
                                      "head runs behind their trunks")
        self.net = net

    @staticmethod
    def _steps(valid_step, B, dev):
        assert valid_step is not None
        v = valid_step.to(dev).flatten()
        v = v if v.dtype == torch.int64 else v.long()
        assert v.numel() == B, (v.shape, B)
        return v if v.is_contiguous() else v.contiguous()

    def run_head(self, training_batch: rlt.MemoryNetworkInput, save: bool, target=None, loss_type: int = 0, threshold=None,
                 apply_threshold: bool = False, want_grad: bool = False):
        """one pass and rg_step_reward_head -> dict(tape, output [B, T], mask [B, T], predicted_reward [B] and, with a target
        [B], loss [1], n_kept [1] int32 and, with want_grad, dh [T, B, P], dw [P], db [1])"""
        net = self.net
        tape = net._run(training_batch.state.float_features, training_batch.action.float_features, save=save)
        T, B = tape["T"], tape["B"]
        h = tape["h"]
        dev, P = h.device, h.shape[2]
        f = dict(dtype=F32, device=dev)
        out = dict(tape=tape, output=torch.empty(B, T, **f), mask=torch.empty(B, T, **f), predicted_reward=torch.empty(B, **f))
        kw = {}
        if target is not None:
            out["loss"], out["n_kept"] = torch.empty(1, **f), torch.empty(1, dtype=torch.int32, device=dev)
            kw = dict(target=target, loss_type=loss_type, threshold=threshold, apply_threshold=apply_threshold, loss=out["loss"],
                      n_kept=out["n_kept"],
                      workspace=torch.empty(ops.step_reward_head_workspace(T, B, P), dtype=torch.float64, device=dev))
            if want_grad:
                out["dh"], out["dw"], out["db"] = torch.empty(T, B, P, **f), torch.empty(P, **f), torch.empty(1, **f)
                kw.update(dh=out["dh"], dw=out["dw"], dbias=out["db"])
        w, b, act = net.head_params()
        ops.step_reward_head(h, w, b, act, self._steps(training_batch.valid_step, B, dev), out["output"], out["mask"],
                             out["predicted_reward"], **kw)
        return out

    def backward(self, tape, dh, dw, db):
        return self.net.backward(tape, dh, dw, db)

    def forward(self, training_batch: rlt.MemoryNetworkInput):
        """:245-266 — no gradient flows through the result"""
        r = self.run_head(training_batch, save=False)
        B = r["predicted_reward"].shape[0]
        guard = lambda t: no_autograd_guard(t, self, "SyntheticRewardNet")  # noqa: E731
        return rlt.SyntheticRewardNetworkOutput(
            predicted_reward=guard(r["predicted_reward"].view(B, 1)),
            mask=r["mask"],
            output=guard(r["output"]),
        )

    def export_mlp(self):
        """:268-272 — the wrapped net, for a predictor wrapper (which this package does not build)"""
        return self.net
