"""NGramConvolutionalNetwork with the surface of reagent/models/synthetic_reward.py:311-370 (over
reagent/models/convolutional_network.py:34-97), executed on the HIP kernels: a per-step reward from a conv tower over the step's
window of context_size steps and an FC trunk, wrapped by SyntheticRewardNet like its siblings.

This module is reagent_amd.models.synthetic_reward_conv, re-exported from reagent_amd.models; the reference keeps the class in
models/synthetic_reward.py (the suite asserts that reagent_amd.models.synthetic_reward has no such attribute).

The reference copies every step into context_size windows, reshapes them to [T * B, 1, n, S + A] and runs Conv2d -> relu ->
MaxPool2d(1) per window.  Its first kernel spans the width and the later ones have width 1, so a layer's output at an absolute
position is the same in every window that holds the position: the tower is a one-dimensional valid convolution along time over
the zero-padded sequence.  Here it is computed once per position — (T + H_i - 1) * B rows per layer where the reference
computes T * B * H_i — and a window is a gather.  Rows are ordered (position, b); H_0 = n, H_{i+1} = H_i - kh_i + 1:

  g_{i+1} = relu(conv_i(g_i))   rg_seqconv_forward per layer; layer 0 reads state | action in place and predicates the padding
  feat[(t, b), c * H_L + h]     rg_ngram_window: g_L[(t + h, b), c], the reference's x.view(-1, fc_input_dim)
  trunk, head                   engine.FCStack over all but the last linear; rg_step_reward_head (SyntheticRewardNet.run_head)
  backward                      FCStack.backward into dfeat (the head's dh with sizes == []), rg_ngram_window_backward (+ relu
                                mask), then rg_seqconv_wgrad and rg_seqconv_dgrad per layer into the gradient slab

The parameters sit under the reference's keys in its parameters() order (conv_net.conv_layers.{i}.weight | bias, then
conv_net.feed_forward.dnn. ...): a state_dict moves either way.  The conv weights are torch's nn.Conv2d followed by
kaiming_normal_, constructed in the reference's order, so the same seed gives the reference's bits; the FC is this package's
FullyConnectedNetwork (the reference's Gaussian law, its own draw), as for the n-gram FC net.

Refused by name: an even context_size; a pool type other than "max"; a pool kernel other than 1 (the reference's own constructor
raises there: MaxPool2d(k > 1) meets width 1); use_layer_norm=True (the reference's GroupNorm(1, C) normalises per window over
channels and height, so positions cannot be shared between windows: not built); kernels that leave no height (sum(kh_i - 1) >=
n); S + A or a conv_dims entry above 512, context_size above 15, more than 4 conv layers; layer lists of different lengths or
none, no state column; an activation outside the six epilogues.  forward carries no autograd graph (training goes through RewardNetTrainer)."""
from typing import List

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core.parameters import ConvNetParameters
from .fully_connected_network import FullyConnectedNetwork
from .lstm_stack import _f32c
from .synthetic_reward import _act_code, _RewardTrunk

F32 = torch.float32
WHO = "NGramConvolutionalNetwork"


class _ConvTower(nn.Module):
    """convolutional_network.py:34-77 as a parameter holder (nothing runs torch's forward): conv_layers, then feed_forward"""

    def __init__(self, conv_dims, height_kernels, width_kernels, fc_layers, activations):
        super().__init__()
        self.conv_layers = nn.ModuleList()
        for i in range(len(conv_dims) - 1):
            self.conv_layers.append(nn.Conv2d(conv_dims[i], conv_dims[i + 1], kernel_size=(height_kernels[i], width_kernels[i])))
            nn.init.kaiming_normal_(self.conv_layers[i].weight)
        self.feed_forward = FullyConnectedNetwork(fc_layers, activations)
        self.feed_forward.precision = L.PREC_F32


class NGramConvolutionalNetwork(_RewardTrunk):
    def __init__(
        self,
        state_dim: int,
        action_dim: int,
        sizes: List[int],
        activations: List[str],
        last_layer_activation: str,
        context_size: int,
        conv_net_params: ConvNetParameters,
        use_layer_norm: bool = False,
    ) -> None:
        p, n, width = conv_net_params, context_size, state_dim + action_dim
        kh, dims = list(p.conv_height_kernels), list(p.conv_dims)
        if n % 2 != 1 or n < 1:
            raise NotImplementedError(f"{WHO}: context_size {n} is not supported (odd, at least 1)")
        if any(t != "max" for t in p.pool_types):
            raise NotImplementedError(f"{WHO}: pool_types {list(p.pool_types)} is not supported (\"max\")")
        if any(k != 1 for k in p.pool_kernel_sizes):
            raise NotImplementedError(f"{WHO}: pool_kernel_sizes {list(p.pool_kernel_sizes)} is not supported (1: a larger "
                                      "MaxPool2d meets width 1, where the reference's constructor raises)")
        if use_layer_norm:
            raise NotImplementedError(f"{WHO}: use_layer_norm=True is not supported (the reference's GroupNorm(1, C) normalises "
                                      "per window over channels and height, so the tower cannot be shared between windows)")
        if not len(dims) == len(kh) == len(p.pool_types) == len(p.pool_kernel_sizes) >= 1:
            raise NotImplementedError(f"{WHO}: conv_dims {dims}, conv_height_kernels {kh}, pool_types {list(p.pool_types)} and "
                                      f"pool_kernel_sizes {list(p.pool_kernel_sizes)} must name the same layers, at least one")
        if state_dim < 1 or action_dim < 0 or min(dims) < 1:
            raise NotImplementedError(f"{WHO}: state_dim {state_dim}, action_dim {action_dim} and conv_dims {dims} are not "
                                      "supported (a state column and a channel per layer at least)")
        if len(dims) > L.SEQCONV_MAX_LAYERS:
            raise NotImplementedError(f"{WHO}: {len(dims)} conv layers are not supported (up to {L.SEQCONV_MAX_LAYERS})")
        if n > L.SEQCONV_MAX_CONTEXT:
            raise NotImplementedError(f"{WHO}: context_size {n} is not supported (up to {L.SEQCONV_MAX_CONTEXT})")
        if width > L.SEQCONV_MAX_CHANNELS or max(dims) > L.SEQCONV_MAX_CHANNELS:
            raise NotImplementedError(f"{WHO}: state_dim + action_dim {width} with conv_dims {dims} is not supported (up to "
                                      f"{L.SEQCONV_MAX_CHANNELS} each)")
        if min(kh) < 1 or sum(k - 1 for k in kh) >= n:
            raise NotImplementedError(f"{WHO}: conv_height_kernels {kh} leave no height of a context of {n}")
        super().__init__()
        names = list(activations) + [last_layer_activation]
        self._act_codes = [_act_code(a, WHO) for a in names]
        self.state_dim, self.action_dim = state_dim, action_dim
        self.context_size = n
        self.input_width, self.input_height, self.num_input_channels = width, n, 1
        self.heights = [n]
        for k in kh:
            self.heights.append(self.heights[-1] - k + 1)
        self.fc_input_dim = dims[-1] * self.heights[-1]
        self.conv_net = _ConvTower([1] + dims, kh, [width] + [1] * (len(kh) - 1), [self.fc_input_dim] + list(sizes) + [1], names)
        self.ngram_padding = torch.zeros(1, 1, width)  # (as in the reference: not a parameter, not a buffer)

    def _linears(self):
        return self.conv_net.feed_forward.linears()

    def _layer_norms(self):
        return self.conv_net.feed_forward.layer_norms()

    def _stack(self):
        st = super()._stack()
        if st is not None:
            st.set_need_input_grad(True)  # the tower's gradient enters through d loss / d feat
        return st

    def _run(self, state, action, save=False):
        """-> the tape of one pass: T, B, the tower's activations g (per layer, [P_i * B, C_i]), the window rows feat, the
        trunk's output h [T, B, P] and (save) the transposed staged feat"""
        dev = self._device()
        state, action = _f32c(state.to(dev)), _f32c(action.to(dev))
        L.require_cuda(state, "state")
        assert state.ndim == 3 and action.ndim == 3 and state.shape[:2] == action.shape[:2], (state.shape, action.shape)
        assert state.shape[2] == self.state_dim and action.shape[2] == self.action_dim, (state.shape, action.shape)
        T, B = state.shape[:2]
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        x, x2, P, pad = state.view(T * B, -1), action.view(T * B, -1), T, self.context_size // 2
        if self.action_dim == 0:
            x2 = None
        g = []
        for conv in self.conv_net.conv_layers:
            w = conv.weight.detach()
            p_out = P + 2 * pad - w.shape[2] + 1
            y = new(p_out * B, w.shape[0])
            ops.seqconv_forward(x, x2, P, pad, B, w, conv.bias.detach(), y)
            g.append(y)
            x, x2, P, pad = y, None, p_out, 0
        feat = new(T * B, self.fc_input_dim)
        ops.ngram_window(g[-1], T, B, self.heights[-1], feat)
        tape = dict(T=T, B=B, state=state, action=action, g=g, x=feat, xt=None)
        st = self._stack()
        if st is None:
            tape["h"] = feat.view(T, B, -1)
            return tape
        st.stage_weights(need_transposed=True)
        tape["x"], tape["xt"] = st.stage_input(feat, need_transposed=save)
        h = new(T * B, st.dims[-1])
        st.forward(tape["x"], h, save=save)
        tape["h"] = h.view(T, B, -1)
        return tape

    def backward(self, tape, dh, dw, db):
        slab, grad = self._grad_views()
        lin = self._linears()
        grad[id(lin[-1].weight)].view(-1).copy_(dw)
        grad[id(lin[-1].bias)].copy_(db)
        T, B, g = tape["T"], tape["B"], tape["g"]
        N, dev = T * B, dh.device
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        st = self._stack()
        if st is None:
            dfeat = dh.view(N, -1)
        else:
            dfeat = new(N, self.fc_input_dim)
            st.backward(dh.view(N, -1), tape["xt"], [grad[id(l.weight)] for l in lin[:-1]], [grad[id(l.bias)] for l in lin[:-1]],
                        dx32=dfeat, out32=tape["h"].view(N, -1))
        convs = list(self.conv_net.conv_layers)
        dz = new(g[-1].shape)
        ops.ngram_window_backward(dfeat, T, B, self.heights[-1], dz, g=g[-1])
        for i in range(len(convs) - 1, -1, -1):
            w = convs[i].weight
            cout, cin, kh = w.shape[0], w.shape[1] * w.shape[3], w.shape[2]
            p_out = dz.shape[0] // B
            ws = new(ops.seqconv_wgrad_workspace_bytes(p_out, B, kh, cin, cout) // 4)
            gw, gb = grad[id(w)].view(w.shape), grad[id(convs[i].bias)]
            if i == 0:
                x2 = tape["action"].view(N, -1) if self.action_dim else None
                ops.seqconv_wgrad(dz, tape["state"].view(N, -1), x2, T, self.context_size // 2, B, gw, gb, ws)
            else:
                ops.seqconv_wgrad(dz, g[i - 1], None, p_out + kh - 1, 0, B, gw, gb, ws)
                dx = new(g[i - 1].shape)
                ops.seqconv_dgrad(dz, p_out, B, w.detach(), dx, below=g[i - 1])
                dz = dx
        return slab
