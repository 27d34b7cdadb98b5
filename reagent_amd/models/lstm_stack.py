"""The host side of an nn.LSTM-shaped stack (sequence first, fp32, no dropout, one direction), once: MDNRNN and
Seq2RewardNetwork run their recurrence through it, CEMPlannerNetwork reads its layers through it.  Plain functions on a
_Parameters holder of nn.LSTM's parameters under torch's own names (weight_ih_l0, ...): the models own the parameters, so
their state_dict keys stay rnn.weight_ih_l0 ...

  forward : per layer rg_fc_forward (x W_ih^T + b_ih of all steps at once) and rg_lstm_forward (the recurrence)
  backward: per layer, from the top, rg_lstm_backward, dW_ih and db_ih = rg_fc_wgrad(dgates, x), dW_hh and db_hh =
            rg_fc_wgrad(dgates, [h0; h_all[:-1]]), dx = rg_fc_dgrad(dgates, W_ih)

A layer's initial hidden state is row k of an [L, B, H] tensor (MDNRNN's `hidden`) or one [B, H] tensor that every layer
starts from (Seq2RewardNetwork's embedding); its initial cell is row k of an [L, B, H] tensor or zero.
"""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..engine import _mat

F32 = torch.float32
LINEAR = L.ACT["linear"]


class _Parameters(nn.Module):
    """the parameters of a torch module under their own names, without the module (nothing here runs torch's forward)"""

    def __init__(self, module: nn.Module):
        super().__init__()
        for name, p in module.named_parameters():
            self.register_parameter(name, nn.Parameter(p.detach().clone()))


def _f32c(t):
    t = t if t.dtype == F32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def layer_params(rnn, k):
    """(w_ih, w_hh, b_ih, b_hh) of layer k"""
    return (getattr(rnn, f"weight_ih_l{k}"), getattr(rnn, f"weight_hh_l{k}"), getattr(rnn, f"bias_ih_l{k}"),
            getattr(rnn, f"bias_hh_l{k}"))


def _initial(s0, k):
    """layer k's initial rows of s0: None, [L, B, H] (row k) or [B, H] (every layer's)"""
    return s0 if s0 is None or s0.ndim == 2 else s0[k]


def transposed(m):
    t = _mat(m.shape[1], m.shape[0], F32, m.device)
    ops.transpose_cast(m, None, t)
    return t


class TransposedWeights:
    """transposed weight copies of the backward's dgrads, remade when the weight has changed: name -> (version key, tensor)"""

    def __init__(self):
        self._wt = {}

    def __call__(self, name, w):
        key = (w._version, getattr(w, "_rg_version", 0), w.data_ptr())
        rec = self._wt.get(name)
        if rec is None or rec[0] != key or rec[1].device != w.device:
            rec = self._wt[name] = (key, transposed(w.detach()))
        return rec[1]


def wgrad(dzt, xt, w_grad, b_grad, rows):
    """dW and db of a linear layer over `rows` rows, from the transposed d loss / d output and the transposed input"""
    nbytes = ops.fc_wgrad_workspace_bytes(w_grad.shape[0], w_grad.shape[1], rows, L.PREC_F32)
    ws = torch.empty((nbytes + 15) // 16 * 4, dtype=F32, device=dzt.device)
    ops.fc_wgrad(dzt, xt, w_grad, b_grad, ws, L.PREC_F32)


def forward(rnn, x, T, B, H, layers, h0=None, c0=None, save=False):
    """the stack over x [T * B, In] -> the tape entries dict(x, h, c, gates): per layer the input rows, h_all and c_all
    [T, B, H] and (save) the gates [T, B, 4 H], else None"""
    N = T * B
    f = dict(dtype=F32, device=x.device)
    tape = dict(x=[], h=[], c=[], gates=[])
    for k in range(layers):
        w_ih, w_hh, b_ih, b_hh = (p.detach() for p in layer_params(rnn, k))
        xproj = torch.empty(N, 4 * H, **f)
        ops.fc_forward(x, w_ih, b_ih, LINEAR, L.PREC_F32, y32=xproj)
        h_all, c_all = torch.empty(T, B, H, **f), torch.empty(T, B, H, **f)
        gates = torch.empty(T, B, 4 * H, **f) if save else None
        ops.lstm_forward(xproj.view(T, B, 4 * H), w_hh, b_hh, _initial(h0, k), _initial(c0, k), h_all, c_all, gates)
        tape["x"].append(x), tape["h"].append(h_all), tape["c"].append(c_all), tape["gates"].append(gates)
        x = h_all.view(N, H)
    return tape


def backward(rnn, tape, dh_top, grad, h0, c0, transposed_weight, want_dh0):
    """d loss / d the stack's parameters from a saving forward's tape and dh_top [T, B, H] = d loss / d the top layer's
    h_all, written through grad (id(parameter) -> its gradient's view); h0 and c0 as forward took them; transposed_weight
    is the model's TransposedWeights.  -> per layer d loss / d its initial hidden state [B, H] (want_dh0), else None"""
    layers = len(tape["h"])
    T, B, H = tape["h"][0].shape
    N = T * B
    f = dict(dtype=F32, device=dh_top.device)
    dh = dh_top
    dh0 = [None] * layers
    for k in range(layers - 1, -1, -1):
        w_ih, w_hh, b_ih, b_hh = layer_params(rnn, k)
        h0_k = _initial(h0, k)
        dgates = torch.empty(T, B, 4 * H, **f)
        if want_dh0:
            dh0[k] = torch.empty(B, H, **f)
        ops.lstm_backward(dh.view(T, B, H), tape["gates"][k], tape["c"][k], _initial(c0, k), w_hh.detach(), dgates, dh0[k])
        dg = dgates.view(N, 4 * H)
        dgt = transposed(dg)
        wgrad(dgt, transposed(tape["x"][k]), grad[id(w_ih)], grad[id(b_ih)], N)
        first = h0_k.unsqueeze(0) if h0_k is not None else torch.zeros(1, B, H, **f)
        h_prev = torch.cat([first, tape["h"][k][:-1]], dim=0).view(N, H)
        wgrad(dgt, transposed(h_prev), grad[id(w_hh)], grad[id(b_hh)], N)
        if k > 0:
            dh = torch.empty(N, H, **f)
            ops.fc_dgrad(dg, transposed_weight(f"ih{k}", w_ih), None, LINEAR, L.PREC_F32, dx32=dh)
    return dh0 if want_dh0 else None
