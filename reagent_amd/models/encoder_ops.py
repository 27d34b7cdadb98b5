"""What the transformer nets share on the host (TransformerSyntheticRewardNet, Seq2SlateTransformerNet): the two-linear block as an
fp32 FC stack, a stack's forward with the staged input its weight gradient reads, the cache of transposed weights for the dgrads,
and the backward closures of a layer norm and of a single linear layer over row slices of packed parameters.  Every launch is an
existing entry point; nothing here is torch math."""
import torch

from .. import _lib as L
from .. import ops
from ..engine import FCStack
from . import lstm_stack

F32 = torch.float32


def block(first, second):
    """a two-linear block Linear -> relu -> Linear as an fp32 FC stack that also returns d loss / d its input"""
    st = FCStack([first.weight, second.weight], [first.bias, second.bias], [L.ACT["relu"], L.ACT["linear"]], L.PREC_F32)
    st.set_need_input_grad(True)
    return st


def stack_forward(st, x, save):
    """-> (the stack's output [N, out] and, with save, the transposed staged input the weight gradient reads)"""
    st.stage_weights(need_transposed=True)
    xc, xt = st.stage_input(x, need_transposed=save)
    out = torch.empty(x.shape[0], st.dims[-1], dtype=F32, device=x.device)
    st.forward(xc, out, save=save)
    return out, xt


class TransposedCache:
    """name -> (version key, W^T of a dgrad), remade when the parameter has changed"""

    def __init__(self):
        self._wt = {}

    def __call__(self, name, p, rows):
        """the transposed copy [in, out] of rows `rows` of parameter p, for rg_fc_dgrad"""
        key = (p._version, getattr(p, "_rg_version", 0), p.data_ptr())
        rec = self._wt.get(name)
        if rec is None or rec[0] != key or rec[1].device != p.device:
            rec = self._wt[name] = (key, lstm_stack.transposed(p.detach()[rows]))
        return rec[1]


def layer_norm_backward(ln, g, pre, stats, dgamma, dbeta):
    """d loss / d the layer norm's input [N, E] from d loss / d its output g, its input pre and saved (mean, rstd); the
    parameter gradients into dgamma, dbeta"""
    N, E = g.shape
    dz = torch.empty(N, E, dtype=F32, device=g.device)
    nb = L.lib().rg_layer_norm_backward_workspace_bytes(N, E)
    ops.layer_norm_backward(g, pre, stats[0], stats[1], ln.weight.detach(), dgamma, dbeta,
                            torch.empty((nb + 15) // 16 * 4, dtype=F32, device=g.device), dz32=dz)
    return dz


def linear_backward(cache, dz, x_in, name, w, dw, db, rows=slice(None), need_dx=True):
    """d input of x_in W^T + b for rows `rows` of the parameter w (None with need_dx=False) and, into rows `rows` of the
    gradients dw and db, dW and db"""
    N = dz.shape[0]
    dx = None
    if need_dx:
        dx = torch.empty(N, w.shape[1], dtype=F32, device=dz.device)
        ops.fc_dgrad(dz, cache(name, w, rows), None, L.ACT["linear"], L.PREC_F32, dx32=dx)
    lstm_stack.wgrad(lstm_stack.transposed(dz), lstm_stack.transposed(x_in), dw[rows], db[rows], N)
    return dx
