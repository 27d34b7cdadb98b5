"""TEST INFRASTRUCTURE: statements of the normalisation kernels of reagent_amd/csrc/layernorm.hip and fcopts.hip, one plain
function each.

Tensors in, tensors out; torch arithmetic in the dtype asked for (float64 is the statement, float32 is "torch fp32 on the
same operation", the calibration of every bound), torch autograd for the gradients.  Nothing here calls a project kernel or
anything from `reagent_amd.ops`: tests/test_norm_kernel_statements.py and tests/fuzz/fuzz_fc_options.py hold the kernels to
these.

  layer_norm_ref            fully_connected_network.py:128-130   Linear -> LayerNorm -> activation, and its backward
  batch_norm_ref            fully_connected_network.py:107-108   nn.BatchNorm1d on [batch, features], training and eval
  dropout_ref               fully_connected_network.py:139-141   y = x * keep / (1 - p) for a GIVEN keep mask
  layer_norm_backward_form  the backward entry point as a function of ITS operands (g, z, mean, rstd, gamma): the closed
  batch_norm_backward_form  form of the autograd result.  Used only to measure conditioning (how far the exact answer moves
                            when an fp32 operand moves by a rounding), never as the yardstick of a kernel.
"""
import torch
import torch.nn.functional as Fn

F64 = torch.float64
F32 = torch.float32

ACTS = {"linear": lambda t: t, "relu": torch.relu, "leaky_relu": lambda t: Fn.leaky_relu(t, 0.01), "tanh": torch.tanh,
        "sigmoid": torch.sigmoid, "softplus": Fn.softplus}


def _opt(t, dtype, grad=False):
    if t is None:
        return None
    t = t.detach().to(dtype).clone()
    return t.requires_grad_() if grad else t


def _grad(t):
    return None if t is None else t.grad


# ---- layer norm -----------------------------------------------------------------------------------------------------------
def layer_norm_ref(z, gamma, beta, eps, act, g=None, dtype=F64):
    """y = act(LayerNorm(z)); mean = the row mean, rstd = 1 / sqrt(biased variance + eps).  g [B, n] is the gradient at the
    LayerNorm OUTPUT (the caller applies the activation's derivative) -> dz, dgamma, dbeta by autograd."""
    n = z.shape[1]
    zr, gr, br = _opt(z, dtype, True), _opt(gamma, dtype, True), _opt(beta, dtype, True)
    ln = Fn.layer_norm(zr, (n,), gr, br, eps)
    zd = zr.detach()
    mean = zd.mean(1)
    out = dict(y=ACTS[act](ln).detach(), mean=mean, rstd=1.0 / torch.sqrt(zd.var(1, unbiased=False) + eps))
    if g is not None:
        ln.backward(g.to(dtype))
        out.update(dz=zr.grad, dgamma=gr.grad, dbeta=br.grad)
    return out


def layer_norm_backward_form(g, z, mean, rstd, gamma):
    """dz = rstd * (g gamma - mean_n(g gamma) - xhat * mean_n(g gamma xhat)), dgamma = sum_b g xhat, dbeta = sum_b g with
    xhat = (z - mean) * rstd, of the operands as given"""
    xh = (z - mean[:, None]) * rstd[:, None]
    gg = g * gamma
    dz = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    return dict(dz=dz, dgamma=(g * xh).sum(0), dbeta=g.sum(0))


# ---- batch norm -----------------------------------------------------------------------------------------------------------
def batch_norm_ref(x, gamma, beta, running_mean, running_var, training, momentum, eps, stat_updates=1, g=None, dtype=F64):
    """torch.nn.functional.batch_norm on [B, n].  gamma None: an affine-free module; beta None with gamma: a zero bias.
    training: the batch statistics normalise (save_mean, save_rstd of the biased variance) and the running statistics, where
    given, are those after `stat_updates` evaluations of the module on this batch (unbiased variance, running <- (1 -
    momentum) running + momentum batch), as torch applies them.  eval: the frozen running statistics normalise, gradients
    pass through the frozen scale.  -> y, save_mean, save_rstd, running_mean, running_var, dx, dgamma, dbeta (None where
    the operand is)."""
    xr, gr, br = _opt(x, dtype, True), _opt(gamma, dtype, True), _opt(beta, dtype, True)
    rm, rv = _opt(running_mean, dtype), _opt(running_var, dtype)
    out = {}
    if training:
        y = Fn.batch_norm(xr, None, None, gr, br, True, 0.0, eps)
        xd = xr.detach()
        out.update(save_mean=xd.mean(0), save_rstd=1.0 / torch.sqrt(xd.var(0, unbiased=False) + eps))
        if rm is not None:
            for _ in range(stat_updates):
                Fn.batch_norm(xd, rm, rv, None, None, True, momentum, eps)
    else:
        y = Fn.batch_norm(xr, rm, rv, gr, br, False, 0.0, eps)
    out.update(y=y.detach(), running_mean=rm, running_var=rv)
    if g is not None:
        y.backward(g.to(dtype))
        out.update(dx=xr.grad, dgamma=_grad(gr), dbeta=_grad(br))
    return out


def batch_norm_backward_form(g, x, mean, rstd, gamma, training):
    """training: dx = gamma rstd (g - mean_b(g) - xhat mean_b(g xhat)); eval: dx = gamma rstd g; dgamma = sum_b g xhat,
    dbeta = sum_b g with xhat = (x - mean) * rstd, of the operands as given (eval: rstd = 1 / sqrt(running_var + eps))"""
    xh = (x - mean) * rstd
    ga = gamma if gamma is not None else torch.ones_like(mean)
    dx = ga * rstd * (g - g.mean(0) - xh * (g * xh).mean(0)) if training else ga * rstd * g
    return dict(dx=dx, dgamma=(g * xh).sum(0), dbeta=g.sum(0))


# ---- dropout --------------------------------------------------------------------------------------------------------------
def dropout_ref(x, keep, p, dtype=F64):
    """y = x * keep / (1 - p) for the mask given: one multiplication by 1 / (1 - p) rounded to `dtype`"""
    return x.to(dtype) * keep.to(dtype) * torch.tensor(1.0 / (1.0 - p), dtype=dtype)
