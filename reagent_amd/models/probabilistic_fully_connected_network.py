"""FullyConnectedProbabilisticNetwork and LinearBBB with the surface of
reagent/models/probabilistic_fully_connected_network.py, executed on the HIP kernels: a network with a Gaussian posterior
N(mu, softplus(rho)) over every weight and bias, drawn anew on every forward, trained on the negative ELBO (Bayes by backprop).

  draw    : rg_bbb_sample — every layer's w = mu + softplus(rho) * eps, log_prior and log_post, in two launches whatever the
            depth (a segment table: a layer's weights and its biases are a segment each); eps is drawn in the kernel
            (Philox4x32-10 keyed by one seed per call from torch's HOST generator, so torch.manual_seed reproduces a run) or
            handed in (noise_source: the explicit-noise path the fixtures use; rg_bbb_fill_noise writes what the kernel draws)
  forward : engine.FCStack in fp32 over the drawn tensors (rg_fc_forward, rg_layer_norm_*), staged anew on every draw
  loss    : rg_bbb_elbo_head — the Gaussian likelihood, loss = log_post - log_prior - log_like and d loss / d out
  backward: the stack's backward into scratch dW / db, then rg_bbb_grad — the chain rule into mu and rho, one launch

The parameters sit under the reference's names (dnn.<i>.w_mu, w_rho, b_mu, b_rho, also reachable through linear_bbbs): a
state_dict moves either way.  w_mu and w_rho are initialised by gaussian_fill_w_gain's law (the reference's law, this
package's use of the generator); the biases' mu and rho start at zero.  forward carries no autograd graph (training goes
through BayesByBackpropTrainer); under grad mode its result raises on backward.  sample_elbo is the loss of num_samples >= 1
draws without gradients.

Kept quirks: prior_var is the prior's SCALE (Normal(0, prior_var)); the posterior's mean is w_mu.data, so d log_post / d mu
flows only through the drawn w.  min_std and orthogonal_init are accepted and ignored: the reference's constructor never
passes them on to LinearBBB.

Departures from the reference's fp32 torch.log(1 + torch.exp(rho)): sigma is computed in double as log1p(exp(rho)) (rho +
log1p(exp(-rho)) above zero), so it is not inf for rho > 88 and not 0 for rho < -17, and neither log-density turns into NaN
there; exp and log differ from torch's by ulps, so a drawn w matches the reference's within a bound, not to the bit.

Refused by name: use_batch_norm, dropout_ratio > 0, an activation outside the six HIP epilogues, more than 8 layers, a last
layer wider than 1 in sample_elbo.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..engine import FCStack, ensure_slab
from .base import ModelBase
from .fully_connected_network import _Activation, gaussian_fill_w_gain, no_autograd_guard

F32, F64 = torch.float32, torch.float64
MAX_LAYERS = L.BBB_MAX_SEGMENTS // 2


def _f32c(t):
    t = t if t.dtype == F32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


class LinearBBB(ModelBase):
    """:26-107 — the parameter holder of one Bayesian layer (nothing runs torch's forward)"""

    def __init__(self, input_dim, output_dim, activation, orthogonal_init: bool = False, min_std: float = 0.0,
                 prior_var: float = 1.0) -> None:
        super().__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.w_mu = nn.Parameter(torch.zeros(output_dim, input_dim))
        self.w_rho = nn.Parameter(torch.zeros(output_dim, input_dim))
        gain = torch.nn.init.calculate_gain(activation)
        if orthogonal_init:
            nn.init.orthogonal_(self.w_mu.data, gain=gain)
            nn.init.orthogonal_(self.w_rho.data, gain=gain)
        else:
            gaussian_fill_w_gain(self.w_mu, gain=gain, dim_in=input_dim, min_std=min_std)
            gaussian_fill_w_gain(self.w_rho, gain=gain, dim_in=input_dim, min_std=min_std)
        self.b_mu = nn.Parameter(torch.zeros(output_dim))
        self.b_rho = nn.Parameter(torch.zeros(output_dim))
        self.prior_var = prior_var
        self.w = None  # the last draw (fp32, on the device)
        self.b = None

    def forward(self, x: torch.Tensor):
        raise NotImplementedError("LinearBBB: a layer alone has no forward here; FullyConnectedProbabilisticNetwork draws all "
                                  "its layers in one launch")


class FullyConnectedProbabilisticNetwork(ModelBase):
    def __init__(
        self,
        layers,
        activations,
        prior_var,
        *,
        noise_tol: float = 0.1,
        use_batch_norm: bool = False,
        min_std: float = 0.0,
        dropout_ratio: float = 0.0,
        use_layer_norm: bool = False,
        normalize_output: bool = False,
        orthogonal_init: bool = False,
    ) -> None:
        super().__init__()
        who = "FullyConnectedProbabilisticNetwork"
        if use_batch_norm:
            raise NotImplementedError(f"{who}: use_batch_norm=True is not supported")
        if dropout_ratio > 0.0:
            raise NotImplementedError(f"{who}: dropout_ratio {dropout_ratio} is not supported (0 alone)")
        assert len(layers) == len(activations) + 1
        if len(activations) > MAX_LAYERS:
            raise NotImplementedError(f"{who}: {len(activations)} layers are not supported (at most {MAX_LAYERS}: the kernels' "
                                      f"table holds {L.BBB_MAX_SEGMENTS} segments, two per layer)")
        for a in activations:
            if a not in L.ACT:
                raise NotImplementedError(f"{who}: activation {a} has no HIP epilogue (one of {sorted(L.ACT)})")
        if not float(prior_var) > 0.0 or not float(noise_tol) > 0.0:
            raise ValueError(f"{who}: prior_var {prior_var} and noise_tol {noise_tol} must be positive")
        self.input_dim = layers[0]
        self.use_batch_norm = use_batch_norm
        self.noise_tol = noise_tol
        self.layers = layers
        self.prior_var = prior_var
        self.activation_names = list(activations)
        modules: List[nn.Module] = []
        linear_bbbs: List[nn.Module] = []
        for i, ((in_dim, out_dim), activation) in enumerate(zip(zip(layers, layers[1:]), activations)):
            # (min_std and orthogonal_init stop here, as in the reference: :144)
            linear_bbb = LinearBBB(in_dim, out_dim, activation, prior_var=prior_var)
            linear_bbbs.append(linear_bbb)
            modules.append(linear_bbb)
            if use_layer_norm and (normalize_output or i < len(activations) - 1):
                modules.append(nn.LayerNorm(out_dim))
            modules.append(_Activation(activation))
        self.dnn = nn.Sequential(*modules)  # (parameter holders under the reference's indices)
        self.linear_bbbs = nn.ModuleList(linear_bbbs)
        # None: every draw's noise comes from the kernel's generator.  A callable(shape) -> tensor: the noise of each tensor,
        # asked for in the reference's order (per layer the weights, then the biases)
        self.noise_source = None
        self._buf = None

    def input_prototype(self):
        return torch.randn(1, self.input_dim)

    # ---- the engine ----------------------------------------------------------------------------------------------------
    def _device(self):
        return next(self.parameters()).device

    def _layer_norms(self):
        mods = list(self.dnn)
        return [mods[i + 1] if isinstance(mods[i + 1], nn.LayerNorm) else None for i, m in enumerate(mods) if isinstance(m, LinearBBB)]

    def _bbb_ws(self):
        """the drawn tensors, their noise, the scratch dW / db, the scalars and the stack over the drawn tensors"""
        dev = self._device()
        if self._buf is None or self._buf["device"] != dev:
            f = dict(dtype=F32, device=dev)
            shapes = [s for l in self.linear_bbbs for s in (l.w_mu.shape, l.b_mu.shape)]
            nan = float("nan")
            b = dict(device=dev, w=[torch.empty(*s, **f) for s in shapes], eps=[torch.empty(*s, **f) for s in shapes],
                     dw=[torch.empty(*s, **f) for s in shapes], log_prior=torch.full((1,), nan, **f), log_post=torch.full((1,), nan, **f),
                     result=torch.full((4,), nan, **f),  # (NaN until the first draw / pass writes them)
                     terms=torch.empty(2, dtype=F64, device=dev), acc=torch.empty(4, dtype=F64, device=dev))
            for l, w, bias in zip(self.linear_bbbs, b["w"][0::2], b["w"][1::2]):
                l.w, l.b = w, bias
            b["stack"] = FCStack(b["w"][0::2], b["w"][1::2], [L.ACT[a] for a in self.activation_names], L.PREC_F32,
                                 layer_norms=self._layer_norms())
            b["ws"] = None
            self._buf = b
        return self._buf

    def _table(self, grads=None):
        """the segment table at the parameters' present addresses; grads: the (dmu, drho) destinations per segment"""
        b = self._bbb_ws()
        segs = []
        for i, l in enumerate(self.linear_bbbs):
            for j, (mu, rho) in enumerate(((l.w_mu, l.w_rho), (l.b_mu, l.b_rho))):
                k = 2 * i + j
                s = dict(mu=mu.detach().view(-1), rho=rho.detach().view(-1), w=b["w"][k].view(-1), eps=b["eps"][k].view(-1))
                if grads is not None:
                    s.update(dw=b["dw"][k].view(-1), dmu=grads[k][0].view(-1), drho=grads[k][1].view(-1))
                segs.append(s)
        table = ops.bbb_table(segs)
        table._keep = segs
        return table

    @staticmethod
    def _draw_seed() -> int:
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())  # torch's HOST generator

    def _draw(self, seed: Optional[int] = None, sample: int = 0):
        """one draw of every weight and bias, log_prior and log_post, and the stack staged on the draw"""
        b = self._bbb_ws()
        table = self._table()
        if b["ws"] is None:
            b["ws"] = torch.empty(2 * ops.bbb_chunks(table), dtype=F64, device=b["device"])
        if self.noise_source is not None:
            for e in b["eps"]:
                e.copy_(self.noise_source(e.shape))
            seed = None
        elif seed is None:
            seed = self._draw_seed()
        ops.bbb_sample(table, self.prior_var, b["log_prior"], b["log_post"], b["terms"], b["ws"], seed=seed, sample=sample)
        b["stack"].stage_weights(need_transposed=True, force=True)
        return b

    def _run(self, input: torch.Tensor, save: bool):
        """the stack on the present draw -> (out [B, layers[-1]], the transposed staged input of a saving pass)"""
        b = self._bbb_ws()
        x = _f32c(input.detach().to(b["device"]))
        L.require_cuda(x, "input")
        assert x.ndim == 2 and x.shape[1] == self.input_dim, x.shape
        xc, xt = b["stack"].stage_input(x, need_transposed=save)
        out = torch.empty(x.shape[0], self.layers[-1], dtype=F32, device=x.device)
        b["stack"].forward(xc, out, save=save)
        return out, xt

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """:168-173 — one draw of the weights and the network on it (no autograd graph)"""
        self._draw()
        out, _ = self._run(input, save=False)
        return no_autograd_guard(out, self, type(self).__name__)

    def log_prior(self):
        """:175-180 — of the last draw, over all the layers (a device scalar; NaN before the first draw, where the reference
        fails on its None)"""
        return self._bbb_ws()["log_prior"].view(()).clone()

    def log_post(self) -> torch.Tensor:
        """:182-188"""
        return self._bbb_ws()["log_post"].view(()).clone()

    def _head_ws(self, B):
        b = self._bbb_ws()
        n = ops.bbb_elbo_head_partials(B)
        if b.get("head_ws") is None or b["head_ws"].numel() < n:
            b["head_ws"] = torch.empty(n, dtype=F64, device=b["device"])
        return b["head_ws"]

    def _check_elbo(self, input, target):
        if self.layers[-1] != 1:
            raise NotImplementedError(f"FullyConnectedProbabilisticNetwork.sample_elbo: a last layer of {self.layers[-1]} outputs "
                                      "is not supported (1 alone: the likelihood is over one output per row)")
        t = _f32c(target.detach().to(self._device())).reshape(-1)
        assert t.numel() == input.shape[0], (target.shape, input.shape)
        return t

    def sample_elbo(self, input: torch.Tensor, target: torch.Tensor, num_samples: int):
        """:190-213 — the negative ELBO over num_samples draws: mean log_post - mean log_prior - mean log_like (a device
        scalar without an autograd graph; elbo_terms() has the three means)"""
        assert num_samples >= 1
        t = self._check_elbo(input, target)
        seed = None if self.noise_source is not None else self._draw_seed()
        for i in range(num_samples):
            b = self._draw(seed, i)
            out, _ = self._run(input, save=False)
            ops.bbb_elbo_head(out, t, self.noise_tol, b["terms"], b["acc"], b["result"], self._head_ws(t.numel()),
                              scale=1.0 / num_samples, accumulate=i > 0)
        return no_autograd_guard(b["result"][0].clone(), self, type(self).__name__)

    def elbo_terms(self):
        """(log_prior, log_post, log_like) of the last sample_elbo or training pass: device scalars"""
        r = self._bbb_ws()["result"]
        return r[1].clone(), r[2].clone(), r[3].clone()

    # ---- training (BayesByBackpropTrainer) -----------------------------------------------------------------------------
    def elbo_forward(self, input: torch.Tensor, target: torch.Tensor):
        """one draw, a saving pass and the head -> the tape elbo_backward reads; the loss is tape["loss"]"""
        t = self._check_elbo(input, target)
        b = self._draw()
        b["result"] = torch.empty(4, dtype=F32, device=b["device"])  # (a step's loss stays its own: no copy, no launch)
        out, xt = self._run(input, save=True)
        dout = torch.empty(t.numel(), 1, dtype=F32, device=out.device)
        ops.bbb_elbo_head(out, t, self.noise_tol, b["terms"], b["acc"], b["result"], self._head_ws(t.numel()), dout=dout)
        return dict(out=out, xt=xt, dout=dout, loss=b["result"][:1])

    def elbo_backward(self, tape):
        """d loss / d every parameter of the tape's pass, written into the parameters' gradient slab (the caller publishes
        it): the stack's backward leaves d (-log_like) / d w in scratch, rg_bbb_grad turns it into d mu and d rho"""
        b = self._bbb_ws()
        params = list(self.parameters())
        slab = ensure_slab(params)
        grad = {id(p): slab.view(slab.grad, i) for i, p in enumerate(params)}
        st = b["stack"]
        st.bind_ln_grads([(grad[id(ln.weight)], grad[id(ln.bias)]) if ln is not None else None for ln in self._layer_norms()])
        st.backward(tape["dout"], tape["xt"], b["dw"][0::2], b["dw"][1::2], out32=tape["out"])
        dst = [pair for l in self.linear_bbbs for pair in ((grad[id(l.w_mu)], grad[id(l.w_rho)]), (grad[id(l.b_mu)], grad[id(l.b_rho)]))]
        ops.bbb_grad(self._table(dst), self.prior_var)
        return slab

    def __deepcopy__(self, memo):
        import copy

        buf, self._buf = self._buf, None  # workspaces are not part of the model
        held = [(l.w, l.b) for l in self.linear_bbbs]
        for l in self.linear_bbbs:
            l.w = l.b = None
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
            return new
        finally:
            self._buf = buf
            for l, (w, bias) in zip(self.linear_bbbs, held):
                l.w, l.b = w, bias
