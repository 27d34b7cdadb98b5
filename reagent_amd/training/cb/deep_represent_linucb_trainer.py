"""DeepRepresentLinUCBTrainer (reagent/training/cb/deep_represent_linucb_trainer.py:17-94): the MLP of a
DeepRepresentLinearRegressionUCB trained by Adam on a weighted mse / mae / binary-cross-entropy loss of the predicted
label, its LinUCB layer updated by hand from the MLP's output.  One step, in the reference's order:

  solve      : rg_linucb_solve (d <= 128) or rg_linucb_solve_blocked (128 < d <= 512) folds the PREVIOUS step's averages
               and inverts (the reference's forward recalculates the coefficients on every step: cur_avg_A is non-zero
               after every update_params)
  forward    : one saving forward of the MLP's stack on the chosen arm's features                 -> mlp_out [B, h]
  head       : rg_drlinucb_head -- z = [1, mlp_out], pred_label, the loss, d loss / d mlp_out and (nn_e2e) d loss /
               d linear_layer.weight
  accumulate : rg_linucb_accumulate on z (LinUCBTrainer.update_params)
  backward   : the stack's backward from d loss / d mlp_out
  Adam       : this package's fused Adam over scorer.parameters(); parameters without a gradient (dummy_param, and
               linear_layer.weight with nn_e2e=False) are skipped as torch skips them

pred_sigma and ucb are NOT computed in the step: the reference computes them in the scorer's forward and discards them.
`cb_training_step` returns the loss through the autograd bridge of training/plumbing.py (``loss.backward(); opt.step()``
behave as under Lightning); `train_step_native` does the whole step without autograd and without a host synchronisation.  With an evaluator attached
(BaseCBTrainerWithEval) both paths run its frozen model and rg_cb_eval_ingest first and give the same bits.
"""
import logging

import torch

from ... import _lib as L
from ... import ops
from ...core.types import CBInput
from ...models.deep_represent_linucb import DeepRepresentLinearRegressionUCB
from ...optimizer import FusedAdam
from ..plumbing import NativeStepMixin, held_gradients, native_step
from .linucb_trainer import LinUCBTrainer
from .utils import add_chosen_arm_features, refuse_disjoint

logger = logging.getLogger(__name__)

LOSS_TYPES = dict(L.CB_LOSS)  # the reference's names (supervised_trainer.py:14-18) -> rg_drlinucb_head's loss codes


class _StackOwner:
    """what plumbing.TrainableNet is built from: the scorer's parameters (ONE slab, the optimizer's) and `.fc`"""

    def __init__(self, scorer):
        self.fc = scorer.deep_represent_layers
        self._scorer = scorer

    def parameters(self):
        return self._scorer.parameters()


class DeepRepresentLinUCBTrainer(NativeStepMixin, LinUCBTrainer):
    """Args: policy -- its scorer has to be a DeepRepresentLinearRegressionUCB; lr, weight_decay -- Adam's; loss_type -- one
    of LOSS_TYPES ("mse", "mae", "cross_entropy")."""

    def __init__(self, policy, lr: float = 1e-3, weight_decay: float = 0.0, loss_type: str = "mse", **kwargs):
        assert isinstance(policy.scorer, DeepRepresentLinearRegressionUCB), (
            "Trainer requires the policy scorer to be DeepRepresentLinearRegressionUCB")
        super().__init__(automatic_optimization=True, policy=policy, **kwargs)
        if loss_type not in LOSS_TYPES:
            raise KeyError(f"DeepRepresentLinUCBTrainer: loss_type {loss_type!r} is none of {sorted(LOSS_TYPES)}")
        self.scorer = policy.scorer
        self.loss_type = loss_type
        self.lr = lr
        self.weight_decay = weight_decay
        self._net = None
        self._bufs = None

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("DeepRepresentLinUCBTrainer: data parallel (world > 1) is not implemented: the LinUCB "
                                  "averages would have to be reduced across the trainers")

    def configure_optimizers(self):
        return FusedAdam(self.scorer.parameters(), lr=self.lr, weight_decay=self.weight_decay)

    def native_optimizers(self):
        if getattr(self, "_native_opts", None) is None:
            self._native_opts, self._native_scheds = [self.configure_optimizers()], [None]
        return self._native_opts

    # ---- the step ---------------------------------------------------------------------------------------------------------
    def _engine(self):
        """the trainable network over the scorer's parameter slab; which parameters the step gives a gradient"""
        s = self.scorer
        params = list(s.parameters())
        if self._net is None or len(self._net.params) != len(params) or any(a is not b for a, b in zip(self._net.params, params)):
            self._net = self._trainable(_StackOwner(s))
            self._lin_index = next(i for i, p in enumerate(params) if p is s.linear_layer.weight)
        else:
            self._net.slab.ensure_bound()
        no_grad = [s.dummy_param] + ([] if s.nn_e2e else [s.linear_layer.weight])
        self._no_grad = [p for p in params if any(p is q for q in no_grad)]
        return self._net

    def _step_buffers(self, B, h, dev):
        key = (B, h, str(dev))
        if self._bufs is None or self._bufs["key"] != key:
            f = dict(dtype=torch.float32, device=dev)
            P = ops.drlinucb_head_partials(B, h)
            self._bufs = dict(key=key, mlp_out=torch.empty(B, h, **f), z=torch.empty(B, h + 1, **f), lin=torch.empty(B, **f),
                              pred=torch.empty(B, **f), row_loss=torch.empty(B, **f), dmlp=torch.empty(B, h, **f),
                              loss_partials=torch.empty(P, **f), dv_partials=torch.empty(P * (h + 1), **f),
                              loss=torch.empty(1, **f), dv=torch.empty(h + 1, **f))
        return self._bufs

    def _forward(self, batch: CBInput, weight, dv_into_slab: bool):
        """solve, saving forward, head, accumulate.  weight: the rows' weight [B, 1] or None.  dv_into_slab: the head writes d loss / d linear_layer.weight straight
        into the gradient slab (the native step); otherwise into a buffer the autograd bridge's backward copies from"""
        s = self.scorer
        if batch.features_of_chosen_arm is None:  # base_trainer.py:107 of the reference: training_step gathers them
            batch = add_chosen_arm_features(batch)
        assert batch.label is not None
        x = batch.features_of_chosen_arm
        L.require_cuda(x, "batch.features_of_chosen_arm")
        if x.dim() != 2 or x.shape[1] != s.raw_input_dim:
            raise ValueError(f"DeepRepresentLinUCBTrainer: chosen-arm features of shape {tuple(x.shape)}, the scorer's MLP "
                             f"takes input_dim = {s.raw_input_dim}")
        x = self._f32c(x)
        B = x.shape[0]
        label = self._f32c(batch.label).reshape(-1)
        assert label.numel() == B, f"Shapes of model prediction {(B,)} and label {tuple(batch.label.shape)} have to match"
        if weight is not None:
            weight = self._f32c(weight).reshape(-1)
        net = self._engine()
        if s._coefs_dirty:  # (what the reference's forward decides by comparing tensors: true after every step)
            s._calculate_coefs()
        h = net.stack.dims[-1]
        w = self._step_buffers(B, h, x.device)
        net.stack.stage_weights(need_transposed=True)
        xc, self._xt = net.stack.stage_input(x, need_transposed=True)
        net.stack.forward(xc, w["mlp_out"], save=True)
        dv = None
        if s.nn_e2e:
            dv = net.slab.view(net.slab.grad, self._lin_index).reshape(-1) if dv_into_slab else w["dv"]
        ops.drlinucb_head(w["mlp_out"], s._mean_vector(), s._act, w["z"], w["lin"], w["pred"], label=label, weight=weight,
                          loss_type=LOSS_TYPES[self.loss_type], row_loss=w["row_loss"], dmlp_out=w["dmlp"],
                          loss_partials=w["loss_partials"], dv_partials=w["dv_partials"] if dv is not None else None,
                          loss=w["loss"], dv=dv)
        self._accumulate(w["z"], label, weight)  # update_params(mlp_out_with_ones.detach(), batch.label, weight)
        return w

    def _backward(self, grad_out=None, held=None):
        net, w = self._net, self._bufs
        net.backward(w["dmlp"], self._xt, grad_out, held=held, out32=w["mlp_out"])
        for p in self._no_grad:  # (the slab holds every parameter of the scorer; these get no gradient, as in torch)
            p.grad = None

    def _backward_bridge(self, grad_out):
        """loss.backward() of the generator path: the gradients a missing zero_grad() left are taken BEFORE the slab view of
        linear_layer.weight is written, and added back by the stack's backward"""
        net = self._net
        held = held_gradients(net.slab, net.params)
        if self.scorer.nn_e2e:
            net.slab.view(net.slab.grad, self._lin_index).reshape(-1).copy_(self._bufs["dv"] * grad_out)
        self._backward(grad_out, held)

    def cb_training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> torch.Tensor:
        refuse_disjoint(batch)
        return self._step_with_weight(batch, self._row_weight(batch), batch_idx, optimizer_idx)

    def _step_with_weight(self, batch: CBInput, weight, batch_idx: int, optimizer_idx: int = 0) -> torch.Tensor:
        with torch.no_grad():
            w = self._forward(batch, weight, dv_into_slab=False)
        return self._net.loss(self._backward_bridge, w["loss"])

    @torch.no_grad()
    @native_step
    def train_step_native(self, batch: CBInput):
        """the whole step -- solve, forward, head, accumulate, backward, Adam -- with no autograd graph and no host
        synchronisation; returns the loss [1] on the device"""
        refuse_disjoint(batch)
        evaluated = self.eval_module is not None
        if evaluated:
            self._check_eval_module(self.eval_module)
        self._check_input(batch, offline_eval=evaluated)
        (opt,) = self.native_optimizers()
        if evaluated:  # (before the step touches the scorer: the frozen model may have to be replaced by a copy of it)
            batch, weight = self._evaluate(batch)
        else:
            weight = self._row_weight(batch)
        net = self._engine()
        net.clear_grads()
        w = self._forward(batch, weight, dv_into_slab=True)
        self._native_segment(net, lambda: self._backward(), opt)
        self.all_batches_processed += 1
        return w["loss"]

    def on_train_epoch_end(self):
        super().on_train_epoch_end()  # _calculate_coefs (the solve) and the discount of the total weight
        self.scorer.check_solve_status()
