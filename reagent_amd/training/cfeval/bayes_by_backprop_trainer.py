"""BayesByBackpropTrainer with the surface of reagent/training/cfeval/bayes_by_backprop_trainer.py:14-66, executed on the HIP
kernels: trains a FullyConnectedProbabilisticNetwork on the negative ELBO of one draw of its weights per step.

  input   : rg_tile_concat — cat(action, state.float_features), action first (the reference's order, kept)
  forward : the net's elbo_forward — rg_bbb_sample (the draw and both log-densities), a saving forward of its fp32 stack on
            the drawn weights, rg_bbb_elbo_head (the likelihood, the loss, d loss / d out)
  backward: the net's elbo_backward — the stack's backward into scratch dW / db, rg_bbb_grad into mu and rho; then
            rg_adam_step over the parameter slab

The generator path and train_step_native run the same launches: with the same noise, the same bits.  The loss reaches the
host only when a reporter is set, and the hundred-batch logger.info follows the same rule; validation_step returns a float.
The reference's train_step_gen counts all_batches_processed itself, on top of the Lightning module's own count: the loop's
count is the only one here.

Refused by name: weighted_by_inverse_propensity (the reference raises NotImplementedError after it has logged; here nothing
runs), LossFunction.BCELoss, a reward_net that is not this package's FullyConnectedProbabilisticNetwork, enable_data_parallel,
HIP-graph capture.  loss_type and reward_ignore_threshold are accepted and unused, as in the reference.
"""
import logging

import torch

from ... import ops
from ...core import types as rlt
from ...engine import ensure_slab
from ...models.probabilistic_fully_connected_network import FullyConnectedProbabilisticNetwork
from ..plumbing import SegmentLoss, held_gradients, native_step, publish_gradients
from .bandit_reward_network_trainer import BanditRewardNetTrainer

logger = logging.getLogger(__name__)


class BayesByBackpropTrainer(BanditRewardNetTrainer):
    _graph_capture_refusal = ("the Bayes-by-backprop step is not captured into a HIP graph: its noise seed is a host-side "
                              "launch argument; run it eagerly")
    _net_type, _net_name = FullyConnectedProbabilisticNetwork, "FullyConnectedProbabilisticNetwork"

    def _check_arguments(self, weighted_by_inverse_propensity):
        if weighted_by_inverse_propensity:
            raise NotImplementedError("BayesByBackpropTrainer: weighted_by_inverse_propensity=True is not supported (the "
                                      "reference raises NotImplementedError on its first step)")

    def _input(self, batch):
        """cat([action, state.float_features], 1) and the target"""
        self._refuse_capture()
        state = self._f32c(batch.state.float_features)
        action = self._f32c(batch.action.to(state.device))
        x = torch.empty(state.shape[0], action.shape[1] + state.shape[1], dtype=torch.float32, device=state.device)
        ops.tile_concat(action, state, x)
        return x, batch.reward

    def _backward(self, tape, grad_out=None):
        net = self.reward_net
        params = list(net.parameters())
        slab = ensure_slab(params)
        held = held_gradients(slab, params)
        net.elbo_backward(tape)
        if grad_out is not None:
            slab.grad.mul_(grad_out)
        publish_gradients(slab, params, held)

    def train_step_gen(self, training_batch: rlt.BanditRewardModelInput, batch_idx: int):
        x, target = self._input(training_batch)
        tape = self.reward_net.elbo_forward(x, target)
        loss = SegmentLoss.apply(lambda g: self._backward(tape, g), tape["loss"], *self.reward_net.parameters())

        if self._listening():  # (nobody listens: no host synchronisation)
            detached_loss = loss.detach().cpu()
            self.reporter.log(loss=detached_loss)

            if (self.all_batches_processed + 1) % 100 == 0:
                logger.info(f"{self.all_batches_processed + 1}-th batch: Loss={detached_loss.item()}")

        yield loss

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch: rlt.BanditRewardModelInput):
        """the step with no autograd graph, generator or host synchronisation -> the loss on the device"""
        (opt,) = self.native_optimizers()
        x, target = self._input(training_batch)
        tape = self.reward_net.elbo_forward(x, target)
        for p in self.reward_net.parameters():
            p.grad = None
        self._backward(tape)
        opt.step()
        self.all_batches_processed += 1
        return dict(loss=tape["loss"].view(()))

    @torch.no_grad()
    def validation_step(self, batch: rlt.BanditRewardModelInput, batch_idx: int):
        if self._training_batch_type and isinstance(batch, dict):
            batch = self._training_batch_type.from_dict(batch)

        x, target = self._input(batch)
        loss = self.reward_net.sample_elbo(x, target, 1)

        detached_loss = loss.detach().cpu()
        self.reporter.log(eval_loss=detached_loss)

        return detached_loss.item()
