"""BanditRewardNetTrainer with the surface of reagent/training/cfeval/bandit_reward_network_trainer.py:20-132, executed on
the HIP kernels: fits a per-action reward model to logged bandit data, optionally weighted by 1 / action_prob.

  forward : one saving forward of the reward net's stack (a FullyConnectedDQN, any precision its stack supports) -> q [B, A]
  head    : rg_bandit_reward_head — the logged action (torch.argmax's rule), its prediction, the loss wrapper of
            reward_network_trainer.py:27-66 (MSE, SmoothL1 or L1, the 1 / action_prob weight, the reward_ignore_threshold
            filter, the mean over the kept rows), the unweighted loss over the same rows and d loss / d q, in two launches
  backward: the stack's backward into the gradient slab, rg_adam_step over it

The generator path (training_step, backward, optimizer step) and train_step_native run the same launches on the same
buffers: the same bits.  The reference moves the loss to the host on every step; here the losses are read, and the kept-row
count checked (the reference's assertion text), only when a reporter is set, and the ten-batch logger.info follows the same
rule.  validation_step always reads the loss back: it returns a float.  The threshold filter is the reference's: on in
training, off in validation (it gates on pred.requires_grad).

Refused by name: LossFunction.BCELoss (the reference reads batch.valid_step, which BanditRewardModelInput does not have), a
reward_net that is not this package's FullyConnectedDQN, enable_data_parallel, HIP-graph capture.
"""
import logging
from typing import Optional

import numpy as np
import torch

from ... import _lib as L
from ... import ops
from ...core import types as rlt
from ...models.base import ModelBase
from ...models.dqn import FullyConnectedDQN
from ...optimizer import Optimizer__Union
from ..plumbing import NativeStepMixin, SegmentLoss, native_step
from ..reagent_lightning_module import ReAgentLightningModule, _NoOpReporter
from ..reward_network_trainer import LossFunction

logger = logging.getLogger(__name__)


class BanditRewardNetTrainer(NativeStepMixin, ReAgentLightningModule):
    _graph_capture_refusal = ("the bandit reward step is not captured into a HIP graph: its buffers are allocated per step; "
                              "run it eagerly")
    _net_type, _net_name = FullyConnectedDQN, "FullyConnectedDQN"

    def __init__(
        self,
        reward_net: ModelBase,
        optimizer: Optional[Optimizer__Union] = None,
        loss_type: LossFunction = LossFunction.MSE,
        reward_ignore_threshold: Optional[float] = None,
        weighted_by_inverse_propensity: bool = False,
    ) -> None:
        super().__init__()
        who = type(self).__name__
        if not isinstance(reward_net, self._net_type):
            raise NotImplementedError(f"{who}: reward_net must be a reagent_amd {self._net_name} "
                                      f"(got {type(reward_net).__name__}): the step runs on its kernels")
        loss_type = LossFunction(loss_type)
        if loss_type == LossFunction.BCELoss:
            raise NotImplementedError(f"{who}: loss_type LossFunction.BCELoss is not supported: the reference's wrapper reads "
                                      "batch.valid_step, which BanditRewardModelInput does not have")
        self._check_arguments(weighted_by_inverse_propensity)
        self.reward_net = reward_net
        self.optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.loss_type = loss_type
        self.reward_ignore_threshold = reward_ignore_threshold
        self.weighted_by_inverse_propensity = weighted_by_inverse_propensity

    def _check_arguments(self, weighted_by_inverse_propensity):
        pass

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError(f"{type(self).__name__} has no data-parallel path (enable_data_parallel: world > 1 is not "
                                  "supported)")

    def configure_optimizers(self):
        optimizers = []
        optimizers.append(self.optimizer.make_optimizer_scheduler(self.reward_net.parameters()))
        return optimizers

    def _get_sample_weight(self, batch: rlt.BanditRewardModelInput):
        """:48-55 — the action probabilities the head turns into 1 / action_prob (None: unweighted)"""
        weight = None
        if self.weighted_by_inverse_propensity:
            assert batch.action_prob is not None
            weight = batch.action_prob
        return weight

    # ---- the step --------------------------------------------------------------------------------------------------------
    def _listening(self):
        return not isinstance(self.reporter, _NoOpReporter)

    def _refuse_capture(self):
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)

    def _forward(self, batch, training: bool):
        """one pass and the head -> dict(predicted_reward [B, 1], loss [1], unweighted_loss [1] or None, n_kept [1] and, in
        training, what the backward reads); training: a saving pass with the threshold filter and the gradients"""
        self._refuse_capture()
        prob = self._get_sample_weight(batch)
        state = self._f32c(batch.state.float_features)
        L.require_cuda(state, "training_batch.state")
        B, dev = state.shape[0], state.device
        e = self._trainable(self.reward_net)
        A = e.stack.dims[-1]
        action, reward = self._f32c(batch.action.to(dev)), self._f32c(batch.reward.to(dev))
        assert action.shape == (B, A), f"action is {tuple(action.shape)}, the reward net has {A} outputs for {B} rows"
        assert len(reward.shape) == 2 and reward.shape == (B, 1), reward.shape
        if prob is not None:
            prob = self._f32c(prob.to(dev))
            assert prob.shape == reward.shape
        f = dict(dtype=torch.float32, device=dev)
        q = torch.empty(B, A, **f)
        e.stack.stage_weights(need_transposed=True)
        xc, xt = e.stack.stage_input(state, need_transposed=training)
        e.stack.forward(xc, q, save=training)
        r = dict(e=e, xt=xt, predicted_reward=torch.empty(B, 1, **f), loss=torch.empty(1, **f),
                 unweighted_loss=torch.empty(1, **f) if prob is not None else None,
                 n_kept=torch.empty(1, dtype=torch.int32, device=dev), dq=torch.empty(B, A, **f) if training else None)
        ops.bandit_reward_head(q, action, reward.view(B), r["predicted_reward"].view(B), r["loss"], r["n_kept"],
                               torch.empty(ops.bandit_reward_head_workspace(B), dtype=torch.float64, device=dev),
                               action_prob=prob.view(B) if prob is not None else None, loss_type=L.SRW_LOSS[self.loss_type.value],
                               threshold=self.reward_ignore_threshold, apply_threshold=training,
                               unweighted_loss=r["unweighted_loss"], dq=r["dq"])
        return r

    def _check_kept(self, r, batch):
        """the reference's assertion (reward_network_trainer.py:59-62), where the loss is read"""
        assert int(r["n_kept"].item()) > 0, (
            f"reward ignore threshold set too small. target={batch.reward}, "
            f"threshold={self.reward_ignore_threshold}"
        )

    def _backward(self, r, grad_out=None):
        r["e"].backward(r["dq"], r["xt"], grad_out)

    def train_step_gen(self, training_batch: rlt.BanditRewardModelInput, batch_idx: int):
        r = self._forward(training_batch, training=True)
        loss = SegmentLoss.apply(lambda g: self._backward(r, g), r["loss"], *self.reward_net.parameters())

        if self._listening():  # (nobody listens: no host synchronisation)
            self._check_kept(r, training_batch)
            detached_loss = loss.detach().cpu()
            self.reporter.log(loss=detached_loss)

            if r["unweighted_loss"] is not None:
                self.reporter.log(unweighted_loss=r["unweighted_loss"].view(()).detach().cpu())

            if self.all_batches_processed % 10 == 0:
                logger.info(f"{self.all_batches_processed}-th batch: {self.loss_type}={detached_loss.item()}")

        yield loss

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch: rlt.BanditRewardModelInput):
        """the step with no autograd graph, generator or host synchronisation -> the losses on the device"""
        (opt,) = self.native_optimizers()
        r = self._forward(training_batch, training=True)
        for p in self.reward_net.parameters():
            p.grad = None
        self._backward(r)
        opt.step()
        self.all_batches_processed += 1
        out = dict(loss=r["loss"].view(()))
        if r["unweighted_loss"] is not None:
            out["unweighted_loss"] = r["unweighted_loss"].view(())
        return out

    @torch.no_grad()
    def validation_step(self, batch: rlt.BanditRewardModelInput, batch_idx: int):
        if self._training_batch_type and isinstance(batch, dict):
            batch = self._training_batch_type.from_dict(batch)

        reward = batch.reward
        self.reporter.log(eval_rewards=reward.flatten().detach().cpu())

        r = self._forward(batch, training=False)
        self.reporter.log(eval_pred_rewards=r["predicted_reward"].flatten().detach().cpu())

        detached_loss = r["loss"].view(()).detach().cpu()
        self.reporter.log(eval_loss=detached_loss)

        if r["unweighted_loss"] is not None:
            self.reporter.log(eval_unweighted_loss=r["unweighted_loss"].view(()).detach().cpu())

        return detached_loss.item()

    def validation_epoch_end(self, outputs):
        self.reporter.update_best_model(np.mean(outputs), self.reward_net)

    def warm_start_components(self):
        return ["reward_net"]
