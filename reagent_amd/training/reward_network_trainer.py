"""RewardNetTrainer with the surface of reagent/training/reward_network_trainer.py:20-190, executed on the HIP kernels: fits a
synthetic-reward net's masked sum of per-step rewards to the reward observed at the end of each sequence.

  forward : SyntheticRewardNet.run_head — rg_ngram_concat, the net's trunk (the FC stack or the LSTM stack), then
            rg_step_reward_head: the last Linear(P, 1) and its activation, the valid-step mask, the masked sum, the loss
            wrapper of :27-66 (BCE's division by valid_step, the reward_ignore_threshold filter, the mean over the kept rows)
            and d loss / d (trunk output, last linear)
  backward: the net's backward into its gradient slab, rg_adam_step over it

The generator path (training_step, backward, optimizer step) and train_step_native run the same launches on the same
buffers: the same bits.  The reference moves the loss to the host on every step (loss.detach().cpu()) and asserts in _gen_mask
and on the number of kept rows there; here the loss is read, and the kept-row count checked (the reference's assertion text),
only when a reporter is set, and the ten-batch logger.info follows the same rule.  validation_step always reads the loss back:
it returns a float.  The threshold filter is the reference's: on in training, off in validation (it gates on
pred.requires_grad).

Refused by name: weighted_by_inverse_propensity on a MemoryNetworkInput (the reference's message), PreprocessedRankingInput
batches, a reward_net that is not this package's SyntheticRewardNet, enable_data_parallel, HIP-graph capture.
"""
import logging
from enum import Enum
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from ..core import types as rlt
from ..engine import ensure_slab
from ..models.base import ModelBase
from ..models.synthetic_reward import SyntheticRewardNet
from ..optimizer import Optimizer__Union
from .plumbing import NativeStepMixin, SegmentLoss, held_gradients, native_step, publish_gradients
from .reagent_lightning_module import ReAgentLightningModule, _NoOpReporter

logger = logging.getLogger(__name__)


class LossFunction(Enum):
    MSE = "MSE_Loss"
    SmoothL1Loss = "SmoothL1_Loss"
    L1Loss = "L1_Loss"
    BCELoss = "BCE_Loss"


class RewardNetTrainer(NativeStepMixin, ReAgentLightningModule):
    _graph_capture_refusal = ("the reward-network step is not captured into a HIP graph: its buffers are allocated per step; "
                              "run it eagerly")

    def __init__(
        self,
        reward_net: ModelBase,
        optimizer: Optional[Optimizer__Union] = None,
        loss_type: LossFunction = LossFunction.MSE,
        reward_ignore_threshold: Optional[float] = None,
        weighted_by_inverse_propensity: bool = False,
    ) -> None:
        super().__init__()
        if not isinstance(reward_net, SyntheticRewardNet):
            raise NotImplementedError("RewardNetTrainer: reward_net must be a reagent_amd SyntheticRewardNet "
                                      f"(got {type(reward_net).__name__}): the step runs on its kernels")
        self.reward_net = reward_net
        self.optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.loss_type = LossFunction(loss_type)
        self.reward_ignore_threshold = reward_ignore_threshold
        self.weighted_by_inverse_propensity = weighted_by_inverse_propensity

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("RewardNetTrainer has no data-parallel path (world > 1 is not supported)")

    def configure_optimizers(self):
        optimizers = []
        optimizers.append(self.optimizer.make_optimizer_scheduler(self.reward_net.parameters()))
        return optimizers

    def _get_sample_weight(self, batch):
        weight = None
        if self.weighted_by_inverse_propensity:
            raise NotImplementedError(f"Sampling weighting not implemented for {type(batch)}")
        return weight

    def _get_target_reward(self, batch):
        if type(batch).__name__ == "PreprocessedRankingInput" or not hasattr(batch, "valid_step"):
            raise NotImplementedError(f"RewardNetTrainer: {type(batch).__name__} batches are not supported (rlt.MemoryNetworkInput "
                                      "with valid_step alone)")
        target_reward = batch.reward
        assert target_reward is not None
        return target_reward

    # ---- the step --------------------------------------------------------------------------------------------------------
    def _listening(self):
        return not isinstance(self.reporter, _NoOpReporter)

    def _forward(self, batch, training: bool):
        """one pass and the head -> the head's results (SyntheticRewardNet.run_head); training: saving, with the threshold
        filter and the gradients"""
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)
        self._get_sample_weight(batch)
        target_reward = self._get_target_reward(batch)
        dev = next(self.reward_net.parameters()).device
        B = batch.action.float_features.shape[1]
        assert len(target_reward.shape) == 2 and target_reward.shape == (B, 1), target_reward.shape
        target = self._f32c(target_reward.to(dev)).view(B)
        return self.reward_net.run_head(batch, save=training, target=target, loss_type=L.SRW_LOSS[self.loss_type.value],
                                        threshold=self.reward_ignore_threshold, apply_threshold=training, want_grad=training)

    def _check_kept(self, r, batch):
        """the reference's assertion (:59-62), where the loss is read"""
        assert int(r["n_kept"].item()) > 0, (
            f"reward ignore threshold set too small. target={self._get_target_reward(batch)}, "
            f"threshold={self.reward_ignore_threshold}"
        )

    def _backward(self, r, grad_out=None):
        net = self.reward_net
        params = list(net.parameters())
        slab = ensure_slab(params)
        held = held_gradients(slab, params)
        grads = (r["dh"], r["dw"], r["db"])
        if grad_out is not None:
            grads = tuple(g * grad_out for g in grads)
        net.backward(r["tape"], *grads)
        publish_gradients(slab, params, held)

    def train_step_gen(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        r = self._forward(training_batch, training=True)
        loss = SegmentLoss.apply(lambda g: self._backward(r, g), r["loss"], *self.reward_net.parameters())

        if self._listening():  # (nobody listens: no host synchronisation)
            self._check_kept(r, training_batch)
            detached_loss = loss.detach().cpu()
            self.reporter.log(loss=detached_loss)

            if self.all_batches_processed % 10 == 0:
                logger.info(f"{self.all_batches_processed}-th batch: {self.loss_type}={detached_loss.item()}")

        yield loss

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch: rlt.MemoryNetworkInput):
        """the step with no autograd graph, generator or host synchronisation -> the loss on the device"""
        (opt,) = self.native_optimizers()
        r = self._forward(training_batch, training=True)
        for p in self.reward_net.parameters():
            p.grad = None
        self._backward(r)
        opt.step()
        self.all_batches_processed += 1
        return dict(loss=r["loss"].view(()))

    @torch.no_grad()
    def validation_step(self, batch: rlt.MemoryNetworkInput, batch_idx: int):
        reward = self._get_target_reward(batch)
        self.reporter.log(eval_rewards=reward.flatten().detach().cpu())

        r = self._forward(batch, training=False)
        self.reporter.log(eval_pred_rewards=r["predicted_reward"].flatten().detach().cpu())

        detached_loss = r["loss"].view(()).detach().cpu()
        self.reporter.log(eval_loss=detached_loss)

        return detached_loss.item()

    def validation_epoch_end(self, outputs):
        self.reporter.update_best_model(np.mean(outputs), self.reward_net)

    def warm_start_components(self):
        return ["reward_net"]
