"""LinUCBTrainer (reagent/training/cb/linucb_trainer.py:18-96): the averages of x x^T and label * x of a LinearRegressionUCB,
updated by rg_linucb_accumulate on device-resident state -- two launches a step, no host synchronisation."""
import logging
from typing import Optional

import torch

from ... import ops
from ...core.types import CBInput
from ...models.linear_regression import LinearRegressionUCB, _world_size
from .base_trainer import BaseCBTrainerWithEval

logger = logging.getLogger(__name__)


class LinUCBTrainer(BaseCBTrainerWithEval):
    """Args: policy -- its scorer has to be a LinearRegressionUCB."""

    def __init__(self, policy, automatic_optimization: bool = False, *args, **kwargs):
        super().__init__(automatic_optimization=automatic_optimization, *args, **kwargs)
        assert isinstance(policy.scorer, LinearRegressionUCB), (
            "LinUCBTrainer requires the policy scorer to be LinearRegressionUCB")
        if _world_size() > 1:
            raise NotImplementedError("LinUCBTrainer: an initialised process group with world > 1 (the reduction of the "
                                      "epoch's averages across trainers) is not implemented")
        self.scorer = policy.scorer
        self._workspace = {}

    def configure_optimizers(self):
        return None  # the averages are updated by hand

    def _ws(self, batch: int, device) -> torch.Tensor:
        key = (batch, str(device))
        if key not in self._workspace:
            self._workspace[key] = ops.linucb_workspace(batch, self.scorer.input_dim, device)
        return self._workspace[key]

    def _accumulate(self, x, y, weight, action=None):
        s = self.scorer
        if x.shape[-1] != s.input_dim:
            raise ValueError(f"LinUCBTrainer: features of dimension {x.shape[-1]}, the scorer's input_dim is {s.input_dim}")
        x = x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()
        y = y if y.dtype == torch.float32 and y.is_contiguous() else y.float().contiguous()
        if weight is not None and not (weight.dtype == torch.float32 and weight.is_contiguous()):
            weight = weight.float().contiguous()
        if action is not None and not (action.dtype == torch.int64 and action.is_contiguous()):
            action = action.long().contiguous()
        ops.linucb_accumulate(x, y, weight, s.cur_avg_A, s.cur_avg_b, s.cur_sum_weight, s.cur_num_obs,
                              self._ws(x.shape[0], x.device), action=action)
        s.mark_dirty()

    def update_params(self, x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None):
        """x [B, d], y [B, 1], weight [B, 1] (None: ones): linucb_trainer.py:50-75, in place on the scorer's buffers"""
        self._accumulate(x, y, weight)

    def cb_training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        return self._step_with_weight(batch, self._row_weight(batch), batch_idx, optimizer_idx)

    def _step_with_weight(self, batch: CBInput, weight, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        assert batch.label is not None
        if batch.features_of_chosen_arm is not None:
            self._accumulate(batch.features_of_chosen_arm, batch.label, weight)
        else:  # [B, A, d] and the logged action, straight to the kernel
            assert batch.action is not None
            self._accumulate(batch.context_arm_features, batch.label, weight, action=batch.action)
        return None

    def apply_discounting_multiplier(self):
        self.scorer.sum_weight *= self.scorer.gamma

    def on_train_epoch_end(self):
        super().on_train_epoch_end()
        self.scorer._calculate_coefs()
        self.apply_discounting_multiplier()
