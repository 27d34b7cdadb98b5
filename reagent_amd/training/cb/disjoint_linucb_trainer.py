"""DisjointLinUCBTrainer (reagent/training/cb/disjoint_linucb_trainer.py:18-115): the per-arm sums of x x^T and reward * x
of a DisjointLinearRegressionUCB.  The reference's step is a Python loop of two small matmuls per arm; here the arms'
sub-batches are packed back to back and rg_dlinucb_accumulate updates every arm on device-resident state -- two launches a
step, no host synchronisation."""
import logging
from typing import List, Optional

import torch

from ... import ops
from ...core.types import CBInput
from ...models.disjoint_linucb_predictor import DisjointLinearRegressionUCB
from ...models.linear_regression import _world_size
from .base_trainer import BaseCBTrainerWithEval

logger = logging.getLogger(__name__)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


class DisjointLinUCBTrainer(BaseCBTrainerWithEval):
    """Args: policy -- its scorer has to be a DisjointLinearRegressionUCB.  A batch is a List[CBInput], one per arm."""

    takes_list_batch = True  # BaseCBTrainerWithEval.training_step lets a List[CBInput] through

    def __init__(self, policy, automatic_optimization: bool = False, *args, **kwargs):
        super().__init__(automatic_optimization=automatic_optimization, *args, **kwargs)
        assert isinstance(policy.scorer, DisjointLinearRegressionUCB), (
            "DisjointLinUCBTrainer requires the policy scorer to be DisjointLinearRegressionUCB")
        if _world_size() > 1:
            raise NotImplementedError("DisjointLinUCBTrainer: an initialised process group with world > 1 (the sum of the "
                                      "epoch's buffers across trainers) is not implemented")
        self.scorer = policy.scorer
        self.num_arms = policy.scorer.num_arms
        self._plans = {}  # (sub-batch sizes, device) -> (row_offsets on the device, longest sub-batch, workspace)

    def configure_optimizers(self):
        return None  # the sums are updated by hand

    def _plan(self, sizes, device):
        key = (tuple(sizes), str(device))
        if key not in self._plans:
            offsets = [0]
            for n in sizes:
                offsets.append(offsets[-1] + n)
            longest = max(sizes)
            self._plans[key] = (torch.tensor(offsets, dtype=torch.int64).to(device), longest,
                                ops.dlinucb_workspace(longest, len(sizes), self.scorer.input_dim, device))
        return self._plans[key]

    def _check_dim(self, x: torch.Tensor) -> None:
        if x.shape[-1] != self.scorer.input_dim:
            raise ValueError(f"DisjointLinUCBTrainer: features of dimension {x.shape[-1]}, the scorer's input_dim is "
                             f"{self.scorer.input_dim}")

    def update_params(self, arm_idx: int, x: torch.Tensor, y: Optional[torch.Tensor], weight: Optional[torch.Tensor] = None):
        """x [n, d], y [n, 1], weight [n, 1] (None: ones): disjoint_linucb_trainer.py:46-76 for one arm, in place on that
        arm's slice of the scorer's buffers -- the same entry point with arms = 1, the packed step's bits"""
        s = self.scorer
        assert x.dim() == 2 and y is not None
        self._check_dim(x)
        offsets, longest, ws = self._plan((x.shape[0],), x.device)
        ops.dlinucb_accumulate(_f32c(x), _f32c(y).reshape(-1), None if weight is None else _f32c(weight).reshape(-1), offsets,
                               longest, s.cur_A[arm_idx:arm_idx + 1], s.cur_b[arm_idx:arm_idx + 1],
                               s.cur_num_obs[arm_idx:arm_idx + 1], ws)

    def _check_input(self, batch: List[CBInput], offline_eval: bool = False):
        assert len(batch) == self.num_arms
        for sub_batch in batch:
            assert sub_batch.context_arm_features.ndim == 2
            assert sub_batch.reward is not None

    def cb_training_step(self, batch: List[CBInput], batch_idx: int, optimizer_idx: int = 0):
        """each element of batch is the sub-batch of one arm (an empty one leaves the arm alone): one torch.cat per field,
        one rg_dlinucb_accumulate"""
        s = self.scorer
        for sub in batch:
            self._check_dim(sub.context_arm_features)
        sizes = [sub.context_arm_features.shape[0] for sub in batch]
        x = _f32c(torch.cat([sub.context_arm_features for sub in batch]))
        y = _f32c(torch.cat([sub.reward.reshape(-1) for sub in batch]))
        weight = None
        if any(sub.weight is not None for sub in batch):  # ones only where some sub-batches carry a weight and others not
            weight = _f32c(torch.cat([sub.weight.reshape(-1) if sub.weight is not None
                                      else torch.ones(n, dtype=torch.float32, device=x.device)
                                      for sub, n in zip(batch, sizes)]))
        offsets, longest, ws = self._plan(sizes, x.device)
        ops.dlinucb_accumulate(x, y, weight, offsets, longest, s.cur_A, s.cur_b, s.cur_num_obs, ws)
        return None

    def apply_discounting_multiplier(self):
        self.scorer.b *= self.scorer.gamma
        self.scorer.A *= self.scorer.gamma

    def on_train_epoch_end(self):
        super().on_train_epoch_end()
        self.scorer._estimate_coefs()
        self.apply_discounting_multiplier()
