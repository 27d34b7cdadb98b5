"""BaseOfflineEval (reagent/evaluation/cb/base_evaluator.py:16-247): the state and the interface of an offline evaluator
of contextual bandits.  Constructor, buffer names, dtypes and ``metric_prefix`` are the reference's, so a ``state_dict``
moves either way.

``ingest_batch`` is ONE entry point here, rg_cb_eval_ingest (two launches, nothing read back): the importance weights and
the batch's sums, added to the ``_local`` buffers where they lie.  The methods the reference splits it into
(``_process_all_data``, ``_process_used_data``) therefore do not exist; a subclass states which sums it keeps by being
the ``PolicyEvaluator``.

KEPT QUIRK of the reference: without ``arm_presence`` its ``sizes`` [B, 1] times ``weights.squeeze()`` [B] broadcasts to
[B, B], so ``sum_size_weighted_*_local`` come out ``batch`` times too large and ``avg_size_accepted`` is B * A, not A.
Users compare these logged metrics between the two implementations, so they are the reference's numbers here too.  With
``arm_presence`` the sizes are the plain ones.
"""
import copy
import logging
from dataclasses import replace
from typing import Optional

import numpy as np
import torch

from ... import ops
from ...core.types import CBInput
from ...models.linear_regression import _world_size
from .utils import N_SUMS, ingest

logger = logging.getLogger(__name__)

# rg_cb_eval_ingest's sums, in the order of its arguments
SUM_BUFFERS = ("sum_weight_all_data_local", "sum_reward_weighted_all_data_local", "sum_size_weighted_all_data_local",
               "sum_reward_importance_weighted_accepted_local", "sum_reward_weighted_accepted_local",
               "sum_weight_accepted_local", "sum_importance_weight_accepted_local", "sum_size_weighted_accepted_local")
assert len(SUM_BUFFERS) == N_SUMS


def refuse_world() -> None:
    if _world_size() > 1:
        raise NotImplementedError("BaseOfflineEval: an initialised process group with world > 1 (the sum of the local "
                                  "buffers across trainers) is not implemented")


def _forget_mirror_after_load(module, incompatible_keys) -> None:
    module.forget_mirror()


class BaseOfflineEval(torch.nn.Module):
    """Base class of the offline evaluation algorithms of contextual bandits.  The evaluated model is copied, which
    freezes its state until update_eval_model() is called.

    Buffers ending in "_local" are per-instance sums since the last aggregation; those without are the totals
    _aggregate_across_instances() adds them to.  "accepted" means "used".  Without arm_presence the two size sums carry
    the reference's factor `batch` (see the module docstring)."""

    metric_prefix: str = "[model]Offline_Eval_"

    def __init__(self, eval_model: torch.nn.Module, logger=None, max_importance_weight: Optional[float] = None):
        super().__init__()
        refuse_world()
        self.eval_model = copy.deepcopy(eval_model)  # (host flags such as a scorer's _coefs_dirty are copied with it)
        self.logger = logger
        self.max_importance_weight = max_importance_weight
        f = dict(dtype=torch.float)
        for name in ("sum_weight_accepted", "sum_weight_accepted_local", "sum_importance_weight_accepted",
                     "sum_importance_weight_accepted_local", "sum_weight_all_data", "sum_weight_all_data_local",
                     "sum_weight_since_update_local"):
            self.register_buffer(name, torch.zeros(1, **f))
        self.register_buffer("num_eval_model_updates", torch.zeros(1, dtype=torch.int))
        for name in ("sum_reward_weighted_accepted", "sum_reward_weighted_accepted_local",
                     "sum_reward_importance_weighted_accepted", "sum_reward_importance_weighted_accepted_local",
                     "sum_reward_weighted_all_data_local", "sum_size_weighted_accepted_local",
                     "sum_size_weighted_all_data_local", "frac_accepted", "avg_reward_accepted", "avg_reward_rejected",
                     "avg_size_accepted", "avg_size_rejected", "accepted_rejected_reward_ratio", "avg_reward_all_data"):
            self.register_buffer(name, torch.zeros(1, **f))
        # sum_weight_since_update_local as the host knows it (None: not known): exact while every batch is unweighted, so
        # the trainer's critical-weight check reads nothing back.  Whoever writes the buffer by hand calls forget_mirror()
        self._since_update_mirror: Optional[float] = 0.0
        # ... and so does every load that reaches this module, its own load_state_dict or the trainer's that holds it (a
        # nested load never calls a load_state_dict override; the frozen scorer refreshes its own host flag the same way)
        self.register_load_state_dict_post_hook(_forget_mirror_after_load)
        self._partials = {}
        self._scratch = None

    # ---- the host mirror of sum_weight_since_update_local ---------------------------------------------------------------
    def forget_mirror(self) -> None:
        self._since_update_mirror = None

    def weight_since_update(self) -> float:
        """sum_weight_since_update_local on the host: the mirror where it is known, else one four-byte read"""
        if self._since_update_mirror is None:
            self._since_update_mirror = float(self.sum_weight_since_update_local.item())
        return self._since_update_mirror

    def reset_weight_since_update(self) -> None:
        self.sum_weight_since_update_local.zero_()
        self._since_update_mirror = 0.0

    # ---- ingest ---------------------------------------------------------------------------------------------------------
    def _ingest(self, batch: CBInput, model_actions: torch.Tensor, count_since_update: bool):
        """-> (the batch with importance_weight [B, 1], effective_weight [B, 1] = weight * importance_weight from the same
        launch); count_since_update: the batch's weight also goes to sum_weight_since_update_local (the trainer's sum)"""
        assert batch.reward is not None
        B, dev = len(batch), batch.action.device
        key = (B, str(dev))
        if key not in self._partials:
            self._partials[key] = ops.cb_eval_partials(B, dev)
        if count_since_update:
            since = self.sum_weight_since_update_local
            if batch.weight is None and self._since_update_mirror is not None:
                # what the finishing launch does: the fp32 buffer plus the batch's total in double, rounded once
                self._since_update_mirror = float(np.float32(self._since_update_mirror + float(B)))
            else:
                self._since_update_mirror = None
        else:
            if self._scratch is None or self._scratch.device != dev:
                self._scratch = torch.zeros(1, dtype=torch.float32, device=dev)
            since = self._scratch
        iw, eff = ingest(batch, model_actions, self.max_importance_weight, [getattr(self, n) for n in SUM_BUFFERS], since,
                         self._partials[key])
        assert iw.shape == batch.reward.shape, (iw.shape, batch.reward.shape)
        return replace(batch, importance_weight=iw), eff

    @torch.no_grad()
    def ingest_batch(self, batch: CBInput, model_actions: torch.Tensor) -> CBInput:
        """base_evaluator.py:147-169: add the batch to the running sums and return it with importance_weight [B, 1] -- zero
        where the logged and the model's action differ"""
        return self._ingest(batch, model_actions, count_since_update=False)[0]

    def _aggregate_across_instances(self) -> None:
        raise NotImplementedError

    def get_avg_reward(self) -> float:
        raise NotImplementedError

    def update_eval_model(self, eval_model: torch.nn.Module) -> None:
        """the evaluated model replaced by a copy of eval_model in eval mode; when to call this mimics when the model
        would be updated in a deployment"""
        self.eval_model = copy.deepcopy(eval_model).eval()

    def attach_logger(self, logger) -> None:
        self.logger = logger

    def log_metrics(self, step: Optional[int] = None) -> None:
        # (the reference logs from rank 0 only, `get_rank() == 0`; one process here -- world > 1 is refused -- so there is no
        # check: whoever lifts that refusal restores it, here and in the trainer's on_train_start)
        logger.info(self.get_formatted_result_string())
        logger_ = self.logger
        if logger_ is not None:
            p = self.metric_prefix
            metric_dict = {
                f"{p}avg_reward": self.get_avg_reward(),
                f"{p}sum_weight_accepted": self.sum_weight_accepted.item(),
                f"{p}sum_weight_all_data": self.sum_weight_all_data.item(),
                f"{p}num_eval_model_updates": self.num_eval_model_updates.item(),
                f"{p}frac_accepted": self.frac_accepted.item(),
                f"{p}avg_reward_accepted": self.avg_reward_accepted.item(),
                f"{p}avg_reward_rejected": self.avg_reward_rejected.item(),
                f"{p}avg_size_accepted": self.avg_size_accepted.item(),
                f"{p}avg_size_rejected": self.avg_size_rejected.item(),
                f"{p}accepted_rejected_reward_ratio": self.accepted_rejected_reward_ratio.item(),
                f"{p}avg_reward_all_data": self.avg_reward_all_data.item(),
            }
            logger_.log_metrics(metric_dict, step=step)

    def get_formatted_result_string(self) -> str:
        return (f"Avg reward {self.get_avg_reward():0.3f} based on {int(self.sum_weight_accepted.item())} processed "
                f"observations (out of {int(self.sum_weight_all_data.item())} observations). The eval model has been "
                f"updated {self.num_eval_model_updates.item()} times")
