"""BaseCBTrainerWithEval (reagent/training/cb/base_trainer.py:22-197) without the offline-evaluation and torchrec-metrics
branches, which are refused by name."""
import logging
from typing import Optional

import torch

from ...core.types import CBInput
from ..reagent_lightning_module import ReAgentLightningModule
from .utils import refuse_disjoint

logger = logging.getLogger(__name__)


class BaseCBTrainerWithEval(ReAgentLightningModule):
    """A subclass implements cb_training_step(); training_step() is final: it checks the batch and hands it on."""

    scorer: torch.nn.Module
    takes_list_batch = False  # a trainer of the disjoint models (a List[CBInput], one batch per arm) declares True

    def __init__(self, eval_model_update_critical_weight: Optional[float] = None, recmetric_module=None,
                 log_every_n_steps: int = 0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert (log_every_n_steps > 0) == (recmetric_module is not None), (
            "recmetric_module should be provided if and only if log_every_n_steps > 0")
        if recmetric_module is not None or log_every_n_steps > 0:
            raise NotImplementedError("recmetric_module / log_every_n_steps > 0 (torchrec metrics of the training batches) "
                                      "is not implemented")
        self.eval_module = None
        self.eval_model_update_critical_weight = eval_model_update_critical_weight
        self.recmetric_module = None
        self.log_every_n_steps = 0

    def train_step_gen(self, training_batch: CBInput, batch_idx: int):  # (the CB trainers do not use the generator protocol)
        raise NotImplementedError

    def _check_input(self, batch: CBInput, offline_eval: bool = False) -> None:
        assert batch.context_arm_features.ndim == 3
        assert batch.label is not None
        assert batch.action is not None
        assert len(batch.action) == len(batch.label)
        assert len(batch.action) == batch.context_arm_features.shape[0]
        if offline_eval:
            assert batch.reward is not None
            assert len(batch.action) == len(batch.reward)

    def attach_eval_module(self, eval_module) -> None:
        raise NotImplementedError("attach_eval_module: an attached eval_module (offline evaluation inside the training loop) "
                                  "is not implemented")

    def cb_training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        raise NotImplementedError

    def training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        """base_trainer.py:84-145 with no evaluation module: check the batch, then cb_training_step on it.  The features of
        the chosen arm are NOT gathered here (add_chosen_arm_features): the trainer's kernel reads them in place."""
        if not self.takes_list_batch:
            refuse_disjoint(batch)
        if self.eval_module is not None:
            raise NotImplementedError("an attached eval_module (offline evaluation inside the training loop) is not "
                                      "implemented")
        self._check_input(batch, offline_eval=False)
        ret = self.cb_training_step(batch, batch_idx, optimizer_idx)
        self.all_batches_processed += 1
        return ret

    def on_train_start(self) -> None:
        pass

    def on_train_epoch_end(self) -> None:
        if self.eval_module is not None:
            raise NotImplementedError("an attached eval_module is not implemented")
