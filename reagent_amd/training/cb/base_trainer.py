"""BaseCBTrainerWithEval (reagent/training/cb/base_trainer.py:22-197): offline evaluation inside the training loop
(reagent_amd/evaluation/cb) and the hand-off to cb_training_step.  The torchrec-metrics branch is refused by name.

An evaluated step (base_trainer.py:98-129):
  1. where eval_model_update_critical_weight is set and the weight ingested since the last update has reached it: the
     evaluator's frozen model is replaced by a copy of the scorer, the local sums are aggregated and logged;
  2. the frozen model's forward_with_actions under arm_presence: the ucb of every arm and its masked arg-max, one call;
  3. rg_cb_eval_ingest: importance weights, effective weights and the nine running sums, on the device;
  4. new_batch = replace(batch, importance_weight=...);
  5. the trainer's step on new_batch with the effective weight the ingest wrote (`_step_with_weight`; a trainer that
     implements cb_training_step alone gets cb_training_step(new_batch, ...) and forms the product itself).
Nothing is read back, with one exception: the check of step 1 needs sum_weight_since_update_local on the host.  While the
batches carry no weight the evaluator keeps an exact host mirror of it; with weights it is one four-byte read a step, and
only where eval_model_update_critical_weight is set."""
import logging
from typing import Optional

import torch

from ...core.types import CBInput
from ...evaluation.cb.base_evaluator import BaseOfflineEval
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
        self.eval_module: Optional[BaseOfflineEval] = None
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

    def _check_eval_module(self, eval_module) -> None:
        if not isinstance(eval_module, BaseOfflineEval):
            raise NotImplementedError(f"eval_module: {type(eval_module).__name__} is not a reagent_amd.evaluation.cb."
                                      "BaseOfflineEval; no other evaluator is implemented")
        model = eval_module.eval_model
        if any(c.__name__ == "MABBaseModel" for c in type(model).__mro__):
            raise NotImplementedError("eval_module: an eval_model that is a MABBaseModel (non-contextual bandits) is not "
                                      "implemented")
        if not hasattr(model, "forward_with_actions"):
            raise NotImplementedError(f"eval_module: eval_model {type(model).__name__} is not one of this package's "
                                      "UCBBaseModel scorers (no forward_with_actions); MABBaseModel and other models are "
                                      "not implemented")

    def attach_eval_module(self, eval_module: BaseOfflineEval) -> None:
        """Attach an offline evaluation module: it keeps track of the reward during training and filters the batches."""
        if self.takes_list_batch:
            raise NotImplementedError("attach_eval_module: an eval_module on a trainer of List[CBInput] batches (the "
                                      "disjoint models) is not implemented")
        self._check_eval_module(eval_module)
        self.eval_module = eval_module

    @staticmethod
    def _row_weight(batch: CBInput) -> Optional[torch.Tensor]:
        """the weight a step's kernel takes for a batch as it is: effective_weight (types.py:1194-1203) without the tensor
        of ones where no weight is given"""
        if batch.importance_weight is not None:
            return batch.effective_weight
        return batch.weight

    def _step_with_weight(self, batch: CBInput, weight: Optional[torch.Tensor], batch_idx: int, optimizer_idx: int = 0):
        """cb_training_step with the rows' weight handed in: an evaluated step passes the product the ingest kernel wrote
        (the bits of _row_weight(batch)).  A trainer whose kernel takes a weight overrides this and has cb_training_step
        call it with _row_weight(batch); the default is for a trainer that implements cb_training_step alone."""
        return self.cb_training_step(batch, batch_idx, optimizer_idx)

    def _evaluate(self, batch: CBInput):
        """steps 1-4 of an evaluated step -> (the batch with its importance weights, its effective weights [B, 1])"""
        eval_module = self.eval_module  # (the caller has checked it)
        critical = self.eval_model_update_critical_weight
        if critical is not None:
            seen = eval_module.weight_since_update()
            if seen >= critical:
                logger.info(f"Updating the evaluated model after {seen} observations")
                eval_module.update_eval_model(self.scorer)
                eval_module.reset_weight_since_update()
                eval_module.num_eval_model_updates += 1
                eval_module._aggregate_across_instances()
                eval_module.log_metrics(step=self.global_step)
        with torch.no_grad():
            out = eval_module.eval_model.forward_with_actions(batch.context_arm_features, arm_presence=batch.arm_presence)
            return eval_module._ingest(batch, out["model_actions"], count_since_update=True)

    def cb_training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        raise NotImplementedError

    def training_step(self, batch: CBInput, batch_idx: int, optimizer_idx: int = 0) -> Optional[torch.Tensor]:
        """base_trainer.py:84-145: check the batch, pass it through the evaluator where one is attached, then
        cb_training_step on it.  The features of the chosen arm are NOT gathered here (add_chosen_arm_features): the
        trainer's kernel reads them in place."""
        if not self.takes_list_batch:
            refuse_disjoint(batch)
        if self.eval_module is None:
            self._check_input(batch, offline_eval=False)
            ret = self.cb_training_step(batch, batch_idx, optimizer_idx)
        else:
            if self.takes_list_batch:
                raise NotImplementedError("an attached eval_module on a trainer of List[CBInput] batches (the disjoint "
                                          "models) is not implemented")
            self._check_eval_module(self.eval_module)
            self._check_input(batch, offline_eval=True)
            new_batch, weight = self._evaluate(batch)
            ret = self._step_with_weight(new_batch, weight, batch_idx, optimizer_idx)
        self.all_batches_processed += 1
        return ret

    def on_train_start(self) -> None:
        # (the reference attaches the logger on rank 0 only; one process here: see BaseOfflineEval.log_metrics)
        eval_module = self.eval_module
        if eval_module is not None and self.logger is not None:
            eval_module.attach_logger(self.logger)

    def on_train_epoch_end(self) -> None:
        eval_module = self.eval_module
        if eval_module is not None:
            self._check_eval_module(eval_module)
            if eval_module.weight_since_update() > 0:  # only where new data came in since the last aggregation
                eval_module._aggregate_across_instances()
            eval_module.log_metrics(step=self.global_step)
