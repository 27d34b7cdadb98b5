"""CEMTrainer with the surface of reagent/training/cem_trainer.py:35-51: an ensemble of world models is fitted, each by its own
MDNRNNTrainer on the HIP kernels, and a CEMPlannerNetwork plans on them.  The planner reads the members' parameters in place,
so a plan made after a training step sees that step."""
from typing import List

import torch
import torch.nn as nn

from ..core import types as rlt
from ..core.parameters import CEMTrainerParameters
from ..models.cem_planner import CEMPlannerNetwork
from .reagent_lightning_module import ReAgentLightningModule
from .world_model.mdnrnn_trainer import MDNRNNTrainer


class CEMTrainer(ReAgentLightningModule):
    def __init__(self, cem_planner_network: CEMPlannerNetwork, world_model_trainers: List[MDNRNNTrainer],
                 parameters: CEMTrainerParameters) -> None:
        super().__init__()
        self.cem_planner_network = cem_planner_network
        self.world_model_trainers = nn.ModuleList(world_model_trainers)

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("CEMTrainer has no data-parallel path (world > 1 is not supported)")

    def configure_optimizers(self):
        return [o for t in self.world_model_trainers for o in t.configure_optimizers()]

    def train_step_gen(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        for t in self.world_model_trainers:
            yield from t.train_step_gen(training_batch, batch_idx)

    @torch.no_grad()
    def train_step_native(self, training_batch: rlt.MemoryNetworkInput):
        """each member's native step in order -> the members' loss dicts"""
        out = [t.train_step_native(training_batch) for t in self.world_model_trainers]
        self.all_batches_processed += 1
        return out
