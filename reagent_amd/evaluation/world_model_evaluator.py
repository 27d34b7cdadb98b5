"""The world-model evaluators with the surface of reagent/evaluation/world_model_evaluator.py (constructors, evaluate
signatures, result keys), executed on the HIP kernels of reagent_amd/csrc/wm_eval.hip.  Every pass runs without autograd and
saves nothing for a backward, which is all the reference's mdnrnn.eval() / .train() toggles change here (no dropout).

  LossEvaluator               host code over MDNRNNTrainer.get_loss: one pass, one read of the four losses
  FeatureImportanceEvaluator  the reference runs F + 1 get_loss passes on cloned, overwritten batches and F + 1 host reads.
                              Here: rg_wm_feature_fill (every replacement value on the device), then ONE sweep over V = F + 1
                              variants x B virtual rows (MDNRNN.ablation_losses: variant 0 is the unablated batch) and one
                              read of the V loss rows.  feature_loss_increase[i] = fp32(loss_{i+1}) - fp32(loss_0), stored
                              as fp32 like the reference's, action features first.
  FeatureSensitivityEvaluator two MDNRNN passes (MemoryNetwork.forward's, without the sigmas / logpi split nobody reads here),
                              the second on actions permuted by torch.randperm(batch_size) from torch's host generator (the
                              reference's own call: a seed reproduces it), rg_wm_mus_sensitivity on the two gmm_linear
                              outputs, one read.

Departure: a single column's replacement value is its mean accumulated in double and rounded once; the reference takes the
mean in fp32.
"""
import logging
from typing import Dict, List

import torch

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..models.lstm_stack import _f32c
from ..training.world_model.mdnrnn_trainer import LOSS_NAMES, MDNRNNTrainer

logger = logging.getLogger(__name__)
F32 = torch.float32


def _checked_trainer(who, trainer):
    if not isinstance(trainer, MDNRNNTrainer):
        raise NotImplementedError(f"{who}: trainer must be a reagent_amd MDNRNNTrainer (got {type(trainer).__name__}): "
                                  "the evaluation runs on its MDNRNN's kernels")
    return trainer


def _refuse_capture(who, trainer):
    if getattr(trainer, "_graph_mode", False):
        raise NotImplementedError(f"{who}: {trainer._graph_capture_refusal}")


def _blocks(who, name, starts, count, dim, offset=0):
    """[(start, end)] of `count` features from their sorted start indices inside a vector `dim` wide, shifted by offset"""
    starts = [int(s) for s in starts]
    if len(starts) != count:
        raise ValueError(f"{who}: {name} has {len(starts)} entries for {count} features")
    if any(b <= a for a, b in zip(starts, starts[1:])) or (starts and (starts[0] < 0 or starts[-1] >= dim)):
        raise ValueError(f"{who}: {name} {starts} is not sorted inside the vector (0 <= strictly increasing < {dim})")
    ends = starts[1:] + [dim]
    wide = max((e - s for s, e in zip(starts, ends)), default=0)
    if wide > L.WM_MAX_BLOCK:
        raise NotImplementedError(f"{who}: {name} holds a block {wide} columns wide (at most {L.WM_MAX_BLOCK})")
    return [(offset + s, offset + e) for s, e in zip(starts, ends)]


class LossEvaluator:
    """Evaluate losses on data pages"""

    def __init__(self, trainer: MDNRNNTrainer, state_dim: int) -> None:
        self.trainer = _checked_trainer("LossEvaluator", trainer)
        self.state_dim = state_dim

    @torch.no_grad()
    def evaluate(self, tdp: rlt.MemoryNetworkInput) -> Dict[str, float]:
        losses = self.trainer.get_loss(tdp, state_dim=self.state_dim)
        values = torch.stack([losses[k] for k in LOSS_NAMES]).cpu().tolist()
        return {k: values[LOSS_NAMES.index(k)] for k in ("loss", "gmm", "bce", "mse")}


class FeatureImportanceEvaluator:
    """Evaluate feature importance weights on data pages"""

    def __init__(self, trainer: MDNRNNTrainer, discrete_action: bool, state_feature_num: int, action_feature_num: int,
                 sorted_action_feature_start_indices: List[int], sorted_state_feature_start_indices: List[int]) -> None:
        """sorted_*_feature_start_indices: the starting index of each feature in the action / state vector (a one-hot enum
        takes several components)"""
        self.trainer = _checked_trainer("FeatureImportanceEvaluator", trainer)
        self.discrete_action = discrete_action
        self.state_feature_num = state_feature_num
        self.action_feature_num = action_feature_num
        self.sorted_action_feature_start_indices = sorted_action_feature_start_indices
        self.sorted_state_feature_start_indices = sorted_state_feature_start_indices

    @torch.no_grad()
    def evaluate(self, batch: rlt.MemoryNetworkInput):
        """feature importance: the loss increase when a state / action feature is set to its mean (one-hot: median) value;
        with discrete actions, an action's is the loss increase when every action is set to it"""
        who = "FeatureImportanceEvaluator"
        tr = self.trainer
        _refuse_capture(who, tr)
        net = tr.memory_network.mdnrnn
        dev = net.gmm_linear.weight.device
        states, actions = batch.state.float_features, batch.action.float_features
        T, B, S = states.shape
        A = actions.shape[2]
        state_blocks = _blocks(who, "sorted_state_feature_start_indices", self.sorted_state_feature_start_indices,
                               self.state_feature_num, S, offset=A)
        if self.discrete_action:
            assert A == self.action_feature_num
            if A > L.WM_MAX_BLOCK:
                raise NotImplementedError(f"{who}: a discrete action vector {A} wide (at most {L.WM_MAX_BLOCK})")
            action_blocks = [(0, A)] * A
        else:
            action_blocks = _blocks(who, "sorted_action_feature_start_indices", self.sorted_action_feature_start_indices,
                                    self.action_feature_num, A)
        table = [(0, 0)] + action_blocks + state_blocks
        V, N, In = len(table), T * B, A + S
        blocks = torch.tensor(table, dtype=torch.int32).to(dev)
        x = _f32c(torch.cat([actions.to(dev).float(), states.to(dev).float()], dim=-1)).view(N, In)
        fill = torch.zeros(In, dtype=F32, device=dev)
        measured = blocks[1 + A:] if self.discrete_action else blocks[1:]  # (the blocks whose value comes from the data)
        if measured.shape[0]:
            ops.wm_feature_fill(x, measured, fill)
        fill_stride = 0
        if self.discrete_action:  # a fill row per variant: action i's is e_i, a state feature's the measured values
            rows = fill.repeat(V, 1)
            rows[1:1 + A, :A] = torch.eye(A, dtype=F32, device=dev)
            fill, fill_stride = rows, In
        p = tr.params

        def rows_of(t, *shape):
            return _f32c(t.to(dev).float()).view(N, *shape)

        losses = net.ablation_losses(actions, states, rows_of(batch.next_state.float_features, S), rows_of(batch.reward),
                                     rows_of(batch.not_terminal), blocks, fill, fill_stride, max(e - s for s, e in table),
                                     (p.next_state_loss_weight, p.not_terminal_loss_weight, p.reward_loss_weight), True,
                                     (T - 1) * B if p.fit_only_one_next_step else 0)
        loss = losses[:, 3].cpu().double()  # the one read: V floats
        feature_importance = (loss[1:] - loss[0]).float()
        logger.info("**** Debug tool feature importance ****: {}".format(feature_importance))
        return {"feature_loss_increase": feature_importance.numpy()}


class FeatureSensitivityEvaluator:
    """Evaluate state feature sensitivity caused by varying actions"""

    def __init__(self, trainer: MDNRNNTrainer, state_feature_num: int, sorted_state_feature_start_indices: List[int]) -> None:
        self.trainer = _checked_trainer("FeatureSensitivityEvaluator", trainer)
        self.state_feature_num = state_feature_num
        self.sorted_state_feature_start_indices = sorted_state_feature_start_indices

    @torch.no_grad()
    def evaluate(self, batch: rlt.MemoryNetworkInput):
        """state feature sensitivity due to actions: randomly permute the actions over the batch and see how much the
        predicted next-state means move"""
        who = "FeatureSensitivityEvaluator"
        assert isinstance(batch, rlt.MemoryNetworkInput)
        _refuse_capture(who, self.trainer)
        net = self.trainer.memory_network.mdnrnn
        T, B, S = batch.next_state.float_features.shape
        table = _blocks(who, "sorted_state_feature_start_indices", self.sorted_state_feature_start_indices,
                        self.state_feature_num, S)
        states, actions = batch.state.float_features, batch.action.float_features
        z = net._run(actions, states)["z"]
        z_shuffled = net._run(actions[:, torch.randperm(B).to(actions.device), :], states)["z"]
        blocks = torch.tensor(table, dtype=torch.int32).to(z.device)
        sensitivity = torch.empty(len(table), dtype=F32, device=z.device)
        ops.wm_mus_sensitivity(z, z_shuffled, net.num_gaussians, S, blocks, sensitivity)
        feature_sensitivity = sensitivity.cpu()
        logger.info("**** Debug tool feature sensitivity ****: {}".format(feature_sensitivity))
        return {"feature_sensitivity": feature_sensitivity.numpy()}
