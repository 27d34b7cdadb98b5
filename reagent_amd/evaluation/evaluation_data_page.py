"""reagent/evaluation/evaluation_data_page.py: EvaluationDataPage for the discrete DQN trainers, resident on the device.

THE PAGE STAYS ON THE DEVICE.  The reference moves every validation batch's page to the host (``validation_step`` ends in
``.cpu()``) and walks it there row by row; here ``validation_step`` does not call ``.cpu()``, the page's fields are device
tensors from creation to the estimators, and the per-row work is in the kernels of csrc/cpe_eval.hip:

  create_from_tensors_dqn   the non-saving forwards of q_network, q_network_cpe and reward_network on `state`, then ONE
                            rg_cpe_page_rows launch; the column slices (model_values, model_rewards, model_metrics,
                            model_metrics_values, optimal_q_values) are views of the forward outputs
  sort                      a stable order by (mdp_id, sequence_number, row): two torch.argsort(stable=True) on the device (once
                            per validation epoch: control plane)
  compute_values            rg_cpe_episode_values, one lane per episode; a column of a wider matrix is scanned at its pitch
  validate                  the reference's assertions; monotone sequence numbers and unbroken MDPs by tensor comparisons

Only ``rlt.DiscreteDqnInput`` is served: ``rlt.ParametricDqnInput``, ranking inputs and anything else raise
NotImplementedError by name.  ``.cpu()`` still works (TensorDataClass) for a caller that wants the page on the host.
"""
from __future__ import annotations

import dataclasses
import logging
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..core import types as rlt

logger = logging.getLogger(__name__)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def episode_offsets(mdp_id: torch.Tensor) -> torch.Tensor:
    """[E + 1] int32 on mdp_id's device: episode e of a SORTED page is rows offsets[e] .. offsets[e + 1] - 1.  Computed with
    torch ops (`mdp_id[1:] != mdp_id[:-1]`, `nonzero`), once per page."""
    flat = mdp_id.reshape(-1)
    n = flat.numel()
    starts = (torch.nonzero(flat[1:] != flat[:-1]).reshape(-1) + 1).to(torch.int32)
    ends = torch.tensor([0], dtype=torch.int32, device=flat.device), torch.tensor([n], dtype=torch.int32, device=flat.device)
    return torch.cat((ends[0], starts, ends[1])).contiguous()


def _sequence_i64(sequence_number: torch.Tensor) -> torch.Tensor:
    return sequence_number.reshape(-1).to(torch.int64).contiguous()


@dataclass
class EvaluationDataPage(rlt.TensorDataClass):
    mdp_id: Optional[torch.Tensor]
    sequence_number: Optional[torch.Tensor]
    logged_propensities: torch.Tensor
    logged_rewards: torch.Tensor
    action_mask: torch.Tensor
    model_propensities: torch.Tensor
    model_rewards: torch.Tensor
    model_rewards_for_logged_action: torch.Tensor
    model_values: Optional[torch.Tensor] = None
    possible_actions_mask: Optional[torch.Tensor] = None
    optimal_q_values: Optional[torch.Tensor] = None
    eval_action_idxs: Optional[torch.Tensor] = None
    logged_values: Optional[torch.Tensor] = None
    logged_metrics: Optional[torch.Tensor] = None
    logged_metrics_values: Optional[torch.Tensor] = None
    model_metrics: Optional[torch.Tensor] = None
    model_metrics_for_logged_action: Optional[torch.Tensor] = None
    model_metrics_values: Optional[torch.Tensor] = None
    model_metrics_values_for_logged_action: Optional[torch.Tensor] = None
    possible_actions_state_concat: Optional[torch.Tensor] = None
    contexts: Optional[torch.Tensor] = None

    def _replace(self, **changes):
        return dataclasses.replace(self, **changes)

    @classmethod
    def create_from_training_batch(cls, tdb, trainer, reward_network=None):
        if isinstance(tdb, rlt.DiscreteDqnInput):
            return EvaluationDataPage.create_from_tensors_dqn(
                trainer,
                tdb.extras.mdp_id,
                tdb.extras.sequence_number,
                tdb.state,
                tdb.action,
                tdb.extras.action_probability,
                tdb.reward,
                tdb.possible_actions_mask,
                metrics=tdb.extras.metrics,
            )
        elif isinstance(tdb, rlt.ParametricDqnInput):
            raise NotImplementedError(
                "EvaluationDataPage.create_from_tensors_parametric_dqn (rlt.ParametricDqnInput) is not built: CPE covers "
                "the discrete DQN trainers")
        else:
            raise NotImplementedError(f"training_input type: {type(tdb)}")

    @classmethod
    def create_from_tensors_seq2slate(cls, *args, **kwargs):
        raise NotImplementedError("EvaluationDataPage.create_from_tensors_seq2slate is not built: there is no ranking model here")

    @classmethod
    def create_from_tensors_parametric_dqn(cls, *args, **kwargs):
        raise NotImplementedError(
            "EvaluationDataPage.create_from_tensors_parametric_dqn is not built: CPE covers the discrete DQN trainers")

    @classmethod
    @torch.no_grad()
    def create_from_tensors_dqn(
        cls,
        trainer,
        mdp_ids: torch.Tensor,
        sequence_numbers: torch.Tensor,
        states: rlt.FeatureData,
        actions: torch.Tensor,
        propensities: torch.Tensor,
        rewards: torch.Tensor,
        possible_actions_mask: torch.Tensor,
        metrics: Optional[torch.Tensor] = None,
    ):
        """evaluation_data_page.py:309-462.  The three networks run in eval mode with their training flags restored (:321-332,
        435-439); the page is left on the device the batch is on."""
        check = getattr(trainer, "_check_cpe_evaluation", None)
        if check is None:
            raise NotImplementedError(
                f"EvaluationDataPage.create_from_tensors_dqn serves DQNTrainer and QRDQNTrainer, not {type(trainer).__name__}")
        check()
        nets = (trainer.q_network, trainer.reward_network, trainer.q_network_cpe)
        old_train_states = [n.training for n in nets]
        for n in nets:
            n.train(False)
        try:
            num_actions = trainer.num_actions
            action_mask = actions.float()
            q_cpe_out = trainer.q_network_cpe(states)
            # model outputs come from the q_network for the DQN trainers (QR-DQN: the mean over atoms)
            model_outputs = _f32c(trainer._cpe_model_outputs(states))
            rewards_and_metric_rewards = trainer.reward_network(states)
        finally:
            for n, was in zip(nets, old_train_states):
                n.train(was)
        B = action_mask.shape[0]
        assert q_cpe_out.shape[1] % num_actions == 0 and q_cpe_out.shape == rewards_and_metric_rewards.shape, (
            "Invalid shape: " + str(q_cpe_out.shape) + " != " + str(rewards_and_metric_rewards.shape))
        M = q_cpe_out.shape[1] // num_actions
        model_values = q_cpe_out[:, 0:num_actions]
        assert model_values.shape == actions.shape, "Invalid shape: " + str(model_values.shape) + " != " + str(actions.shape)
        assert model_values.shape == possible_actions_mask.shape, (
            "Invalid shape: " + str(model_values.shape) + " != " + str(possible_actions_mask.shape))
        model_rewards = rewards_and_metric_rewards[:, 0:num_actions]
        model_metrics = rewards_and_metric_rewards[:, num_actions:]
        num_metrics = M - 1
        boosts = trainer.reward_boosts.reshape(-1) if getattr(trainer, "_has_reward_boost", True) else None
        if boosts is not None and boosts.device != action_mask.device:
            boosts = boosts.to(action_mask.device)
        (logged_rewards, model_propensities, eval_action_idxs, model_rewards_for_logged_action, model_metrics_for_logged_action,
         model_metrics_values_for_logged_action) = ops.cpe_page_rows(
            model_outputs, _f32c(q_cpe_out), _f32c(rewards_and_metric_rewards), _f32c(action_mask),
            _f32c(possible_actions_mask), _f32c(rewards).reshape(-1), None if boosts is None else _f32c(boosts),
            trainer.rl_temperature, M)
        assert logged_rewards.shape[0] == B
        return cls(
            mdp_id=mdp_ids,
            sequence_number=sequence_numbers,
            logged_propensities=propensities,
            logged_rewards=logged_rewards,
            action_mask=action_mask,
            model_rewards=model_rewards,
            model_rewards_for_logged_action=model_rewards_for_logged_action,
            model_values=model_values,
            model_metrics_values=q_cpe_out[:, num_actions:] if num_metrics > 0 else None,
            model_metrics_values_for_logged_action=model_metrics_values_for_logged_action,
            model_propensities=model_propensities,
            logged_metrics=metrics,
            model_metrics=model_metrics,
            model_metrics_for_logged_action=model_metrics_for_logged_action,
            # Will compute later
            logged_values=None,
            logged_metrics_values=None,
            possible_actions_mask=possible_actions_mask,
            optimal_q_values=model_outputs,
            eval_action_idxs=eval_action_idxs,
        )

    def append(self, edp):
        new_edp = {}
        for x in fields(EvaluationDataPage):
            t = getattr(self, x.name)
            other_t = getattr(edp, x.name)
            assert int(t is not None) + int(other_t is not None) != 1, (
                "Tried to append when a tensor existed in one training page but not the other: " + x.name
            )
            if other_t is not None:
                if isinstance(t, torch.Tensor):
                    new_edp[x.name] = torch.cat((t, other_t), dim=0)
                elif isinstance(t, np.ndarray):
                    new_edp[x.name] = np.concatenate((t, other_t), axis=0)
                else:
                    raise Exception("Invalid type in training data page")
            else:
                new_edp[x.name] = None
        return EvaluationDataPage(**new_edp)

    def sort(self):
        """a stable order by (mdp_id, sequence_number, row), on the page's device"""
        by_seq = torch.argsort(self.sequence_number.reshape(-1).to(torch.int64), stable=True)
        order = by_seq[torch.argsort(self.mdp_id.reshape(-1)[by_seq], stable=True)]
        new_edp = {}
        for x in fields(EvaluationDataPage):
            t = getattr(self, x.name)
            new_edp[x.name] = t[order] if t is not None else None
        return EvaluationDataPage(**new_edp)

    def compute_values(self, gamma: float):
        assert self.mdp_id is not None and self.sequence_number is not None
        offsets = episode_offsets(self.mdp_id)
        seq = _sequence_i64(self.sequence_number)
        logged_values = _episode_values(self.logged_rewards, seq, offsets, gamma)
        logged_metrics_values: Optional[torch.Tensor] = None
        if self.logged_metrics is not None:
            logged_metrics_values = _episode_values(self.logged_metrics, seq, offsets, gamma)
        return self._replace(logged_values=logged_values, logged_metrics_values=logged_metrics_values)

    @staticmethod
    def compute_values_for_mdps(
        rewards: torch.Tensor, mdp_ids: torch.Tensor, sequence_numbers: torch.Tensor, gamma: float
    ) -> torch.Tensor:
        """evaluation_data_page.py:523-540 on a sorted page.  KEPT QUIRK of the reference: it scans `values[x, 0]` alone, so of a
        [N, C] `rewards` (logged_metrics with more than one extra metric) only column 0 becomes values; the other columns
        leave as the clone left them.  Users compare logged_metrics_values between the two implementations, so they do here
        too."""
        return _episode_values(rewards, _sequence_i64(sequence_numbers), episode_offsets(mdp_ids), gamma)

    def validate(self):
        assert len(self.logged_propensities.shape) == 2
        assert len(self.logged_rewards.shape) == 2
        assert len(self.logged_values.shape) == 2
        assert len(self.model_propensities.shape) == 2
        assert len(self.model_rewards.shape) == 2
        assert len(self.model_values.shape) == 2

        assert self.logged_propensities.shape[1] == 1
        assert self.logged_rewards.shape[1] == 1
        assert self.logged_values.shape[1] == 1
        num_actions = self.model_propensities.shape[1]
        assert self.model_rewards.shape[1] == num_actions
        assert self.model_values.shape[1] == num_actions

        assert self.action_mask.shape == self.model_propensities.shape

        if self.logged_metrics is not None:
            assert len(self.logged_metrics.shape) == 2
            assert len(self.logged_metrics_values.shape) == 2
            assert len(self.model_metrics.shape) == 2
            assert len(self.model_metrics_values.shape) == 2

            num_metrics = self.logged_metrics.shape[1]
            assert self.logged_metrics_values.shape[1] == num_metrics, (
                "Invalid shape: " + str(self.logged_metrics_values.shape) + " != " + str(num_metrics)
            )
            assert self.model_metrics.shape[1] == num_metrics * num_actions, (
                "Invalid shape: " + str(self.model_metrics.shape) + " != " + str(num_metrics * num_actions)
            )
            assert self.model_metrics_values.shape[1] == num_metrics * num_actions

        minibatch_size = self.logged_propensities.shape[0]
        logger.info("EvaluationDataPage data size: {}".format(minibatch_size))
        assert minibatch_size == self.logged_rewards.shape[0]
        assert minibatch_size == self.logged_values.shape[0]
        assert minibatch_size == self.model_propensities.shape[0]
        assert minibatch_size == self.model_rewards.shape[0]
        assert minibatch_size == self.model_values.shape[0]
        if self.logged_metrics is not None:
            assert minibatch_size == self.logged_metrics.shape[0]
            assert minibatch_size == self.logged_metrics_values.shape[0]
            assert minibatch_size == self.model_metrics.shape[0]
            assert minibatch_size == self.model_metrics_values.shape[0]

        if logger.isEnabledFor(logging.INFO):  # (each mean is a read-back: only where somebody listens)
            logger.info("Average logged reward = %s", self.logged_rewards.mean())
            for a in range(min(2, num_actions)):
                logger.info("Average model propensity for action %d = %s", a, self.model_propensities[:, a].mean())
            logger.info("Average logged propensity = %s", self.logged_propensities.mean())

        # sequence numbers increase inside an MDP, and an MDP's rows are adjacent: tensor comparisons, no per-row loop
        flatten_mdp_id = self.mdp_id.reshape(-1)
        seq = self.sequence_number.reshape(-1)
        same = flatten_mdp_id[1:] == flatten_mdp_id[:-1]
        not_increasing = same & (seq[1:] <= seq[:-1])
        if bool(not_increasing.any()):
            x = int(torch.nonzero(not_increasing)[0]) + 1
            raise AssertionError(
                f"For mdp_id {flatten_mdp_id[x].item()}, got {seq[x].item()} <= {seq[x - 1].item()}."
                f"Sequence number must be in increasing order.\n")
        mdp_count = int((~same).sum()) + 1 if flatten_mdp_id.numel() else 0
        unique_count = int(torch.unique(flatten_mdp_id).numel())
        assert unique_count == mdp_count, "MDPs are broken up. {} vs {}".format(unique_count, mdp_count)

    def set_metric_as_reward(self, i: int, num_actions: int):
        assert self.logged_metrics is not None, "metrics must not be none"
        assert self.logged_metrics_values is not None, "metrics must not be none"
        assert self.model_metrics is not None, "metrics must not be none"
        assert self.model_metrics_values is not None, "metrics must not be none"

        return self._replace(
            logged_rewards=self.logged_metrics[:, i : i + 1],
            logged_values=self.logged_metrics_values[:, i : i + 1],
            model_rewards=self.model_metrics[:, i * num_actions : (i + 1) * num_actions],
            model_values=self.model_metrics_values[:, i * num_actions : (i + 1) * num_actions],
            logged_metrics=None,
            logged_metrics_values=None,
            model_metrics=None,
            model_metrics_values=None,
        )


def _episode_values(columns: torch.Tensor, seq: torch.Tensor, offsets: torch.Tensor, gamma: float) -> torch.Tensor:
    """rg_cpe_episode_values over column 0 of `columns` [N, C], scanned at the matrix's pitch; the other columns are copies
    (see compute_values_for_mdps)"""
    src = _f32c(columns)
    out = src.clone()
    ops.cpe_episode_values(src[:, 0:1], seq, offsets, gamma, out[:, 0:1])
    return out
