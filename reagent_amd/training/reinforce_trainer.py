"""ReinforceTrainer with the constructor / generator surface of reagent/training/reinforce_trainer.py:22-161, executed on
the HIP kernels (training/policy_gradient.py).  A batch is ONE trajectory: the packed step with offsets = [0, N].

  loss        = -(offset_reinforcement - baselines) @ log_prob                                          (:105, :132)
  off policy  = -(...) @ exp(clamp(log_prob - logged log_prob, max = log clip_param))                    (:124-130)
  value loss  = MSELoss(mean)(baselines, offset_reinforcement), yielded first                            (:117-122)
"""
from typing import List, Optional

import torch

from .. import _lib as L
from ..core import types as rlt
from ..optimizer import Optimizer__Union
from .plumbing import native_step
from .policy_gradient import PolicyGradientMixin
from .reagent_lightning_module import ReAgentLightningModule


class ReinforceTrainer(PolicyGradientMixin, ReAgentLightningModule):
    def __init__(
        self,
        policy,
        gamma: float = 0.0,
        optimizer: Optional[Optimizer__Union] = None,
        optimizer_value_net: Optional[Optimizer__Union] = None,
        actions: Optional[List[str]] = None,
        off_policy: bool = False,
        reward_clip: float = 1e6,
        clip_param: float = 1e6,
        normalize: bool = True,
        subtract_mean: bool = True,
        offset_clamp_min: bool = False,
        value_net=None,
        do_log_metrics: bool = False,
    ):
        super().__init__()
        # field(default_factory=...) of the reference: materialised here
        self._actions = actions if actions is not None else []
        self.scorer = policy.scorer
        self.sampler = policy.sampler
        self.gamma = gamma
        self.off_policy = off_policy
        self.reward_clip = reward_clip
        self.clip_param = clip_param
        self.normalize = normalize
        self.subtract_mean = subtract_mean
        self.offset_clamp_min = offset_clamp_min
        self.optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.optimizer_value_net = optimizer_value_net if optimizer_value_net is not None else Optimizer__Union.default()
        if value_net is not None:
            if self.normalize or self.subtract_mean:
                raise RuntimeError(
                    "Can't apply a baseline and reward normalization \
                    (or mean subtraction) simultaneously."
                )
            self.value_net = value_net
            self.value_loss_fn = torch.nn.MSELoss(reduction="mean")
        else:
            self.value_net = None
        self.do_log_metrics = do_log_metrics
        if self.do_log_metrics:
            raise NotImplementedError("ReinforceTrainer: do_log_metrics (per-iteration logger metrics, a host "
                                      "synchronisation per step) is not supported; read the losses the step returns")
        self._check_networks()

    def _check_input(self, training_batch: rlt.PolicyGradientInput):
        assert training_batch.reward.ndim == 1
        if self.off_policy:
            assert training_batch.log_prob.ndim == 1

    def configure_optimizers(self):
        optimizers = []
        # value net optimizer
        if self.value_net is not None:
            optimizers.append(self.optimizer_value_net.make_optimizer_scheduler(self.value_net.parameters()))
        # policy optimizer
        optimizers.append(self.optimizer.make_optimizer_scheduler(self.scorer.parameters()))
        return optimizers

    def _forward(self, b):
        self._check_input(b)
        self._refuse_graph_input(b)
        state = b.state.float_features
        n = state.shape[0]
        mode = L.PG_REINFORCE_OFF_POLICY if self.off_policy else L.PG_REINFORCE
        self._pg_forward(state, b.action, b.reward.detach(), b.log_prob if self.off_policy else None, b.possible_actions_mask,
                         self._one_trajectory(n, state.device), mode, float(self.clip_param), 0.0, 1.0 / n,
                         bool(self.normalize), bool(self.subtract_mean))

    def train_step_gen(self, training_batch: rlt.PolicyGradientInput, batch_idx: int):
        self._forward(training_batch)
        if self.value_net is not None:
            assert not (self.normalize or self.subtract_mean)
            yield self._ve.loss(self._backward_value, self._vloss)
        yield self._pe.loss(self._backward_policy, self._ploss)

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch):
        """the value segment (with a value net) and the policy segment with no autograd graph / generator / host sync"""
        opts = iter(self.native_optimizers())
        self._forward(training_batch)
        out = dict(loss=self._ploss, value_loss=None)
        if self.value_net is not None:
            self._native_segment(self._ve, self._backward_value, next(opts))
            out["value_loss"] = self._vloss
        self._native_segment(self._pe, self._backward_policy, next(opts))
        self.all_batches_processed += 1
        return out
