"""PPOTrainer (the "clip" version, https://arxiv.org/pdf/1707.06347.pdf) with the constructor / update surface of
reagent/training/ppo_trainer.py:27-412, executed on the HIP kernels (training/policy_gradient.py).

`training_step` buffers trajectories up to `update_freq`; `update_model` runs `update_epochs` passes over them in
minibatches of `ppo_batch_size` trajectories.  The reference runs its networks once per trajectory and sums the losses
(:386-402); here `_update_model` PACKS the minibatch — torch.cat of the trajectories' tensors plus an offsets tensor, the
one torch copy on this path — and runs one saving forward per network, one rg_pg_returns, one rg_pg_head and the loss
sums, then the value net's backward and step, then the policy's (:391-402).  The summed losses are the same numbers:
every per-trajectory quantity (returns, whitening) is computed per trajectory by the kernels.

  ppo_loss       = -sum min(adv * rho, adv * clamp(rho, 1 - eps, 1 + eps)) - entropy_weight * sum H       (:127-152)
  value_net_loss = MSELoss(sum)(baselines, offset_reinforcement)                                          (:234-242)
"""
from typing import Dict, List, Optional, Union

import torch

from .. import _lib as L
from ..core import types as rlt
from ..optimizer import Optimizer__Union
from .plumbing import native_step
from .policy_gradient import PolicyGradientMixin
from .reagent_lightning_module import ReAgentLightningModule, _NoOpReporter


class PPOTrainer(PolicyGradientMixin, ReAgentLightningModule):
    def __init__(
        self,
        policy,
        gamma: float = 0.9,
        optimizer: Optional[Optimizer__Union] = None,
        optimizer_value_net: Optional[Optimizer__Union] = None,
        actions: Optional[List[str]] = None,
        reward_clip: float = 1e6,  # rewards are clamped to this UPPER bound only (no lower bound)
        normalize: bool = True,
        subtract_mean: bool = True,
        offset_clamp_min: bool = False,
        update_freq: int = 1,  # how many env steps between updates
        update_epochs: int = 1,  # how many epochs to run when updating (for PPO)
        ppo_batch_size: int = 1,  # batch size (number of trajectories) used for PPO updates
        ppo_epsilon: float = 0.2,  # clamp importance weights between 1-epsilon and 1+epsilon
        entropy_weight: float = 0.0,  # weight of the entropy term in the PPO loss
        value_net=None,
        td_error_advantage: bool = False,
    ):
        # PPO relies on customized update schemas, achieved by manual_backward()
        super().__init__(automatic_optimization=False)
        # field(default_factory=...) of the reference: materialised here
        self.scorer = policy.scorer
        self.sampler = policy.sampler
        self.gamma = gamma
        self.optimizer_value_net = optimizer_value_net if optimizer_value_net is not None else Optimizer__Union.default()
        self.actions = actions if actions is not None else []
        self.reward_clip = reward_clip
        self.normalize = normalize
        self.subtract_mean = subtract_mean
        self.offset_clamp_min = offset_clamp_min
        self.update_freq = update_freq
        self.update_epochs = update_epochs
        self.ppo_batch_size = ppo_batch_size
        self.ppo_epsilon = ppo_epsilon
        self.entropy_weight = entropy_weight

        self.optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.value_net = value_net
        self.td_error_advantage = td_error_advantage
        if value_net is not None:
            self.value_loss_fn = torch.nn.MSELoss(reduction="sum")
            assert not self.normalize, "Can't apply a value baseline and normalize rewards simultaneously"
        if td_error_advantage:
            assert value_net is not None, "td_error_advantage requires a value_net to estimate V(s)"
        assert (ppo_epsilon >= 0) and (ppo_epsilon <= 1), "ppo_epsilon has to be in [0;1]"
        assert update_freq >= 1, "update_freq has to be >= 1"
        assert update_epochs >= 1, "update_epochs has to be >= 1"
        assert ppo_batch_size >= 1, "ppo_batch_size has to be >= 1"
        if td_error_advantage:
            raise NotImplementedError("PPOTrainer: td_error_advantage (the one-step TD error as the advantage) is not "
                                      "supported; the advantage is the reward-to-go minus the baseline")
        self._check_networks()

        self.traj_buffer = []

    # ---- the packed pass ---------------------------------------------------------------------------------------------
    def _forward_packed(self, trajectories: List[rlt.PolicyGradientInput]):
        """torch.cat of the trajectories' tensors + their offsets -> PolicyGradientMixin._pg_forward"""
        for t in trajectories:
            self._check_input(t)
            self._refuse_graph_input(t)
        masks = [t.possible_actions_mask for t in trajectories]
        assert all(m is None for m in masks) or all(m is not None for m in masks), (
            "the trajectories of a minibatch all carry a possible_actions_mask or none does")
        one = len(trajectories) == 1
        cat = (lambda ts: ts[0]) if one else (lambda ts: torch.cat(ts, dim=0))
        state = cat([t.state.float_features for t in trajectories])
        self._fwd_token = dict(policy=None, value=None)  # (what _trajectory_to_losses' backwards check the stacks against)
        offsets = [0]
        for t in trajectories:
            offsets.append(offsets[-1] + t.action.shape[0])
        return self._pg_forward(state, cat([t.action for t in trajectories]), cat([t.reward.detach() for t in trajectories]),
                                cat([t.log_prob.detach() for t in trajectories]), None if masks[0] is None else cat(masks),
                                torch.tensor(offsets, dtype=torch.int32, device=state.device), L.PG_PPO,
                                float(self.ppo_epsilon), float(self.entropy_weight), 1.0, bool(self.normalize),
                                bool(self.normalize and self.subtract_mean))

    @staticmethod
    def _weight_versions(net):
        """what changes when a parameter is written: torch's in-place counter and the HIP optimizers' own"""
        return None if net is None else tuple((p._version, getattr(p, "_rg_version", 0)) for p in net.parameters())

    def _trajectory_to_losses(self, trajectory: rlt.PolicyGradientInput) -> Dict[str, torch.Tensor]:
        """Get a dict of losses for the trajectory. Dict always includes PPO loss.
        If a value baseline is trained, a loss for the value network is also included.

        Each loss carries its own backward: the output gradients of THIS trajectory are kept with it, and a backward
        that runs after another trajectory went through the networks repeats its network's saving forward first (the
        reference's autograd graph keeps every trajectory's activations; the stacks keep the latest).  A network's
        weights must not move between building its loss and running that loss's backward — autograd would go back through
        the weights it saved, the stack through the current ones — and a backward that finds them moved raises."""
        self._forward_packed([trajectory])
        token = object()
        built = dict(policy=self._weight_versions(self.scorer), value=self._weight_versions(self.value_net))

        def unmoved(which, net):
            if self._weight_versions(net) != built[which]:
                raise RuntimeError(f"PPOTrainer._trajectory_to_losses: the {which} network's weights changed between building "
                                   "this loss and its backward; build the loss again after the optimizer step")

        self._fwd_token = dict(policy=token, value=token)
        state = self._f32c(trajectory.state.float_features)
        n = state.shape[0]
        dscores = self._dscores.clone()

        def policy_backward(grad_out):
            unmoved("policy", self.scorer)
            if self._fwd_token["policy"] is not token:
                self._pg_workspace(n, dscores.shape[1], state.device)
                self._pe = self._trainable(self.scorer)
                self._p_xt = self._forward_net(self._pe, state, self._scores)
                self._fwd_token["policy"] = token
            self._pe.backward(dscores, self._p_xt, grad_out)

        losses = {"ppo_loss": self._pe.loss(policy_backward, self._ploss)}
        if self.value_net is not None:
            dvalues = self._dvalues.clone().view(n, 1)

            def value_backward(grad_out):
                unmoved("value", self.value_net)
                if self._fwd_token["value"] is not token:
                    self._pg_workspace(n, dscores.shape[1], state.device)
                    self._ve = self._trainable(self.value_net)
                    self._v_xt = self._forward_net(self._ve, state, self._values.view(n, 1))
                    self._fwd_token["value"] = token
                self._ve.backward(dvalues, self._v_xt, grad_out)

            losses["value_net_loss"] = self._ve.loss(value_backward, self._vloss)
        return losses

    def _check_input(self, trajectory: rlt.PolicyGradientInput) -> None:
        assert trajectory.action.ndim == 2, f"action must be 2-D, got {trajectory.action.shape}"
        trajectory_length = trajectory.action.shape[0]
        assert trajectory_length > 0, "trajectory must contain at least one step"
        assert trajectory.reward.ndim == 1, f"reward must be 1-D, got {trajectory.reward.shape}"
        assert trajectory.log_prob.ndim == 1, f"log_prob must be 1-D, got {trajectory.log_prob.shape}"
        assert trajectory.reward.shape[0] == trajectory_length, (
            f"reward length {trajectory.reward.shape[0]} != action length {trajectory_length}")
        assert trajectory.log_prob.shape[0] == trajectory_length, (
            f"log_prob length {trajectory.log_prob.shape[0]} != action length {trajectory_length}")
        if trajectory.possible_actions_mask is not None:
            assert trajectory.possible_actions_mask.ndim == 2, (
                f"possible_actions_mask must be 2-D, got {trajectory.possible_actions_mask.shape}")
            assert trajectory.possible_actions_mask.shape[0] == trajectory_length, (
                f"possible_actions_mask length {trajectory.possible_actions_mask.shape[0]} != action length {trajectory_length}")
        if trajectory.not_terminal is not None:
            assert trajectory.not_terminal.ndim == 1, f"not_terminal must be 1-D, got {trajectory.not_terminal.shape}"
            assert trajectory.not_terminal.shape[0] == trajectory_length, (
                f"not_terminal length {trajectory.not_terminal.shape[0]} != action length {trajectory_length}")
        if trajectory.next_state is not None:
            assert trajectory.next_state.float_features.shape[0] == trajectory_length, (
                f"next_state length {trajectory.next_state.float_features.shape[0]} != action length {trajectory_length}")

    def configure_optimizers(self):
        optimizers = []
        # value net optimizer
        if self.value_net is not None:
            optimizers.append(self.optimizer_value_net.make_optimizer_scheduler(self.value_net.parameters()))
        # policy optimizer
        optimizers.append(self.optimizer.make_optimizer_scheduler(self.scorer.parameters()))
        return optimizers

    def optimizers(self, use_pl_optimizer: bool = True):
        return self.native_optimizers()  # one set of optimizer states for the packed update and a manual caller

    def get_optimizers(self):
        opts = self.optimizers()
        if self.value_net is not None:
            return opts[0], opts[1]
        return None, opts[0]

    def train_step_gen(self, training_batch: rlt.PolicyGradientInput, batch_idx: int):
        raise NotImplementedError("PPOTrainer optimizes manually: call training_step(trajectory, batch_idx)")

    def training_step(self, training_batch: Union[rlt.PolicyGradientInput, Dict[str, torch.Tensor]], batch_idx: int):
        if isinstance(training_batch, dict):
            training_batch = rlt.PolicyGradientInput.from_dict(training_batch)

        self.traj_buffer.append(training_batch)
        if len(self.traj_buffer) == self.update_freq:
            self.update_model()

    def _minibatch_order(self, n: int) -> torch.Tensor:
        """the order in which an epoch visits the n buffered trajectories (a test feeds the reference's recorded order)"""
        return torch.randperm(n)

    def update_model(self):
        assert len(self.traj_buffer) == self.update_freq, (
            "trajectory buffer does not have sufficient samples for model_update")
        for _ in range(self.update_epochs):
            # iterate through minibatches of PPO updates in random order
            random_order = self._minibatch_order(len(self.traj_buffer))
            for i in range(0, len(self.traj_buffer), self.ppo_batch_size):
                idx = random_order[i : i + self.ppo_batch_size]
                training_batch_list = [self.traj_buffer[i] for i in idx]
                self._update_model(training_batch_list)

        self.traj_buffer = []  # empty the buffer

    @torch.no_grad()
    @native_step
    def _update_model(self, training_batch_list: List[rlt.PolicyGradientInput]):
        if self.logger is not None:
            raise NotImplementedError("PPOTrainer: a logger (the per-update _eval_metrics pass: a second run of the networks "
                                      "per trajectory and a host synchronisation) is not supported; set a reporter")
        value_net_opt, ppo_opt = self.get_optimizers()
        self._forward_packed(training_batch_list)
        if self.value_net is not None:
            # TD loss for the baseline value network
            self._native_segment(self._ve, self._backward_value, value_net_opt)
        # PPO "loss" for the policy network
        self._native_segment(self._pe, self._backward_policy, ppo_opt)
        # Report training metrics so they surface in the training output.
        if not isinstance(self.reporter, _NoOpReporter):
            self.reporter.log(
                ppo_loss=self._ploss.detach().clone().reshape(1),
                value_net_loss=self._vloss.detach().clone().reshape(1) if self.value_net is not None else torch.zeros(1),
            )
        return dict(ppo_loss=self._ploss, value_net_loss=self._vloss if self.value_net is not None else None)
