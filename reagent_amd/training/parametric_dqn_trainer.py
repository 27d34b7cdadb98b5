"""ParametricDQNTrainer with the constructor / generator surface of reagent/training/parametric_dqn_trainer.py:23-214,
executed on the HIP kernels: Q(s, a) over a per-state list of M = max_num_actions candidate actions given as feature
vectors (ReAgent's recommendation workload).

One step, in the reference's segment order:
  seg q      : maxq_learning — both critics on the B * M rows cat(next_state[b], possible_next_actions[b * M + j])
               (:122-146), masked arg-max per state (get_max_q_values_with_target); SARSA — the target critic on
               (next_state, next_action) (:151-158); y = r + not_terminal * discount * next_q (:160);
               q = q_network(state, action); loss = mse / huber / bce_with_logits(q, y) (:166-171)   -> Adam(q)
  seg reward : (reward_network only) mse(reward_network(state, action), reward) (:182-190)           -> Adam(reward)
  soft update of the target critic (:213-214).
The tiled next state is never written: a fused stack reads row r / M of next_state and row r of the candidates in place
(rg_mlp_desc.x_tile); every other engine gets the rows from rg_tile_concat.  The arg-max, the target, the loss and
d(mean loss)/dq are one rg_pdqn_head launch.
"""
from typing import Optional, Tuple

import torch

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..core.parameters import RLParameters
from ..optimizer import Optimizer__Union, SoftUpdate
from .dqn_trainer_base import DQNTrainerMixin
from .plumbing import NativeStepMixin, PanelCriticMixin, native_step
from .reagent_lightning_module import ReAgentLightningModule
from .rl_trainer_pytorch import RLTrainerMixin

_LOSS = dict(L.LOSS, bce_with_logits=L.LOSS_BCE_LOGITS)


class ParametricDQNTrainer(PanelCriticMixin, NativeStepMixin, DQNTrainerMixin, RLTrainerMixin, ReAgentLightningModule):
    def __init__(
        self,
        q_network,
        q_network_target,
        reward_network: Optional[torch.nn.Module] = None,
        # Start ParametricDQNTrainerParameters
        rl: Optional[RLParameters] = None,
        double_q_learning: bool = True,
        minibatches_per_step: int = 1,
        optimizer: Optional[Optimizer__Union] = None,
        log_tensorboard: bool = False,
    ) -> None:
        super().__init__()
        # @resolve_defaults of the reference: default_factory values materialised here
        rl = rl if rl is not None else RLParameters()
        self.rl_parameters = rl
        self.double_q_learning = double_q_learning
        self.minibatches_per_step = minibatches_per_step or 1
        self.q_network = q_network
        self.q_network_target = q_network_target
        self.reward_network = reward_network
        self.optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.log_tensorboard = log_tensorboard
        if rl.q_network_loss == "bce_with_logits":
            # The loss is only used when gamma = 0, reward is between 0 and 1 (:55-61)
            assert rl.gamma == 0, "bce_with_logits loss is only supported when gamma is 0."
        elif rl.q_network_loss not in _LOSS:
            raise Exception("Q-Network loss type {} not valid loss.".format(rl.q_network_loss))
        self._loss_type = _LOSS[rl.q_network_loss]
        self._ws_key = None

    # ---- optimizers (:67-87) -------------------------------------------------------------------------
    def configure_optimizers(self):
        optimizers = [self.optimizer.make_optimizer_scheduler(self.q_network.parameters())]
        if self.reward_network is not None:
            optimizers.append(self.optimizer.make_optimizer_scheduler(self.reward_network.parameters()))
        target_params = list(self.q_network_target.parameters())
        source_params = list(self.q_network.parameters())
        optimizers.append(SoftUpdate.make_optimizer_scheduler(target_params, source_params, tau=self.tau))
        return optimizers

    def _check_input(self, training_batch: rlt.ParametricDqnInput):
        assert isinstance(training_batch, rlt.ParametricDqnInput)
        assert training_batch.not_terminal.dim() == training_batch.reward.dim() == 2
        assert training_batch.not_terminal.shape[1] == training_batch.reward.shape[1] == 1
        assert training_batch.action.float_features.dim() == training_batch.next_action.float_features.dim() == 2

    @torch.no_grad()
    def get_detached_model_outputs(self, state, action) -> Tuple[torch.Tensor, torch.Tensor]:
        """Gets the q values from the model and target networks"""
        q_values = self.q_network(state, action)
        q_values_target = self.q_network_target(state, action)
        return q_values, q_values_target

    # ---- engine --------------------------------------------------------------------------------------
    def _engine(self, B, M, dev, S, A):
        nets = dict(q=self.q_network, reward=self.reward_network)
        self._e = {k: self._trainable(n) for k, n in nets.items() if n is not None}
        self._t = self.q_network_target.fc.stack()
        key = (B, M, S, A, dev)
        if self._ws_key != key:
            f = dict(dtype=torch.float32, device=dev)
            P = ops.pdqn_head_partials(B)
            for n in ("qv", "y", "dq", "nq", "rv", "ry", "rdq", "rnq"):
                setattr(self, "_" + n, torch.empty(B, 1, **f))
            self._qn_on, self._qn_tg = torch.empty(B * M, 1, **f), torch.empty(B * M, 1, **f)
            self._next_idx = torch.empty(B, dtype=torch.int64, device=dev)
            self._parts = {n: torch.empty(P, **f) for n in ("q", "reward")}
            self._losses = {n: torch.empty(1, **f) for n in ("q", "reward")}
            self._cat = {}  # rows -> assembled [rows, S + A] critic input (engines that do not read panels)
            self._ws_key = key

    # ---- segments ------------------------------------------------------------------------------------
    def _q_forward(self, b):
        state, next_state = b.state.float_features, b.next_state.float_features
        action = self._f32c(b.action.float_features)
        L.require_cuda(state, "training_batch.state")
        B, S, A, dev = state.shape[0], state.shape[1], action.shape[1], state.device
        maxq = bool(self.maxq_learning)
        M = 1
        if maxq:
            pna = self._f32c(b.possible_next_actions.float_features)
            product, batch_size = pna.shape[0], b.possible_next_actions_mask.shape[0]
            assert product % batch_size == 0, (
                f"batch_size * max_num_action {product} is not divisible by batch_size {batch_size}")
            M = product // batch_size
        self._engine(B, M, dev, S, A)
        e, t = self._e["q"], self._t
        e.stack.stage_weights(need_transposed=True)
        t.stage_weights(need_transposed=False)
        if maxq:
            if self.double_q_learning:  # the arg-max keys on the online values (single-q never reads them)
                self._critic_rows(e.stack, next_state, pna, self._qn_on, M=M)
            self._critic_rows(t, next_state, pna, self._qn_tg, M=M)
            qn_tg, mask = self._qn_tg, self._f32c(b.possible_next_actions_mask)
        else:  # SARSA (Use the target network)
            qn_tg, mask = self._qn_tg[:B], None
            self._critic_rows(t, next_state, self._f32c(b.next_action.float_features), qn_tg)
        gamma_exp = self._gamma_exponent(b)
        self._x_t = self._critic_rows(e.stack, state, action, self._qv, save=True)  # Q-value of action taken
        ops.pdqn_head(self._qv, self._qn_on if maxq and self.double_q_learning else None, qn_tg, mask,
                      self._f32c(b.reward).reshape(-1), self._f32c(b.not_terminal).reshape(-1), self.gamma, gamma_exp,
                      self.double_q_learning, self._loss_type, self._y, self._dq, self._parts["q"], self._nq, self._next_idx)
        ops.reduce_sum(self._parts["q"], self._parts["q"].numel(), 1.0 / B, self._losses["q"])

    def _reward_forward(self, b):
        """reward_estimates = reward_network(state, action); mse against the logged reward (:182-190) — rg_pdqn_head with a
        zero discount is exactly that regression"""
        if b.extras is not None and b.extras.metrics is not None:
            raise NotImplementedError("ParametricDQNTrainer: a reward_network with training_batch.extras.metrics (a "
                                      "multi-column reward target) is not supported; pass extras.metrics=None")
        e = self._e["reward"]
        assert e.stack.dims[-1] == 1, "the reward network has one output column"
        e.stack.stage_weights(need_transposed=True)
        B = b.state.float_features.shape[0]
        self._xr_t = self._critic_rows(e.stack, b.state.float_features, self._f32c(b.action.float_features), self._rv,
                                       save=True)
        ops.pdqn_head(self._rv, None, self._rv, None, self._f32c(b.reward).reshape(-1),
                      self._f32c(b.not_terminal).reshape(-1), 0.0, None, False, L.LOSS["mse"], self._ry, self._rdq,
                      self._parts["reward"], self._rnq, None)
        ops.reduce_sum(self._parts["reward"], self._parts["reward"].numel(), 1.0 / B, self._losses["reward"])

    def _backward(self, which, grad_out=None):
        dq, xt = (self._dq, self._x_t) if which == "q" else (self._rdq, self._xr_t)
        self._e[which].backward(dq, xt, grad_out)

    # ---- reference surface ---------------------------------------------------------------------------
    def validation_step(self, batch, batch_idx):
        raise NotImplementedError("ParametricDQNTrainer.validation_step: CPE (EvaluationDataPage) is built for DQNTrainer and QRDQNTrainer only")

    def train_step_gen(self, training_batch: rlt.ParametricDqnInput, batch_idx: int):
        self._check_input(training_batch)
        b = training_batch
        self._q_forward(b)
        yield self._e["q"].loss(lambda g: self._backward("q", g), self._losses["q"])
        if self.reward_network is not None:
            self._reward_forward(b)
            yield self._e["reward"].loss(lambda g: self._backward("reward", g), self._losses["reward"])
            reward_loss = self._losses["reward"].reshape(()).detach().cpu()
        else:
            reward_loss = torch.tensor([0.0])
        # Logging loss, rewards, and model values (:194-204)
        self.reporter.log(td_loss=self._losses["q"].reshape(()).detach().cpu(), reward_loss=reward_loss,
                          logged_rewards=b.reward, model_values_on_logged_actions=self._qv.detach().cpu())
        # Use the soft update rule to update target network
        yield self.soft_update_result()

    # ---- fused native step ---------------------------------------------------------------------------
    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch):
        """the q segment, the reward segment when there is a reward network, and the soft update, with no autograd
        graph / generator / host sync; max_num_actions comes from the shapes"""
        opts = self.native_optimizers()
        b = training_batch
        it = iter(opts)
        self._q_forward(b)
        out = dict(td_loss=self._losses["q"], reward_loss=None)
        for which in ("q", "reward"):
            if which == "reward":
                if self.reward_network is None:
                    continue
                self._reward_forward(b)
                out["reward_loss"] = self._losses["reward"]
            self._native_segment(self._e[which], lambda which=which: self._backward(which), next(it))
        next(it).step()  # soft update
        self.all_batches_processed += 1
        return out
