"""SlateQTrainer with the constructor / generator surface of reagent/training/slate_q_trainer.py:21-276, executed on the
HIP kernels: every state has C candidate documents, a slate of K of them is shown, the critic scores (state, document)
pairs and the TD target of every slate item is its reward plus the value-weighted sum of the next slate's item Q-values.

One step, in the reference's order:
  next slate : maxq_learning — the target critic on all B * C rows cat(next_state[b], candidates[b, c]) (the candidate
               panel is candidate_docs.float_features as it lies, x_tile = C), rg_slate_topk (:145-160); its q_sel ARE
               the target critic's values of the chosen documents (the reference runs the target a second time on the
               same rows), rg_slate_gather supplies their value * mask.
               SARSA — rg_slate_gather on next_action (terminal rows read document 0, :112-117; the caller's tensor is
               left as it is), the target critic on the gathered panel (x_tile = K).
  q          : rg_slate_gather on action (the same launch counts reward_mask's true entries), the online critic on the
               gathered panel, rg_slateq_head (:204-259): target, loss, d(mean loss)/dq  -> backward -> Adam(q)
  soft update of the target critic.
A fused stack reads cat(state[r / M], panel[r]) in place in its non-saving forwards; its saving forward on tiled rows,
and every other engine, takes the rows rg_tile_concat assembles (the tiled two-panel forward is forward-only).
"""
import enum
from typing import Optional

import torch

from .. import _lib as L
from .. import ops
from ..core import parameters as rlp
from ..core import types as rlt
from ..optimizer import Optimizer__Union, SoftUpdate
from .plumbing import NativeStepMixin, PanelCriticMixin, native_step
from .reagent_lightning_module import ReAgentLightningModule
from .rl_trainer_pytorch import RLTrainerMixin


class NextSlateValueNormMethod(enum.Enum):
    """The Q value of the current slate item is the sum of the item's short-term reward and the normalized sum of all item
    Q-values on the next slate, normalized by the current slate size or by the next slate size (:21-31)."""

    NORM_BY_CURRENT_SLATE_SIZE = "norm_by_current_slate_size"
    NORM_BY_NEXT_SLATE_SIZE = "norm_by_next_slate_size"


class SlateQTrainer(PanelCriticMixin, NativeStepMixin, RLTrainerMixin, ReAgentLightningModule):
    def __init__(
        self,
        q_network,
        q_network_target,
        slate_size,
        # Start SlateQTrainerParameters
        rl: Optional[rlp.RLParameters] = None,
        optimizer: Optional[Optimizer__Union] = None,
        slate_opt_parameters: Optional[rlp.SlateOptParameters] = None,
        discount_time_scale: Optional[float] = None,
        single_selection: bool = True,
        next_slate_value_norm_method: NextSlateValueNormMethod = NextSlateValueNormMethod.NORM_BY_CURRENT_SLATE_SIZE,
        minibatch_size: int = 1024,
        evaluation: Optional[rlp.EvaluationParameters] = None,
    ) -> None:
        super().__init__()
        # @resolve_defaults of the reference: default_factory values materialised here
        self.rl_parameters = rl if rl is not None else rlp.RLParameters(maxq_learning=False)
        self.discount_time_scale = discount_time_scale
        self.single_selection = single_selection
        self.next_slate_value_norm_method = next_slate_value_norm_method
        self.q_network = q_network
        self.q_network_target = q_network_target
        self.q_network_optimizer = optimizer if optimizer is not None else Optimizer__Union.default()
        self.slate_size = slate_size
        self.slate_opt_parameters = slate_opt_parameters
        self._ws_key = None

    def configure_optimizers(self):
        optimizers = [self.q_network_optimizer.make_optimizer_scheduler(self.q_network.parameters())]
        target_params = list(self.q_network_target.parameters())
        source_params = list(self.q_network.parameters())
        optimizers.append(SoftUpdate.make_optimizer_scheduler(target_params, source_params, tau=self.tau))
        return optimizers

    # ---- engine (PanelCriticMixin: the parametric trainer's critic on the same kind of rows) ------------------------
    def _engine(self, B, C, K, S, D, dev):
        self._e = self._trainable(self.q_network)
        self._t = self.q_network_target.fc.stack()
        key = (B, C, K, S, D, dev)
        if self._ws_key != key:
            f = dict(dtype=torch.float32, device=dev)
            self._panel, self._next_panel = torch.empty(B * K, D, **f), torch.empty(B * K, D, **f)
            self._w, self._wn = torch.empty(B, K, **f), torch.empty(B, K, **f)
            self._q_all, self._qn, self._qv = torch.empty(B * C, 1, **f), torch.empty(B * K, 1, **f), torch.empty(B * K, 1, **f)
            self._next_idx = torch.empty(B, K, dtype=torch.int64, device=dev)
            self._y, self._dq, self._nq = torch.empty(B, K, **f), torch.empty(B, K, **f), torch.empty(B, **f)
            self._n = torch.zeros(1, dtype=torch.int32, device=dev)
            self._parts, self._loss = torch.empty(ops.slateq_head_partials(B), **f), torch.empty(1, **f)
            self._cat = {}  # rows -> assembled [rows, S + D] critic input
            self._ws_key = key

    @staticmethod
    def _docs(docs):
        """(features [B, C, D] fp32, mask [B, C] bool, value [B, C] fp32), contiguous"""
        assert docs is not None
        mask = docs.mask if docs.mask.dtype == torch.bool else docs.mask != 0
        return SlateQTrainer._f32c(docs.float_features), mask.contiguous(), SlateQTrainer._f32c(docs.value)

    def _norm_mask(self, b, mask, next_mask):
        m = getattr(self.next_slate_value_norm_method, "value", self.next_slate_value_norm_method)
        if m == NextSlateValueNormMethod.NORM_BY_NEXT_SLATE_SIZE.value:
            return next_mask
        if m == NextSlateValueNormMethod.NORM_BY_CURRENT_SLATE_SIZE.value:
            return mask
        raise NotImplementedError(
            f"The next_slate_value_norm_method {self.next_slate_value_norm_method} has not been implemented")

    def _q_forward(self, b):
        assert isinstance(b, rlt.SlateQInput), f"learning input is a {type(b)}"
        state, next_state = b.state.float_features, b.next_state.float_features
        L.require_cuda(state, "training_batch.state")
        maxq = bool(self.rl_parameters.maxq_learning)
        if maxq:
            assert self.slate_opt_parameters is not None
            method = self.slate_opt_parameters.method
            if getattr(method, "value", method) != rlp.SlateOptMethod.TOP_K.value:
                raise NotImplementedError("SlateQ with optimization method other than TOP_K is not implemented.")
        feats, mask, value = self._docs(b.state.candidate_docs)
        nfeats, nmask, nvalue = self._docs(b.next_state.candidate_docs)
        single = bool(self.single_selection)
        norm_mask = None if single else self._norm_mask(b, mask, nmask)
        action = b.action if b.action.is_contiguous() else b.action.contiguous()
        (B, S), (C, D), K, dev = state.shape, feats.shape[1:], action.shape[1], state.device
        reward, reward_mask = self._f32c(b.reward), b.reward_mask.contiguous()
        assert reward.shape == (B, K) and reward_mask.shape == (B, K) and reward_mask.dtype == torch.bool
        not_terminal = self._f32c(b.not_terminal).reshape(-1)
        self._engine(B, C, K, S, D, dev)
        e, t = self._e, self._t
        e.stack.stage_weights(need_transposed=True)
        t.stage_weights(need_transposed=False)
        if maxq:
            assert 0 < self.slate_size <= C
            assert self.slate_size == K, f"the next slate has {self.slate_size} items, the logged one {K}"
            self._critic_rows(t, next_state, nfeats.view(B * C, D), self._q_all, M=C)
            ops.slate_topk(self._q_all, nvalue, nmask, single, self._next_idx, self._qn)
            ops.slate_gather(nfeats, nmask, nvalue, self._next_idx, None, self._wn, not_terminal=not_terminal)
        else:  # SARSA
            next_action = b.next_action if b.next_action.is_contiguous() else b.next_action.contiguous()
            assert next_action.shape == (B, K)
            ops.slate_gather(nfeats, nmask, nvalue, next_action, self._next_panel, self._wn, not_terminal=not_terminal)
            self._critic_rows(t, next_state, self._next_panel, self._qn, M=K)
        # Get Q-value of action taken
        ops.slate_gather(feats, mask, value, action, self._panel, self._w, count_mask=reward_mask if single else None,
                         count_out=self._n if single else None)
        self._x_t = self._critic_rows(e.stack, state, self._panel, self._qv, M=K, save=True)
        # Adjust the discount factor by the time_diff if the discount_time_scale is provided (:211-214)
        time_diff = None
        if self.discount_time_scale and b.time_diff is not None:
            time_diff = self._f32c(b.time_diff).reshape(-1)
        ops.slateq_head(self._qv, self._qn, self._wn, reward, reward_mask, not_terminal, self.gamma, time_diff,
                        self.discount_time_scale, single, norm_mask, self.slate_size, self._n if single else None, self._y,
                        self._dq, self._parts, self._nq)
        ops.reduce_sum(self._parts, self._parts.numel(), 1.0, self._loss)
        return B, K, reward_mask

    def _backward(self, grad_out=None):
        self._e.backward(self._dq.view(-1, 1), self._x_t, grad_out)

    # ---- reference surface ---------------------------------------------------------------------------
    def train_step_gen(self, training_batch: rlt.SlateQInput, batch_idx: int):
        B, K, reward_mask = self._q_forward(training_batch)
        yield self._e.loss(self._backward, self._loss)
        q_values = self._qv.detach().view(B, K).cpu()
        if self.single_selection:
            all_action_scores = q_values[reward_mask.cpu()]  # (the reporter is fed on the host: a data-dependent shape)
        else:
            all_action_scores = q_values.sum(dim=1, keepdim=True)
        # Logging at the end to schedule all the cuda operations first
        self.reporter.log(td_loss=self._loss.reshape(()).detach().cpu(), model_values_on_logged_actions=all_action_scores)
        # Use the soft update rule to update the target networks
        yield self.soft_update_result()

    # ---- fused native step ---------------------------------------------------------------------------
    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("SlateQTrainer has no data-parallel path: the single-selection loss is a mean over the "
                                  "GLOBAL number of observed rewards, which the ranks would have to agree on")

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch):
        """the q segment and the soft update with no autograd graph / generator / host sync (the number of observed
        rewards stays on the device)"""
        q_opt, soft = self.native_optimizers()
        self._q_forward(training_batch)
        self._native_segment(self._e, self._backward, q_opt)
        soft.step()
        self.all_batches_processed += 1
        return dict(td_loss=self._loss)
