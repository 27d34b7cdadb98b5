"""What ReinforceTrainer and PPOTrainer share: one policy-gradient pass over PACKED trajectories on the HIP kernels.

  scorer  : one saving forward of the policy's FullyConnectedDQN stack on all N rows            -> scores [N, A]
  baseline: one saving forward of the value net's stack (when there is one)                      -> values [N]
  returns : rg_pg_returns — clamp, reverse discounted scan, whitening / mean subtraction, per trajectory
  head    : rg_pg_head — possible-actions penalty, temperature log-softmax, the logged action's log-probability, ratio,
            REINFORCE's clamp or PPO's clip, entropy bonus, baseline MSE, d loss / d scores and d loss / d values
  losses  : rg_reduce_sum on the head's per-workgroup partials (twice with a value net)
followed by the value net's backward and step, then the policy's.  A single trajectory is the packed batch with
offsets = [0, N].
"""
import inspect

import torch

from .. import _lib as L
from .. import ops
from ..models.dqn import FullyConnectedDQN
from .plumbing import NativeStepMixin


class PolicyGradientMixin(NativeStepMixin):
    """needs: scorer, sampler, value_net, gamma, reward_clip, normalize, subtract_mean, offset_clamp_min"""

    _graph_capture_refusal = ("the policy-gradient steps are not captured into a HIP graph: trajectory lengths, and with them "
                              "every launch's shape, change from step to step; run them eagerly")

    def _check_networks(self):
        if not isinstance(self.scorer, FullyConnectedDQN):
            raise NotImplementedError(
                f"{type(self).__name__}: the policy's scorer must be a FullyConnectedDQN (got {type(self.scorer).__name__}); "
                "other scorers, such as DuelingQNetwork, have no single FC stack for the native step")
        if self.value_net is not None and not hasattr(self.value_net, "fc"):
            raise NotImplementedError(f"{type(self).__name__}: the value net must be a FloatFeatureFullyConnected "
                                      f"(got {type(self.value_net).__name__})")
        self._pg_cap = None

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError(f"{type(self).__name__} has no data-parallel path: the native step folds a MEAN over the "
                                  "ranks into Adam, and the policy-gradient losses are sums over a rank's own trajectories")

    @staticmethod
    def _refuse_graph_input(batch):
        if inspect.getattr_static(batch, "graph", None) is not None:
            raise NotImplementedError("policy-gradient trainers: a `graph` (GNN) input is not supported; the scorer reads "
                                      "training_batch.state")

    # ---- workspace: grow-only flat buffers, viewed at the step's N ---------------------------------------------------
    def _pg_workspace(self, N, A, dev):
        key = (A, dev)
        if self._pg_cap is None or self._pg_cap[0] != key or self._pg_cap[1] < N:
            cap = max(N, 2 * self._pg_cap[1] if self._pg_cap is not None and self._pg_cap[0] == key else N)
            f = dict(dtype=torch.float32, device=dev)
            self._pg_buf = dict(scores=torch.empty(cap * A, **f), dscores=torch.empty(cap * A, **f),
                                **{n: torch.empty(cap, **f) for n in ("returns", "values", "dvalues", "log_prob", "ratio",
                                                                       "advantage")},
                                pp=torch.empty(cap, **f), vp=torch.empty(cap, **f))
            self._pg_cap = (key, cap)
            self._ploss, self._vloss = torch.empty(1, **f), torch.zeros(1, **f)
        b = self._pg_buf
        self._scores, self._dscores = b["scores"][:N * A].view(N, A), b["dscores"][:N * A].view(N, A)
        for n in ("returns", "values", "dvalues", "log_prob", "ratio", "advantage"):
            setattr(self, "_" + n, b[n][:N])
        P = ops.pg_head_partials(N, A)
        self._pp, self._vp = b["pp"][:P], b["vp"][:P]

    def _forward_net(self, e, state, out):
        """one saving forward of a trainable net's stack -> the transposed staged input its backward reads"""
        e.stack.stage_weights(need_transposed=True)
        xc, xt = e.stack.stage_input(state, need_transposed=True)
        e.stack.forward(xc, out, save=True)
        return xt

    def _pg_forward(self, state, action, reward, old_log_prob, mask, offsets, mode, clip, entropy_weight, value_scale,
                    normalize, subtract_mean):
        """both forwards, the returns, the head and the loss sums of N packed rows; offsets: int32 [T + 1] on the device"""
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)
        L.require_cuda(state, "training_batch.state")
        state = self._f32c(state)
        N, dev = state.shape[0], state.device
        A = self.scorer.fc.stack().dims[-1]
        assert action.shape == (N, A), f"action is {tuple(action.shape)}, the scorer has {A} outputs for {N} rows"
        if action.dtype not in (torch.float32, torch.int64):
            action = action.float()
        action = action if action.is_contiguous() else action.contiguous()
        reward = self._f32c(reward)
        assert reward.shape == (N,)
        if old_log_prob is not None:
            old_log_prob = self._f32c(old_log_prob.detach())
            assert old_log_prob.shape == (N,)
        if mask is not None:
            mask = self._f32c(mask)
            assert mask.shape == (N, A)
        self._pg_workspace(N, A, dev)
        self._pe = self._trainable(self.scorer)
        self._p_xt = self._forward_net(self._pe, state, self._scores)
        values = None
        if self.value_net is not None:
            self._ve = self._trainable(self.value_net)
            assert self._ve.stack.dims[-1] == 1, "the value net has one output"
            self._v_xt = self._forward_net(self._ve, state, self._values.view(N, 1))
            values = self._values
        ops.pg_returns(reward, offsets, self.gamma, self.reward_clip, normalize, subtract_mean, self.offset_clamp_min,
                       self._returns)
        ops.pg_head(self._scores, action, self._returns, values, old_log_prob, self.sampler.temperature, mode, clip,
                    entropy_weight, value_scale, self._dscores, self._dvalues if values is not None else None, self._log_prob,
                    self._ratio, self._advantage, self._pp, self._vp if values is not None else None,
                    possible_actions_mask=mask)
        ops.reduce_sum(self._pp, self._pp.numel(), 1.0, self._ploss)
        if values is not None:
            ops.reduce_sum(self._vp, self._vp.numel(), 1.0, self._vloss)
        return N

    @staticmethod
    def _one_trajectory(n, dev):
        return torch.tensor([0, n], dtype=torch.int32, device=dev)

    def _backward_policy(self, grad_out=None):
        self._pe.backward(self._dscores, self._p_xt, grad_out)

    def _backward_value(self, grad_out=None):
        self._ve.backward(self._dvalues.view(-1, 1), self._v_xt, grad_out)
