"""LinearRegressionUCB (reagent/models/linear_regression.py:92-251, on reagent/models/cb_base_model.py:15-45): the LinUCB
scorer.  Constructor, buffer names and initial values are the reference's, so a ``state_dict`` moves either way.

The scores come from one entry point (``rg_linucb_score``): the mean ``x . coefs``, ``sqrt(x^T inv_avg_A x / sum_weight)``
and the upper confidence bound, without the ``[N, d]`` product ``x @ inv_avg_A`` ever being written.

Whether the coefficients are still valid is a HOST flag here.  The reference compares two device tensors on every
``forward`` (``(coefs_valid_for_avg_A == avg_A).all()`` and ``abs(cur_avg_A).max().item() > 0``, :202-204), a
synchronisation each; this class sets ``_coefs_dirty`` where those comparisons can change their answer -- a training step
(``mark_dirty``, called by LinUCBTrainer), ``load_state_dict`` (which evaluates the reference's two comparisons once on
the loaded buffers) -- and clears it in ``_calculate_coefs``.  A caller that writes the buffers by hand calls
``mark_dirty()``.

``_calculate_coefs`` runs once per epoch, off the step path: the d x d inverse is ``torch.linalg.inv`` with the
reference's ``pinv`` fallback on a host copy of the buffers, in the reference's fp32 operation order, uploaded afterwards.
"""
import logging
from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops

logger = logging.getLogger(__name__)


def matrix_inv_fallback_pinv(matrix: torch.Tensor) -> torch.Tensor:
    """torch.linalg.inv, and the pseudo-inverse where it raises (linear_regression.py:17-38)"""
    try:
        return torch.linalg.inv(matrix).contiguous()
    except RuntimeError as e:
        logger.warning("Exception raised during matrix inversion, falling back to pseudo-inverse: %s", e)
        hermitian = torch.allclose(matrix, matrix.T, atol=1e-4, rtol=1e-4)
        return torch.linalg.pinv(matrix, hermitian=hermitian).contiguous()


def batch_quadratic_form(x: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """out[...] = x[...]^T A x[...] for x [B, d] or [B, arms, d] (linear_regression.py:41-51) in torch operations: the
    statement `rg_linucb_score` is tested against, not the path `forward` takes"""
    return (torch.matmul(x, A) * x).sum(-1)


def _world_size() -> int:
    import torch.distributed as dist

    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _refresh_dirty_after_load(module, incompatible_keys) -> None:
    module.refresh_dirty()


class UCBBaseModel(nn.Module):
    def __init__(self, input_dim: int):
        super().__init__()
        self.input_dim = input_dim

    def input_prototype(self) -> torch.Tensor:
        return torch.randn(1, self.input_dim)

    def forward_inference(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        return self.forward(inp, ucb_alpha=ucb_alpha)


class LinearRegressionUCB(UCBBaseModel):
    """A ridge regression kept as weighted AVERAGES of x x^T and label * x, "all data" and "current epoch" apart.

    Args:
        input_dim: feature dimension d (1 <= d <= 512, the kernels' limit)
        l2_reg_lambda: weight of the L2 regularisation
        ucb_alpha: coefficient of the standard deviation in the bound; 0 predicts the mean alone
        gamma: per-epoch discount of the total weight
    Outputs: {"pred_label", "pred_sigma", "ucb"}, each of the input's shape without its last dimension.
    """

    def __init__(self, input_dim: int, *, l2_reg_lambda: float = 1.0, ucb_alpha: float = 1.0, gamma: float = 1.0) -> None:
        super().__init__(input_dim=input_dim)
        if not 1 <= input_dim <= L.LINUCB_MAX_DIM:
            raise NotImplementedError(f"LinearRegressionUCB: input_dim = {input_dim} is outside the LinUCB kernels' range "
                                      f"1 .. {L.LINUCB_MAX_DIM}")
        self.ucb_alpha = ucb_alpha
        self.l2_reg_lambda = l2_reg_lambda
        self.gamma = gamma
        assert self.gamma <= 1.0 and self.gamma > 0.0
        d = self.input_dim
        self.register_buffer("avg_A", torch.zeros(d, d))
        self.register_buffer("avg_b", torch.zeros(d))
        self.register_buffer("cur_avg_A", torch.zeros(d, d))
        self.register_buffer("cur_avg_b", torch.zeros(d))
        self.register_buffer("_coefs", torch.zeros(d))
        self.register_buffer("inv_avg_A", torch.zeros(d, d))
        self.register_buffer("coefs_valid_for_avg_A", -torch.ones((d, d)))
        self.register_buffer("num_obs", torch.zeros(1, dtype=torch.int64))
        self.register_buffer("cur_num_obs", torch.zeros(1, dtype=torch.int64))
        self.register_buffer("sum_weight", 1e-5 * torch.ones(1, dtype=torch.float))
        self.register_buffer("cur_sum_weight", 1e-5 * torch.ones(1, dtype=torch.float))
        self.dummy_param = nn.parameter.Parameter(torch.zeros(1))
        self._coefs_dirty = True  # (coefs_valid_for_avg_A = -1 != avg_A = 0: the reference's first forward calculates too)
        # after ANY load that reaches this module -- its own load_state_dict or that of a module that holds it (a trainer, an
        # evaluator's frozen copy): nested loads go through _load_from_state_dict and never call a load_state_dict override
        self.register_load_state_dict_post_hook(_refresh_dirty_after_load)

    def mark_dirty(self) -> None:
        """the buffers moved: the next `coefs` / `forward` recalculates"""
        self._coefs_dirty = True

    def refresh_dirty(self) -> None:
        """the reference's two comparisons (:202-204) on the buffers as they are, once per load"""
        self._coefs_dirty = bool(not (self.coefs_valid_for_avg_A == self.avg_A).all()
                                 or torch.abs(self.cur_avg_A).max().item() > 0)

    def _calculate_coefs(self) -> None:
        """linear_regression.py:157-199 on a host copy: fold the epoch's averages into the all-data ones (reduce_avg, :54-89,
        one process), invert avg_A + l2_reg_lambda * I / sum_weight, coefs = inv_avg_A @ avg_b, reset the epoch's buffers to
        exactly zero."""
        if _world_size() > 1:
            raise NotImplementedError("LinearRegressionUCB: reducing the epoch's averages over a process group (world > 1) "
                                      "is not implemented")
        avg_A, avg_b, sum_weight = self.avg_A.cpu(), self.avg_b.cpu(), self.sum_weight.cpu()
        cur_A, cur_b, cur_w = self.cur_avg_A.cpu(), self.cur_avg_b.cpu(), self.cur_sum_weight.cpu()
        total_weight = cur_w.clone() + sum_weight
        avg_A = (avg_A * sum_weight + cur_A * cur_w) / total_weight
        avg_b = (avg_b * sum_weight + cur_b * cur_w) / total_weight
        sum_weight = sum_weight + cur_w
        A_extended = avg_A + self.l2_reg_lambda * torch.eye(self.input_dim) / sum_weight
        inv_avg_A = matrix_inv_fallback_pinv(matrix=A_extended)
        coefs = torch.matmul(inv_avg_A, avg_b)
        self.num_obs += self.cur_num_obs
        self.avg_A.copy_(avg_A)
        self.avg_b.copy_(avg_b)
        self.sum_weight.copy_(sum_weight)
        self.inv_avg_A.copy_(inv_avg_A)
        self._coefs.copy_(coefs)
        self.coefs_valid_for_avg_A.copy_(avg_A)
        self.cur_avg_A.zero_()
        self.cur_avg_b.zero_()
        self.cur_num_obs.zero_()
        self.cur_sum_weight.zero_()
        self._coefs_dirty = False

    def calculate_coefs_if_necessary(self) -> torch.Tensor:
        if self._coefs_dirty:
            self._calculate_coefs()
        return self._coefs

    @property
    def coefs(self) -> torch.Tensor:
        return self.calculate_coefs_if_necessary()

    def _score(self, inp: torch.Tensor, ucb_alpha: Optional[float], arm_presence: Optional[torch.Tensor], want_actions: bool):
        if ucb_alpha is None:
            ucb_alpha = self.ucb_alpha
        if inp.shape[-1] != self.input_dim:
            raise ValueError(f"LinearRegressionUCB: the input's last dimension is {inp.shape[-1]}, the model's {self.input_dim}")
        lead = inp.shape[:-1]
        x = inp.reshape(-1, self.input_dim)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        N, dev = x.shape[0], x.device
        out = torch.empty(3, N, dtype=torch.float32, device=dev)
        nan_partials = torch.empty(ops.linucb_score_partials(N) + 1, dtype=torch.int32, device=dev)
        arms, best, mask = 0, None, None
        if want_actions:
            assert inp.dim() == 3, "model actions need [batch, arms, dim] features"
            arms = inp.shape[1]
            best = torch.empty(inp.shape[0], dtype=torch.int64, device=dev)
            if arm_presence is not None:
                mask = arm_presence.reshape(-1)
                mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
        ops.linucb_score(x, self._coefs, self.inv_avg_A, self.sum_weight, float(ucb_alpha), out[0], out[1], out[2],
                         nan_partials[1:], nan_partials[:1], arms=arms, arm_presence=mask, best_arm=best)
        if int(nan_partials[0].item()) != 0:  # (the reference's torch.any(torch.isnan(pred_sigma)), :229-231)
            raise Exception("pred_sigma has nan values")
        res = {"pred_label": out[0].reshape(lead), "pred_sigma": out[1].reshape(lead), "ucb": out[2].reshape(lead)}
        if want_actions:
            res["model_actions"] = best.reshape(-1, 1)
        return res

    def _forward_no_coefs_check(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        return self._score(inp, ucb_alpha, None, False)

    def forward(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """the mean, its standard deviation and the bound mean + ucb_alpha * deviation (ucb_alpha None: the model's own);
        raises where a deviation is NaN, as the reference does"""
        self.calculate_coefs_if_necessary()
        return self._forward_no_coefs_check(inp, ucb_alpha)

    def forward_inference(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        return self._forward_no_coefs_check(inp, ucb_alpha)

    def forward_with_actions(self, inp: torch.Tensor, arm_presence: Optional[torch.Tensor] = None,
                             ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """`forward` on [batch, arms, dim] features plus "model_actions" [batch, 1]: get_model_actions(ucb, arm_presence) from
        the same call"""
        self.calculate_coefs_if_necessary()
        return self._score(inp, ucb_alpha, arm_presence, True)
