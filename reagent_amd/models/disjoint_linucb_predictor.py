"""DisjointLinearRegressionUCB (reagent/models/disjoint_linucb_predictor.py:34-174): the disjoint LinUCB scorer, one ridge
regression per arm.  Constructor, buffer names, shapes, dtypes and initial values are the reference's, so a ``state_dict``
moves either way; ``cur_num_obs`` is, as there, a plain int64 tensor outside the ``state_dict`` (here it follows
``.to(device)``: the training kernel counts into it).

The scores come from one launch (``rg_dlinucb_score``): the means ``x . coefs[a]``, ``sqrt(x^T inv_A[a] x)`` for every arm
with the products held in MFMA accumulators, the bound and, for ``forward_with_actions``, the masked arg-max.  As in the
reference there is no coefficient-validity check in ``forward``, no division by a total weight and no NaN check.

``_estimate_coefs`` runs once per epoch, off the step path: the batched pseudo-inverse and the einsum are torch's, on a host
copy of the buffers in the reference's fp32 operation order, uploaded afterwards.
"""
import logging
from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from .base import ModelBase
from .linear_regression import _world_size

logger = logging.getLogger(__name__)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def batch_quadratic_form_multi_arms(x: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """out[r, a] = x[r]^T A[a] x[r] for x [B, d] and A [arms, d, d] (disjoint_linucb_predictor.py:17-31): the square of
    rg_dlinucb_score's sigma with zero coefficients (one fp32 multiply on top of the kernel's sum)"""
    assert x.dim() == 2 and A.dim() == 3 and A.shape[1] == A.shape[2] == x.shape[1]
    x, A = _f32c(x), _f32c(A)
    B, arms = x.shape[0], A.shape[0]
    out = torch.empty(2, B, arms, dtype=torch.float32, device=x.device)
    ops.dlinucb_score(x, torch.zeros(arms, x.shape[1], dtype=torch.float32, device=x.device), A, 1.0, out[0], sigma=out[1])
    return out[1] * out[1]


class DisjointLinearRegressionUCB(ModelBase):
    """Args:
        num_arms: number of arms, each with a regression of its own
        input_dim: feature dimension d (1 <= d <= 512, the kernels' limit)
        l2_reg_lambda: weight of the L2 regularisation
        ucb_alpha: coefficient of the standard deviation in the bound; 0 predicts the means alone
        gamma: per-epoch discount of A and b
    Output of forward: [batch, num_arms] scores.
    """

    def __init__(self, num_arms: int, input_dim: int, l2_reg_lambda: float = 1.0, ucb_alpha: float = 1.0,
                 gamma: float = 1.0):
        super().__init__()
        if not 1 <= input_dim <= L.LINUCB_MAX_DIM:
            raise NotImplementedError(f"DisjointLinearRegressionUCB: input_dim = {input_dim} is outside the LinUCB kernels' "
                                      f"range 1 .. {L.LINUCB_MAX_DIM}")
        self.num_arms = num_arms
        self.input_dim = input_dim
        self.ucb_alpha = ucb_alpha
        self.cur_num_obs = torch.zeros(self.num_arms, dtype=torch.int64)
        self.gamma = gamma
        assert self.gamma <= 1.0 and self.gamma > 0.0
        self.l2_reg_lambda = l2_reg_lambda
        arms, d = num_arms, input_dim
        self.register_buffer("A", torch.zeros(arms, d, d))
        self.register_buffer("cur_A", torch.zeros(arms, d, d))
        self.register_buffer("b", torch.zeros(arms, d))
        self.register_buffer("cur_b", torch.zeros(arms, d))
        self.register_buffer("coefs", torch.zeros(arms, d))
        self.register_buffer("inv_A", torch.eye(d).repeat(arms, 1, 1))
        self.register_buffer("coefs_valid_for_A", -torch.ones(arms, d, d))
        self.dummy_param = nn.parameter.Parameter(torch.zeros(1))

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        moved = fn(self.cur_num_obs)  # (a plain attribute: .to(device) / .cuda() / .cpu() take it along, its dtype stays)
        self.cur_num_obs = moved if moved.dtype == torch.int64 else self.cur_num_obs.to(moved.device)
        return out

    def input_prototype(self) -> torch.Tensor:
        return torch.randn(1, self.input_dim)

    def _estimate_coefs(self):
        """disjoint_linucb_predictor.py:107-147 on a host copy: fold the epoch's sums into the all-data ones, invert
        A + l2_reg_lambda * I per arm (pinv, batched), coefs[a] = inv_A[a] b[a], coefs_valid_for_A = gamma * A, and the
        epoch's buffers back to zero"""
        if _world_size() > 1:
            raise NotImplementedError("DisjointLinearRegressionUCB: summing the epoch's buffers over a process group "
                                      "(world > 1) is not implemented")
        A = self.A.cpu() + self.cur_A.cpu()
        b = self.b.cpu() + self.cur_b.cpu()
        m = A + self.l2_reg_lambda * torch.eye(self.input_dim)
        inv_A = torch.linalg.pinv(m).contiguous()
        assert inv_A.size()[0] == b.size()[0]
        coefs = torch.einsum("jkl,jl->jk", inv_A, b)
        self.A.copy_(A)
        self.b.copy_(b)
        self.cur_A.zero_()
        self.cur_b.zero_()
        self.inv_A.copy_(inv_A)
        self.coefs.copy_(coefs)
        self.coefs_valid_for_A.copy_(self.gamma * A)
        logger.info(f"current round num of observations for {self.num_arms} arms are {self.cur_num_obs}")
        self.cur_num_obs.zero_()

    def _score(self, inp: torch.Tensor, ucb_alpha: Optional[float], arm_presence: Optional[torch.Tensor], want_actions: bool):
        if ucb_alpha is None:
            ucb_alpha = self.ucb_alpha
        if inp.dim() != 2 or inp.shape[-1] != self.input_dim:
            raise ValueError(f"DisjointLinearRegressionUCB: the input has shape {tuple(inp.shape)}, the model takes "
                             f"[batch, {self.input_dim}]")
        x = _f32c(inp)
        B, dev = x.shape[0], x.device
        ucb = torch.empty(B, self.num_arms, dtype=torch.float32, device=dev)
        best, mask = None, None
        if want_actions:
            best = torch.empty(B, dtype=torch.int64, device=dev)
            if arm_presence is not None:
                assert arm_presence.shape == ucb.shape
                mask = (arm_presence if arm_presence.dtype in (torch.bool, torch.uint8) else arm_presence != 0).contiguous()
        ops.dlinucb_score(x, self.coefs, self.inv_A, float(ucb_alpha), ucb, arm_presence=mask, best_arm=best)
        return ucb, best

    def forward(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> torch.Tensor:
        """[batch, num_arms]: the mean of every arm, plus ucb_alpha times its standard deviation (ucb_alpha None: the
        model's own; 0: the means alone, the matrices are not read)"""
        return self._score(inp, ucb_alpha, None, False)[0]

    def forward_with_actions(self, inp: torch.Tensor, arm_presence: Optional[torch.Tensor] = None,
                             ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """{"ucb": forward(inp), "model_actions": [batch, 1] = get_model_actions(ucb, arm_presence)} from one launch"""
        ucb, best = self._score(inp, ucb_alpha, arm_presence, True)
        return {"ucb": ucb, "model_actions": best.reshape(-1, 1)}
