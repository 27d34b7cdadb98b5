"""DeepRepresentLinearRegressionUCB (reagent/models/deep_represent_linucb.py:16-210): an MLP maps an arm's raw features to
a low-dimensional representation, LinUCB runs on [1, representation].  Constructor, attribute and ``state_dict`` names are
the reference's (``deep_represent_layers.dnn.*``, ``linear_layer.weight`` and LinearRegressionUCB's buffers), so a
``state_dict`` moves either way.

What runs where:
  MLP        : this package's FullyConnectedNetwork (batch norm, layer norm and residual layers on GeneralFCStack)
  head       : rg_drlinucb_head -- the ones column, the mean through ``linear_layer`` (nn_e2e) or ``_coefs``, the output
               activation; in a training step also the loss and its gradients (training/cb/deep_represent_linucb_trainer.py)
  sigma, ucb : rg_linucb_score on mlp_out_with_ones, unchanged; a non-linear output activation on pred_label and ucb is
               one elementwise launch (rg_drlinucb_activate)
  ridge solve: on the device-resident buffers, no synchronisation: rg_linucb_solve, ONE launch, for d = sizes[-1] + 1
               <= 128; rg_linucb_solve_blocked, a blocked Cholesky route in d / 32 + 3 launches on a workspace the model
               keeps (a non-persistent buffer: it follows .to(device) and stays out of the state_dict), for 128 < d <= 512.
               The reference recalculates the coefficients on every training step (cur_avg_A is non-zero after every
               update_params, :148-151): the parent's host path (six downloads, LAPACK, seven uploads) stays only as the
               fallback behind the kernels' status flag.

The status flag (a pivot of the elimination was not positive or not finite) is read at the trainer's epoch end and in
``forward`` outside a training step; where it is set the inverse is recomputed once through the parent's inv / pinv host
path from the already folded avg_A, and the flag cleared.

``forward`` does not raise on a NaN sigma (the reference's does not, :154-159); ``forward_inference`` does, through the
parent (:198-200).  The TRAINING STEP does not compute pred_sigma / ucb at all: the reference computes them in its forward
and the trainer discards them (deep_represent_linucb_trainer.py:72-78).
"""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from .fully_connected_network import FullyConnectedNetwork
from .linear_regression import LinearRegressionUCB, _world_size, matrix_inv_fallback_pinv


class DeepRepresentLinearRegressionUCB(LinearRegressionUCB):
    """Args: input_dim -- the MLP's input width; sizes, activations -- its layers (sizes[-1] + 1 is the LinUCB dimension);
    output_activation -- applied to pred_label and ucb; nn_e2e -- the mean comes from ``linear_layer`` (trained by the
    optimizer) instead of the LinUCB coefficients, which still give sigma.
    Outputs: {"pred_label", "pred_sigma", "ucb"} of the input's shape without its last dimension, "mlp_out_with_ones"
    [..., sizes[-1] + 1]."""

    def __init__(
        self,
        input_dim: int,
        sizes: List[int],
        activations: List[str],
        *,
        output_activation: str = "linear",
        l2_reg_lambda: float = 1.0,
        ucb_alpha: float = 1.0,
        gamma: float = 1.0,
        use_batch_norm: bool = True,
        dropout_ratio: float = 0.0,
        normalize_output: bool = True,
        use_layer_norm: bool = False,
        use_skip_connections: bool = True,
        mlp_layers: Optional[nn.Module] = None,
        nn_e2e: bool = True,
    ):
        super().__init__(input_dim=sizes[-1] + 1, l2_reg_lambda=l2_reg_lambda, ucb_alpha=ucb_alpha, gamma=gamma)
        assert input_dim > 0, "input_dim must be > 0, got {}".format(input_dim)
        assert sizes[-1] > 0, "Last layer size must be > 0, got {}".format(sizes[-1])
        assert len(sizes) == len(activations), (
            "The numbers of sizes and activations must match; got {} vs {}".format(len(sizes), len(activations)))
        if output_activation not in L.ACT:
            raise NotImplementedError(f"DeepRepresentLinearRegressionUCB: output_activation {output_activation!r} is none of "
                                      f"{sorted(L.ACT)}")
        self.nn_e2e = nn_e2e
        self.raw_input_dim = input_dim
        self.linear_layer = nn.Linear(in_features=sizes[-1] + 1, out_features=1, bias=False)
        self.output_activation_name = output_activation
        if mlp_layers is None:
            self.deep_represent_layers = FullyConnectedNetwork(
                [self.raw_input_dim] + sizes, activations, use_batch_norm=use_batch_norm, dropout_ratio=dropout_ratio,
                normalize_output=normalize_output, use_layer_norm=use_layer_norm, use_skip_connections=use_skip_connections)
        else:
            if not isinstance(mlp_layers, FullyConnectedNetwork):
                raise NotImplementedError(f"DeepRepresentLinearRegressionUCB: mlp_layers must be a reagent_amd "
                                          f"FullyConnectedNetwork (got {type(mlp_layers).__name__}): the training step runs "
                                          "its FC stack on the HIP kernels")
            dims = mlp_layers.stack().dims
            assert dims[0] == input_dim and dims[-1] == sizes[-1], "mlp_layers does not map input_dim to sizes[-1]"
            self.deep_represent_layers = mlp_layers
        self.register_buffer("_solve_status", torch.zeros(1, dtype=torch.int32), persistent=False)
        # rg_linucb_solve_blocked's workspace (d > 128): sized by the library at the first solve, then kept
        self.register_buffer("_solve_workspace", torch.empty(0, dtype=torch.uint8), persistent=False)

    @property
    def _act(self) -> int:
        return L.ACT[self.output_activation_name]

    def input_prototype(self) -> torch.Tensor:
        return torch.randn(1, self.raw_input_dim)

    # ---- the ridge solve -----------------------------------------------------------------------------------------------
    def _calculate_coefs(self) -> None:
        """linear_regression.py:157-199 on the buffers where they lie: rg_linucb_solve (d <= 128) or
        rg_linucb_solve_blocked (128 < d <= 512).  No synchronisation: the status flag is looked at later
        (`check_solve_status`)."""
        if _world_size() > 1:
            raise NotImplementedError("LinearRegressionUCB: reducing the epoch's averages over a process group (world > 1) "
                                      "is not implemented")
        state = (self.avg_A, self.avg_b, self.sum_weight, self.num_obs, self.cur_avg_A, self.cur_avg_b, self.cur_sum_weight,
                 self.cur_num_obs, self.inv_avg_A, self._coefs, self.coefs_valid_for_avg_A, self._solve_status)
        if self.input_dim <= L.LINUCB_SOLVE_MAX_DIM:
            ops.linucb_solve(self.l2_reg_lambda, *state)
        else:
            if self._solve_workspace.numel() == 0:
                self._solve_workspace = ops.linucb_solve_blocked_workspace(self.input_dim, self.avg_A.device)
            ops.linucb_solve_blocked(self.l2_reg_lambda, *state, self._solve_workspace)
        self._coefs_dirty = False
        self._solve_unchecked = True

    _solve_unchecked = False

    def check_solve_status(self) -> None:
        """one read of the device flag since the last solve; where it is set: inv / pinv of A_extended on the host from the
        folded avg_A (the fold itself is exact whatever the pivots were), coefficients from it, flag cleared"""
        if not self._solve_unchecked:
            return
        self._solve_unchecked = False
        if int(self._solve_status.item()) == 0:
            return
        avg_A, sum_weight = self.avg_A.cpu(), self.sum_weight.cpu()
        A_extended = avg_A + self.l2_reg_lambda * torch.eye(self.input_dim) / sum_weight
        inv_avg_A = matrix_inv_fallback_pinv(matrix=A_extended)
        self.inv_avg_A.copy_(inv_avg_A)
        self._coefs.copy_(torch.matmul(inv_avg_A, self.avg_b.cpu()))
        self._solve_status.zero_()

    def calculate_coefs_if_necessary(self) -> torch.Tensor:
        """the public path (`coefs`, `forward`): recalculate where the buffers moved, then look at the solve's flag.  The
        trainer's step calls `_calculate_coefs` itself and leaves the flag for its epoch end"""
        out = super().calculate_coefs_if_necessary()
        self.check_solve_status()
        return out

    # ---- forward -------------------------------------------------------------------------------------------------------
    def _represent(self, inp: torch.Tensor):
        """-> (mlp_out [N, h], the leading shape): [B, A, F] inputs are B * A rows (the rows SlateBatchNorm1d normalises
        over, fully_connected_network.py:48-64)"""
        if inp.shape[-1] != self.raw_input_dim:
            raise ValueError(f"DeepRepresentLinearRegressionUCB: the input's last dimension is {inp.shape[-1]}, the MLP's "
                             f"input_dim is {self.raw_input_dim}")
        lead = inp.shape[:-1]
        x = inp.reshape(-1, self.raw_input_dim)
        with torch.no_grad():
            return self.deep_represent_layers._forward_no_grad(x), lead

    def _mean_vector(self) -> torch.Tensor:
        """what the mean is a dot product with: linear_layer.weight[0] (nn_e2e) or the LinUCB coefficients"""
        return self.linear_layer.weight.detach().reshape(-1) if self.nn_e2e else self._coefs

    def _score_deep(self, inp, v, ucb_alpha, arm_presence, want_actions: bool, inference: bool):
        """MLP, head in its forward-only mode (z = [1, mlp_out]), rg_linucb_score on z with `v` in the coefficients' place
        (pred_label = z . v, pred_sigma, ucb = pred_label + ucb_alpha * pred_sigma), the output activation"""
        if ucb_alpha is None:
            ucb_alpha = self.ucb_alpha
        mlp_out, lead = self._represent(inp)
        N, h = mlp_out.shape
        dev = mlp_out.device
        z = torch.empty(N, h + 1, dtype=torch.float32, device=dev)
        out = torch.empty(4, N, dtype=torch.float32, device=dev)  # the head's lin; pred_label, pred_sigma, ucb
        ops.drlinucb_head(mlp_out, v, L.ACT["linear"], z, out[0], out[1])
        nan_partials = torch.empty(ops.linucb_score_partials(N) + 1, dtype=torch.int32, device=dev)
        arms, best, mask = 0, None, None
        if want_actions:
            assert inp.dim() == 3, "model actions need [batch, arms, dim] features"
            arms = inp.shape[1]
            best = torch.empty(inp.shape[0], dtype=torch.int64, device=dev)
            if arm_presence is not None:
                mask = arm_presence.reshape(-1)
                mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
        # forward divides by clamp(sum_weight, min=1e-5) (:157: a one-element op, off the step path), the parent's
        # forward_inference by sum_weight itself
        sum_weight = self.sum_weight if inference else torch.clamp(self.sum_weight, min=0.00001)
        ops.linucb_score(z, v, self.inv_avg_A, sum_weight, float(ucb_alpha), out[1], out[2], out[3], nan_partials[1:],
                         nan_partials[:1], arms=arms, arm_presence=mask, best_arm=best)
        if inference and int(nan_partials[0].item()) != 0:  # (LinearRegressionUCB._forward_no_coefs_check, :229-231)
            raise Exception("pred_sigma has nan values")
        if self._act != L.ACT["linear"]:
            ops.drlinucb_activate(out[1], out[3], self._act)
        res = {"pred_label": out[1].reshape(lead), "pred_sigma": out[2].reshape(lead), "ucb": out[3].reshape(lead),
               "mlp_out_with_ones": z.reshape(*lead, h + 1)}
        if want_actions:
            res["model_actions"] = best.reshape(-1, 1)
        return res

    def forward(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """deep_represent_linucb.py:122-172: recalculates the coefficients where the buffers moved; no NaN check"""
        self.calculate_coefs_if_necessary()
        return self._score_deep(inp, self._mean_vector(), ucb_alpha, None, False, inference=False)

    def forward_inference(self, inp: torch.Tensor, ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """:174-210: the mean from the LinUCB coefficients whatever nn_e2e says, no recalculation, raises on a NaN sigma"""
        return self._score_deep(inp, self._coefs, ucb_alpha, None, False, inference=True)

    def forward_with_actions(self, inp: torch.Tensor, arm_presence: Optional[torch.Tensor] = None,
                             ucb_alpha: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """`forward` on [batch, arms, F] features plus "model_actions" [batch, 1] = get_model_actions(ucb, arm_presence): from
        the scoring call itself under a linear output activation; otherwise the arg-max runs on the ACTIVATED ucb (an
        activation that saturates makes ties the bound did not have)"""
        self.calculate_coefs_if_necessary()
        v = self._mean_vector()
        if self._act == L.ACT["linear"]:
            return self._score_deep(inp, v, ucb_alpha, arm_presence, True, inference=False)
        from ..training.cb.utils import get_model_actions

        res = self._score_deep(inp, v, ucb_alpha, None, False, inference=False)
        res["model_actions"] = get_model_actions(res["ucb"], arm_presence)
        return res
