"""reagent/evaluation/cb/utils.py: the importance weights of the replay estimator, on rg_cb_eval_ingest."""
from dataclasses import replace
from typing import Optional, Tuple

import torch

from ... import ops
from ...core.types import CBInput

N_SUMS = 8  # rg_cb_eval_ingest's running sums (the ninth, sum_weight_since_update, is the first one again)


def _f32(t: Optional[torch.Tensor], B: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    assert t.numel() == B, f"batch.{what} has {t.numel()} entries, the batch {B} rows"
    t = t.detach()
    return (t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()).reshape(-1)


def _i64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return (t if t.dtype == torch.int64 and t.is_contiguous() else t.long().contiguous()).reshape(-1)


def ingest(batch: CBInput, model_actions: torch.Tensor, max_importance_weight: Optional[float], sums, since_update,
           partials: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rg_cb_eval_ingest on a batch -> (importance_weight, effective_weight), each [B, 1]; the batch's eight sums are added
    to `sums` and its total weight to `since_update` (one-element fp32 tensors on the batch's device)"""
    logged_actions = batch.action
    assert logged_actions is not None
    assert logged_actions.shape == model_actions.shape, (logged_actions.shape, model_actions.shape)
    B, arms = len(batch), batch.context_arm_features.shape[1]
    dev = logged_actions.device
    presence = batch.arm_presence
    if presence is not None:
        assert presence.shape == (B, arms), (presence.shape, (B, arms))
        presence = (presence if presence.dtype in (torch.bool, torch.uint8) else presence != 0).contiguous()
    reward = _f32(batch.reward, B, "reward")
    if reward is None:  # (add_importance_weights does not need one; the sums it would feed are thrown away)
        reward = torch.zeros(B, dtype=torch.float32, device=dev)
    out = torch.empty(2, B, 1, dtype=torch.float32, device=dev)
    if partials is None:
        partials = ops.cb_eval_partials(B, dev)
    ops.cb_eval_ingest(_i64(logged_actions), _i64(model_actions), reward, _f32(batch.weight, B, "weight"),
                       _f32(batch.action_log_probability, B, "action_log_probability"), presence, arms,
                       max_importance_weight, out[0], out[1], partials, sums, since_update)
    return out[0], out[1]


def add_importance_weights(batch: CBInput, model_actions: torch.Tensor,
                           max_importance_weight: Optional[float] = None) -> CBInput:
    """the batch with importance_weight [B, 1] (evaluation/cb/utils.py:9-47): zero where the logged and the model's action
    differ, else 1 / probability of the logged action (exp(action_log_probability), or 1 / slate size where no probability
    was logged), clipped at max_importance_weight where one is given.  It runs on the evaluator's kernel."""
    scratch = torch.zeros(N_SUMS + 1, dtype=torch.float32, device=batch.action.device)
    iw, _ = ingest(batch, model_actions, max_importance_weight, [scratch[k:k + 1] for k in range(N_SUMS)], scratch[N_SUMS:])
    return replace(batch, importance_weight=iw)
