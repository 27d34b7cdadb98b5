"""reagent/training/cb/utils.py: the chosen arm's features and the model's actions."""
from dataclasses import replace
from typing import List, Optional, Union

import torch

from ... import ops
from ...core.types import CBInput


def refuse_disjoint(batch) -> None:
    if isinstance(batch, list):
        raise NotImplementedError("a List[CBInput] (one batch per arm: the disjoint models, DisjointLinUCB) is not "
                                  "implemented; LinUCBTrainer takes one CBInput with [batch, arms, dim] features")


def add_chosen_arm_features(batch: Union[CBInput, List[CBInput]]) -> CBInput:
    """the batch with features_of_chosen_arm [B, d] = context_arm_features[b, action[b]] (and chosen_arm_id from `arms`),
    utils.py:15-70.  LinUCBTrainer.training_step does NOT go through this: its kernel reads the chosen rows in place."""
    refuse_disjoint(batch)
    if not isinstance(batch, CBInput):
        raise ValueError(f"Unexpected input type {type(batch)} for _add_chosen_arm_features")
    assert batch.context_arm_features.ndim == 3
    assert batch.action is not None
    d = batch.context_arm_features.shape[2]
    index = batch.action.unsqueeze(-1).expand(-1, 1, d)
    batch = replace(batch, features_of_chosen_arm=torch.gather(batch.context_arm_features, 1, index).squeeze(1))
    if batch.arms is not None:
        batch = replace(batch, chosen_arm_id=torch.gather(batch.arms, 1, batch.action))
    return batch


def get_model_actions(scores: torch.Tensor, mask: Optional[torch.Tensor] = None, randomize_ties: bool = False) -> torch.Tensor:
    """[B, 1] int64: each row's arg-max of scores [B, arms] over the arms `mask` marks present, the lowest index among
    equals (utils.py:113-139 with randomize_ties = False).  Non-finite scores follow the reference too: the first present
    NaN wins; an absent arm counts as -inf, so a row with no arm present, or whose present arms are all -inf, gives arm 0.
    It is rg_linucb_score's arg-max: the scores pass as a one-feature model with coefficient 1 and ucb_alpha 0, whose ucb
    is the score itself, bit for bit."""
    if randomize_ties:
        raise NotImplementedError("get_model_actions(randomize_ties=True) (argmax_random_tie_breaks) is not implemented")
    assert scores.ndim == 2
    B, arms = scores.shape
    dev = scores.device
    x = scores.detach().float().contiguous().reshape(-1, 1)
    N = B * arms
    one = torch.ones(1, dtype=torch.float32, device=dev)
    out = torch.empty(3, N, dtype=torch.float32, device=dev)
    nan = torch.empty(ops.linucb_score_partials(N) + 1, dtype=torch.int32, device=dev)
    best = torch.empty(B, dtype=torch.int64, device=dev)
    if mask is not None:
        assert mask.shape == scores.shape
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
    ops.linucb_score(x, one, one.reshape(1, 1), one, 0.0, out[0], out[1], out[2], nan[1:], nan[:1], arms=arms,
                     arm_presence=mask, best_arm=best)
    return best.reshape(-1, 1)
