"""Policy (reagent/gym/policies/policy.py:13-39): the scorer's scores handed to the sampler."""
from typing import Any, Optional

import torch

from ...core import types as rlt
from ..types import Sampler, Scorer


class Policy:
    def __init__(self, scorer: Scorer, sampler: Sampler) -> None:
        """scorer: preprocessed input (and an optional possible-actions mask) -> scores; sampler: scores -> action"""
        self.scorer = scorer
        self.sampler = sampler

    def act(self, obs: Any, possible_actions_mask: Optional[torch.Tensor] = None) -> rlt.ActorOutput:
        """the action that goes into the replay buffer (with its log-probability), on the host"""
        scorer_inputs = (obs,)
        if possible_actions_mask is not None:
            scorer_inputs += (possible_actions_mask,)
        scores = self.scorer(*scorer_inputs)
        actor_output = self.sampler.sample_action(scores)
        return actor_output.cpu().detach()
