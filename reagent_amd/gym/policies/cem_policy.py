"""CEMPolicy (reagent/model_managers/model_based/cross_entropy_method.py:35-53): acting with a CEMPlannerNetwork.  It lives
here because this package has no model_managers."""
from typing import Optional

import torch

from ...core import types as rlt
from ...models.cem_planner import CEMPlannerNetwork
from .policy import Policy


class CEMPolicy(Policy):
    def __init__(self, cem_planner_network: CEMPlannerNetwork, discrete_action: bool):
        self.cem_planner_network = cem_planner_network
        self.discrete_action = discrete_action

    def act(self, obs: rlt.FeatureData, possible_actions_mask: Optional[torch.Tensor] = None) -> rlt.ActorOutput:
        """possible_actions_mask is not read (the reference's TODO)"""
        greedy = self.cem_planner_network(obs)
        if self.discrete_action:
            _, onehot = greedy
            return rlt.ActorOutput(action=onehot.unsqueeze(0), log_prob=torch.tensor(0.0))
        return rlt.ActorOutput(action=greedy.unsqueeze(0), log_prob=torch.tensor(0.0))
