"""SoftmaxActionSampler (reagent/gym/policies/samplers/discrete_sampler.py:14-83): a categorical distribution over
scores / temperature, with a temperature that `update()` decays down to a floor."""
import torch
import torch.nn.functional as F

from ....core import types as rlt
from ...types import Sampler


class SoftmaxActionSampler(Sampler):
    def __init__(self, temperature: float = 1.0, temperature_decay: float = 1.0, minimum_temperature: float = 0.1) -> None:
        assert temperature > 0, f"Invalid non-positive temperature {temperature}."
        self.temperature = temperature
        self.temperature_decay = temperature_decay
        self.minimum_temperature = minimum_temperature
        assert temperature_decay <= 1.0, f"Invalid temperature_decay>1: {temperature_decay}."
        assert minimum_temperature <= temperature, (
            f"minimum_temperature ({minimum_temperature}) exceeds initial temperature ({temperature})")

    def _get_distribution(self, scores: torch.Tensor) -> torch.distributions.Categorical:
        return torch.distributions.Categorical(logits=scores / self.temperature)

    @torch.no_grad()
    def sample_action(self, scores: torch.Tensor) -> rlt.ActorOutput:
        assert scores.dim() == 2, f"scores shape is {scores.shape}, not (batch_size, num_actions)"
        batch_size, num_actions = scores.shape
        m = self._get_distribution(scores)
        raw_action = m.sample()
        assert raw_action.shape == (batch_size,), f"{raw_action.shape} != ({batch_size}, )"
        action = F.one_hot(raw_action, num_actions)
        assert action.ndim == 2
        log_prob = m.log_prob(raw_action)
        assert log_prob.ndim == 1
        return rlt.ActorOutput(action=action, log_prob=log_prob)

    def log_prob(self, scores: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        assert len(scores.shape) == 2, f"{scores.shape}"
        assert scores.shape == action.shape, f"{scores.shape} != {action.shape}"
        m = self._get_distribution(scores)
        return m.log_prob(action.argmax(dim=1))

    def entropy(self, scores: torch.Tensor) -> torch.Tensor:
        """the policy's entropy, averaged over the batch"""
        assert len(scores.shape) == 2, f"{scores.shape}"
        m = self._get_distribution(scores)
        return m.entropy().mean()

    def update(self) -> None:
        self.temperature *= self.temperature_decay
        self.temperature = max(self.temperature, self.minimum_temperature)
