from .bandit_reward_network_trainer import BanditRewardNetTrainer

__all__ = [
    "BanditRewardNetTrainer",
]
