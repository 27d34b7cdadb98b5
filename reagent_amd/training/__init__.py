from .dqn_trainer import BCQConfig, DQNTrainer  # noqa: F401
from .qrdqn_trainer import QRDQNTrainer  # noqa: F401
from .reagent_lightning_module import ReAgentLightningModule  # noqa: F401
from .sac_trainer import CRRWeightFn, SACTrainer  # noqa: F401
from .td3_trainer import TD3Trainer  # noqa: F401
from .c51_trainer import C51Trainer  # noqa: F401
from .discrete_crr_trainer import DiscreteCRRTrainer  # noqa: F401
from .parametric_dqn_trainer import ParametricDQNTrainer  # noqa: F401
from .slate_q_trainer import NextSlateValueNormMethod, SlateQTrainer  # noqa: F401
from .reinforce_trainer import ReinforceTrainer  # noqa: F401
from .ppo_trainer import PPOTrainer  # noqa: F401
from .cem_trainer import CEMTrainer  # noqa: F401
from .reward_network_trainer import LossFunction, RewardNetTrainer  # noqa: F401
from .cfeval import BanditRewardNetTrainer  # noqa: F401
from .cb import DeepRepresentLinUCBTrainer, DisjointLinUCBTrainer, LinUCBTrainer  # noqa: F401
from .ranking import Seq2SlateTrainer  # noqa: F401
from .parameters import (  # noqa: F401
    C51TrainerParameters,
    CRRTrainerParameters,
    DQNTrainerParameters,
    ParametricDQNTrainerParameters,
    PPOTrainerParameters,
    QRDQNTrainerParameters,
    ReinforceTrainerParameters,
    RewardNetworkTrainerParameters,
    SACTrainerParameters,
    Seq2SlateTrainerParameters,
    SlateQTrainerParameters,
    TD3TrainerParameters,
)
