from .base_trainer import BaseCBTrainerWithEval  # noqa: F401
from .deep_represent_linucb_trainer import DeepRepresentLinUCBTrainer  # noqa: F401
from .disjoint_linucb_trainer import DisjointLinUCBTrainer  # noqa: F401
from .linucb_trainer import LinUCBTrainer  # noqa: F401
from .utils import add_chosen_arm_features, get_model_actions  # noqa: F401
