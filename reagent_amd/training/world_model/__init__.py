from .compress_model_trainer import CompressModelTrainer  # noqa: F401
from .mdnrnn_trainer import MDNRNNTrainer  # noqa: F401
from .seq2reward_trainer import Seq2RewardTrainer  # noqa: F401
