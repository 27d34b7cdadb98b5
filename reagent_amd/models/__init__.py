from .actor import FullyConnectedActor, GaussianFullyConnectedActor  # noqa: F401
from .base import ModelBase  # noqa: F401
from .critic import FullyConnectedCritic  # noqa: F401
from .dqn import FullyConnectedDQN  # noqa: F401
from .dueling_q_network import DuelingQNetwork  # noqa: F401
from .fully_connected_network import (  # noqa: F401
    FloatFeatureFullyConnected,
    FullyConnectedNetwork,
    get_default_precision,
    set_default_precision,
)
from .categorical_dqn import CategoricalDQN  # noqa: F401
from .linear_regression import LinearRegressionUCB  # noqa: F401
from .deep_represent_linucb import DeepRepresentLinearRegressionUCB  # noqa: F401
from .disjoint_linucb_predictor import DisjointLinearRegressionUCB  # noqa: F401
from .synthetic_reward import (  # noqa: F401
    NGramFullyConnectedNetwork,
    SequenceSyntheticRewardNet,
    SingleStepSyntheticRewardNet,
    SyntheticRewardNet,
)
from .synthetic_reward_transformer import TransformerSyntheticRewardNet  # noqa: F401
from .seq2slate import BaselineNet, Seq2SlateTransformerNet, Seq2SlateTransformerOutput  # noqa: F401
