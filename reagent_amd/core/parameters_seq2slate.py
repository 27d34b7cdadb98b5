"""The Seq2Slate parameter classes with the names, fields and defaults of reagent/core/parameters_seq2slate.py (LearningMethod
:12-23, IPSClampMethod :32-38, IPSClamp :41-44) and of Seq2SlateParameters (reagent/core/parameters.py:204-209).  Objects of the
reference's own classes are accepted wherever these are (duck typing: rg_frechet_head's clamp code is looked up by the enum's
value)."""
from dataclasses import dataclass
from enum import Enum
from typing import Optional

from .. import _lib as L


class LearningMethod(Enum):
    TEACHER_FORCING = "teacher_forcing"
    REINFORCEMENT_LEARNING = "reinforcement_learning"
    PAIRWISE_ATTENTION = "pairwise_attention"
    SIMULATION = "simulation"

    @property
    def expect_slate_wise_reward(self) -> bool:
        return self in (LearningMethod.REINFORCEMENT_LEARNING, LearningMethod.SIMULATION)


class IPSClampMethod(Enum):
    UNIVERSAL = "universal"    # the importance weight is held within [0, clamp_max]
    AGGRESSIVE = "aggressive"  # an importance weight above clamp_max becomes 0 (Bottou et al., JMLR 2013)


@dataclass(frozen=True)
class IPSClamp:
    clamp_method: IPSClampMethod
    clamp_max: float


@dataclass(frozen=True)
class Seq2SlateParameters:
    on_policy: bool = True
    learning_method: LearningMethod = LearningMethod.REINFORCEMENT_LEARNING
    ips_clamp: Optional[IPSClamp] = None
    simulation: Optional[object] = None  # the reference's SimulationParameters: accepted only as None

    def __post_init__(self):
        if self.simulation is not None:
            raise NotImplementedError("Seq2SlateParameters: simulation is not supported (None: there is no simulation trainer here)")


_CLAMP_CODES = {IPSClampMethod.UNIVERSAL.value: L.IPS_CLAMP_UNIVERSAL, IPSClampMethod.AGGRESSIVE.value: L.IPS_CLAMP_AGGRESSIVE}


def ips_clamp_code(ips_clamp: Optional[IPSClamp]):
    """-> (rg_frechet_head's clamp_method, clamp_max) of an IPSClamp, this package's or the reference's (None: no clamp)"""
    if not ips_clamp:
        return L.IPS_CLAMP_NONE, 0.0
    return _CLAMP_CODES[ips_clamp.clamp_method.value], float(ips_clamp.clamp_max)
