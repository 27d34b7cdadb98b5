"""reagent/evaluation/cpe.py: the result containers of counterfactual policy evaluation and the bootstrapped standard
error of a mean, drawn and summed on the device (rg_cpe_bootstrap) instead of 1 000 ``np.random.choice`` calls."""
import logging
import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .. import ops

logger = logging.getLogger(__name__)


class CpeEstimate(NamedTuple):
    raw: float
    normalized: float
    raw_std_error: float
    normalized_std_error: float


class CpeEstimateSet(NamedTuple):
    direct_method: Optional[CpeEstimate] = None
    inverse_propensity: Optional[CpeEstimate] = None
    doubly_robust: Optional[CpeEstimate] = None

    sequential_doubly_robust: Optional[CpeEstimate] = None
    weighted_doubly_robust: Optional[CpeEstimate] = None
    magic: Optional[CpeEstimate] = None

    switch: Optional[CpeEstimate] = None
    switch_dr: Optional[CpeEstimate] = None

    def check_estimates_exist(self):
        assert self.direct_method is not None
        assert self.inverse_propensity is not None
        assert self.doubly_robust is not None
        assert self.sequential_doubly_robust is not None
        assert self.weighted_doubly_robust is not None
        assert self.magic is not None

    def log(self):
        self.check_estimates_exist()
        for title, e in (
            ("Reward Inverse Propensity Score", self.inverse_propensity),
            ("Reward Direct Method", self.direct_method),
            ("Reward Doubly Robust P.E.", self.doubly_robust),
            ("Value Weighted Doubly Robust P.E.", self.weighted_doubly_robust),
            ("Value Sequential Doubly Robust P.E.", self.sequential_doubly_robust),
            ("Value Magic Doubly Robust P.E.", self.magic),
        ):
            logger.info("%s : normalized %.3f +/- %.3f raw %.3f +/- %.3f", title, e.normalized, e.normalized_std_error, e.raw,
                        e.raw_std_error)

    def log_to_tensorboard(self, metric_name: str) -> None:
        raise NotImplementedError("CpeEstimateSet.log_to_tensorboard is not built: there is no SummaryWriterContext here; "
                                  "read the estimates from the CpeDetails the reporter receives")

    def fill_empty_with_zero(self):
        retval = self
        for name, value in self._asdict().items():
            if value is None:
                retval = retval._replace(
                    **{name: CpeEstimate(raw=0.0, normalized=0.0, raw_std_error=0.0, normalized_std_error=0.0)}
                )
        return retval


class CpeDetails:
    def __init__(self):
        self.reward_estimates: CpeEstimateSet = CpeEstimateSet()
        self.metric_estimates: Dict[str, CpeEstimateSet] = {}
        self.q_value_means: Optional[Dict[str, float]] = None
        self.q_value_stds: Optional[Dict[str, float]] = None
        self.action_distribution: Optional[Dict[str, float]] = None

    def log(self):
        logger.info("Reward Estimates:")
        logger.info("-----------------")
        self.reward_estimates.log()
        logger.info("-----------------")
        for metric in self.metric_estimates.keys():
            logger.info(metric + " Estimates:")
            logger.info("-----------------")
            self.metric_estimates[metric].log()
            logger.info("-----------------")

    def log_to_tensorboard(self) -> None:
        self.reward_estimates.log_to_tensorboard("Reward")
        for metric_name, estimate_set in self.metric_estimates.items():
            estimate_set.log_to_tensorboard(metric_name)


def _draw_seed(seed: Optional[int]) -> int:
    """seed=None takes ONE draw from torch's default generator, so torch.manual_seed makes a run repeatable"""
    if seed is not None:
        return int(seed)
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def bootstrapped_std_errors_of_means(columns: torch.Tensor, sample_percent=0.25, num_samples=1000, seed=None) -> torch.Tensor:
    """bootstrapped_std_error_of_mean of each of the C <= 4 rows of `columns` [C, n] (fp32, on the device) from ONE stream
    of resampled indices, in one rg_cpe_bootstrap call -> [C] float64 on the device."""
    n = columns.shape[1]
    sample_size = int(sample_percent * n)
    _means, std = ops.cpe_bootstrap(columns, sample_size, num_samples, _draw_seed(seed))
    return std


def bootstrapped_std_error_of_mean(data, sample_percent=0.25, num_samples=1000, seed=None):
    """
    Compute bootstrapped standard error of mean of input data.

    :param data: Input data (1D torch tensor or numpy array).
    :param sample_percent: Size of sample to use to calculate bootstrap statistic.
    :param num_samples: Number of times to sample.
    :param seed: the resampler's 64-bit seed (see rg_cpe_bootstrap for the draw recipe); None takes one draw from
        torch's default generator.  A tensor is resampled where it lives; a numpy array is moved to the current device.
    """
    if not isinstance(data, torch.Tensor):
        data = torch.as_tensor(np.asarray(data), dtype=torch.float32)
        if torch.cuda.is_available():
            data = data.cuda()
    data = data.reshape(1, -1)
    data = data if data.dtype == torch.float32 else data.float()
    if data.shape[1] == 0:
        return math.nan
    std = bootstrapped_std_errors_of_means(data.contiguous(), sample_percent, num_samples, seed)
    return float(std[0])
