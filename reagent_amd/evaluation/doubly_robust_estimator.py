"""reagent/evaluation/doubly_robust_estimator.py: the one-step direct-method, inverse-propensity and doubly-robust
estimates (https://arxiv.org/pdf/1612.01205.pdf) of a device-resident EvaluationDataPage.

``estimate`` is rg_cpe_dr_rows (the row quantities and their five totals: two launches) and one rg_cpe_bootstrap call
that resamples dm, ips and dr together; the five totals and three standard errors are read back once each."""
import logging
from typing import Dict, NamedTuple, Optional, Tuple, Union

import torch

from .. import ops
from .cpe import bootstrapped_std_errors_of_means, CpeEstimate
from .evaluation_data_page import EvaluationDataPage

logger = logging.getLogger(__name__)


DEFAULT_FRAC_TRAIN = 0.4
DEFAULT_FRAC_VALID = 0.1


class DoublyRobustHP(NamedTuple):
    frac_train: float = DEFAULT_FRAC_TRAIN
    frac_valid: float = DEFAULT_FRAC_VALID
    bootstrap_num_samples: int = 1000
    bootstrap_sample_percent: float = 0.25
    xgb_params: Optional[Dict[str, Union[float, int, str]]] = None
    bope_mode: Optional[str] = None
    bope_num_samples: Optional[int] = None


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def _rows(t: torch.Tensor) -> torch.Tensor:
    """a [N, C] fp32 operand whose rows the kernel reads at their pitch (a column slice of a wider matrix stays a view)"""
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


def dr_row_quantities(edp: EvaluationDataPage):
    """rg_cpe_dr_rows on a page: what DoublyRobustEstimator and SequentialDoublyRobustEstimator both start from"""
    return ops.cpe_dr_rows(_f32c(edp.model_propensities), _f32c(edp.action_mask), _rows(edp.model_rewards),
                           _rows(edp.model_values if edp.model_values is not None else edp.model_rewards),
                           _f32c(edp.logged_propensities).reshape(-1), _rows(edp.logged_rewards),
                           _rows(edp.model_rewards_for_logged_action))


class DoublyRobustEstimator:
    """
    For details, visit https://arxiv.org/pdf/1612.01205.pdf
    """

    def estimate(
        self, edp: EvaluationDataPage, hp: Optional[DoublyRobustHP] = None
    ) -> Tuple[CpeEstimate, CpeEstimate, CpeEstimate]:
        hp = hp or DoublyRobustHP()
        for name in ("xgb_params", "bope_mode", "bope_num_samples"):
            if getattr(hp, name) is not None:
                raise NotImplementedError(f"DoublyRobustHP.{name} is not served: the estimated-propensity (xgboost) and "
                                          "BOP-E estimators are not built")
        rows = dr_row_quantities(edp)
        num_examples = edp.logged_rewards.shape[0]
        stds = bootstrapped_std_errors_of_means(rows["dm_ips_dr"], sample_percent=hp.bootstrap_sample_percent,
                                                num_samples=hp.bootstrap_num_samples)
        totals = rows["totals"].cpu().tolist()  # one read-back: sum logged_rewards, dm, mr_logged, ips, dr
        stds = stds.cpu().tolist()
        # The score we would get if we evaluate the logged policy against itself
        logged_policy_score = totals[0] / num_examples
        if logged_policy_score < 1e-6:
            logger.warning("Can't normalize DR-CPE because of small or negative " + "logged_policy_score")
            normalizer = 0.0
        else:
            normalizer = 1.0 / logged_policy_score
        direct_method_score, ips_score, dr_score = (totals[k] / num_examples for k in (1, 3, 4))
        logger.info(f"Normalized Direct method score = {direct_method_score * normalizer}")
        logger.info(f"Normalized IPS score = {ips_score * normalizer}")

        def make(score, std):
            return CpeEstimate(raw=score, normalized=score * normalizer, raw_std_error=std,
                               normalized_std_error=std * normalizer)

        return make(direct_method_score, stds[0]), make(ips_score, stds[1]), make(dr_score, stds[2])
