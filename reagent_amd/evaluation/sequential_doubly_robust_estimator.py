"""reagent/evaluation/sequential_doubly_robust_estimator.py (https://arxiv.org/pdf/1511.03722.pdf) on a device-resident,
sorted EvaluationDataPage: rg_cpe_dr_rows for the row quantities, rg_cpe_sdr for the per-episode recurrence (one lane per
episode instead of a Python loop over every row), rg_cpe_bootstrap for the standard error."""
import logging

import torch

from .. import ops
from .cpe import bootstrapped_std_errors_of_means, CpeEstimate
from .doubly_robust_estimator import _rows, dr_row_quantities
from .evaluation_data_page import EvaluationDataPage, episode_offsets

logger = logging.getLogger(__name__)


class SequentialDoublyRobustEstimator:
    def __init__(self, gamma):
        self.gamma = gamma

    def episode_values(self, edp: EvaluationDataPage):
        """-> (doubly_robust [E], episode_value [E]) fp32 on the page's device"""
        assert edp.mdp_id is not None
        rows = dr_row_quantities(edp)
        return ops.cpe_sdr(rows["state_value"], rows["importance_weight"], _rows(edp.logged_rewards), rows["q_logged"],
                           episode_offsets(edp.mdp_id), self.gamma)

    def estimate(self, edp: EvaluationDataPage) -> CpeEstimate:
        num_examples = edp.logged_rewards.shape[0]
        if num_examples == 0:
            raise RuntimeError(
                f"No valid doubly robusts data is generated.\n"
                f"gamma={self.gamma};\n"
                f"Did you specify wrong metric names?"
            )
        doubly_robusts, episode_values = self.episode_values(edp)
        std = bootstrapped_std_errors_of_means(doubly_robusts.reshape(1, -1))
        # the reference averages the per-episode floats in double (np.mean of a float64 array)
        dr_score = float(doubly_robusts.double().mean())
        logged_policy_score = float(episode_values.double().mean())
        dr_score_std_error = float(std[0])
        if logged_policy_score < 1e-6:
            logger.warning(
                "Can't normalize SDR-CPE because of small"
                f" or negative logged_policy_score ({logged_policy_score})."
            )
            return CpeEstimate(raw=dr_score, normalized=0.0, raw_std_error=dr_score_std_error, normalized_std_error=0.0)
        return CpeEstimate(
            raw=dr_score,
            normalized=dr_score / logged_policy_score,
            raw_std_error=dr_score_std_error,
            normalized_std_error=dr_score_std_error / logged_policy_score,
        )
