"""reagent/evaluation/evaluator.py: Evaluator for the discrete DQN trainers, on a device-resident EvaluationDataPage.

NOT the reference's result in one place: weighted sequential DR and MAGIC are OPT-IN.  ``score_cpe`` fills
``weighted_doubly_robust`` and ``magic`` (weighted_sequential_doubly_robust_estimator.py: rg_cpe_wsdr plus a numpy quadratic
program) only where ``SCORE_WEIGHTED_ESTIMATORS`` is true, on the class or on an instance
(``trainer.evaluator.SCORE_WEIGHTED_ESTIMATORS = True``); it is False by default, and then both stay None, nothing of
that estimator runs and nothing is drawn from any generator.  ``evaluate_post_training`` returns every CpeEstimateSet after
``fill_empty_with_zero()``, so fields left None read 0.0 and ``CpeEstimateSet.log`` / ``check_estimates_exist`` work on what
is returned.  A page of fewer than four episodes has no MAGIC estimate: score_cpe warns and leaves ``magic`` None.
The observer notification of the reference (``@observable``) is not built: the trainer hands the CpeDetails to its reporter.
"""
import logging
from typing import Dict, List, Optional

import torch

from .cpe import CpeDetails, CpeEstimateSet
from .doubly_robust_estimator import DoublyRobustEstimator
from .evaluation_data_page import EvaluationDataPage
from .sequential_doubly_robust_estimator import SequentialDoublyRobustEstimator
from .weighted_sequential_doubly_robust_estimator import WeightedSequentialDoublyRobustEstimator

logger = logging.getLogger(__name__)


def get_tensor(x, dtype=None):
    """
    Input:
        - x: list or a sequence
        - dtype: target data type of the elements in tensor [optional]
                 It will be inferred automatically if not provided.
    Output:
        Tensor given a list or a sequence.
        If the input is None, it returns None
        If the input is a tensor it returns the tensor.
        If type is provides the output Tensor will have that type
    """
    if x is None:
        return None

    if not isinstance(x, torch.Tensor):
        x = torch.tensor(x)

    if dtype is not None:
        x = x.type(dtype)

    return x


def get_metrics_to_score(metric_reward_values: Optional[Dict[str, float]]) -> List[str]:
    if metric_reward_values is None:
        return []
    return sorted([*metric_reward_values.keys()])


class Evaluator:
    NUM_J_STEPS_FOR_MAGIC_ESTIMATOR = 25
    SCORE_WEIGHTED_ESTIMATORS = False  # settable on an instance: score_cpe then fills weighted_doubly_robust and magic

    def __init__(self, action_names, gamma, model, metrics_to_score=None) -> None:
        self.action_names = action_names
        self.metrics_to_score = metrics_to_score

        self.gamma = gamma
        self.model = model

        self.doubly_robust_estimator = DoublyRobustEstimator()
        self.sequential_doubly_robust_estimator = SequentialDoublyRobustEstimator(gamma)
        self.weighted_sequential_doubly_robust_estimator = WeightedSequentialDoublyRobustEstimator(gamma)

    def evaluate_post_training(self, edp: EvaluationDataPage) -> CpeDetails:
        """evaluator.py:73-117.  Every estimate set is returned after fill_empty_with_zero(): weighted_doubly_robust and
        magic read 0.0 where score_cpe leaves them None (SCORE_WEIGHTED_ESTIMATORS unset)."""
        cpe_details = CpeDetails()

        cpe_details.reward_estimates = self.score_cpe("Reward", edp).fill_empty_with_zero()

        if self.metrics_to_score is not None and edp.logged_metrics is not None and self.action_names is not None:
            for i, metric in enumerate(self.metrics_to_score):
                logger.info("--------- Running CPE on metric: {} ---------".format(metric))

                metric_reward_edp = edp.set_metric_as_reward(i, len(self.action_names))

                cpe_details.metric_estimates[metric] = self.score_cpe(metric, metric_reward_edp).fill_empty_with_zero()

        if self.action_names is not None:
            # per-action numbers by torch reductions on the device page, one read-back each
            if edp.optimal_q_values is not None:
                value_means = edp.optimal_q_values.mean(dim=0).tolist()
                cpe_details.q_value_means = {action: float(value_means[i]) for i, action in enumerate(self.action_names)}
                value_stds = edp.optimal_q_values.std(dim=0).tolist()  # unbiased, as Tensor.std
                cpe_details.q_value_stds = {action: float(value_stds[i]) for i, action in enumerate(self.action_names)}
            if edp.eval_action_idxs is not None:
                n = edp.eval_action_idxs.shape[0]
                counts = torch.bincount(edp.eval_action_idxs.reshape(-1), minlength=len(self.action_names)).tolist()
                cpe_details.action_distribution = {
                    action: float(counts[i]) / n for i, action in enumerate(self.action_names)
                }
        return cpe_details

    def score_cpe(self, metric_name, edp: EvaluationDataPage):
        """evaluator.py:119-143; the weighted sequential DR and MAGIC estimates only where SCORE_WEIGHTED_ESTIMATORS is set,
        else both stay None."""
        direct_method, inverse_propensity, doubly_robust = self.doubly_robust_estimator.estimate(edp)
        sequential_doubly_robust = self.sequential_doubly_robust_estimator.estimate(edp)
        weighted_doubly_robust = magic = None
        if self.SCORE_WEIGHTED_ESTIMATORS:
            weighted_doubly_robust = self.weighted_sequential_doubly_robust_estimator.estimate(
                edp, num_j_steps=1, whether_self_normalize_importance_weights=True
            )
            try:
                magic = self.weighted_sequential_doubly_robust_estimator.estimate(
                    edp,
                    num_j_steps=Evaluator.NUM_J_STEPS_FOR_MAGIC_ESTIMATOR,
                    whether_self_normalize_importance_weights=True,
                )
            except ValueError as e:
                if "at least 4 episodes" not in str(e):
                    raise
                logger.warning("No MAGIC estimate for %s: %s", metric_name, e)
        return CpeEstimateSet(
            direct_method=direct_method,
            inverse_propensity=inverse_propensity,
            doubly_robust=doubly_robust,
            sequential_doubly_robust=sequential_doubly_robust,
            weighted_doubly_robust=weighted_doubly_robust,
            magic=magic,
        )

    def get_target_distribution_error(self, actions, target_distribution, actual_distribution):
        """Calculate MSE between actual and target action distribution."""
        if not target_distribution:
            return None
        error = 0
        for i, action in enumerate(actions):
            error += (target_distribution[i] - actual_distribution[action]) ** 2
        return error / len(actions)

    @staticmethod
    def huberLoss(label, output):
        if abs(label - output) > 1:
            return abs(label - output) - 0.5
        else:
            return 0.5 * (label - output) * (label - output)
