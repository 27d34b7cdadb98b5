"""PolicyEvaluator (reagent/evaluation/cb/policy_evaluator.py:16-167): the replay estimator of Li et al.
(https://arxiv.org/pdf/1003.0146.pdf, Algorithm 3).  The per-batch sums are rg_cb_eval_ingest's (BaseOfflineEval); the
aggregation runs once per epoch or model update and stays in torch on one-element tensors."""
import logging

from .base_evaluator import BaseOfflineEval, refuse_world

logger = logging.getLogger(__name__)

EPSILON = 1e-9


class PolicyEvaluator(BaseOfflineEval):
    """Rows where the frozen model picks the logged arm are replayed, the others get importance weight 0; the running sums
    give the average reward of the policy as it learns.  Without arm_presence the size metrics carry the reference's
    factor `batch` (avg_size_accepted = B * A): see BaseOfflineEval."""

    def _aggregate_across_instances(self) -> None:
        """policy_evaluator.py:70-153 in one process: the local sums join the totals, the window's averages are formed from
        them, the local sums return to zero"""
        refuse_world()
        sum_weight_accepted = self.sum_weight_accepted_local.clone()
        sum_importance_weight_accepted = self.sum_importance_weight_accepted_local.clone()
        sum_weight_all_data = self.sum_weight_all_data_local.clone()
        sum_weight_rejected = sum_weight_all_data - sum_weight_accepted
        sum_reward_weighted_accepted = self.sum_reward_weighted_accepted_local.clone()
        sum_reward_importance_weighted_accepted = self.sum_reward_importance_weighted_accepted_local.clone()
        sum_reward_weighted_all_data = self.sum_reward_weighted_all_data_local.clone()
        sum_reward_weighted_rejected = sum_reward_weighted_all_data - sum_reward_weighted_accepted
        sum_size_weighted_accepted = self.sum_size_weighted_accepted_local.clone()
        sum_size_weighted_all_data = self.sum_size_weighted_all_data_local.clone()
        sum_size_weighted_rejected = sum_size_weighted_all_data - sum_size_weighted_accepted

        self.sum_reward_weighted_accepted += sum_reward_weighted_accepted
        self.sum_reward_importance_weighted_accepted += sum_reward_importance_weighted_accepted
        self.sum_weight_accepted += sum_weight_accepted
        self.sum_importance_weight_accepted += sum_importance_weight_accepted
        self.sum_weight_all_data += sum_weight_all_data

        self.frac_accepted = sum_weight_accepted / sum_weight_all_data
        self.avg_reward_accepted = sum_reward_weighted_accepted / sum_weight_accepted
        self.avg_reward_rejected = sum_reward_weighted_rejected / sum_weight_rejected
        self.avg_reward_all_data = sum_reward_weighted_all_data / sum_weight_all_data
        self.accepted_rejected_reward_ratio = self.avg_reward_accepted / self.avg_reward_rejected
        self.avg_size_accepted = sum_size_weighted_accepted / sum_weight_accepted
        self.avg_size_rejected = sum_size_weighted_rejected / sum_weight_rejected

        self.sum_reward_importance_weighted_accepted_local.zero_()
        self.sum_reward_weighted_accepted_local.zero_()
        self.sum_reward_weighted_all_data_local.zero_()
        self.sum_weight_accepted_local.zero_()
        self.sum_importance_weight_accepted_local.zero_()
        self.sum_weight_all_data_local.zero_()
        self.sum_size_weighted_accepted_local.zero_()
        self.sum_size_weighted_all_data_local.zero_()

    def get_avg_reward(self) -> float:
        local = self.sum_importance_weight_accepted_local.item()
        assert local == 0.0, (
            f"Non-zero local weight {local} in the evaluator. _aggregate_across_instances() Should have beed called to "
            "aggregate across all instances and zero-out the local values.")
        return (self.sum_reward_importance_weighted_accepted / (self.sum_importance_weight_accepted + EPSILON)).item()
