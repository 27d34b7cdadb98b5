"""reagent/evaluation: what of the reference's evaluation package exists here -- offline evaluation of contextual bandits
(cb/) and counterfactual policy evaluation of the discrete DQN trainers (evaluation_data_page, cpe, doubly_robust_estimator,
sequential_doubly_robust_estimator, evaluator)."""
