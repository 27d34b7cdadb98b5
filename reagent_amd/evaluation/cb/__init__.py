"""reagent/evaluation/cb: offline policy evaluation inside the contextual-bandit training loop."""
from .base_evaluator import BaseOfflineEval  # noqa: F401
from .policy_evaluator import PolicyEvaluator  # noqa: F401
from .utils import add_importance_weights  # noqa: F401
