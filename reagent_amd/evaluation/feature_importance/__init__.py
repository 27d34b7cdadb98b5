from .feature_importance_base import FeatureImportanceBase
from .feature_importance_perturbation import FeatureImportancePerturbation, create_default_perturb_fn

__all__ = ["FeatureImportanceBase", "FeatureImportancePerturbation", "create_default_perturb_fn"]
