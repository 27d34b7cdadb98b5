"""The common part of the feature-importance methods (module path and names of
reagent/evaluation/feature_importance/feature_importance_base.py)."""
from dataclasses import dataclass
from typing import List

import pandas as pd
import torch


@dataclass
class FeatureImportanceBase:
    """What every method holds: the model under study, and the ids its importances are labelled with (id i names raw input
    column i).  A method returns a table with the columns feature_id and feature_importance."""

    model: torch.nn.Module
    sorted_feature_ids: List[int]

    def compute_feature_importance(self) -> pd.DataFrame:
        raise NotImplementedError(f"{type(self).__name__} does not compute a feature importance")
