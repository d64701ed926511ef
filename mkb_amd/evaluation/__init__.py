from .classif import (accuracy, classification_report, find_threshold, find_thresholds_per_relation, threshold_accuracy,
                      threshold_search)
from .evaluation import Evaluation

__all__ = ["Evaluation", "accuracy", "classification_report", "find_threshold", "find_thresholds_per_relation",
           "threshold_accuracy", "threshold_search"]
