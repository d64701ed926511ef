from .adversarial import Adversarial
from .kl_divergence import KlDivergence
from .kvs_all import KvsAll
from .ns_losses import CrossEntropy, MarginRanking, PairwiseLogistic
from .one_vs_all import OneVsAll
from .relation_prediction import RelationPrediction

__all__ = ["Adversarial", "KlDivergence", "MarginRanking", "PairwiseLogistic", "CrossEntropy", "OneVsAll", "KvsAll", "RelationPrediction"]
