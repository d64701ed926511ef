from .negative_sampling import NegativeSampling, positive_triples
from .pool_sampling import InBatchNegativeSampling, PoolNegativeSampling, WeightedNegativeSampling, negatives_from_pool

__all__ = ["NegativeSampling", "positive_triples", "PoolNegativeSampling", "WeightedNegativeSampling", "InBatchNegativeSampling",
           "negatives_from_pool"]
