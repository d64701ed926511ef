from .distillation import Distillation
from .kdmkb_model import KdmkbModel
from .top_k_sampling import FastTopKSampling, TopKSampling, TopKSamplingTransE
from .uniform_sampling import UniformSampling

__all__ = ["Distillation", "FastTopKSampling", "KdmkbModel", "TopKSampling", "TopKSamplingTransE", "UniformSampling"]
