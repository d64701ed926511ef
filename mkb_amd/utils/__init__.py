from .bar import Bar, BarRange
from .io import read_csv, read_json
from .predict import FetchToPredict, make_prediction
from .predict_relations import predict_top_k_relations, relation_scores
from .predict_top_k import candidate_bits, predict_top_k, topk_block
from .stats import Mean, RollingMean
from .top_k import TopK
from .true_keys import true_keys

__all__ = ["Bar", "BarRange", "FetchToPredict", "Mean", "RollingMean", "TopK", "candidate_bits", "make_prediction", "predict_top_k", "predict_top_k_relations", "read_csv", "read_json", "relation_scores", "topk_block", "true_keys"]
