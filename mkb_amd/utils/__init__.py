from .bar import Bar, BarRange
from .io import read_csv, read_json
from .predict import FetchToPredict, make_prediction
from .predict_top_k import predict_top_k
from .stats import Mean, RollingMean
from .top_k import TopK
from .true_keys import true_keys

__all__ = ["Bar", "BarRange", "FetchToPredict", "Mean", "RollingMean", "TopK", "make_prediction", "predict_top_k", "read_csv", "read_json", "true_keys"]
