"""Callers on the candidate side of the hot path (SURVEY.md section 8 f): feature engineering over the candidate arrays the
covisitation lookup leaves on the device."""

from . import evaluate  # noqa: E402,F401
from .blend import blend_predictions, blend_topk, robust_scale  # noqa: E402,F401
from .features import (AID_COLUMNS, SESSION_COLUMNS, aid_feature_table, feature_matrix, session_feature_table,  # noqa: E402,F401
                       to_frames)
from .folds import cross_validate, feature_importance, fold_indices, gather_bins, group_kfold  # noqa: E402,F401
from .gbdt import (BinMapper, Sampling, TrainResult, ap_at_k, bin_matrix, fit_bins, lambdarank_gradients,  # noqa: E402,F401
                   sampling_from_params, train, write_lightgbm_model)
from . import xgb  # noqa: E402,F401
from . import objectives  # noqa: E402,F401
