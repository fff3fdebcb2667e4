"""ctypes binding of ``csrc/libotto_amd.so`` (the C-ABI declared in ``include/*.h``).

The product path has NO CPU fallback: if the HIP library is missing or a symbol is
absent this module raises at first use, and every entry point raises
``OttoError`` with ``otto_last_error()`` on a non-zero return code.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OTTO_AMD_LIB selects another build of the SAME library (the phase-profiling build of tools/perf_covis.py --prof)
LIB_PATH = os.environ.get('OTTO_AMD_LIB') or os.path.join(_HERE, 'csrc', 'libotto_amd.so')

MAX_FILTERS = 4
MAX_TYPE_WEIGHTS = 4
GROUP_TYPE, GROUP_FILTER, GROUP_TIME = 0, 1, 2
STAT_NAMES = ('sessions', 'tail_events', 'pair_slots', 'pairs', 'runs', 'items_s', 'items_m', 'items_l', 'retries',
              'pairs_s', 'pairs_m', 'pairs_l', 'runs_s', 'runs_m', 'runs_l', 'shared_runs', 'row_records')
TIMING_NAMES = ('winscan', 'expand', 'index', 'partition', 'reduce_s', 'reduce_m', 'reduce_l', 'merge')


class OttoError(RuntimeError):
    pass


class CandParams(C.Structure):
    # mirrors otto_cand_params (include/otto_cand.h)
    _fields_ = [
        ('n_aids', C.c_uint32),
        ('k', C.c_int32),
        ('n_matrices', C.c_int32),
        ('d_mat_y', C.c_void_p * 8),
        ('d_mat_n', C.c_void_p * 8),
        ('n_terms', C.c_int32),
        ('term_matrix', C.c_int32 * 8),
        ('term_source', C.c_int32 * 8),
        ('n_common', C.c_int32),
        ('mat_k', C.c_int32 * 8),
    ]


class RecencyParams(C.Structure):
    # mirrors otto_recency_params (include/otto_cand.h)
    _fields_ = [
        ('n_curves', C.c_int32),
        ('start', C.c_double * 4),
        ('stop', C.c_double * 4),
        ('type_coef', C.c_double * 3),
    ]


class RecencyPredParams(C.Structure):
    # mirrors otto_recency_pred_params (include/otto_cand.h)
    _fields_ = [
        ('n_targets', C.c_int32),
        ('start', C.c_double * 3),
        ('stop', C.c_double * 3),
        ('bump', C.c_double * 3),
        ('type_coef', C.c_double * 3),
        ('n_common', C.c_int32),
        ('n_pred', C.c_int32),
        ('min_unique', C.c_int32),
        ('d_cand', C.c_void_p * 3),
        ('d_count', C.c_void_p * 3),
        ('d_n_cand', C.c_void_p * 3),
        ('d_self_count', C.c_void_p * 3),
    ]


class CovisParams(C.Structure):
    # mirrors otto_covis_params (include/otto_covis.h)
    _fields_ = [
        ('window', C.c_int32),
        ('max_gap', C.c_int32),
        ('n_aids', C.c_uint32),
        ('ts_min', C.c_int32),
        ('ts_max', C.c_int32),
        ('want_time', C.c_int32),
        ('n_filters', C.c_int32),
        ('filter_mask', C.c_uint16 * MAX_FILTERS),
        ('n_type_weights', C.c_int32),
        ('type_weight', (C.c_int32 * 3) * MAX_TYPE_WEIGHTS),
    ]


class SgnsTable(C.Structure):
    # mirrors otto_sgns_table (include/otto_sgns.h)
    _fields_ = [
        ('d_cum', C.c_void_p),
        ('d_bucket', C.c_void_p),
        ('n_aids', C.c_int64),
        ('n_buckets', C.c_int64),
        ('total', C.c_uint64),
        ('shift', C.c_int32),
    ]


class SgnsCbowJob(C.Structure):
    # mirrors otto_sgns_cbow_job (include/otto_sgns.h)
    _fields_ = [('d_tok_aid', C.c_void_p), ('d_tok_src', C.c_void_p), ('d_tok_left', C.c_void_p), ('d_pair_off', C.c_void_p),
                ('d_tok_off', C.c_void_p), ('T', C.c_int64), ('S', C.c_int64), ('t0', C.c_int64), ('t1', C.c_int64),
                ('d_In', C.c_void_p), ('d_Out', C.c_void_p), ('d_Syn1', C.c_void_p), ('d_Doc', C.c_void_p),
                ('n_aids', C.c_int64), ('n_inner', C.c_int64), ('d', C.c_int32), ('neg', C.c_int32), ('lr', C.c_float),
                ('arch', C.c_int32), ('variant', C.c_int32), ('mode', C.c_int32), ('seed', C.c_uint64), ('epoch', C.c_uint64),
                ('table', SgnsTable), ('d_path_off', C.c_void_p), ('d_path_node', C.c_void_p), ('d_code', C.c_void_p),
                ('d_loss_sum', C.c_void_p), ('d_neg_out', C.c_void_p), ('d_gin', C.c_void_p), ('d_gout', C.c_void_p),
                ('d_gsyn1', C.c_void_p), ('d_gdoc', C.c_void_p), ('stream', C.c_void_p)]


SGNS_MAX_INFER_PASSES = 64          # OTTO_SGNS_MAX_INFER_PASSES


class SgnsInferJob(C.Structure):
    # mirrors otto_sgns_infer_job (include/otto_sgns.h)
    _fields_ = [('d_tok_aid', C.c_void_p), ('d_tok_off', C.c_void_p), ('T', C.c_int64), ('S', C.c_int64),
                ('d_sess_key', C.c_void_p), ('d_order', C.c_void_p), ('d_In', C.c_void_p), ('d_Out', C.c_void_p),
                ('d_Syn1', C.c_void_p), ('n_aids', C.c_int64), ('n_inner', C.c_int64), ('d', C.c_int32), ('neg', C.c_int32),
                ('ws', C.c_int32), ('arch', C.c_int32), ('variant', C.c_int32), ('passes', C.c_int32),
                ('lr', C.c_float * SGNS_MAX_INFER_PASSES), ('seed', C.c_uint64), ('table', SgnsTable), ('d_path_off', C.c_void_p),
                ('d_path_node', C.c_void_p), ('d_code', C.c_void_p), ('d_Doc', C.c_void_p), ('d_loss', C.c_void_p),
                ('d_neg_out', C.c_void_p), ('d_radius_out', C.c_void_p), ('stream', C.c_void_p)]


class XgbTree(C.Structure):
    # mirrors otto_xgb_tree (include/otto_xgb.h): 16 host arrays, then what the call writes
    _fields_ = [(name, C.c_void_p) for name in (
        'split_feature', 'split_bin', 'threshold', 'decision_type', 'left_child', 'right_child', 'split_gain', 'cover',
        'sum_grad', 'count', 'left_id', 'right_id', 'leaf_value', 'leaf_cover', 'leaf_sum_grad', 'leaf_count')] + [
        ('n_leaves', C.c_int32), ('n_syncs', C.c_int32), ('hist_rows', C.c_int64)]


class PqwColumn(C.Structure):
    # mirrors otto_pqw_column (include/otto_pqwrite.h)
    _fields_ = [('d_data', C.c_void_p), ('n_rows', C.c_int64), ('elem_bytes', C.c_int32), ('kind', C.c_int32),
                ('encoding', C.c_int32), ('reserved', C.c_int32)]


class PqwPage(C.Structure):
    # mirrors otto_pqw_page (include/otto_pqwrite.h); parquet_write.PAGE_DTYPE is its NumPy image
    _fields_ = [('first_row', C.c_int64), ('n_values', C.c_int32), ('column', C.c_int32)]


class PqwJob(C.Structure):
    # mirrors otto_pqw_job (include/otto_pqwrite.h)
    _fields_ = [('columns', C.POINTER(PqwColumn)), ('n_columns', C.c_int64), ('pages', C.POINTER(PqwPage)), ('n_pages', C.c_int64),
                ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class SnappyJob(C.Structure):
    # mirrors otto_snappy_job (include/otto_snappy.h)
    _fields_ = [('d_in', C.c_void_p), ('n_bytes', C.c_int64), ('src_off', C.c_void_p), ('src_len', C.c_void_p), ('n_streams', C.c_int64),
                ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class RowsJob(C.Structure):
    # mirrors otto_rows_job (include/otto_rows.h)
    _fields_ = [('d_aid_x', C.c_void_p), ('d_aid_y', C.c_void_p), ('d_wgt', C.c_void_p), ('n_rows', C.c_int64), ('d_y', C.c_void_p),
                ('d_w', C.c_void_p), ('d_n', C.c_void_p), ('n_aids', C.c_int64), ('k', C.c_int32), ('reserved', C.c_int32),
                ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class PqlistJob(C.Structure):
    # mirrors otto_pqlist_job (include/otto_pqlist.h)
    _fields_ = [('d_bytes', C.c_void_p), ('n_bytes', C.c_int64), ('h_pages', C.c_void_p), ('n_pages', C.c_int64), ('d_off', C.c_void_p),
                ('d_null', C.c_void_p), ('n_rows', C.c_int64), ('value_base', C.c_int64), ('h_page_out', C.c_void_p),
                ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class LabelsJob(C.Structure):
    # mirrors otto_labels_job (include/otto_labels.h)
    _fields_ = [('d_session', C.c_void_p), ('d_type', C.c_void_p), ('d_off', C.c_void_p), ('d_value', C.c_void_p), ('d_null', C.c_void_p),
                ('n_rows', C.c_int64), ('n_values', C.c_int64), ('d_label_session', C.c_void_p), ('n_sessions', C.c_int64),
                ('n_aids', C.c_int64), ('d_out_off', C.c_void_p * 3), ('d_out_aid', C.c_void_p * 3), ('d_work', C.c_void_p),
                ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class TfidfFitJob(C.Structure):
    # mirrors otto_tfidf_fit_job (include/otto_tfidf.h)
    _fields_ = [('d_tok_aid', C.c_void_p), ('d_doc_off', C.c_void_p), ('n_tokens', C.c_int64), ('n_docs', C.c_int64), ('n_aids', C.c_int64),
                ('min_aid', C.c_int32), ('reserved', C.c_int32), ('d_row_off', C.c_void_p), ('d_df', C.c_void_p), ('d_col', C.c_void_p),
                ('d_tf', C.c_void_p), ('nnz', C.c_int64), ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class TfidfWeightsJob(C.Structure):
    # mirrors otto_tfidf_weights_job (include/otto_tfidf.h)
    _fields_ = [('d_row_off', C.c_void_p), ('d_col', C.c_void_p), ('d_tf', C.c_void_p), ('d_idf', C.c_void_p), ('d_val', C.c_void_p),
                ('n_rows', C.c_int64), ('n_cols', C.c_int64), ('stream', C.c_void_p)]


class TfidfTransposeJob(C.Structure):
    # mirrors otto_tfidf_transpose_job (include/otto_tfidf.h)
    _fields_ = [('d_off', C.c_void_p), ('d_idx', C.c_void_p), ('d_val', C.c_void_p), ('n_rows', C.c_int64), ('n_cols', C.c_int64),
                ('nnz', C.c_int64), ('d_t_off', C.c_void_p), ('d_t_idx', C.c_void_p), ('d_t_val', C.c_void_p), ('d_work', C.c_void_p),
                ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class TfidfCosineJob(C.Structure):
    # mirrors otto_tfidf_cosine_job (include/otto_tfidf.h)
    _fields_ = [('d_a_off', C.c_void_p), ('d_a_idx', C.c_void_p), ('d_a_val', C.c_void_p), ('d_t_off', C.c_void_p), ('d_t_idx', C.c_void_p),
                ('d_t_val', C.c_void_p), ('n_rows', C.c_int64), ('n_cols', C.c_int64), ('d_queries', C.c_void_p), ('n_queries', C.c_int64),
                ('k', C.c_int32), ('exclude_self', C.c_int32), ('d_ids', C.c_void_p), ('d_sim', C.c_void_p), ('d_n', C.c_void_p),
                ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class GruPlanJob(C.Structure):
    # mirrors otto_gru_plan_job (include/otto_gru.h)
    _fields_ = [('d_aid', C.c_void_p), ('d_sess_off', C.c_void_p), ('n_events', C.c_int64), ('n_sessions', C.c_int64), ('n_aids', C.c_int64),
                ('max_len', C.c_int32), ('reserved', C.c_int32), ('seed', C.c_uint64), ('epoch', C.c_uint64), ('d_p', C.c_void_p),
                ('d_seq_lo', C.c_void_p), ('d_seq_len', C.c_void_p), ('d_target', C.c_void_p), ('d_neg', C.c_void_p), ('d_work', C.c_void_p),
                ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class GruJob(C.Structure):
    # mirrors otto_gru_job (include/otto_gru.h)
    _fields_ = [('d_E', C.c_void_p), ('d_W_ih', C.c_void_p), ('d_W_hh', C.c_void_p), ('d_W_d', C.c_void_p), ('d_b_d', C.c_void_p),
                ('n_aids', C.c_int64), ('De', C.c_int32), ('H', C.c_int32), ('d_aid', C.c_void_p), ('n_events', C.c_int64),
                ('d_seq_lo', C.c_void_p), ('d_seq_len', C.c_void_p), ('d_target', C.c_void_p), ('d_neg', C.c_void_p), ('B', C.c_int64),
                ('max_len', C.c_int32), ('reserved', C.c_int32), ('d_o', C.c_void_p), ('d_gW_ih', C.c_void_p), ('d_gW_hh', C.c_void_p),
                ('d_gW_d', C.c_void_p), ('d_gb_d', C.c_void_p), ('d_ids', C.c_void_p), ('d_rows', C.c_void_p), ('cap', C.c_int64),
                ('d_count', C.c_void_p), ('d_loss_sum', C.c_void_p), ('d_work', C.c_void_p), ('work_bytes', C.c_int64), ('stream', C.c_void_p)]


class GruApplyJob(C.Structure):
    # mirrors otto_gru_apply_job (include/otto_gru.h)
    _fields_ = [('d_E', C.c_void_p), ('d_mE', C.c_void_p), ('d_vE', C.c_void_p), ('n_aids', C.c_int64), ('De', C.c_int32), ('H', C.c_int32),
                ('d_W', C.c_void_p * 4), ('d_m', C.c_void_p * 4), ('d_v', C.c_void_p * 4), ('d_g', C.c_void_p * 4), ('d_ids', C.c_void_p),
                ('d_rows', C.c_void_p), ('cap', C.c_int64), ('d_count', C.c_void_p), ('lr', C.c_double), ('beta1', C.c_double),
                ('beta2', C.c_double), ('eps', C.c_double), ('t', C.c_int64), ('stream', C.c_void_p)]


_vp, _i64, _i32, _u32 = C.c_void_p, C.c_int64, C.c_int, C.c_uint32
_p_i64 = C.POINTER(C.c_int64)

# every symbol include/*.h declares: name -> (restype, argtypes)
SIGNATURES = {
    # include/otto_covis.h
    'otto_last_error': (C.c_char_p, []),
    'otto_covis_create': (_i32, [C.POINTER(_vp), C.POINTER(CovisParams)]),
    'otto_covis_destroy': (None, [_vp]),
    'otto_covis_reset': (_i32, [_vp]),
    'otto_covis_feed': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'otto_covis_finalize': (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    'otto_covis_stats': (_i32, [_vp, _p_i64]),
    'otto_covis_set_option': (_i32, [_vp, C.c_char_p, _i64]),
    'otto_covis_export_count': (_i32, [_vp, _u32, _u32, _p_i64, _p_i64, _vp]),
    'otto_covis_export_runs': (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    'otto_covis_import_runs': (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    'otto_covis_import_reserve': (_i32, [_vp, _i64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _vp]),
    'otto_covis_export_plan': (_i32, [_vp, _i32, _vp, _p_i64, _p_i64, _vp]),
    'otto_covis_export_fill': (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    'otto_covis_export_plan_range': (_i32, [_vp, _i32, _vp, _i64, _i64, _p_i64, _p_i64, _vp]),
    'otto_covis_export_fill_range': (_i32, [_vp, _i32, _vp, _i64, _i64, _p_i64, _p_i64, _vp, _vp, _vp, _vp]),
    'otto_covis_copy_records': (_i32, [_vp, _vp, _vp, _vp, _vp]),
    'otto_covis_timings': (_i32, [_vp, C.POINTER(C.c_float)]),
    'otto_covis_kernel_names': (_i32, [_vp, _i32, C.c_char_p, _i32]),
    'otto_debug_calibrate': (_i32, [_vp, _i64, _i32, _vp]),
    # include/otto_cand.h
    'otto_cand_lookup': (_i32, [C.POINTER(CandParams), _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'otto_cand_lookup_self': (_i32, [C.POINTER(CandParams), _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    'otto_recency_predictions': (_i32, [C.POINTER(RecencyPredParams), _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'otto_cand_predictions': (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    'otto_cand_ranker_workspace': (_i64, [_i64]),
    'otto_cand_ranker_rows': (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _p_i64, _vp, _i64, _vp]),
    'otto_cand_ranker_table': (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'otto_recency_candidates': (_i32, [C.POINTER(RecencyParams), _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    # include/otto_events.h
    'otto_events_sort_workspace': (_i64, [_i64]),
    'otto_events_sort': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    'otto_events_type_from_strings': (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    # include/otto_jsonl.h
    'otto_jsonl_workspace': (_i64, [_i64]),
    'otto_jsonl_count': (_i32, [_vp, _i64, _p_i64, _vp, _i64, _vp]),
    'otto_jsonl_parse': (_i32, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    'otto_jsonl_newlines': (_i32, [_vp, _i64, _i64, _p_i64, _vp]),
    # include/otto_parquet.h
    'otto_parquet_workspace': (_i64, [_vp, _i64]),
    'otto_parquet_decode': (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _vp]),
    'otto_parquet_snappy_workspace': (_i64, [_i64]),
    'otto_parquet_snappy': (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    'otto_parquet_reason': (C.c_char_p, [_i32]),
    # include/otto_pairs.h
    'otto_pairs_raw_count': (_i32, [_vp, _i64, _i32, _p_i64, _vp]),
    'otto_pairs_workspace': (_i64, [_i64]),
    'otto_pairs_time': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    'otto_pairs_diff': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    # include/otto_inter.h
    'otto_inter_workspace': (_i64, [_u32]),
    'otto_inter_features': (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _u32, _vp, _vp, _vp, _vp, _i64, _vp]),
    'otto_inter_features_rows': (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _i64, _vp]),
    # include/otto_feat.h
    'otto_feat_aid_table_workspace': (_i64, [_i64, _u32]),
    'otto_feat_aid_table': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _u32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    'otto_feat_session_table_workspace': (_i64, [_i64]),
    'otto_feat_session_table': (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    'otto_feat_matrix_workspace': (_i64, [_i64]),
    'otto_feat_matrix': (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _i32, _vp, _vp, _i64, _vp]),
    # include/otto_mf.h
    'otto_mf_create': (_i32, [C.POINTER(_vp), _i64, _i64, _i32, _i64, _i32]),
    'otto_mf_destroy': (None, [_vp]),
    'otto_mf_forward': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    'otto_mf_eval': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    'otto_mf_eval_sums': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    'otto_mf_read_sums': (_i32, [_vp, C.POINTER(C.c_double), _i32, _vp]),
    'otto_mf_check': (_i32, [_vp, _p_i64, _vp]),
    'otto_mf_step_sparse_adam': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32,
                                        C.c_double, C.c_double, C.c_double, C.c_double, _i64, _vp, _vp]),
    'otto_mf_dp_local': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, C.c_double, C.c_double,
                                C.c_double, C.c_double, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    'otto_mf_dp_apply': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, C.c_double, C.c_double, C.c_double,
                                C.c_double, _i64, _vp]),
    'otto_mf_bpr_step': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, C.c_uint64, C.c_uint64, _i64, C.c_float, C.c_float,
                                _i32, _vp, _vp, _vp]),
    'otto_mf_score_topk': (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i64, _vp, _vp, _vp, _i64, _vp]),
    'otto_mf_score_workspace': (_i64, [_i64, _i64, _i32]),
    'otto_mf_topk_merge': (_i32, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp]),
    # include/otto_knn.h
    'otto_knn_workspace': (_i64, [_i64, _i64, _i32, _i32, _i32]),
    'otto_knn_table': (_i32, [_vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    # include/otto_forest.h
    'otto_forest_packed_bytes': (_i64, [_i32, _i64, _i64]),
    'otto_forest_pack': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64]),
    'otto_forest_predict': (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, C.c_double, _vp]),
    'otto_forest_leaves': (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp]),
    'otto_forest_session_topk': (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    # include/otto_blend.h
    'otto_blend_select_workspace': (_i64, [_i64]),
    'otto_blend_robust_stats': (_i32, [_vp, _i64, _p_i64, C.POINTER(C.c_double), _vp, _i64, _vp]),
    'otto_blend_scale': (_i32, [_vp, _i64, C.c_double, C.c_double, _vp, _vp]),
    'otto_blend_join_workspace': (_i64, [_i64, _i32]),
    'otto_blend_join': (_i32, [_i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _p_i64, C.POINTER(C.c_double),
                               C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _p_i64, _p_i64, _vp, _i64, _vp]),
    # include/otto_eval.h
    'otto_eval_last_click': (_i32, [_vp, _vp, _i64, _vp, _vp]),
    'otto_eval_cutoffs': (_i32, [_vp, _vp, _i64, C.c_uint64, _vp, _p_i64, _vp]),
    'otto_eval_split_workspace': (_i64, [_i64, _i64]),
    'otto_eval_split_count': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    'otto_eval_split': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                               _vp]),
    'otto_eval_hits_workspace': (_i64, [_i64]),
    'otto_eval_hits': (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _p_i64, _vp, _i64, _vp]),
    # include/otto_gbdt.h
    'otto_gbdt_workspace_bytes': (_i64, [_i64, _i32, _i32]),
    'otto_gbdt_bin': (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    'otto_gbdt_lambdarank': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, C.c_double, C.c_double, _vp, C.c_double, _i32, _i32, _vp, _vp,
                                    _vp]),
    'otto_gbdt_quantize': (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    'otto_gbdt_hist': (_i32, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _i32, _vp, _vp]),
    'otto_gbdt_best_split': (_i32, [_vp, _i32, _vp, _vp, _i64, C.c_double, C.c_double, C.c_double, _vp, _i32, _vp, _vp]),
    'otto_gbdt_partition': (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    'otto_gbdt_add_tree': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'otto_gbdt_ap_at_k': (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    'otto_gbdt_grow_tree': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i64, C.c_double, C.c_double, C.c_double, C.c_double,
                                   _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'otto_gbdt_bag_workspace_bytes': (_i64, [_i64]),
    'otto_gbdt_bag': (_i32, [_i64, _i64, C.c_uint64, _vp, _i64, _vp, _i64, _vp]),
    # include/otto_xgb.h
    'otto_xgb_lambdamart': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, C.c_double, C.c_double, C.c_uint64, _i32, _vp, _vp, _vp, _vp]),
    'otto_xgb_workspace_bytes': (_i64, [_i64, _i32, _i32]),
    'otto_xgb_grow_tree': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _vp,
                                  _i64, _vp, _i32, C.POINTER(XgbTree), _vp, _i64, _vp]),
    'otto_xgb_level_hist': (_i32, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    'otto_xgb_level_split': (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, C.c_double, C.c_double, C.c_double, _vp, _i32, _vp, _vp,
                                    _i64, _vp]),
    'otto_xgb_level_partition': (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    # include/otto_objective.h
    'otto_obj_constants': (None, [C.POINTER(C.c_int32)]),
    'otto_obj_binary': (_i32, [_vp, _vp, _i64, _vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp,
                               _vp]),
    'otto_obj_label_counts': (_i32, [_vp, _i64, _vp, _vp]),
    'otto_obj_ndcg_at_k': (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    'otto_obj_auc_workspace_bytes': (_i64, [_i64]),
    'otto_obj_auc': (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    'otto_obj_logloss': (_i32, [_vp, _vp, _i64, C.c_double, _vp, _vp, _vp]),
    'otto_obj_logloss_grid': (_i32, [_vp, _vp, _i64, C.c_double, _i32, _vp, _vp, _vp]),
    # include/otto_folds.h
    'otto_folds_kfold_workspace': (_i64, [_i64]),
    'otto_folds_group_kfold': (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, C.POINTER(C.c_float), _vp, _i64, _vp]),
    'otto_folds_state_bytes': (_i64, [_i64]),
    'otto_folds_classify': (_i32, [_vp, _i32, _vp, _i64, _i64, _vp, _i32, _vp, _p_i64, _vp]),
    'otto_folds_emit_workspace': (_i64, [_i64]),
    'otto_folds_emit': (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _i64, _vp]),
    'otto_folds_gather_u8': (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    # include/otto_sgns.h
    'otto_sgns_neg_table_workspace': (_i64, [_i64]),
    'otto_sgns_neg_table': (_i32, [_vp, _i64, _i64, _vp, _vp, C.POINTER(SgnsTable), _vp, _i64, _vp]),
    'otto_sgns_draw': (_i32, [C.POINTER(SgnsTable), _vp, _i64, _vp, _vp]),
    'otto_sgns_plan_workspace': (_i64, [_i64]),
    'otto_sgns_plan': (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, C.c_uint64, C.c_uint64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp,
                              _vp, _p_i64, _vp, _i64, _vp]),
    'otto_sgns_step': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, C.c_float, _i32, C.c_uint64, C.c_uint64,
                              C.POINTER(SgnsTable), _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'otto_sgns_step_hs': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, C.c_float, _i32, C.c_uint64,
                                 C.c_uint64, C.POINTER(SgnsTable), _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp,
                                 _vp]),
    'otto_sgns_hs_tree_sizes': (_i32, [_vp, _i64, _i64, _p_i64]),
    'otto_sgns_hs_tree': (_i32, [_vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    'otto_sgns_cbow_step': (_i32, [C.POINTER(SgnsCbowJob)]),
    'otto_sgns_infer': (_i32, [C.POINTER(SgnsInferJob)]),
    # include/otto_submit.h
    'otto_submit_workspace': (_i64, [_i64, _i32]),
    'otto_submit_measure': (_i32, [_i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int32), _vp, _i64, _i32, _i64, _i32, _p_i64,
                                   _vp, _i64, _vp]),
    'otto_submit_format': (_i32, [_i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int32), _vp, _i64, _i32, _i64, _i32, _vp, _i64,
                                  _i64, _vp, _i64, _vp]),
    'otto_freq_count': (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    'otto_freq_topk': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    # include/otto_deflate.h
    'otto_deflate_bound': (_i64, [_i64, _i32]),
    'otto_deflate_workspace': (_i64, [_i64, _i32]),
    'otto_deflate_plan': (_i32, [_vp, _i64, _i32, _p_i64, _vp, _i64, _vp]),
    'otto_deflate_emit': (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp]),
    # include/otto_snappy.h
    'otto_snappy_bound': (_i64, [_i64]),
    'otto_snappy_workspace': (_i64, [C.POINTER(SnappyJob)]),
    'otto_snappy_plan': (_i32, [C.POINTER(SnappyJob), _vp]),
    'otto_snappy_emit': (_i32, [C.POINTER(SnappyJob), _vp, _vp, _i64]),
    # include/otto_pqwrite.h
    'otto_pqw_workspace': (_i64, [C.POINTER(PqwJob)]),
    'otto_pqw_plan': (_i32, [C.POINTER(PqwJob), _vp]),
    'otto_pqw_emit': (_i32, [C.POINTER(PqwJob), _vp, _vp, _i64]),
    # include/otto_rows.h
    'otto_rows_workspace': (_i64, [C.POINTER(RowsJob)]),
    'otto_rows_topk': (_i32, [C.POINTER(RowsJob), _vp]),
    # include/otto_pqlist.h
    'otto_pqlist_workspace': (_i64, [C.POINTER(PqlistJob)]),
    'otto_pqlist_levels': (_i32, [C.POINTER(PqlistJob), _vp]),
    'otto_pqlist_reason': (C.c_char_p, [_i32]),
    # include/otto_labels.h
    'otto_labels_workspace': (_i64, [C.POINTER(LabelsJob)]),
    'otto_labels_count': (_i32, [C.POINTER(LabelsJob), _vp, _vp]),
    'otto_labels_fill': (_i32, [C.POINTER(LabelsJob)]),
    # include/otto_tfidf.h
    'otto_tfidf_fit_workspace': (_i64, [C.POINTER(TfidfFitJob)]),
    'otto_tfidf_count': (_i32, [C.POINTER(TfidfFitJob), _vp, _vp]),
    'otto_tfidf_fill': (_i32, [C.POINTER(TfidfFitJob)]),
    'otto_tfidf_weights': (_i32, [C.POINTER(TfidfWeightsJob)]),
    'otto_tfidf_transpose_workspace': (_i64, [C.POINTER(TfidfTransposeJob)]),
    'otto_tfidf_transpose': (_i32, [C.POINTER(TfidfTransposeJob), _vp]),
    'otto_tfidf_cosine_workspace': (_i64, [C.POINTER(TfidfCosineJob)]),
    'otto_tfidf_cosine_topk': (_i32, [C.POINTER(TfidfCosineJob), _vp]),
    # include/otto_gru.h
    'otto_gru_plan_workspace': (_i64, [C.POINTER(GruPlanJob)]),
    'otto_gru_plan': (_i32, [C.POINTER(GruPlanJob), _vp, _vp]),
    'otto_gru_workspace': (_i64, [C.POINTER(GruJob), _i32]),
    'otto_gru_encode': (_i32, [C.POINTER(GruJob)]),
    'otto_gru_grad': (_i32, [C.POINTER(GruJob)]),
    'otto_gru_apply': (_i32, [C.POINTER(GruApplyJob)]),
}

_lib = None


def register(signatures):
    """Let sibling modules (matrix_factorization) add their header's symbols."""
    SIGNATURES.update(signatures)
    _POINTERS.clear()
    global _lib
    if _lib is not None:
        _bind(_lib, signatures)


def _bind(lib, signatures):
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise OttoError(f'{LIB_PATH} does not export {name}; rebuild with __graft_entry__.build()') from e
        fn.restype = res
        fn.argtypes = args


def lib():
    """Load (once) and return the shared library; raises OttoError when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OttoError(
                f'HIP library {LIB_PATH} is not built. Run `python -c "import __graft_entry__ as g; g.build()"` '
                f'(or `make -C {os.path.dirname(LIB_PATH)}`). There is no CPU fallback.')
        try:
            loaded = C.CDLL(LIB_PATH)
        except OSError as e:
            raise OttoError(f'cannot load {LIB_PATH}: {e}') from e
        _bind(loaded, SIGNATURES)
        _lib = loaded
    return _lib


def rocm_device(device, what):
    """``torch.device(device)`` with its index filled in (the tensors' device carries one); ``OttoError`` in the name of
    ``what`` unless it is a ROCm device."""
    import torch
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise OttoError(f'{what} needs a ROCm device (no CPU fallback)')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def check(rc, what):
    if rc != 0:
        msg = lib().otto_last_error()
        raise OttoError(f'{what} failed (code {rc}): {msg.decode() if msg else "?"}')


def ptr(t, dev=None, what='tensor'):
    """The address of a tensor's first element as a ``c_void_p``, NULL for None. With ``dev`` the tensor must be
    contiguous device memory on ``dev`` (``ValueError``): the rule of ``marshal``, for a pointer stored into a
    ``Structure`` field. Without, nothing is checked: for a matrix that goes in as rows with a leading dimension."""
    if t is None:
        return C.c_void_p(0)
    if dev is not None and (t.device != dev or not t.is_contiguous()):
        raise ValueError(_not_on(dev, t, what))
    return C.c_void_p(t.data_ptr())


def _not_on(dev, t, what):
    return f'{what}: expected a contiguous tensor on {dev}, got a{"" if t.is_contiguous() else " strided"} tensor on {t.device}'


def stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_stream_of = stream             # ``call`` has a flag of that name


_Tensor = _ndarray = None      # torch.Tensor and numpy.ndarray, imported at first use: marshal and need run once per launch


_POINTERS = {}                 # name -> (number of parameters, positions of the void* ones): what marshal looks at


def _load_types():
    global _Tensor, _ndarray
    from numpy import ndarray as _ndarray
    from torch import Tensor as _Tensor


def marshal(name, dev, args, stream=True):
    """The ctypes values of ``args`` for entry point ``name`` (a list; the stream that ``call`` appends is not in it).

    A torch tensor always means device memory on ``dev``: it must live there and be contiguous, and goes in as its
    address. Anything else is host: ``None`` is NULL (ctypes' own rule for every pointer parameter), a NumPy array is a
    C-contiguous host buffer passed as its address, ctypes values, ``byref(...)``, ctypes arrays, bytes, ints and floats
    go to ctypes as they are. Raises ``ValueError`` before anything is launched, also when the number of arguments is
    not the one ``SIGNATURES[name]`` declares -- ctypes takes surplus cdecl arguments silently."""
    if _Tensor is None:
        _load_types()
    pointers = _POINTERS.get(name)
    if pointers is None:
        argtypes = SIGNATURES[name][1]
        pointers = _POINTERS[name] = (len(argtypes), tuple(i for i, t in enumerate(argtypes) if t is C.c_void_p))
    if len(args) + (1 if stream else 0) != pointers[0]:
        raise ValueError(f'{name}: {len(args)} arguments{" + the stream" if stream else ""}, the header declares {pointers[0]}')
    out = list(args)
    for i in pointers[1][:-1] if stream else pointers[1]:
        a = out[i]
        if isinstance(a, _Tensor):
            if a.device != dev or not a.is_contiguous():
                raise ValueError(_not_on(dev, a, f'{name}: argument {i}'))
            out[i] = C.c_void_p(a.data_ptr())
        elif isinstance(a, _ndarray):
            if not a.flags.c_contiguous:
                raise ValueError(f'{name}: argument {i}: expected a C-contiguous host array')
            out[i] = a.ctypes.data_as(C.c_void_p)
    return out


def call(name, dev, *args, stream=True):
    """Run entry point ``name`` on ``dev``: ``marshal`` the arguments, enter the device, append its current stream
    (``stream=False`` for the entry points that take none) and raise ``OttoError`` on a non-zero return code.
    ``dev=None``: an entry point that works on host arrays alone; no device is entered."""
    import torch
    argv = marshal(name, dev, args, stream)
    fn = getattr(lib(), name)
    if dev is None:
        return check(fn(*argv), name)
    with torch.cuda.device(dev):
        if stream:
            argv.append(_stream_of(dev))
        check(fn(*argv), name)


def need(t, what, dtype, dim=None, device=None, numel=None, copy=False):
    """The argument check of the wrappers; returns ``t``. ``ValueError`` unless ``t`` is a ``dtype`` tensor (of ``dim``
    dimensions, of ``numel`` elements, where given) that is contiguous -- ``copy=True`` returns ``t.contiguous()``
    instead of refusing a strided one. ``device``: where it must live (``ValueError``); None: on any ROCm device, and a
    tensor elsewhere is an ``OttoError``, since there is no CPU fallback."""
    if _Tensor is None:
        _load_types()
    if not isinstance(t, _Tensor) or t.dtype != dtype or (dim is not None and t.dim() != dim):
        raise ValueError(f'{what}: expected a {"" if dim is None else f"{dim}-d "}{dtype} tensor')
    if device is None:
        if t.device.type != 'cuda':
            raise OttoError(f'{what} needs a ROCm device (no CPU fallback)')
    elif t.device != device:
        raise ValueError(f'{what}: expected a tensor on {device}, got one on {t.device}')
    if not t.is_contiguous():
        if not copy:
            raise ValueError(f'{what}: expected a contiguous tensor')
        t = t.contiguous()
    if numel is not None and t.numel() != numel:
        raise ValueError(f'{what}: expected {numel} elements, got {t.numel()}')
    return t


def workspace(n_bytes, dev):
    """Scratch for one call: uint8, never below the 256 bytes ``device_scratch`` keeps on the C side."""
    import torch
    return torch.empty(max(int(n_bytes), 256), dtype=torch.uint8, device=dev)
