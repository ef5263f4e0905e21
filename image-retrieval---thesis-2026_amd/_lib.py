"""ctypes binding of libmirx.so -- the only way the package reaches the HIP kernels.

There is no CPU fallback: if the library is missing or a symbol of include/mirx.h is absent
the import raises, and every wrapper turns a negative return code into MirxError.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIRX_LIB_PATH", os.path.join(_HERE, "libmirx.so"))   # override: kernel experiments only

METRIC_IP = 0
ESTATE = -4                        # MIRX_ESTATE: call not valid in the index's current state
METRIC_NEG_L2 = 1
TIER_AUTO = 0
TIER_EXACT_ONLY = 3
OPT_TIERS = 1
OPT_SAMPLE_RANK = 2
OPT_FORCE_TAU = 3
OPT_PROFILE = 4
OPT_RANK_SORT = 5                  # which sort rank_all runs
OPT_COMPACT_CHUNK_ROWS = 6         # test hook: rows per compaction chunk of mirx_index_remove_ids (0 = default)
OPT_MASK_GATHER_BYTES = 7          # test hook: scratch limit of a masked search's gather of its allowed rows (-1 = default)
OPT_RANGE_MAX_HITS = 8             # test hook: most hits one range search may return (0 = default, 2^28)
RANK_SORT_AUTO = 0                 # bitonic up to 65536 rows, radix above
RANK_SORT_BITONIC = 1
RANK_SORT_RADIX = 2
MAX_SEARCH_K = 1024                # mirx_index_search's k limit; FlatIndex.search goes to rank_top above it
GROUP_MAX_LIMIT, GROUP_MAX_SIZE, GROUP_MAX_HITS, GROUP_FILL_MAX = 1024, 64, 16384, 4096   # the grouping calls' limits (include/mirx.h)
FUSE_MAX_REQUESTS, FUSE_MAX_ENTRIES, FUSE_MAX_LIMIT = 8, 4096, 1024   # mirx_fuse_ranked's limits (include/mirx.h)
FUSE_RRF, FUSE_WEIGHTED = 0, 1     # mirx_fuse_ranked `ranker`
FUSE_NORMS = {"RAW": 0, "COSINE": 1, "IP": 2, "L2": 3}   # and its per-request `norms`
TUNE_CONV1X1_SMALL_MAX_WG = 1      # mirx_set_tuning keys
TUNE_CONV3X3_SMALL_MAX_WG = 2
TUNE_CONV1X1_RING = 3
SIMCAM_MAPS_BOTH = 0               # mirx_simcam `maps`
SIMCAM_MAPS_RETRIEVED = 1
SIMATT_GROUP = 0                   # mirx_simatt `mode`
SIMATT_PAIRS = 1
ANOMALY_BAD_SCORE = 1              # bits of the anomaly calls' bad_flag
ANOMALY_BAD_NORM = 2
ANOMALY_BAD_ONE_CLASS = 4
ANOMALY_BAD_EMPTY_CLASS = 8
RESAMPLE_MAX_SIDE = 8192           # the caps of mirx_resample_batch (include/mirx.h)
RESAMPLE_MAX_TAPS = 65
RESAMPLE_MAX_OUT = 1024
RESAMPLE_MAX_BATCH = 65536
RESAMPLE_MAX_LDS = 65536
RESAMPLE_TILE_W, RESAMPLE_TILE_H = 32, 16
RESAMPLE_DESC_WORDS = 8
RESAMPLE_OUT_U8, RESAMPLE_OUT_F32 = 0, 1
RESAMPLE_BILINEAR, RESAMPLE_BICUBIC = 0, 1
IVF_MAX_NLIST, IVF_MAX_DIM = 65536, 2048   # mirx_ivf_create's limits (include/mirx.h)
IVF_FLAT, IVF_SQ8 = 0, 1           # mirx_ivf_create_typed's kinds
IVF_PQ = 2                         # mirx_ivf_create_pq's kind
PQ_MAX_M = 64                      # mirx_ivf_create_pq: m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0
IVF_OPT_SCORE_BYTES = 1            # test hook: the score workspace budget of mirx_ivf_search in bytes (0 = default, 1 GiB)
ROLLOUT_FUSE = {"mean": 0, "max": 1, "min": 2}   # mirx_rollout_layer `fusion`
STAGES = ("prep", "sample", "gemm", "finalize", "exact")
FORCE_TAU_OFF = 0x7FC00000


class MirxError(RuntimeError):
    """A libmirx call failed (message from mirx_last_error())."""


class SearchStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ("nq", "tier1_answered", "exact_answered", "candidates", "reranked",
                 "overflowed", "incomplete", "left_out")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RangeStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("nq", "filter_answered", "exact_answered", "candidates", "hits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class IvfStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("nq", "rows_scored", "pairs", "work_items", "batches")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# name -> (restype, argtypes): every symbol include/mirx.h declares
_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
SYMBOLS = {
    "mirx_last_error": (ctypes.c_char_p, []),
    "mirx_version": (_int, []),
    "mirx_set_tuning": (_int, [_int, _i64]),
    "mirx_index_create": (_int, [_int, _int, _int, ctypes.POINTER(_vp)]),
    "mirx_index_destroy": (None, [_vp]),
    "mirx_index_add": (_int, [_vp, _vp, _i64, _vp]),
    "mirx_index_reserve": (_int, [_vp, _i64]),
    "mirx_index_size": (_i64, [_vp]),
    "mirx_index_dim": (_int, [_vp]),
    "mirx_index_set_option": (_int, [_vp, _int, _i64]),
    "mirx_index_get_rows": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "mirx_index_remove_ids": (_int, [_vp, _vp, _i64, ctypes.POINTER(_i64), _vp]),
    "mirx_compact_tile": (_int, []),
    "mirx_index_search": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mirx_index_search_f64": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mirx_index_search_begin": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "mirx_index_search_end": (_int, [_vp]),
    "mirx_index_search_masked": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirx_index_search_deep": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mirx_index_search_leave_out": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirx_tier1_max_k": (_int, []),
    "mirx_deep_min_rows": (_i64, [_int, _i64]),
    "mirx_index_rank_top_masked": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirx_index_range_search": (_int, [_vp, _vp, _i64, ctypes.c_double, ctypes.c_double, _vp, _vp, _i64, _vp,
                                       ctypes.POINTER(_i64), _vp]),
    "mirx_index_range_fetch": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "mirx_index_range_last_stats": (_int, [_vp, ctypes.POINTER(RangeStats)]),
    "mirx_index_last_stats": (_int, [_vp, _vp, ctypes.POINTER(SearchStats)]),
    "mirx_index_last_timings": (_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "mirx_index_rank_all": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirx_index_rank_top": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "mirx_rank_key": (ctypes.c_uint64, [ctypes.c_double]),
    "mirx_rank_sort_tile": (_int, []),
    "mirx_topk_merge": (_int, [_vp, _vp, _int, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "mirx_rank_metrics": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _int, _int, ctypes.c_double, _int,
                                 ctypes.POINTER(ctypes.c_int32), _int, _vp, _vp, _vp, _vp, _vp]),
    "mirx_rank_metrics_grouped": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _int, _int, ctypes.c_double, _int,
                                         ctypes.POINTER(ctypes.c_int32), _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mirx_index_rank_metrics": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _vp, _vp, _vp, _int, ctypes.c_double, _int,
                                       ctypes.POINTER(ctypes.c_int32), _int, _vp, _vp, _vp, _vp, _vp]),
    "mirx_group_walk": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp,
                               _vp]),
    "mirx_group_count": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "mirx_index_group_fill": (_int, [_vp, _vp, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _int, _vp, _vp, _vp]),
    "mirx_index_get_ids": (_int, [_vp, _i64, _i64, _vp]),
    "mirx_fuse_ranked": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _int, ctypes.c_double, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp,
                                _vp]),
    "mirx_linear_split2h": (_int, [_vp, _i64, _int, _vp, _vp, _int, _int, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "mirx_rows_to_terms": (_int, [_vp, _i64, _int, _i64, ctypes.c_float, _vp, _vp]),
    "mirx_layernorm_patch2_nhwc": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp, ctypes.c_float, _vp, _vp]),
    "mirx_layernorm_terms": (_int, [_vp, _i64, _int, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "mirx_linear_terms": (_int, [_vp, _i64, _int, _vp, _vp, _int, _int, _vp, _vp, ctypes.c_float, _vp, _vp, ctypes.c_float, _vp, _i64,
                                 _vp]),
    "mirx_linear_terms_workspace_bytes": (_i64, [_i64, _int, _int]),
    "mirx_linear_split3": (_int, [_vp, _i64, _int, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "mirx_linear_split3_nchw": (_int, [_vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
    "mirx_linear_split2h_nchw": (_int, [_vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, ctypes.c_float, _vp, ctypes.c_float, _vp,
                                        _vp]),
    "mirx_linear_split2h_gelu_grn": (_int, [_vp, _i64, _int, _int, _vp, _vp, _int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp]),
    "mirx_linear_split2h_grn_rows": (_int, [_vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, ctypes.c_float, _vp, ctypes.c_float, _vp,
                                            _vp]),
    "mirx_grn_norm_nhwc": (_int, [_vp, _i64, _int, _int, _vp, _vp]),
    "mirx_grn_scale": (_int, [_vp, _vp, _i64, _int, ctypes.c_float, _vp, _vp, _vp]),
    "mirx_conv1x1_bn_relu_split3": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp, _i64, _vp]),
    "mirx_conv1x1_bn_relu_split2h": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp, _i64,
                                            _vp, ctypes.c_float, ctypes.c_float, _vp, _i64, _i64, _vp]),
    "mirx_layernorm": (_int, [_vp, _i64, _int, _vp, _vp, ctypes.c_float, _vp, _int, _vp]),
    "mirx_patchify_nchw": (_int, [_vp, _i64, _int, _int, _int, _int, _vp, _vp, ctypes.c_float, _vp, _int, _vp]),
    "mirx_attention_small": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _int, _int, _int, _int, ctypes.c_float, _vp, _vp]),
    "mirx_range_absmax": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "mirx_range_absmax_u8": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "mirx_stem_conv7_bn_relu_pool_split2h_u8_into": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _i64, _vp, _vp,
                                                            _vp]),
    "mirx_stem_conv7_bn_relu_pool_split2h_into": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _i64, _vp, _vp, _vp]),
    "mirx_conv1x1_bn_relu_split2h_terms": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, ctypes.c_float,
                                                  ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _i64, _vp]),
    "mirx_dense_layer_fused": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp]),
    "mirx_conv3x3_direct_terms_nchw": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _i64, _vp, _vp, _i64, _vp]),
    "mirx_conv3x3_direct_terms_nchw_pool": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "mirx_conv3x3_small_launch": (_int, [_i64, _int]),
    "mirx_conv3x3_winograd_split3_nchw": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp]),
    "mirx_conv3x3_direct_split3_nchw": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp]),
    "mirx_conv3x3_winograd_nchw": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp]),
    "mirx_attention_qkv_f32": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, _vp, _vp]),
    "mirx_attention_qkv_f32_split2h": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "mirx_attention_qkv_f32_split2h_terms": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                    ctypes.c_float, _vp, _vp]),
    "mirx_attention_qkv_f32_split3": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, _vp, _vp]),
    "mirx_l2_normalize": (_int, [_vp, _i64, _int, _vp]),
    "mirx_bn_relu_gap_l2norm": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "mirx_bn_relu_nchw": (_int, [_vp, _i64, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "mirx_bn_relu_avgpool2": (_int, [_vp, _i64, _vp, _vp, _i64, _int, _int, _int, _vp, _i64, _vp]),
    "mirx_bn_relu_avgpool2_into": (_int, [_vp, _i64, _vp, _vp, _i64, _int, _int, _int, _vp, _i64, _i64, _vp]),
    "mirx_conv1x1_bn_relu": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "mirx_dwconv7x7_nchw_to_nhwc": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "mirx_dwconv7x7_nhwc": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "mirx_stem_conv7_bn_relu_pool_split3": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "mirx_stem_conv7_bn_relu_pool": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "mirx_conv_terms": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _vp, _int, ctypes.c_float,
                               ctypes.c_float, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "mirx_nchw_to_terms": (_int, [_vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "mirx_gap_nhwc_l2norm": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp]),
    "mirx_window_attention_split2h": (_int, [_vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, ctypes.c_float, _vp]),
    "mirx_swin_postnorm": (_int, [_vp, _vp, _i64, _int, _vp, _vp, ctypes.c_float, _vp, _vp, ctypes.c_float, _vp]),
    "mirx_patch_merge_terms": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, _vp, _vp]),
    "mirx_sra_head_nhwc": (_int, [_vp, _i64, _int, _int, _vp, _int, _vp, _vp, ctypes.c_float, ctypes.c_float, _int, _vp, _vp]),
    "mirx_pcam_head_nhwc": (_int, [_vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, ctypes.c_float, ctypes.c_float, _int, _vp, _vp,
                                   _vp]),
    "mirx_hamming_words": (_int, [_int]),
    "mirx_hamming_pack": (_int, [_vp, _int, _i64, _int, _vp, _vp, _vp]),
    "mirx_hamming_workspace_bytes": (_i64, [_i64, _i64, _int, _int]),
    "mirx_hamming_topk": (_int, [_vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _i64, _vp, _vp, _vp]),
    "mirx_ath_workspace_floats": (_i64, [_i64, _int]),
    "mirx_ath_forward": (_int, [_vp, _i64, _int, _vp, _int, _int, _vp, _i64, _vp, _vp, _vp]),
    "mirx_simcam_workspace_floats": (_i64, [_i64, _i64]),
    "mirx_simcam": (_int, [_vp, _vp, _i64, _i64, _int, _int, _i64, ctypes.c_float, _int, ctypes.POINTER(ctypes.c_double), _int, _int,
                           _vp, _i64, _vp, _vp]),
    "mirx_bn_relu_rows": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "mirx_rollout_workspace_floats": (_i64, [_int, _i64, _i64]),
    "mirx_rollout_layer": (_int, [_vp, _i64, _int, _int, _int, ctypes.c_float, _int, _int, _int, _int, _vp, _i64, _vp]),
    "mirx_rollout_rows": (_int, [_vp, _i64, _int, _int, _vp]),
    "mirx_rollout_finish": (_int, [_vp, _i64, _int, _i64, _int, _int, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "mirx_gradcam_workspace_floats": (_i64, [_i64, _int, _int, _int]),
    "mirx_gradcam_pool": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _i64, _vp, _vp]),
    "mirx_gradcam_tokens": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mirx_gradcam_finish": (_int, [_vp, _i64, _int, _int, _int, _vp, _i64, _int, _int, _vp, _vp]),
    "mirx_gradcam_gemv": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _int, _int, _int, _int, _i64, _i64, _vp]),
    "mirx_gradcam_layernorm": (_int, [_vp, _i64, _int, _vp, _vp, ctypes.c_float, _int, _vp, _vp, _vp]),
    "mirx_gradcam_layernorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp]),
    "mirx_gradcam_gelu": (_int, [_vp, _vp, _i64, _int, _vp, _vp]),
    "mirx_gradcam_cosine_bwd": (_int, [_vp, _i64, _int, _vp, _i64, _vp, _vp]),
    "mirx_lesion_rerank": (_int, [_vp, _i64, _vp, _vp, _int, _vp, _vp, _vp, _i64, _int, _vp, _vp, _int, _int, ctypes.c_double, _vp, _vp,
                                  _vp, _vp]),
    "mirx_simatt_workspace_floats": (_i64, [_i64, _i64, _i64, _int]),
    "mirx_simatt": (_int, [_vp, _i64, _int, _int, _i64, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _i64, _vp, _vp]),
    "mirx_class_centroids_workspace_bytes": (_i64, [_i64, _int, _int]),
    "mirx_class_centroids": (_int, [_vp, _i64, _int, _vp, _vp, _int, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirx_centroid_min_dist": (_int, [_vp, _i64, _int, _vp, _int, _vp, _vp, _vp, _vp]),
    "mirx_binary_rank_metrics_workspace_bytes": (_i64, [_i64, _i64]),
    "mirx_binary_rank_metrics": (_int, [_vp, _vp, _i64, _i64, _vp, ctypes.c_double, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp]),
    "mirx_insdel_steps_workspace_bytes": (_i64, [_i64, _i64]),
    "mirx_insdel_steps": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "mirx_blur2d_same": (_int, [_vp, _i64, _int, _int, _int, _vp, _int, _vp, _vp]),
    "mirx_insdel_compose": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "mirx_insdel_curves": (_int, [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "mirx_sbsm_compose": (_int, [_vp, _i64, _int, _int, _int, _vp, _int, _vp, _int, _i64, _i64, _vp, _vp]),
    "mirx_sbsm_gain": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _int, _vp, _vp]),
    "mirx_sbsm_workspace_bytes": (_i64, [_i64, _int, _int]),
    "mirx_sbsm_accumulate": (_int, [_vp, _i64, _vp, _int, _vp, _int, _int, _int, _vp, _i64, _vp, _vp]),
    "mirx_resample_taps": (_int, [_int, _int]),
    "mirx_resample_plan": (_int, [_int, _int, _int, _int, _vp, _i64]),
    "mirx_resample_batch": (_int, [_vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "mirx_resample_taps_filter": (_int, [_int, _int, _int]),
    "mirx_resample_plan_filter": (_int, [_int, _int, _int, _int, _int, _vp, _i64]),
    "mirx_ivf_create": (_int, [_int, _int, _int, _int, ctypes.POINTER(_vp)]),
    "mirx_ivf_destroy": (None, [_vp]),
    "mirx_ivf_train": (_int, [_vp, _vp, _i64, _vp, _int, _vp]),
    "mirx_ivf_set_centroids": (_int, [_vp, _vp]),
    "mirx_ivf_get_centroids": (_int, [_vp, _vp]),
    "mirx_ivf_add": (_int, [_vp, _vp, _i64, _vp]),
    "mirx_ivf_remove_ids": (_int, [_vp, _vp, _i64, ctypes.POINTER(_i64), _vp]),
    "mirx_ivf_size": (_i64, [_vp]),
    "mirx_ivf_list_sizes": (_int, [_vp, _vp]),
    "mirx_ivf_assign": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "mirx_ivf_search": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mirx_ivf_last_stats": (_int, [_vp, _vp, ctypes.POINTER(IvfStats)]),
    "mirx_ivf_set_option": (_int, [_vp, _int, _i64]),
    "mirx_ivf_query_tile": (_int, [_int]),
    "mirx_ivf_row_block": (_int, []),
    "mirx_ivf_create_typed": (_int, [_int, _int, _int, _int, _int, ctypes.POINTER(_vp)]),
    "mirx_ivf_kind": (_int, [_vp]),
    "mirx_ivf_sq8_train": (_int, [_vp, _vp, _i64, _vp]),
    "mirx_ivf_sq8_set_range": (_int, [_vp, _vp, _vp]),
    "mirx_ivf_sq8_get_range": (_int, [_vp, _vp, _vp]),
    "mirx_ivf_get_codes": (_int, [_vp, _vp, _vp, _vp]),
    "mirx_ivf_reconstruct": (_int, [_vp, _vp, _vp]),
    "mirx_sq8_encode": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mirx_sq8_decode": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mirx_ivf_create_pq": (_int, [_int, _int, _int, _int, _int, _int, ctypes.POINTER(_vp)]),
    "mirx_ivf_pq_train": (_int, [_vp, _vp, _i64, _int, _vp]),
    "mirx_ivf_pq_set_codebooks": (_int, [_vp, _vp]),
    "mirx_ivf_pq_get_codebooks": (_int, [_vp, _vp]),
    "mirx_ivf_pq_m": (_int, [_vp]),
    "mirx_ivf_pq_item_rows": (_int, []),
    "mirx_pq_encode": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp]),
    "mirx_pq_decode": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp]),
    "mirx_pq_tables": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp, _vp]),
    "mirx_ivf_create_pq_ex": (_int, [_int, _int, _int, _int, _int, _int, _int, ctypes.POINTER(_vp)]),
    "mirx_ivf_pq_by_residual": (_int, [_vp]),
    "mirx_ivf_get_norms": (_int, [_vp, _vp]),
    "mirx_pq_residuals": (_int, [_vp, _i64, _int, _vp, _vp, _int, _vp, _vp]),
    "mirx_pq_bases": (_int, [_vp, _i64, _int, _int, _vp, _int, _vp, _int, _vp, _vp, _vp]),
}

_lib = None
ABI_VERSION = 305          # include/mirx.h MIRX_VERSION this binding was written against


def load():
    """Load libmirx.so once; raise MirxError with build instructions when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirxError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {os.path.join(_HERE, 'csrc')}` (needs hipcc; there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise MirxError(f"libmirx.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mirx_version() != ABI_VERSION:
        raise MirxError(f"{LIB_PATH} is ABI version {lib.mirx_version()}, this package binds version {ABI_VERSION}: "
                        f"rebuild with `make -C {os.path.join(_HERE, 'csrc')}`")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mirx_last_error()
        raise MirxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
