"""ctypes binding of ``libava_hip.so`` (C ABI declared in ``include/ava_hip.h``).

The library is the only compute backend of this package.  There is no CPU or
PyTorch fallback: if the shared object is missing or a call returns an error the
caller gets an exception.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# AVA_HIP_LIB_TAG=x loads csrc/libava_hip_x.so instead: same-box A/B of two builds (tools/lab/ab_prev.sh), nothing else
_TAG = os.environ.get("AVA_HIP_LIB_TAG", "")
LIB_PATH = os.path.join(CSRC, "libava_hip_%s.so" % _TAG if _TAG else "libava_hip.so")

_ERR = {-1: "AVA_EINVAL (bad argument / unsupported shape)", -2: "AVA_ELAUNCH (HIP launch failure)",
        -3: "AVA_EWORKSPACE (workspace too small)"}


class AvaHipError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"] + (["-B"] if force else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise AvaHipError("building libava_hip.so failed")
    return LIB_PATH


_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_f = C.c_float
_d = C.c_double
_sz = C.c_size_t

# name -> (restype, argtypes); mirrors include/ava_hip.h one to one
SIGNATURES = {
    "ava_version": (_i, []),
    "ava_arena_floats": (_i64, [_i]),
    "ava_param_offset": (_i64, [_i, _i, C.POINTER(_i64)]),
    "ava_workspace_bytes": (_sz, [_i, _i]),
    "ava_model_create": (_i, [C.POINTER(_p), _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _sz]),
    "ava_model_destroy": (None, [_p]),
    "ava_arena_floats_hw": (_i64, [_i, _i, _i]),
    "ava_param_offset_hw": (_i64, [_i, _i, _i, _i, C.POINTER(_i64)]),
    "ava_workspace_bytes_hw": (_sz, [_i, _i, _i, _i]),
    "ava_model_create_hw": (_i, [C.POINTER(_p), _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _sz]),
    "ava_model_create_ex": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _sz]),
    "ava_forward": (_i, [_p, _p, _i, _p, _p, _i, _p, _p, _p, _p]),
    "ava_forward_noise": (_i, [_p, _p, _i, _p, C.c_uint64, C.c_uint64, _i, _p, _p, _p, _p]),
    "ava_backward": (_i, [_p, _p, _i, _p]),
    "ava_set_backward_scale": (_i, [_p, _p]),
    "ava_backward_num_parts": (_i, []),
    "ava_backward_part": (_i, [_p, _p, _i, _i, _p]),
    "ava_grad_bucket": (_i, [_p, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "ava_adam_step": (_i, [_p, _d, _d, _d, _d, _i, _p]),
    "ava_adam_step_range": (_i, [_p, _i64, _i64, _d, _d, _d, _d, _i, _p]),
    "ava_encode": (_i, [_p, _p, _i, _i, _p, _p, _p, _p]),
    "ava_decode": (_i, [_p, _p, _i, _i, _p, _p]),
    "ava_last_z": (_p, [_p]),
    "ava_last_xrec": (_p, [_p]),
    "ava_debug_buffer": (_p, [_p, C.c_char_p, C.POINTER(_i64)]),
    "ava_set_cu_reserve": (_i, [_i]),
    "ava_get_cu_reserve": (_i, []),
    "ava_model_set_cu_reserve": (_i, [_p, _i]),
    "ava_model_get_cu_reserve": (_i, [_p]),
    "ava_occupy_cus": (_i, [_i, _i, _f, _p]),
    "ava_profile_enable": (_i, [_p, _i]),
    "ava_profile_read": (_i, [_p, C.POINTER(_f), C.POINTER(_i)]),
    "ava_fill_normal": (_i, [_p, _i64, C.c_uint64, C.c_uint64, _p]),
    "ava_pack_conv_weight": (_i, [_p, _p, _i, _i, _i, _p]),
    "ava_conv_grid": (_i, [_i, _i, _i, _i]),
    "ava_conv3x3": (_i, [_p] * 13 + [_i] * 9 + [_f, _p]),
    "ava_conv3x3_wgrad": (_i, [_p] * 9 + [_i] * 7 + [_p]),
    "ava_conv_wgrad_grid": (_i, [_i, _i, _i, _i]),
    "ava_conv_wgrad_rows": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "ava_conv_fused_grid": (_i, [_i, _i, _i, _i, _i, _i]),
    "ava_conv3x3_bwd_fused": (_i, [_p] * 14 + [_i] * 7 + [_p]),
    "ava_conv_wgrad_reduce": (_i, [_p, _i, _p, _p, _i, _i, _i, _p]),
    "ava_bn_stats": (_i, [_p, _i64, _i, _p, C.POINTER(_i), _p]),
    "ava_bn_finalize": (_i, [_p, _i, _i64, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p]),
    "ava_bn_finalize_bwd": (_i, [_p, _i, _i64, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ava_acc_shards": (_i, []),
    "ava_acc_shard_ll": (_i, []),
    "ava_layout_nchw_to_nhwc_stats": (_i, [_p, _p, _p, _i, _p, _p, _p, _p, _i, _i, _i, C.POINTER(_i), _p]),
    "ava_layout_nhwc_to_nchw": (_i, [_p, _p, _i, _i, _p]),
    "ava_layout_relu_mask_to_nhwc": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "ava_layout_bn_bwd_apply_to_nchw": (_i, [_p] * 6 + [_i, _i, _i] + [_p] * 7 + [_d, _i, _i, _p]),
    "ava_layout_scale_backward_roots": (_i, [_p, _i64, _p, _i64, _p, _p, _p]),
    "ava_gemm_workspace_bytes": (_sz, [_i, _i, _i]),
    "ava_gemm": (_i, [_p, _i, _p, _i, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "ava_gemm_path": (_i, [_p, _i, _p, _i, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "ava_latent_fwd": (_i, [_p] * 9 + [_i, _i, _p]),
    "ava_latent_bwd": (_i, [_p] * 9 + [_i, _i, _p]),
    "ava_elbo_finalize": (_i, [_p, _i, _p, _i, _i, _f, _p, _p]),
    "ava_adam_flat": (_i, [_p, _p, _p, _p, _i64, _d, _d, _d, _d, _i, _p]),
    "ava_cast_to_f32": (_i, [_p, _i, _i64, _p, _p]),
    "ava_host_gather_rows": (_i, [_p, _p, _p, _i64, _i64, _sz, _i]),
    "ava_gather_rows_f32": (_i, [_p, _i, _i64, _i64, _p, _i64, _p, _p]),
    "ava_mmd2_matrix_workspace_bytes": (_sz, [_p, _i, _i]),
    "ava_mmd2_matrix": (_i, [_p, _i, _p, _p, _p, _i, _p, _i64, _d, _p, _p, _p, _sz, _p]),
    "ava_mmd2_matrix_linear": (_i, [_p, _i, _p, _p, _p, _i, _p, _i64, _d, _p, _p, _sz, _p]),
    "ava_mmd2_perm_tile": (_i, []),
    "ava_mmd2_perm_workspace_bytes": (_sz, [_p, _i, _i]),
    "ava_mmd2_perm_membership": (_i, [_p, _p, _i, _i64, _i64, C.c_uint64, _p, _p]),
    "ava_mmd2_perm": (_i, [_p, _i, _p, _i64, _p, _p, _i, _i64, _i64, C.c_uint64, _d, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_pair_sqdist": (_i, [_p, _i, _p, _p, _i, _p, _p]),
    "ava_spec_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "ava_get_spec_batch": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _d, _i, _i, _p, _d, _p, _i, _i, _d, _d, _d, _i,
                                _i, _i, _d, _p, _p, _p, _sz, _p]),
    "ava_amp_workspace_bytes": (_sz, [_i64]),
    "ava_amp_trace": (_i, [_p, _i, _p, _p, _p, _i, _i64, _i, _i, _p, _d, _i, _i, _d, _d, _i, _d, _p, _i, _i, _p, _p, _p,
                           _sz, _p]),
    "ava_amp_decide": (_i, [_p, _i, _p, _i, _i64, _d, _d, _d, _p, _p, _p, _p, _i64, _p]),
    "ava_tpl_workspace_bytes": (_sz, [_i64]),
    "ava_tpl_tile_lags": (_i, []),
    "ava_tpl_spec": (_i, [_p, _i, _p, _p, _p, _i, _i64, _i, _i, _p, _d, _i, _i, _d, _d, _p, _p, _p]),
    "ava_tpl_xcorr": (_i, [_p, _p, _i, _i64, _p, _p, _p, _i, _i64, _i64, _p, _i, _i, _p, _p, _sz, _p]),
    "ava_warp_cache_bytes": (_sz, [_i, _d, _d, _i, _i, _d, _d]),
    "ava_warp_cache_layout": (_i, [_i, _d, _d, _i, _i, _d, _d, C.POINTER(_i64)]),
    "ava_warp_cache_workspace_bytes": (_sz, [_i, _d, _d, _i, _i]),
    "ava_warp_cache_build": (_i, [_p, _i, _p, _p, _i, _d, _d, _i, _i, _p, _d, _d, _d, _i, _p, _sz, _p, _sz, _p]),
    "ava_warp_windows_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ava_warp_windows": (_i, [_p, _sz, _i, _d, _d, _i, _i, _d, _d, _p, _p, _i, _p, _i, _i, _d, _d, _d, _i, _i, _d, _p, _p,
                              _sz, _p]),
    "ava_warp_band_spec": (_i, [_p, _i, _p, _p, _p, _i, _i64, _i, _i, _p, _d, _i, _i, _d, _d, _p, _p, _p]),
    "ava_warpfit_max_t": (_i, []),
    "ava_warpfit_apply": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
    "ava_warpfit_mean": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "ava_warpfit_candidates": (_i, [_p, _i, _i, _i, _i, _d, _d, _p, _p]),
    "ava_warpfit_loss": (_i, [_p, _i, _i, _i, _i, _p, _p, _i, _d, _d, _p, _p]),
    "ava_warpfit_argmin": (_i, [_p, _p, _i, _i, _p, _p, _p, _p]),
    "ava_warpfit_max_knots": (_i, []),
    "ava_warpfit_pl_apply": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _p]),
    "ava_warpfit_pl_candidates": (_i, [_p, _i, _i, _i, _i, _d, _p, _p]),
    "ava_warpfit_pl_loss": (_i, [_p, _i, _i, _i, _i, _p, _p, _i, _i, _d, _d, _p, _p]),
    "ava_warpfit_pl_argmin": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "ava_warpfit_group_loss": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _p, _p, _i, _i, _p, _p]),
    "ava_warpfit_group_pl_loss": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _i, _p, _p, _i, _i, _p, _p]),
    "ava_warpfit_group_mean": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _i, _p, _i, _p, _p]),
    "ava_warpfit_group_pl_mean": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _i, _p, _i, _i, _p, _p]),
    "ava_shiftfit_max_t": (_i, []),
    "ava_shiftfit_workspace_bytes": (_sz, [_i, _i, _i]),
    "ava_shiftfit_template": (_i, [_p, _i, _i, _i, _i, _p, _d, _d, _p, _p, _p, _sz, _p]),
    "ava_shiftfit_loss": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _p]),
    "ava_shiftfit_argmin": (_i, [_p, _i, _i, _p, _p, _p]),
    "ava_shiftfit_apply": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
    "ava_nn_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ava_nn_argmin": (_i, [_p, _i, _i, _p, _i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "ava_nn_merge": (_i, [_p, _p, _p, _p, _i, _i64, _i, _p]),
    "ava_pj_knn": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ava_pj_smooth": (_i, [_p, _p, _i, _i, _d, _p, _p, _p, _p, _p]),
    "ava_pj_layout": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i64, _i, _i, _i, _d, _d, _d, _d, C.c_uint64, _p, _p]),
    "ava_pj_knn_query": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ava_pj_row_stats": (_i, [_p, _i, _i, _i, _p, _p]),
    "ava_pj_knn_corr": (_i, [_p, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ava_pj_knn_corr_query": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ava_pj_smooth_bipartite": (_i, [_p, _p, _i, _i, _d, _p, _p, _p, _p, _p]),
    "ava_pj_transform_init": (_i, [_p, _p, _p, _i, _i, _p, _p, _p]),
    "ava_pj_transform_layout": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _d, _d, _d, C.c_uint64, _p, _p]),
    "ava_pj_gram_workspace_bytes": (_sz, [_i, _i]),
    "ava_pj_gram": (_i, [_p, _i, _i, _i, _p, _p, _sz, _p]),
    "ava_pj_project": (_i, [_p, _i, _i, _i, _p, _p, _i, _p, _p]),
    "ava_ts_max_n": (_i, []),
    "ava_ts_col_chunks": (_i, [_i]),
    "ava_ts_workspace_bytes": (_sz, [_i, _i]),
    "ava_ts_sqdist": (_i, [_p, _i, _i, _i, _i, _p, _i, _p]),
    "ava_ts_square": (_i, [_p, _i, _p, _i, _p]),
    "ava_ts_joint": (_i, [_p, _i, _i, _d, _p, _sz, _p]),
    "ava_ts_kl_gradient": (_i, [_p, _p, _i, _i, _d, _i, _p, _p, _p, _sz, _p]),
    "ava_ts_descend": (_i, [_p, _p, _p, _p, _i, _i, _i, _d, _d, _d, _i, _p, _p, _sz, _p]),
    "ava_gm_max_d": (_i, []),
    "ava_gm_max_k": (_i, []),
    "ava_gm_chunk_rows": (_i, []),
    "ava_gm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ava_gm_e_step": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ava_gm_means": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_gm_m_step": (_i, [_p, _i, _i, _i, _i, _i, _p, _d, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_gm_fit": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _d, _d, _i, _i, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_gm_onehot": (_i, [_p, _p, _i, _i, _p, _p, _p]),
    "ava_sil_max_k": (_i, []),
    "ava_sil_chunk_cols": (_i, []),
    "ava_sil_workspace_bytes": (_sz, [_i, _i, _i]),
    "ava_sil_cluster_sums": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "ava_sil_cluster_sums_pre": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "ava_sil_finish": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_sil_centroid_stats": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_db_max_eps": (_i, []),
    "ava_db_workspace_bytes": (_sz, [_i, _i, _i]),
    "ava_db_counts": (_i, [_p, _i, _i, _i, _p, _i, _p, _p]),
    "ava_db_counts_pre": (_i, [_p, _i, _i, _p, _i, _p, _p]),
    "ava_db_union": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _sz, _p]),
    "ava_db_union_pre": (_i, [_p, _i, _i, _p, _i, _i, _p, _p, _sz, _p]),
    "ava_db_assign": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_db_assign_pre": (_i, [_p, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_db_labels": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_db_labels_pre": (_i, [_p, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_hd_workspace_bytes": (_sz, [_i, _i]),
    "ava_hd_max_rounds": (_i, [_i]),
    "ava_hd_core": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    "ava_hd_core_pre": (_i, [_p, _i, _i, _i, _p, _p]),
    "ava_hd_mst": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_hd_mst_pre": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_hd_tree": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "ava_kp_max_sweep": (_i, []),
    "ava_kp_max_classes": (_i, []),
    "ava_kp_max_outputs": (_i, []),
    "ava_kp_knn_masked": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p]),
    "ava_kp_vote": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _p, _p]),
    "ava_kp_proba": (_i, [_p, _p, _i, _i, _p, _i, _i, _p, _p]),
    "ava_kp_regress": (_i, [_p, _p, _i, _i, _p, _i, _p, _i, _i, _p, _p]),
    "ava_km_max_d": (_i, []),
    "ava_km_max_k": (_i, []),
    "ava_km_chunk_rows": (_i, []),
    "ava_km_workspace_bytes": (_sz, [_i, _i, _i]),
    "ava_km_assign": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_km_update": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "ava_km_fit": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _d, _p, _i, _i, _p, _p, _p, _sz, _p]),
    "ava_km_pp_start": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "ava_km_pp_step": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ava_km_variance": (_i, [_p, _i, _i, _i, _p, _p, _sz, _p]),
    "ava_km_transform": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
}

# the embedding-quality entry points (row f26); mirrors include/ava_embed_quality.h one to one
EQ_SIGNATURES = {
    "ava_eq_max_targets": (_i, []),
    "ava_eq_max_sweep": (_i, []),
    "ava_eq_workspace_bytes": (_sz, [_i, _i]),
    "ava_eq_ranks": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _sz, _p]),
    "ava_eq_penalties": (_i, [_p, _i, _i, C.POINTER(_i), _i, _p, _p, _p]),
    "ava_eq_overlap": (_i, [_p, _p, _i, _i, C.POINTER(_i), _i, _p, _p, _p]),
}

# the sparse-graph components and eigensolver entry points (row f27); mirrors include/ava_spectral.h one to one
SP_SIGNATURES = {
    "ava_sp_max_n": (_i, []),
    "ava_sp_max_basis": (_i, []),
    "ava_sp_chunk_rows": (_i, []),
    "ava_sp_rotate_tile": (_i, []),
    "ava_sp_workspace_bytes": (_sz, [_i, _i]),
    "ava_sp_components": (_i, [_p, _p, _p, _i, _i64, _p, C.POINTER(_i), _p, _sz, _p]),
    "ava_sp_degrees": (_i, [_p, _p, _p, _i, _i64, _p, _p, _p, _sz, _p]),
    "ava_sp_apply": (_i, [_p, _p, _p, _p, _i, _i64, _p, _p, _p, _sz, _p]),
    "ava_sp_null_vectors": (_i, [_p, _p, _i, _i, _p, _i, _p, _sz, _p]),
    "ava_sp_start": (_i, [_p, _i, _i, _i, C.c_uint64, _d, _p, _p, _sz, _p]),
    "ava_sp_lanczos": (_i, [_p, _p, _p, _p, _i, _i64, _p, _i, _i, _i, _i, _d, _p, _p, _p, _sz, _p]),
    "ava_sp_rotate": (_i, [_p, _i, _i, _i, _i, _p, _p, _sz, _p]),
}

_lib = None


def load():
    """Load libava_hip.so (after torch, so that both share the HIP runtime torch ships)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AvaHipError(
            "%s not found: the HIP extension is the only backend of this package. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s`." % (LIB_PATH, CSRC))
    import torch  # noqa: F401  (loads torch's libamdhip64.so first; same SONAME as ROCm's)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(EQ_SIGNATURES.items()) + list(SP_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise AvaHipError("%s failed: %s" % (what, _ERR.get(rc, rc)))


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dtype_code(t):
    """the ABI's dtype argument of a tensor, an array, or a torch or numpy dtype: 0 for float32, 1 for float64"""
    dtype = getattr(t, "dtype", t)
    code = {"float32": 0, "float64": 1}.get(str(dtype).replace("torch.", ""))
    if code is None:
        raise AvaHipError("the kernels read float32 or float64 rows, got %s" % (dtype,))
    return code


def workspace(nbytes, dev, what):
    """``nbytes`` of device scratch (uint8), as an ``ava_*_workspace_bytes`` call sized it; that call answers 0 for a
    shape the entry points reject, which ``what`` describes in the error"""
    import torch
    if nbytes == 0:
        raise ValueError("unsupported shape: " + what)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def device(what):
    """the current GPU as a ``torch.device``; ``what`` names the caller's kernels in the error raised without one"""
    import torch
    if not torch.cuda.is_available():
        raise AvaHipError("the %s kernels only run on an MI355X: there is no CPU fallback in this package" % what)
    return torch.device("cuda", torch.cuda.current_device())
