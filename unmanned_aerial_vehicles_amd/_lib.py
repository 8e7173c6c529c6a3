"""ctypes binding of libgpk.so (include/gpk.h).  No torch types cross this boundary:
device buffers are passed as integer addresses (`torch.Tensor.data_ptr()`), host arrays as
`numpy` double pointers.

The library is mandatory: if it is missing or cannot be loaded this module raises — there is
no CPU fallback for the product path.
"""
import ctypes as C
import os

import numpy as np

from ._build import LIB_PATH

GPK_F32, GPK_F64 = 0, 1
GPK_OK, GPK_NOT_PD, GPK_BAD_ARG, GPK_HIP_ERROR = 0, 1, 2, 3
GPK_TILE, GPK_MAX_D, GPK_MAX_P = 128, 64, 16
GPK_HOST_MAX_M = 4096
GPK_TIMED_K5, GPK_TIMED_GRAM, GPK_TIMED_GRAD, GPK_TIMED_POTRF = 1, 2, 3, 4
GPK_TIMED_COV = 5
GPK_TIMED_JAC = 6
GPK_TIMED_SPARSE_STATS, GPK_TIMED_SPARSE_PASS = 7, 8
GPK_TIMED_PROPAGATE = 9

_vp, _i64, _int, _dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
_dp = C.POINTER(C.c_double)
_f64 = np.dtype(np.float64)      # (a dtype instance: comparing against the type object costs several times as much)

# name -> (restype, argtypes); mirrors include/gpk.h one to one
SIGNATURES = {
    "gpk_create": (_int, [C.POINTER(_vp), _int]),
    "gpk_destroy": (None, [_vp]),
    "gpk_last_error": (C.c_char_p, [_vp]),
    "gpk_set_stream": (_int, [_vp, _vp]),
    "gpk_synchronize": (_int, [_vp]),
    "gpk_padded": (_i64, [_i64]),
    "gpk_fit": (_int, [_vp, _dp, _i64, _int, _dp, _int, _dp, _int, _dbl, _dbl, _dbl, _int]),
    "gpk_predict": (_int, [_vp, _vp, _i64, _vp, _vp, _int, _int]),
    "gpk_lml": (_int, [_vp, _dp, _int, _dp, _dp]),
    "gpk_fit_batched": (_int, [_vp, _int, _dp, _i64, _int, _dp, _dp, _int, _dp, _dp, _dbl, _int, C.POINTER(C.c_int)]),
    "gpk_predict_batched": (_int, [_vp, _dp, _i64, _dp, _dp, _int]),
    "gpk_lml_batched": (_int, [_vp, _dp, _int, _dp, _dp]),
    "gpk_export": (_int, [_vp, C.POINTER(_i64), C.POINTER(_int), C.POINTER(_int), _dp, _dp, _dp, _dp, _dp]),
    "gpk_import": (_int, [_vp, _dp, _i64, _int, _dp, _dp, _int, _dp, _int, _dbl, _dbl, _dp, _dp]),
    "gpk_model_release": (_int, [_vp]),
    "gpk_split2_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "gpk_split2_rows_f64": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "gpk_split2_rows_f64_absmax": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "gpk_predict_var_inv_split2": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64, _vp, _i64, _dbl, _dbl, _vp, _vp]),
    "gpk_predict_mean_var_split2": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dbl, _dp, _dp, _dp, _vp, _vp, _i64, _vp, _i64,
                                           _dbl, _dbl, _vp, _vp, _dbl, _vp, _vp]),
    "gpk_pack_mean_var": (_int, [_vp, _int, _vp, _vp, _i64, _int, _dp, _vp]),
    "gpk_set_option": (_int, [_vp, C.c_char_p, _int]),
    "gpk_set_option_str": (_int, [_vp, C.c_char_p, C.c_char_p]),
    "gpk_timing": (_int, [_vp, _int]),
    "gpk_kernel_times": (_int, [_vp, _int, _dp, _int, C.POINTER(_int)]),
    "gpk_batch_begin": (_int, [_vp, _int]),
    "gpk_batch_buffer": (_int, [_vp, _vp, _i64]),
    "gpk_batch_end": (_int, [_vp]),
    "gpk_version": (C.c_char_p, []),
    "gpk_gram": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _dbl, _vp, _i64]),
    "gpk_gram_rows": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _dbl, _i64, _i64, _vp, _i64]),
    "gpk_cross_gram_t": (_int, [_vp, _int, _vp, _i64, _vp, _i64, _int, _dp, _dbl, _vp, _i64]),
    "gpk_rbf_kernel_grad": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64]),
    "gpk_potrf": (_int, [_vp, _vp, _i64, _i64, _vp, C.POINTER(_int)]),
    "gpk_leaf_inverses": (_int, [_vp, _vp, _i64, _i64, _vp]),
    "gpk_factor_to_f32": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "gpk_potrs": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _int, _vp]),
    "gpk_potrs_inv": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _int, _vp]),
    "gpk_wtw": (_int, [_vp, _vp, _i64, _i64, _vp, _i64]),
    "gpk_trsm_lower_left": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _vp, _i64, _i64]),
    "gpk_colsumsq": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp]),
    "gpk_predict_mean": (_int, [_vp, _int, _vp, _vp, _i64, _int, _int, _dp, _dbl, _dp, _dp, _vp, _i64, _vp]),
    "gpk_split3": (_int, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "gpk_predict_var_inv_split": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _vp, _i64, _dbl, _dbl, _vp, _vp, _vp]),
    # (host pointers as void*: the serving path passes cached integer addresses)
    "gpk_predict_host": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _dbl, _vp, _vp, _vp, _i64, _i64, _dbl, _dbl, _vp,
                                _i64, _vp, _vp]),
    "gpk_predict_host_multi": (_int, [_vp, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _dbl, _vp,
                                      _i64, _vp, _vp]),
    "gpk_predict_mean_mfma": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dbl, _dp, _dp, _dp, _vp, _i64, _vp]),
    "gpk_predict_mean_multi": (_int, [_vp, _int, _vp, _vp, _i64, _int, _int, _dp, _dp, _dp, _dp, _vp, _i64, _vp]),
    "gpk_predict_var": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _i64, _vp, _vp, _i64, _dbl,
                               _dbl, _vp, _vp]),
    "gpk_trtri": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "gpk_trtri_absmax": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "gpk_tril_to_f32": (_int, [_vp, _vp, _i64, _i64, _vp, _i64]),
    "gpk_predict_var_inv": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _i64, _vp, _i64, _dbl, _dbl,
                                   _vp, _vp]),
    "gpk_predict_cov_inv": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _i64, _vp, _i64, _dbl, _vp, _vp,
                                   _i64]),
    "gpk_predict_cov": (_int, [_vp, _int, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _i64, _vp, _vp, _i64, _dbl, _vp, _vp,
                               _i64]),
    "gpk_predict_host_cov": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _dbl, _vp, _vp, _vp, _i64, _i64, _dbl, _vp, _i64,
                                    _vp, _vp]),
    "gpk_predict_model_cov": (_int, [_vp, _dp, _i64, _dp, _dp]),
    # (host pointers as void*, as gpk_predict_host_multi)
    "gpk_predict_host_multi_cov": (_int, [_vp, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64,
                                          _vp, _vp]),
    "gpk_predict_batched_cov": (_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpk_predict_mean_grad": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dbl, _dp, _vp, _i64, _vp]),
    "gpk_predict_var_grad_inv": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _i64, _i64, _vp, _i64, _dbl, _dbl, _vp, _vp, _vp]),
    # (host pointers as void*, as gpk_predict_host)
    "gpk_predict_host_grad": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _dbl, _vp, _vp, _vp, _i64, _i64, _dbl, _dbl, _vp,
                                     _i64, _vp, _vp, _vp, _vp]),
    "gpk_predict_model_grad": (_int, [_vp, _dp, _i64, _dp, _dp, _dp, _dp, _int]),
    # (host pointers as void*, as gpk_predict_host_multi)
    "gpk_predict_host_multi_grad": (_int, [_vp, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _dbl, _vp,
                                           _i64, _vp, _vp, _vp, _vp]),
    "gpk_predict_mean_grad_multi": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dp, _dp, _vp, _i64, _vp]),
    "gpk_predict_batched_grad": (_int, [_vp, _dp, _i64, _dp, _dp, _dp, _dp, _int]),
    # the mean's input Hessian: the gradient entries' arguments without the variance ones, hess last
    "gpk_predict_mean_hess": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dbl, _dp, _vp, _i64, _vp]),
    "gpk_predict_host_hess": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _dbl, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gpk_predict_host_multi_hess": (_int, [_vp, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gpk_predict_mean_hess_multi": (_int, [_vp, _vp, _vp, _i64, _int, _int, _dp, _dp, _dp, _vp, _i64, _vp]),
    "gpk_predict_model_hess": (_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpk_predict_batched_hess": (_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpk_sparse_predict_hess": (_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpk_sparse_predict_multi_hess": (_int, [_vp, _int, C.POINTER(_vp), _dp, _i64, _dp, _dp, _dp]),
    "gpk_lml_terms": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _int, _dp]),
    "gpk_potri": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "gpk_lml_grad": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _dbl, _vp, _int, _vp, _i64, _dp]),
    "gpk_lml_eval": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _dbl, _dbl, _vp, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _dp, _dp,
                            C.POINTER(C.c_int)]),
    "gpk_sparse_accumulate": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dbl, _vp, _i64]),
    "gpk_sparse_accumulate_fitc": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dbl, _vp, _i64, _vp, _i64, _dbl, _vp, _vp]),
    "gpk_sparse_set_approximation": (_int, [_vp, _int, C.POINTER(_int)]),
    "gpk_sparse_get_approximation": (_int, [_vp, C.POINTER(_int), _dp]),
    "gpk_sparse_restore_approximation": (_int, [_vp, _int, _dbl, C.POINTER(_int)]),
    "gpk_sparse_grad_pass": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dbl, _vp, _i64, _vp]),
    "gpk_sparse_zgrad_pass": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dbl, _vp, _i64, _vp]),
    "gpk_sparse_hold": (_int, [_vp, _dp, _dp, _i64]),
    "gpk_sparse_eval": (_int, [_vp, _dp, _int, _dbl, _dbl, _dp, _dp, C.POINTER(_int)]),
    "gpk_sparse_eval_z": (_int, [_vp, _dp, _dp, _int, _dbl, _dbl, _dp, _dp, _dp, C.POINTER(_int)]),
    "gpk_greedy_select_bytes": (C.c_size_t, [_i64, _i64]),
    "gpk_greedy_select": (_int, [_vp, _vp, _i64, _int, _dp, _int, _dbl, _i64, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "gpk_sparse_select": (_int, [_vp, _dp, _i64, _i64, _dbl, _dbl, C.POINTER(_i64), _dp, _dp, C.POINTER(_i64)]),
    "gpk_sparse_begin": (_int, [_vp, _dp, _i64, _int, _int, _dp, _int, _dbl, _dbl, _dbl, _dbl, _dp, _dp]),
    "gpk_sparse_update": (_int, [_vp, _dp, _dp, _i64]),
    "gpk_sparse_finalize": (_int, [_vp, C.POINTER(_int)]),
    "gpk_sparse_predict": (_int, [_vp, _dp, _i64, _dp, _dp, _int]),
    "gpk_sparse_predict_grad": (_int, [_vp, _dp, _i64, _dp, _dp, _dp, _dp, _int]),
    "gpk_sparse_predict_cov": (_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpk_sparse_predict_multi": (_int, [_vp, _int, C.POINTER(_vp), _dp, _i64, _dp, _dp, _int]),
    "gpk_sparse_predict_multi_grad": (_int, [_vp, _int, C.POINTER(_vp), _dp, _i64, _dp, _dp, _dp, _dp, _int]),
    "gpk_sparse_predict_multi_cov": (_int, [_vp, _int, C.POINTER(_vp), _dp, _i64, _dp, _dp]),
    "gpk_sparse_bound": (_int, [_vp, _dp, C.POINTER(_i64)]),
    "gpk_sparse_export": (_int, [_vp, C.POINTER(_i64), C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), _dp, _dp, _dp, _dp,
                                 C.POINTER(_i64), _dp, _dp, _dp, _dp]),
    "gpk_sparse_import": (_int, [_vp, _dp, _i64, _int, _int, _dp, _int, _dbl, _dbl, _dbl, _dbl, _dp, _dp, _dp, _dp, _dp, _i64]),
    "gpk_gemm_tiles": (_int, [_vp, _int, _int, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _dbl,
                              _dbl, _int]),
    "gpk_rff_features": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _i64, _dbl, _vp, _i64]),
    "gpk_paths_prepare": (_int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _i64, _i64, _vp, _vp, _i64, _dbl, _vp, _vp, _int, _vp, _i64]),
    "gpk_paths_step": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp]),
    "gpk_paths_rollout": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dp, _dp, _int, _dp,
                                 _int, _dp, _dp]),
    "gpk_paths_step_multi": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp, _vp, _vp]),
    "gpk_paths_rollout_multi": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp, _int,
                                       C.POINTER(_int), _dp, _dp, _dp, _int, _dp, _int, _dp, _dp]),
    "gpk_sparse_paths_prepare": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _int, _vp, _i64, _vp]),
    "gpk_paths_step_multi_z": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp, _vp, _vp]),
    "gpk_paths_rollout_multi_z": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp, _int,
                                         C.POINTER(_int), _dp, _dp, _dp, _int, _dp, _int, _dp, _dp]),
    # the gradient forms: the value entry's arguments, then jac
    "gpk_paths_step_grad": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _vp]),
    "gpk_paths_rollout_grad": (_int, [_vp, _vp, _i64, _int, _dp, _dbl, _vp, _vp, _i64, _vp, _i64, _int, _int, _dp, _dp, _dp, _int,
                                      _dp, _int, _dp, _dp, _dp]),
    "gpk_paths_step_multi_grad": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp, _vp,
                                         _vp, _vp]),
    "gpk_paths_rollout_multi_grad": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp,
                                            _int, C.POINTER(_int), _dp, _dp, _dp, _int, _dp, _int, _dp, _dp, _dp]),
    "gpk_paths_step_multi_grad_z": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp,
                                           _vp, _vp, _vp]),
    "gpk_paths_rollout_multi_grad_z": (_int, [_vp, _vp, _i64, _int, _int, _dp, _dp, _vp, _vp, _i64, _vp, _i64, _i64, _int, _dp, _dp,
                                              _int, C.POINTER(_int), _dp, _dp, _dp, _int, _dp, _int, _dp, _dp, _dp]),
    # horizon propagation (host pointers as void*, as gpk_predict_host_grad / gpk_predict_host_multi_grad): the model, kss, floor,
    # var_includes_noise, noise, [nx, coord, in_shift, in_scale,] x0, rows, U, rows, lin, Sigma0, rows, Q, R, H, the five outputs
    "gpk_propagate_host": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, _dbl, _vp, _vp, _vp, _i64, _i64, _dbl, _dbl, _int, _dbl,
                                  _vp, _int, _vp, _int, _vp, _vp, _int, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "gpk_propagate_host_multi": (_int, [_vp, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _dbl, _int, _vp,
                                        _int, C.POINTER(_int), _vp, _vp, _vp, _int, _vp, _int, _vp, _vp, _int, _vp, _int, _int,
                                        _vp, _vp, _vp, _vp, _vp]),
    # ... on the sparse posteriors: var_includes_noise, [nx, coord, in_shift, in_scale, out_shift, out_scale,] then as above
    "gpk_sparse_propagate": (_int, [_vp, _int, _dp, _int, _dp, _int, _dp, _dp, _int, _dp, _int, _int, _dp, _dp, _dp, _dp, _dp]),
    "gpk_sparse_propagate_multi": (_int, [_vp, _int, C.POINTER(_vp), _int, _int, C.POINTER(_int), _dp, _dp, _dp, _dp, _dp, _int,
                                          _dp, _int, _dp, _dp, _int, _dp, _int, _int, _dp, _dp, _dp, _dp, _dp]),
}
# ... at second order in the mean: the four entries above with (order, corr) appended
SIGNATURES["gpk_propagate2_host"] = (_int, SIGNATURES["gpk_propagate_host"][1] + [_int, _vp])
SIGNATURES["gpk_propagate2_host_multi"] = (_int, SIGNATURES["gpk_propagate_host_multi"][1] + [_int, _vp])
SIGNATURES["gpk_sparse_propagate2"] = (_int, SIGNATURES["gpk_sparse_propagate"][1] + [_int, _dp])
SIGNATURES["gpk_sparse_propagate2_multi"] = (_int, SIGNATURES["gpk_sparse_propagate_multi"][1] + [_int, _dp])
# ... with the gradient of a horizon cost: the four first-order entries with (gx, gS, dU, dx0, dSigma0) appended
SIGNATURES["gpk_propagate_grad_host"] = (_int, SIGNATURES["gpk_propagate_host"][1] + [_vp] * 5)
SIGNATURES["gpk_propagate_grad_host_multi"] = (_int, SIGNATURES["gpk_propagate_host_multi"][1] + [_vp] * 5)
SIGNATURES["gpk_sparse_propagate_grad"] = (_int, SIGNATURES["gpk_sparse_propagate"][1] + [_dp] * 5)
SIGNATURES["gpk_sparse_propagate_grad_multi"] = (_int, SIGNATURES["gpk_sparse_propagate_multi"][1] + [_dp] * 5)
# exact moment matching: the chain takes the siblings' arguments with (Kinv, Np, ldk) in the place of (W, Np, ldw) and (mean, cov,
# xcov) in the place of (mean, var, jac); the query entries end with [nx, in_shift, in_scale,] Xq, Sq, M, mean, cov, xcov
SIGNATURES["gpk_propagate_mm_host"] = (_int, list(SIGNATURES["gpk_propagate_host"][1]))
SIGNATURES["gpk_propagate_mm_host_multi"] = (_int, list(SIGNATURES["gpk_propagate_host_multi"][1]))
SIGNATURES["gpk_moments_host"] = (_int, SIGNATURES["gpk_propagate_host"][1][:17] + [_int, _vp, _vp, _int, _vp, _vp, _vp])
SIGNATURES["gpk_moments_host_multi"] = (_int, SIGNATURES["gpk_propagate_host_multi"][1][:17]
                                        + [_int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp])
# ... with the adjoint of the moments: the query entries with (gmean, gcov, gxcov, dXq, dSq) appended, the chains with (gx, gS, dU,
# dx0, dSigma0) as the linear gradient entries
SIGNATURES["gpk_moments_vjp_host"] = (_int, SIGNATURES["gpk_moments_host"][1] + [_vp] * 5)
SIGNATURES["gpk_moments_vjp_host_multi"] = (_int, SIGNATURES["gpk_moments_host_multi"][1] + [_vp] * 5)
SIGNATURES["gpk_propagate_mm_grad_host"] = (_int, SIGNATURES["gpk_propagate_mm_host"][1] + [_vp] * 5)
SIGNATURES["gpk_propagate_mm_grad_host_multi"] = (_int, SIGNATURES["gpk_propagate_mm_host_multi"][1] + [_vp] * 5)
# ... on the sparse posteriors (the engine above on (Z, alpha_u, Q)): the chains take the arguments of gpk_sparse_propagate[_multi]
# with (mean, cov, xcov) as the stage outputs; the query entries: var_includes_noise, nx, [in_shift, in_scale, out_shift,
# out_scale,] Xq, Sq, M, mean, cov, xcov
SIGNATURES["gpk_sparse_propagate_mm"] = (_int, list(SIGNATURES["gpk_sparse_propagate"][1]))
SIGNATURES["gpk_sparse_propagate_mm_multi"] = (_int, list(SIGNATURES["gpk_sparse_propagate_multi"][1]))
SIGNATURES["gpk_sparse_moments"] = (_int, [_vp, _int, _int, _dp, _dp, _int, _dp, _dp, _dp])
SIGNATURES["gpk_sparse_moments_multi"] = (_int, [_vp, _int, C.POINTER(_vp), _int, _int, _dp, _dp, _dp, _dp, _dp, _dp, _int, _dp, _dp,
                                                 _dp])
# ... with their adjoint: (gmean, gcov, gxcov, dXq, dSq) behind the query entries, (gx, gS, dU, dx0, dSigma0) behind the chains
SIGNATURES["gpk_sparse_moments_vjp"] = (_int, SIGNATURES["gpk_sparse_moments"][1] + [_dp] * 5)
SIGNATURES["gpk_sparse_moments_vjp_multi"] = (_int, SIGNATURES["gpk_sparse_moments_multi"][1] + [_dp] * 5)
SIGNATURES["gpk_sparse_propagate_mm_grad"] = (_int, SIGNATURES["gpk_sparse_propagate_mm"][1] + [_dp] * 5)
SIGNATURES["gpk_sparse_propagate_mm_grad_multi"] = (_int, SIGNATURES["gpk_sparse_propagate_mm_multi"][1] + [_dp] * 5)

_lib = None


class GPKError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libgpk error {code}: {message}")
        self.code = code


class NotPositiveDefinite(np.linalg.LinAlgError):
    """Raised where the reference's LAPACK call raises `numpy.linalg.LinAlgError`
    (scipy.linalg.cholesky at sklearn/gaussian_process/_gpr.py:349)."""


def load():
    """Load libgpk.so and declare every prototype.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime (libamdhip64): it must be in the process BEFORE libgpk.so is
    # dlopen'ed, so that libgpk binds to that same runtime (one HIP context, shared streams and allocations).
    # Loading libgpk first would pull in the system runtime and leave torch without a usable device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("GPK_LIBRARY") or LIB_PATH      # GPK_LIBRARY: an experimental build (see _build.build)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the GP kernels)")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def dev_ptr(t):
    """Device tensor -> c_void_p (None: NULL).  The tensor must be contiguous and stay alive during the call."""
    return None if t is None else C.c_void_p(t.data_ptr())


def host_ptr(a):
    """Host array -> POINTER(c_double) (None: NULL).  Only a C-contiguous float64 ndarray is taken - anything else would
    hand the library an address it reads with the wrong strides or element size; the array must stay alive during the call."""
    if a is None:
        return None
    if not (isinstance(a, np.ndarray) and a.dtype == _f64 and a.flags.c_contiguous):
        raise TypeError("host_ptr takes a C-contiguous float64 ndarray, got "
                        + (f"{a.dtype} with strides {a.strides}" if isinstance(a, np.ndarray) else type(a).__name__))
    try:        # (through the buffer protocol: a third of the time of numpy's `ctypes.data_as`, and these run at the control rate)
        return _dp(C.c_double.from_buffer(a))
    except (TypeError, ValueError):     # a read-only or empty array has no writable buffer to export
        return a.ctypes.data_as(_dp)
