"""ctypes binding of libwatroo_hip.so (C ABI: include/watroo_hip.h).

There is no CPU fallback: if the shared library is missing or no MI355X is visible the
import of the binding (or the first device call) raises.  numpy is the only dependency.
"""
import atexit
import ctypes
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WATROO_HIP_LIB", os.path.join(_HERE, "libwatroo_hip.so"))   # override: A/B builds

TRIANGLE, B3SPLINE = 0, 1
PLANE_INPUT, PLANE_OUT, PLANE_NONE = -1, -2, -1000
NUM_SCRATCH = 32
FLAG_FUSED, FLAG_NO_EXCHANGE, FLAG_SEPARATE_VARIANCE, FLAG_TAPS_REVERSED = 1, 2, 4, 8
FLAG_MEDIAN_HIST = 16     # wt_decompose_pass: the pass histograms |w_0| for the next wt_abs_median
PAD_POLY_SYMMETRIC, PAD_POLY_MIRROR = 5, 6     # wt_taps_conv_ex: the border rules of the recursive algorithm


def PLANE_SCRATCH(i):
    assert 0 <= i < NUM_SCRATCH
    return -3 - i


class WatrooHipError(RuntimeError):
    pass


_c = ctypes
_fp = _c.POINTER(_c.c_float)
_vp = _c.c_void_p
_i64 = _c.c_int64

# name -> (restype, argtypes); every symbol declared in include/watroo_hip.h
SIGNATURES = {
    "wt_abi_version": (_c.c_int, []),
    "wt_comm_version": (_c.c_int, [_c.POINTER(_c.c_int)]),
    "wt_unit_count": (_c.c_int, []),
    "wt_unit_name": (_c.c_char_p, [_c.c_int]),
    "wt_ctx_device_info": (_c.c_int, [_vp, _c.c_char_p, _c.c_int]),
    "wt_last_error": (_c.c_char_p, []),
    "wt_device_count": (_c.c_int, [_c.POINTER(_c.c_int)]),
    "wt_set_option": (_c.c_int, [_c.c_char_p, _c.c_int]),
    "wt_ctx_create": (_c.c_int, [_c.c_int, _c.POINTER(_vp)]),
    "wt_ctx_destroy": (_c.c_int, [_vp]),
    "wt_ctx_sync": (_c.c_int, [_vp]),
    "wt_device_memory": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_timer_start": (_c.c_int, [_vp]),
    "wt_timer_stop": (_c.c_int, [_vp, _c.POINTER(_c.c_float)]),
    "wt_profile_enable": (_c.c_int, [_vp, _c.c_int]),
    "wt_profile_reset": (_c.c_int, [_vp]),
    "wt_profile_count": (_c.c_int, [_vp, _c.POINTER(_c.c_int)]),
    "wt_profile_entry": (_c.c_int, [_vp, _c.c_int, _c.c_char_p, _c.POINTER(_i64),
                                    _c.POINTER(_c.c_double)]),
    "wt_comm_unique_id": (_c.c_int, [_vp]),
    "wt_ctx_comm_init": (_c.c_int, [_vp, _c.c_int, _c.c_int, _vp]),
    "wt_ctx_comm_info": (_c.c_int, [_vp, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "wt_comm_selftest": (_c.c_int, [_vp, _i64, _c.POINTER(_c.c_int)]),
    "wt_plan_create": (_c.c_int, [_vp, _i64, _i64, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_plan_create_placed": (_c.c_int, [_vp, _i64, _i64, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_plan_create_strip": (_c.c_int, [_vp, _i64, _i64, _c.c_int, _c.c_int, _i64, _i64, _i64,
                                        _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_plan_destroy": (_c.c_int, [_vp]),
    "wt_plan_info": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_plan_memory": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_plan_trim": (_c.c_int, [_vp]),
    "wt_ctx_scatter_status": (_c.c_int, [_vp, _c.POINTER(_c.c_int), _c.c_char_p, _c.c_int]),
    "wt_schedule": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.c_int,
                               _c.POINTER(_c.c_int)]),
    "wt_plan_set_border": (_c.c_int, [_vp, _c.c_int]),
    "wt_plan_set_taps": (_c.c_int, [_vp, _fp, _c.c_int]),
    "wt_crop_plane": (_c.c_int, [_vp, _c.c_int, _vp, _c.c_int, _i64, _i64]),
    "wt_paste_plane": (_c.c_int, [_vp, _c.c_int, _vp, _c.c_int, _i64, _i64]),
    "wt_copy_window": (_c.c_int, [_vp, _c.c_int, _vp, _c.c_int] + [_i64] * 6),
    "wt_plane_ptr": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_vp)]),
    "wt_host_alloc": (_c.c_int, [_vp, _c.c_size_t, _c.POINTER(_vp)]),
    "wt_host_free": (_c.c_int, [_vp]),
    "wt_upload": (_c.c_int, [_vp, _c.c_int, _fp, _i64]),
    "wt_upload_int": (_c.c_int, [_vp, _c.c_int, _vp, _i64, _c.c_int]),
    "wt_download": (_c.c_int, [_vp, _c.c_int, _fp, _i64]),
    "wt_copy_plane": (_c.c_int, [_vp, _c.c_int, _c.c_int]),
    "wt_fill_plane": (_c.c_int, [_vp, _c.c_int, _c.c_float]),
    "wt_fill_normal": (_c.c_int, [_vp, _c.c_int, _c.c_uint64, _c.c_uint32]),
    "wt_halo_exchange_local": (_c.c_int, [_vp, _vp, _c.c_int, _i64]),
    "wt_halo_exchange": (_c.c_int, [_vp, _c.c_int, _i64]),
    "wt_decompose": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose_pass": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose_pass_sum": (_c.c_int, [_vp] + [_c.c_int] * 8),
    "wt_decompose_sum_host": (_c.c_int, [_vp, _fp, _i64, _c.c_int, _c.c_int, _fp, _i64, _c.c_int]),
    "wt_denoise_sum_host": (_c.c_int, [_vp, _fp, _i64, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                       _c.POINTER(_c.c_double), _c.c_int, _c.c_int, _fp, _i64, _c.c_int]),
    "wt_plan_fused_ok": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_atrous_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_smooth": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_local_variance": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float,
                                     _c.c_int, _c.c_int]),
    "wt_bilateral_conv": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose_bilateral": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                          _c.c_int, _c.c_int]),
    "wt_plane_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_abs_median": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_float)]),
    "wt_significance": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int]),
    "wt_denoise": (_c.c_int, [_vp, _c.c_int, _c.c_double, _c.c_double, _c.c_int, _c.c_int]),
    "wt_denoise_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                  _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.c_int,
                                  _c.c_int, _c.c_int]),
    "wt_wow_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int,
                                 _c.c_float, _c.c_int]),
    "wt_wow_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int,
                                _c.c_float, _c.c_int, _c.c_int]),
    "wt_reduce": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt_gamma_blend": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_float,
                                  _c.c_float]),
    "wt_smooth3d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose3d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_decompose_cube": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_wow_cube_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_float, _c.c_int]),
    "wt_local_variance3d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float]),
    "wt_bilateral3d_conv": (_c.c_int, [_vp] + [_c.c_int] * 5),
    "wt_filter2d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _fp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_filter2d_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _fp] + [_c.c_int] * 6),
    "wt_binary": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_taps_conv": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _fp, _c.c_int,
                                _c.c_float, _c.c_int, _c.c_int, _c.c_int, _c.c_float]),
    "wt_taps_conv_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _fp, _c.c_int,
                                   _c.c_float, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_int]),
    "wt_variance_from_moments": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_int]),
    "wt_mrs_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int,
                                 _c.c_int, _c.c_float]),
    "wt_anscombe": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_float,
                               _c.c_int]),
    # float64 engine (wt_plan64)
    "wt64_plan_create": (_c.c_int, [_vp, _i64, _i64, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                    _c.POINTER(_vp)]),
    "wt64_plan_destroy": (_c.c_int, [_vp]),
    "wt64_plan_set_border": (_c.c_int, [_vp, _c.c_int]),
    "wt64_upload": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double), _i64]),
    "wt64_upload_int": (_c.c_int, [_vp, _c.c_int, _vp, _i64, _c.c_int]),
    "wt64_download": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double), _i64]),
    "wt64_decompose": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_decompose_cube": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_wow_cube_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_double, _c.c_int]),
    "wt64_decompose_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt64_smooth": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_local_variance": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                       _c.c_double, _c.c_int, _c.c_int]),
    "wt64_bilateral_conv": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int]),
    "wt_axis_filter": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.POINTER(_c.c_float), _c.c_int,
                                  _c.c_int, _c.c_int, _c.c_float, _c.c_int]),
    "wt64_axis_filter": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.POINTER(_c.c_double), _c.c_int,
                                    _c.c_int, _c.c_int, _c.c_double, _c.c_int]),
    "wt64_decompose_bilateral": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int]),
    "wt64_copy_window": (_c.c_int, [_vp, _c.c_int, _vp, _c.c_int, _i64, _i64, _i64, _i64, _i64,
                                    _i64]),
    "wt64_taps_conv": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32),
                                  _c.POINTER(_c.c_double), _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_double]),
    "wt64_taps_conv_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32),
                                     _c.POINTER(_c.c_double), _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_double, _c.c_int]),
    "wt64_variance_from_moments": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_int]),
    "wt64_abs_median": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt64_significance": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_int,
                                     _c.c_int, _c.c_int]),
    "wt64_plane_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_plane_sum_early": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt64_plane_sum_resume": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_plane_sum_early": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_plane_sum_resume": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_binary": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_anscombe": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_double,
                                 _c.c_int]),
    "wt64_wow_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int,
                                   _c.c_double, _c.c_int]),
    "wt64_wow_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_double, _c.c_int]),
    "wt64_gamma_blend": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_double,
                                    _c.c_double, _c.c_double]),
    "wt64_fill_plane": (_c.c_int, [_vp, _c.c_int, _c.c_double]),
    "wt_fft_supported": (_c.c_int, [_i64, _i64, _c.POINTER(_c.c_int)]),
    "wt_fft_spectrum": (_c.c_int, [_vp, _c.c_int]),
    "wt_fft_apply": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_fft_spectrum": (_c.c_int, [_vp, _c.c_int]),
    "wt64_fft_apply": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_decompose_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_plan_fused_ok": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt64_decompose_pass": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_decompose_pass_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int]),
    "wt64_denoise_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                    _c.POINTER(_c.c_double), _c.c_int, _c.c_int, _c.c_int]),
    "wt64_reduce": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt64_filter2d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                 _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt64_mrs_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int,
                                   _c.c_int, _c.c_double]),
    # batches of same-shape frames (wt_batch)
    "wt_batch_create": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_batch_destroy": (_c.c_int, [_vp]),
    "wt_batch_info": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_batch_upload": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _fp, _i64]),
    "wt_batch_download": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _fp, _i64]),
    "wt_batch_plane_ptr": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_vp), _c.POINTER(_i64)]),
    "wt_batch_decompose": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_decompose_bilateral": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                                _c.c_int, _c.c_int]),
    "wt_batch_decompose_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_decompose_pass": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_decompose_pass_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_abs_median": (_c.c_int, [_vp, _c.c_int, _c.c_int, _fp]),
    "wt_batch_denoise_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                        _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch_enhance_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                        _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch_denoise_sum_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                            _c.POINTER(_c.c_double), _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_replicate": (_c.c_int, [_vp, _c.c_int, _c.c_int]),
    "wt_batch_anscombe": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_float,
                                     _c.c_int]),
    "wt_batch_fill": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_float]),
    "wt_batch_fill_normal": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_uint64, _c.c_uint32]),
    "wt_batch_wow_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _fp, _c.c_int]),
    "wt_batch_wow_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _fp,
                                      _c.c_int]),
    "wt_batch_wow_update_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _fp, _c.c_int,
                                           _c.c_int]),
    "wt_batch_wow_scale_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _fp,
                                          _c.c_int, _c.c_int]),
    "wt_batch_reduce": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt_batch_gamma_blend": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _fp, _fp, _c.c_float, _c.c_float]),
    "wt_batch_plane_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_set_psf": (_c.c_int, [_vp, _c.c_int, _fp, _c.c_int, _c.c_int]),
    "wt_batch_psf_ok": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_batch_filter2d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_binary": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch_mrs_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _c.c_int,
                                       _c.c_float]),
    "wt_batch_fft_ok": (_c.c_int, [_i64, _i64, _c.POINTER(_c.c_int)]),
    "wt_batch_fft_spectrum": (_c.c_int, [_vp, _c.c_int]),
    "wt_batch_fft_apply": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    # batches of same-shape frames in float64 (wt_batch64)
    "wt_batch64_fused_ok": (_c.c_int, [_c.c_int, _i64, _i64, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_batch64_create": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_batch64_destroy": (_c.c_int, [_vp]),
    "wt_batch64_info": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_batch64_upload": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _i64]),
    "wt_batch64_download": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _i64]),
    "wt_batch64_upload_elems": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_int]),
    "wt_batch64_plane_ptr": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_vp), _c.POINTER(_i64)]),
    "wt_batch64_decompose": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_bilateral_ok": (_c.c_int, [_c.c_int, _i64, _i64, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_batch64_decompose_bilateral": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                                  _c.c_int, _c.c_int]),
    "wt_batch64_decompose_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_decompose_pass": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_decompose_pass_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                                 _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_abs_median": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt_batch64_denoise_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                          _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch64_enhance_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                          _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch64_denoise_sum_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                              _c.POINTER(_c.c_double), _c.c_int, _c.c_int, _c.c_int,
                                              _c.POINTER(_c.c_int)]),
    "wt_batch64_fill": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double]),
    "wt_batch64_replicate": (_c.c_int, [_vp, _c.c_int, _c.c_int]),
    "wt_batch64_anscombe": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_double,
                                       _c.c_int]),
    "wt_batch64_wow_ok": (_c.c_int, [_c.c_int, _i64, _i64, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_batch64_wow_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                         _c.POINTER(_c.c_double), _c.c_int]),
    "wt_batch64_wow_scale": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                        _c.POINTER(_c.c_double), _c.c_int]),
    "wt_batch64_wow_update_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                             _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch64_wow_scale_map": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                            _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch64_reduce": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt_batch64_gamma_blend": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double),
                                          _c.POINTER(_c.c_double), _c.c_double, _c.c_double]),
    "wt_batch64_plane_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_psf_ok": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "wt_batch64_set_psf": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _c.c_int]),
    "wt_batch64_filter2d": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_binary": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "wt_batch64_mrs_update": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int, _c.c_int,
                                         _c.c_double]),
    # stacks of 1-D signals of one length (wt_signals)
    "wt_signals_ok": (_c.c_int, [_c.c_int, _i64, _c.c_int, _c.c_int]),
    "wt_signals_create": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_signals_destroy": (_c.c_int, [_vp]),
    "wt_signals_info": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_signals_upload": (_c.c_int, [_vp, _c.c_int, _c.c_int, _vp]),
    "wt_signals_decompose": (_c.c_int, [_vp, _c.c_int, _c.c_int]),
    "wt_signals_decompose_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int]),
    "wt_signals_abs_median": (_c.c_int, [_vp, _c.c_int, _vp]),
    "wt_signals_denoise_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                          _c.c_int]),
    "wt_signals_denoise_sum_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                             _c.c_int, _c.c_int]),
    "wt_signals_moments": (_c.c_int, [_vp, _c.c_int, _c.POINTER(_c.c_double)]),
    "wt_signals_wow_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                      _c.c_int, _c.c_int, _c.c_int]),
    "wt_signals_download_planes":(_c.c_int, [_vp, _c.c_int, _c.c_int, _vp]),
    "wt_signals_download_sum": (_c.c_int, [_vp, _c.c_int, _c.c_int, _vp]),
    # the 1-D transform along an axis that is not the last one (wt_along)
    "wt_along_ok": (_c.c_int, [_c.c_int, _i64, _i64, _c.c_int, _c.c_int]),
    "wt_along_create": (_c.c_int, [_vp, _i64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_vp)]),
    "wt_along_destroy": (_c.c_int, [_vp]),
    "wt_along_info": (_c.c_int, [_vp, _c.POINTER(_i64)]),
    "wt_along_upload": (_c.c_int, [_vp, _c.c_int, _c.c_int, _vp, _i64]),
    "wt_along_decompose": (_c.c_int, [_vp, _c.c_int]),
    "wt_along_abs_median": (_c.c_int, [_vp, _vp]),
    "wt_along_abs_median_ex": (_c.c_int, [_vp, _vp, _c.c_int]),
    "wt_along_denoise": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.c_int]),
    "wt_along_denoise_ex": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.c_int,
                                       _c.c_int]),
    "wt_along_download_planes": (_c.c_int, [_vp, _vp, _i64, _i64]),
    "wt_along_download_sum": (_c.c_int, [_vp, _vp, _i64]),
    # arrays that stay on the device (wt_resident)
    "wt_device_alloc": (_c.c_int, [_vp, _c.c_size_t, _c.POINTER(_vp)]),
    "wt_device_free": (_c.c_int, [_vp, _vp]),
    "wt_device_copy": (_c.c_int, [_vp, _vp, _vp, _c.c_size_t, _c.c_int]),
    "wt_batch_load_device": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_int, _c.POINTER(_i64), _vp, _c.c_int]),
    "wt_batch_store_device": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.POINTER(_i64), _vp, _c.c_int]),
    "wt_batch64_load_device": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_int, _c.POINTER(_i64), _vp, _c.c_int]),
    "wt_batch64_store_device": (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _vp, _c.POINTER(_i64), _vp, _c.c_int]),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load libwatroo_hip.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise WatrooHipError(
                    f"{LIB_PATH} not found - the HIP engine is not built "
                    "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
                fn.restype, fn.argtypes = res, args
            if L.wt_abi_version() != 8:
                raise WatrooHipError("libwatroo_hip.so ABI version mismatch")
            _lib = L
    return _lib


def comm_version():
    """ncclGetVersion of the RCCL library the engine loads (0: unknown); loads the library."""
    v = _c.c_int(0)
    check(load().wt_comm_version(_c.byref(v)))
    return v.value


def unit_names():
    """the translation units of the library's device code, as its warm-up threads know them (host logic)"""
    L = load()
    return [L.wt_unit_name(i).decode() for i in range(L.wt_unit_count())]


def check(rc):
    if rc != 0:
        raise WatrooHipError(load().wt_last_error().decode("utf-8", "replace"))


def fft_supported(H, W):
    """True when an H x W image can take the FFT path of the circular products (powers of two, 2 .. 8192)."""
    ok = _c.c_int(0)
    check(load().wt_fft_supported(H, W, _c.byref(ok)))
    return bool(ok.value)


_option_values = {"scatter": int(os.environ.get("WT_SCATTER", "4")),      # options restored after a temporary change
                  "scatter_strips": int(os.environ.get("WT_SCATTER_STRIPS", "0"))}


def set_option(name, value):
    check(load().wt_set_option(name.encode(), int(value)))
    if name in _option_values:
        _option_values[name] = int(value)


def device_count():
    n = _c.c_int(0)
    check(load().wt_device_count(_c.byref(n)))
    return n.value


class Context:
    """One GPU + one HIP stream (+ optional RCCL communicator).  wt_ctx."""

    def __init__(self, device=0):
        self._h = _vp()
        self.device = device
        self.rank, self.nranks = 0, 1
        L = load()
        if device_count() == 0:
            raise WatrooHipError("no HIP device visible: the a-trous engine needs an MI355X "
                                 "(there is no CPU fallback) ["
                                 + L.wt_last_error().decode("utf-8", "replace") + "]")
        check(L.wt_ctx_create(device, _c.byref(self._h)))
        _live.add(self)

    def close(self):
        if self._h:
            load().wt_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(load().wt_ctx_sync(self._h))

    def device_memory(self):
        """(free, total) bytes of the device (hipMemGetInfo)."""
        out = (_i64 * 2)()
        check(load().wt_device_memory(self._h, out))
        return int(out[0]), int(out[1])

    def scatter_status(self):
        """(disabled, reason): whether this context has fallen back from planes over scattered
        chunks to plain hipMalloc, and the HIP call that failed when it did."""
        d = _c.c_int(0)
        buf = _c.create_string_buffer(256)
        check(load().wt_ctx_scatter_status(self._h, _c.byref(d), buf, 256))
        return bool(d.value), buf.value.decode("utf-8", "replace")

    def timer_start(self):
        check(load().wt_timer_start(self._h))

    def timer_stop(self):
        ms = _c.c_float(0)
        check(load().wt_timer_stop(self._h, _c.byref(ms)))
        return ms.value

    def profile(self, on):
        check(load().wt_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(load().wt_profile_reset(self._h))

    def profile_entries(self):
        """{kernel name: (calls, total_ms)} measured with HIP events on the launch stream."""
        L = load()
        n = _c.c_int(0)
        check(L.wt_profile_count(self._h, _c.byref(n)))
        out = {}
        for i in range(n.value):
            name = _c.create_string_buffer(64)
            calls, ms = _i64(0), _c.c_double(0)
            check(L.wt_profile_entry(self._h, i, name, _c.byref(calls), _c.byref(ms)))
            out[name.value.decode()] = (calls.value, ms.value)
        return out

    # ---- RCCL
    @staticmethod
    def unique_id():
        buf = _c.create_string_buffer(128)
        check(load().wt_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, nranks, unique_id):
        assert len(unique_id) == 128
        buf = _c.create_string_buffer(unique_id, 128)
        check(load().wt_ctx_comm_init(self._h, rank, nranks, buf))
        self.rank, self.nranks = rank, nranks

    def comm_info(self):
        """(rank, size) as the RCCL communicator reports them; (0, 1) without one."""
        r, n = _c.c_int(0), _c.c_int(1)
        check(load().wt_ctx_comm_info(self._h, _c.byref(r), _c.byref(n)))
        return r.value, n.value

    def device_info(self):
        """{'device': ordinal, 'pci': bus id, 'cus': compute units, 'name': ...} of this context's GPU"""
        buf = _c.create_string_buffer(256)
        check(load().wt_ctx_device_info(self._h, buf, 256))
        text = buf.value.decode("utf-8", "replace")
        head, _, name = text.partition(" name=")
        info = dict(kv.split("=", 1) for kv in head.split())
        return {"device": int(info.get("device", -1)), "pci": info.get("pci", "?"), "cus": int(info.get("cus", 0)), "name": name}

    def comm_selftest(self, nfloats=1 << 20):
        ok = _c.c_int(0)
        check(load().wt_comm_selftest(self._h, nfloats, _c.byref(ok)))
        return bool(ok.value)


_default_ctx = {}
_live = weakref.WeakSet()        # Plans and Contexts still holding device resources


@atexit.register
def _shutdown():
    """Release device resources while the HIP runtime is still alive (interpreter teardown
    otherwise destroys planes after the runtime's own static destructors ran)."""
    _host_pool.close()
    objs = list(_live)
    for kind in ((Plan, Plan64, BatchPlan, BatchPlan64, SignalBatch, AlongBatch), (Context,)):
        for o in objs:
            if isinstance(o, kind):
                try:
                    o.close()
                except Exception:           # (interpreter exit: report nothing, keep releasing)
                    pass
    _default_ctx.clear()
    _lane_ctx.clear()
    del _pool[:]
    for cache in (_batch_cache, _signal_cache, _along_cache):
        cache.lists.clear()


_tls = threading.local()          # .ctx: the context the API calls of THIS thread run on (use_context)
_lane_ctx = {}                    # device -> [Context]: the extra contexts of sequence.map_frames' worker lanes


class use_context:
    """`with use_context(ctx):` - the numpy-to-numpy calls of this thread (denoise, wow, AtrousTransform ...) run on
    `ctx` (its stream, its scratch, plans pooled under it) instead of the process-wide default context.  What the
    worker lanes of sequence.map_frames use: one context per lane, so that the upload of one frame, the passes of
    another and the download of a third overlap."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.prev = getattr(_tls, "ctx", None)
        _tls.ctx = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        _tls.ctx = self.prev
        return False


def lane_contexts(n, device=None):
    """`n` contexts of their own (HIP stream, scratch, warm-up) on `device`, created once per process and reused."""
    if device is None:
        device = int(os.environ.get("WATROO_HIP_DEVICE", "0"))
    with _pool_lock:
        lanes = _lane_ctx.setdefault(device, [])
        while len(lanes) < n:
            lanes.append(Context(device))
        return lanes[:n]


def default_context(device=None):
    """Process-wide context (device from WATROO_HIP_DEVICE, default 0); inside `use_context(ctx)`: that context."""
    if device is None:
        ctx = getattr(_tls, "ctx", None)
        if ctx is not None and ctx._h:
            return ctx
        device = int(os.environ.get("WATROO_HIP_DEVICE", "0"))
    ctx = _default_ctx.get(device)
    if ctx is None:
        with _pool_lock:
            ctx = _default_ctx.get(device)
            if ctx is None:
                ctx = _default_ctx[device] = Context(device)
    return ctx


def schedule(family, level, fused=True):
    """Pass schedule [(first_scale, n_scales, halo_rows)] - host logic, needs no GPU."""
    tr = (_c.c_int32 * (3 * 32))()
    n = _c.c_int(0)
    check(load().wt_schedule(family, level, int(fused), tr, 32, _c.byref(n)))
    return [(tr[3 * i], tr[3 * i + 1], tr[3 * i + 2]) for i in range(n.value)]


class _HostPool:
    """Page-locked host blocks behind the ndarrays handed back to the caller.

    A fresh pageable `np.empty` target costs one page fault per 4 KiB during the device-to-host
    copy (8192^2 float32: 17-31 ms instead of 4.7 ms at PCIe rate).  Results >= 1 MiB are
    therefore allocated with wt_host_alloc and wrapped as ordinary writable ndarrays; when the
    last view of such an array dies its block returns to this pool and backs the next result
    of the same size.  WATROO_HIP_HOST_POOL_MB bounds the idle bytes kept (default 4096;
    0 disables the mechanism: plain np.empty)."""

    MIN_BYTES = 1 << 20

    def __init__(self):
        self.lock = threading.Lock()
        self.idle = {}            # nbytes -> [address]
        self.idle_bytes = 0
        self.limit = int(os.environ.get("WATROO_HIP_HOST_POOL_MB", "4096")) << 20
        self.closed = False

    def empty(self, ctx, shape, dtype=np.float32):
        shape = tuple(int(n) for n in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        if self.limit == 0 or self.closed or nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype)
        nbytes = (nbytes + 65535) & ~65535
        addr = None
        with self.lock:
            lst = self.idle.get(nbytes)
            if lst:
                addr = lst.pop()
                self.idle_bytes -= nbytes
        if addr is None:
            ptr = _vp()
            if load().wt_host_alloc(ctx._h, nbytes, _c.byref(ptr)) != 0 or not ptr.value:
                return np.empty(shape, dtype)          # pinned memory exhausted: pageable
            addr = ptr.value
        block = (_c.c_char * nbytes).from_address(addr)
        weakref.finalize(block, self._give, addr, nbytes)
        n = int(np.prod(shape, dtype=np.int64))
        return np.frombuffer(block, dtype=dtype, count=n).reshape(shape)

    def _give(self, addr, nbytes):
        drop = []
        with self.lock:
            if self.closed:
                return                                  # interpreter exit: the OS reclaims it
            if nbytes > self.limit:
                drop.append(addr)
            else:
                while self.idle_bytes + nbytes > self.limit:
                    k = next(k for k, v in self.idle.items() if v)
                    drop.append(self.idle[k].pop())
                    self.idle_bytes -= k
                self.idle.setdefault(nbytes, []).append(addr)
                self.idle_bytes += nbytes
        for a in drop:
            load().wt_host_free(_vp(a))

    def close(self):
        with self.lock:
            self.closed = True
            blocks = [a for v in self.idle.values() for a in v]
            self.idle.clear()
            self.idle_bytes = 0
        for a in blocks:
            load().wt_host_free(_vp(a))


_host_pool = _HostPool()


def host_empty(shape, ctx=None, dtype=np.float32):
    """ndarray (float32 unless told otherwise) for a result coming back from the device (see _HostPool)."""
    return _host_pool.empty(ctx if ctx is not None else default_context(), shape, dtype)


# element types the device widens itself (wt_upload_int / wt64_upload_int): integers, bool (as uint8) and -
# in the other byte order only - float32 / float64 (FITS data is big-endian)
_ELEM_CODES = {"b1": 2, "i1": 1, "u1": 2, "i2": 3, "u2": 4, "i4": 5, "u4": 6, "i8": 7, "u8": 8, "f4": 9, "f8": 10}


def device_widens(dtype):
    """True for element types Plan.upload / Plan64.upload send over PCIe as they are."""
    dtype = np.dtype(dtype)
    if dtype.str[1:] not in _ELEM_CODES:
        return False
    return dtype.kind in "iub" or (dtype.kind == "f" and not dtype.isnative)


def _elem_source(host, shape):
    """(address, row pitch in bytes, type code) of a host image the device can widen, else None"""
    h = host
    if not device_widens(h.dtype) or h.ndim != 2 or h.shape != tuple(shape) or not h.size:
        return None
    if h.strides[1] != h.itemsize or h.strides[0] < h.shape[1] * h.itemsize:
        return None
    code = _ELEM_CODES[h.dtype.str[1:]]
    if not h.dtype.isnative and h.itemsize > 1:
        code |= 16                                       # WT_BYTESWAPPED
    return h.ctypes.data, h.strides[0], code


def _seed64(seed):
    """the 64-bit seed of the normal fill as an int, or ValueError"""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed: an integer in 0 .. 2**64-1 expected (got {seed!r})")
    return int(seed)


def _trial32(trial):
    """the trial number of the normal fill: counter word 2 is 32 bits wide"""
    if isinstance(trial, bool) or not isinstance(trial, (int, np.integer)) or not 0 <= int(trial) < 1 << 32:
        raise ValueError(f"trial: an integer in 0 .. 2**32-1 expected (got {trial!r})")
    return int(trial)


def _as_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("expected a 2-D image")
    return a


def _as_f32_rows(a):
    """float32 2-D array whose rows are contiguous (unit column stride, row stride a multiple of 4 bytes
    and >= the width): a row-strided view is handed to the library as it is (its row stride goes down
    as the host stride), anything else is copied"""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("expected a 2-D image")
    if a.dtype == np.float32 and a.shape[1] > 0 and a.strides[1] == 4 and a.strides[0] % 4 == 0 \
            and a.strides[0] >= 4 * a.shape[1]:
        return a
    return np.ascontiguousarray(a, dtype=np.float32)


class Plan:
    """Device planes of one image (or one row strip of it).  wt_plan."""

    cold = False             # True: created by the pool (acquire_plan), planes on plain hipMalloc

    def __init__(self, ctx, H, W, family, max_level, row0=0, nrows=None, halo_rows=0,
                 rank=0, nranks=1, scatter=None):
        self._h = _vp()
        self.ctx = ctx
        nrows = H if nrows is None else nrows
        # `family` is TRIANGLE / B3SPLINE, or a tuple of 1-D taps for a user-defined scaling
        # function (wt_plan_set_taps); the tuple is kept as self.family (plan-pool key)
        taps = tuple(float(t) for t in family) if isinstance(family, (tuple, list)) else None
        if scatter is not None and nranks == 1 and row0 == 0 and nrows == H:
            # placement of THIS plan's planes (0: plain hipMalloc), whatever the process-wide "scatter" option says
            check(load().wt_plan_create_placed(ctx._h, H, W, B3SPLINE if taps else family, max_level, int(scatter),
                                               _c.byref(self._h)))
        else:
            check(load().wt_plan_create_strip(ctx._h, H, W, B3SPLINE if taps else family, max_level,
                                              row0, nrows, halo_rows, rank, nranks,
                                              _c.byref(self._h)))
        info = (_i64 * 8)()
        check(load().wt_plan_info(self._h, info))
        (self.H, self.W, self.pitch, self.row0, self.nrows, self.halo, self.max_level,
         self.family) = [int(v) for v in info]
        self.rank, self.nranks = rank, nranks
        _live.add(self)
        if taps:
            self.set_taps(taps)
            self.family = taps

    @property
    def custom(self):
        """True when the plan filters with user-defined taps (generic kernels, no fusion)."""
        return isinstance(self.family, tuple)

    def set_taps(self, taps):
        arr = (_c.c_float * max(len(taps), 1))(*taps)
        check(load().wt_plan_set_taps(self._h, arr, len(taps)))

    def close(self):
        if self._h:
            h, self._h = self._h, _vp()
            check(load().wt_plan_destroy(h))     # a failed release (leaked HBM) is not silent

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory(self):
        """(bytes held, bytes in scattered planes, idle chunk bytes, scatter disabled on this
        context) - wt_plan_memory."""
        out = (_i64 * 4)()
        check(load().wt_plan_memory(self._h, out))
        return int(out[0]), int(out[1]), int(out[2]), bool(out[3])

    def trim(self):
        check(load().wt_plan_trim(self._h))

    @property
    def shape(self):
        return (self.nrows, self.W)

    # ---- transfers
    def upload(self, plane, host):
        """plane <- host image as float32; integer and byte-swapped images cross PCIe as they are and
        are widened on the device (wt_upload_int) instead of by a host astype."""
        src = _elem_source(np.asarray(host), self.shape)
        if src is not None:
            check(load().wt_upload_int(self._h, plane, _vp(src[0]), src[1], src[2]))
            return
        host = _as_f32(host)
        if host.shape != self.shape:
            raise ValueError(f"image shape {host.shape} != plan strip shape {self.shape}")
        check(load().wt_upload(self._h, plane, host.ctypes.data_as(_fp), host.shape[1]))

    def download(self, plane, out=None):
        if out is None:
            out = host_empty(self.shape, self.ctx)
        assert out.dtype == np.float32 and out.shape == self.shape and out.strides[1] == 4
        check(load().wt_download(self._h, plane, out.ctypes.data_as(_fp), out.strides[0] // 4))
        return out

    def set_border(self, border):
        check(load().wt_plan_set_border(self._h, int(border)))

    def crop_from(self, src_plan, src_plane, dst_plane, y0, x0):
        check(load().wt_crop_plane(src_plan._h, src_plane, self._h, dst_plane, y0, x0))

    def copy_window_from(self, src_plan, src_plane, dst_plane, sy, sx, dy, dx, rows, cols):
        """self[dst_plane][dy:dy+rows, dx:dx+cols] = src_plan[src_plane][sy:sy+rows, sx:sx+cols]"""
        check(load().wt_copy_window(src_plan._h, src_plane, self._h, dst_plane, sy, sx, dy, dx,
                                    rows, cols))

    def paste_into(self, dst_plan, src_plane, dst_plane, y0, x0):
        check(load().wt_paste_plane(self._h, src_plane, dst_plan._h, dst_plane, y0, x0))

    def copy(self, src, dst):
        check(load().wt_copy_plane(self._h, src, dst))

    def fill(self, plane, value):
        check(load().wt_fill_plane(self._h, plane, value))

    def fill_normal(self, plane, seed, trial=0):
        """`plane` <- standard normal deviates of (seed, trial): Philox4x32-10, counter (x >> 2, y, trial, 0) (rng.py)"""
        check(load().wt_fill_normal(self._h, plane, _seed64(seed), _trial32(trial)))

    def plane_ptr(self, plane):
        p = _vp()
        check(load().wt_plane_ptr(self._h, plane, _c.byref(p)))
        return p.value

    def halo_exchange(self, plane, rows):
        check(load().wt_halo_exchange(self._h, plane, rows))

    @staticmethod
    def halo_exchange_local(upper, lower, plane, rows):
        check(load().wt_halo_exchange_local(upper._h, lower._h, plane, rows))

    # ---- hot path
    def decompose(self, src, level, flags=FLAG_FUSED):
        check(load().wt_decompose(self._h, src, level, flags))

    def decompose_sum(self, src, level, dst=PLANE_OUT, flags=FLAG_FUSED):
        """decompose + plane sum in the same passes (bit-identical to the two calls)."""
        check(load().wt_decompose_sum(self._h, src, level, dst, flags))

    def decompose_sum_host(self, host, level, dst=PLANE_OUT, out=None, block_rows=0):
        """upload + decompose_sum + download(dst) with the PCIe legs pipelined behind the passes
        (wt_decompose_sum_host): returns the reconstruction as an ndarray; the device state is
        that of the three calls."""
        host = _as_f32_rows(host)                 # (a row-strided view goes down as it is: hipMemcpy2D)
        if host.shape != self.shape:
            raise ValueError(f"image shape {host.shape} != plan strip shape {self.shape}")
        if out is None:
            out = host_empty(self.shape, self.ctx)
        assert out.dtype == np.float32 and out.shape == self.shape and out.strides[1] == 4
        check(load().wt_decompose_sum_host(self._h, host.ctypes.data_as(_fp), host.strides[0] // 4, level, dst,
                                           out.ctypes.data_as(_fp), out.strides[0] // 4, block_rows))
        return out

    def denoise_sum_host(self, host, level, k_passes, taus, wgts, soft, dst=PLANE_OUT, out=None, block_rows=0):
        """upload + first k_passes passes + denoise_sum over their planes + remaining passes +
        download(dst), pipelined over blocks of rows (wt_denoise_sum_host): the denoised image."""
        host = _as_f32_rows(host)
        if host.shape != self.shape:
            raise ValueError(f"image shape {host.shape} != plan strip shape {self.shape}")
        if out is None:
            out = host_empty(self.shape, self.ctx)
        assert out.dtype == np.float32 and out.shape == self.shape and out.strides[1] == 4
        n = len(taus)
        t = (_c.c_double * n)(*[float(v) for v in taus])
        w = (_c.c_double * n)(*[float(v) for v in wgts])
        check(load().wt_denoise_sum_host(self._h, host.ctypes.data_as(_fp), host.strides[0] // 4, level, k_passes, n, t, w,
                                         int(soft), dst, out.ctypes.data_as(_fp), out.strides[0] // 4, block_rows))
        return out

    def decompose_pass_sum(self, cur, nxt, s0, ns, flags, sum_plane, first, last):
        check(load().wt_decompose_pass_sum(self._h, cur, nxt, s0, ns, flags, sum_plane,
                                           int(first), int(last)))

    def fused_ok(self, level):
        """True when decompose_sum(level) runs as accumulate passes (wt_plan_fused_ok)."""
        ok = _c.c_int(0)
        check(load().wt_plan_fused_ok(self._h, level, _c.byref(ok)))
        return bool(ok.value)

    def decompose_pass(self, cur, nxt, s0, ns, flags=FLAG_FUSED):
        check(load().wt_decompose_pass(self._h, cur, nxt, s0, ns, flags))

    def atrous_scale(self, src, dst_c, dst_w, s, flags=0):
        check(load().wt_atrous_scale(self._h, src, dst_c, dst_w, s, flags))

    def smooth(self, src, dst, s, square_input=False, flags=0):
        check(load().wt_smooth(self._h, src, dst, s, int(square_input), flags))

    def local_variance(self, src, dst, s, f1=1.0, f2=1.0, take_sqrt=False, flags=0):
        check(load().wt_local_variance(self._h, src, dst, s, f1, f2, int(take_sqrt), flags))

    def bilateral_conv(self, src, var, dst, s, flags=0):
        check(load().wt_bilateral_conv(self._h, src, var, dst, s, flags))

    def decompose_bilateral(self, src, level, sigma_b, bilateral_scaling=False, flags=0):
        arr = (_c.c_double * max(level, 1))(*[float(v) for v in sigma_b[:level]])
        check(load().wt_decompose_bilateral(self._h, src, level, arr, int(bilateral_scaling),
                                            flags))

    def plane_sum(self, first, count, dst=PLANE_OUT):
        check(load().wt_plane_sum(self._h, first, count, dst))

    def plane_sum_early(self, count, dst=PLANE_OUT):
        """planes [0, count) summed into dst on the side stream, if the plan is in the overlapped state of a
        bilateral transform (True), else nothing (False)"""
        done = _c.c_int(0)
        check(load().wt_plane_sum_early(self._h, count, dst, _c.byref(done)))
        return bool(done.value)

    def plane_sum_resume(self, first, count, dst=PLANE_OUT):
        check(load().wt_plane_sum_resume(self._h, first, count, dst))

    def abs_median(self, plane):
        m = _c.c_float(0)
        check(load().wt_abs_median(self._h, plane, _c.byref(m)))
        return np.float32(m.value)

    def significance(self, plane, dst, tau, soft=True, noise_plane=PLANE_NONE):
        check(load().wt_significance(self._h, plane, dst, float(tau), int(soft), noise_plane))

    def denoise(self, plane, tau, wgt=1.0, soft=True, noise_plane=PLANE_NONE):
        check(load().wt_denoise(self._h, plane, float(tau), float(wgt), int(soft), noise_plane))

    def denoise_sum(self, count, taus, wgts, soft=True, noise_plane=PLANE_NONE, write_back=False,
                    dst=PLANE_OUT, first=0):
        n = len(taus)
        ta = (_c.c_double * max(n, 1))(*[float(t) for t in taus])
        wa = (_c.c_double * max(n, 1))(*[float(w) for w in wgts])
        check(load().wt_denoise_sum(self._h, first, count, dst, n, ta, wa, int(soft), noise_plane,
                                    int(write_back)))

    def wow_update(self, plane, power_plane, tau, soft, noise_plane, factor, gamma_plane):
        check(load().wt_wow_update(self._h, plane, power_plane, float(tau), int(soft),
                                   noise_plane, float(factor), gamma_plane))

    def wow_scale(self, plane, s, tau, soft, noise_plane, factor, gamma_plane, flags=0):
        check(load().wt_wow_scale(self._h, plane, s, float(tau), int(soft), noise_plane,
                                  float(factor), gamma_plane, flags))

    def reduce(self, plane):
        """(sum, sumsq, min, max) over the GLOBAL image, fp64."""
        out = (_c.c_double * 4)()
        check(load().wt_reduce(self._h, plane, out))
        return tuple(out)

    def gamma_blend(self, recon, gamma_plane, gmin, gmax, inv_gamma, h):
        check(load().wt_gamma_blend(self._h, recon, gamma_plane, gmin, gmax, inv_gamma, h))

    def smooth3d(self, src, dst, s, depth):
        check(load().wt_smooth3d(self._h, src, dst, s, depth))

    def local_variance3d(self, src, dst, s, depth, f1=1.0, f2=1.0):
        check(load().wt_local_variance3d(self._h, src, dst, s, depth, f1, f2))

    def bilateral3d_conv(self, src, var, dst, s, depth):
        check(load().wt_bilateral3d_conv(self._h, src, var, dst, s, depth))

    def decompose3d(self, src, level, depth):
        check(load().wt_decompose3d(self._h, src, level, depth))

    def decompose_cube(self, src, level, depth):
        """decompose3d's planes, bit for bit, with one launch per scale (the float32 cube engine, cubes.py)"""
        check(load().wt_decompose_cube(self._h, src, level, depth))

    def wow_cube_scale(self, plane, s, depth, tau, soft, noise_plane, factor, gamma_plane):
        """binary("mul") + smooth3d + wow_update of one scale of a cube, bit for bit, in one launch (wt_wow_cube_scale)"""
        check(load().wt_wow_cube_scale(self._h, plane, s, depth, float(tau), int(soft), noise_plane, float(factor), gamma_plane))

    def filter2d(self, src, dst, kernel, flags=0, anchor=None, periodic=False):
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        if k.ndim != 2:
            raise ValueError("filter2d kernel must be 2-D")
        ay, ax = (k.shape[0] // 2, k.shape[1] // 2) if anchor is None else anchor
        check(load().wt_filter2d_ex(self._h, src, dst, k.ctypes.data_as(_fp), k.shape[0],
                                    k.shape[1], ay, ax, 3 if periodic else 0, flags))

    def binary(self, op, a, b, dst):
        check(load().wt_binary(self._h, {"sub": 0, "add": 1, "mul": 2, "div": 3,
                                         "add_div": 4}[op], a, b, dst))

    def taps_conv(self, src, var, dst, offsets, weights, center_weight=None, depth=0, pad_mode=0,
                  fill_value=0.0, dilation=1):
        """generic tap-list operator (wt_taps_conv_ex): offsets (n, 3) int32 = (dz, dy, dx); dilation:
        the stride of the polyphase pad modes (5 / 6)"""
        offs = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        wts = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        assert len(offs) == len(wts)
        check(load().wt_taps_conv_ex(self._h, src, var, dst, offs.ctypes.data_as(_c.POINTER(_c.c_int32)),
                                     wts.ctypes.data_as(_fp), len(wts),
                                     0.0 if center_weight is None else float(center_weight),
                                     int(center_weight is not None), depth, pad_mode, float(fill_value),
                                     int(dilation)))

    def axis_filter(self, src, dst, axis, offsets, weights, depth=0, pad_mode=0, fill_value=0.0, dilation=1):
        """K-tap filter along one axis (2 = x, 1 = y, 0 = z) on the tiled kernels (wt_axis_filter)"""
        offs = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
        wts = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        assert len(offs) == len(wts)
        check(load().wt_axis_filter(self._h, src, dst, axis, offs.ctypes.data_as(_c.POINTER(_c.c_int32)), wts.ctypes.data_as(_fp),
                                    len(wts), depth, pad_mode, float(fill_value), int(dilation)))

    def variance_from_moments(self, mean, meansq, dst, f1=1.0, f2=1.0, take_sqrt=False):
        """sdev_loc's last step (ref wavelets.py:27-32) from conv(I) and conv(I^2)"""
        check(load().wt_variance_from_moments(self._h, mean, meansq, dst, f1, f2, int(take_sqrt)))

    def mrs_update(self, plane, mrs_plane, tau, soft, noise_plane, persistent, inv_pow):
        check(load().wt_mrs_update(self._h, plane, mrs_plane, float(tau), int(soft), noise_plane,
                                   int(persistent), float(inv_pow)))

    def fft_spectrum(self, src):
        """kernel spectrum of the plan <- FFT2 of plane src (wt_fft_spectrum)"""
        check(load().wt_fft_spectrum(self._h, src))

    def fft_apply(self, src, dst, conj=False):
        """dst = irfft2(rfft2(src) * K) or, conj, * conj(K) (wt_fft_apply)"""
        check(load().wt_fft_apply(self._h, src, dst, int(conj)))

    def anscombe(self, src, dst, alpha=1.0, g=0.0, sigma=0.0, inverse=False):
        check(load().wt_anscombe(self._h, src, dst, alpha, g, sigma, int(inverse)))


# ------------------------------------------------------------------------------------------
# batches of same-shape frames (wt_batch): every fused pass runs over all frames in one launch
# ------------------------------------------------------------------------------------------
MAX_SUM_PLANES = 16                        # WT_MAX_SUM_PLANES: planes one launch of a plane sum folds
BATCH_MAX_FRAMES = 65535                  # grid z of the fused launches (one frame per z slice)
BATCH_BYTES = int(os.environ.get("WATROO_HIP_BATCH_BYTES", str(4 << 30)))   # device bytes of one chunk of frames


def _batch_pitch(W, itemsize):
    """row pitch in elements of a batch's planes: a wt_plan's (4 floats) or a wt_plan64's (2 doubles)"""
    if itemsize not in (4, 8):
        raise ValueError(f"itemsize {itemsize}: 4 (float32 batches) or 8 (float64 batches)")
    return (W + 3) // 4 * 4 if itemsize == 4 else (W + 1) // 2 * 2


def batch_frame_bytes(H, W, level, itemsize=4):
    """device bytes one frame of a batch takes: planes 0..level, input, output and two scratch planes at the
    plan pitch (host logic, wt_batch_create; itemsize=8: wt_batch64_create's double planes)"""
    return (level + 5) * H * _batch_pitch(W, itemsize) * itemsize


def batch_chunks(n, H, W, level, budget=None, max_frames=BATCH_MAX_FRAMES, extra_planes=0, itemsize=4):
    """[(first frame, frames)] of a stack of `n` frames: as many frames per chunk as `budget` bytes of planes
    (default BATCH_BYTES; at least one frame) and the grid allow, the last chunk the remainder.  `extra_planes`:
    planes per frame beyond batch_frame_bytes' (wow's spare and gamma planes).  `itemsize`: bytes per pixel of
    the planes (4: wt_batch, 8: wt_batch64)."""
    if n < 0:
        raise ValueError("negative frame count")
    if extra_planes < 0:
        raise ValueError("negative extra plane count")
    budget = BATCH_BYTES if budget is None else budget
    frame = batch_frame_bytes(H, W, level, itemsize) + int(extra_planes) * H * _batch_pitch(W, itemsize) * itemsize
    per = max(1, min(int(budget // frame), int(max_frames)))
    return [(f0, min(per, n - f0)) for f0 in range(0, n, per)]


def _enhance_rows(nf, taus, wgts):
    """(n_den, thresholds, weights) of BatchPlan.enhance_sum / BatchPlan64.enhance_sum: nf rows of n_den doubles each"""
    n = len(taus[0]) if len(taus) else 0
    if len(taus) != nf or len(wgts) != nf or n < 1 or any(len(t) != n for t in taus) or any(len(w) != n for w in wgts):
        raise ValueError("enhance_sum: one row of n_den >= 1 thresholds and one of n_den weights per frame")
    ta = (_c.c_double * (nf * n))(*[float(t) for row in taus for t in row])
    wa = (_c.c_double * (nf * n))(*[float(w) for row in wgts for w in row])
    return n, ta, wa


def batch_psf_ok(kh, kw):
    """True when a batch takes a kh x kw PSF (host logic, wt_batch_psf_ok): one Plan.filter2d applies in a single
    launch without bands - at most 4096 taps in rows of at most 512, an LDS tile of at most 96 KB"""
    ok = _c.c_int(0)
    check(load().wt_batch_psf_ok(int(kh), int(kw), _c.byref(ok)))
    return bool(ok.value)


def batch64_psf_ok(kh, kw):
    """True when a float64 batch takes a kh x kw PSF (host logic, wt_batch64_psf_ok): RLBatchPlan64.filter2d applies it
    in a single launch - at most 4096 taps in rows of at most 512, an LDS tile of doubles of at most 96 KB"""
    ok = _c.c_int(0)
    check(load().wt_batch64_psf_ok(int(kh), int(kw), _c.byref(ok)))
    return bool(ok.value)


def batch_fft_ok(H, W):
    """True when a batch of H x W frames takes the circular products through the FFT (host logic, wt_batch_fft_ok):
    fft_supported's rule on the frame shape - sides 2 .. 8192 without a prime factor above 5"""
    ok = _c.c_int(0)
    check(load().wt_batch_fft_ok(int(H), int(W), _c.byref(ok)))
    return bool(ok.value)


STREAM_NONE, STREAM_LEGACY, STREAM_PER_THREAD, STREAM_HANDLE = 0, 1, 2, 3     # WT_STREAM_*
COPY_HOST_TO_DEVICE, COPY_DEVICE_TO_HOST, COPY_DEVICE_TO_DEVICE = 1, 2, 3      # WT_COPY_*


def stream_arg(stream):
    """(handle, WT_STREAM_* kind) of a stream in the convention of __cuda_array_interface__: None - nothing to order;
    1 - the legacy default stream; 2 - the per-thread default stream; any other positive int - a hipStream_t; 0 - the
    null hipStream_t, which is the legacy default stream (what torch.cuda.current_stream().cuda_stream is on torch's
    default stream).  A bool or a negative value: ValueError (host logic)."""
    if stream is None:
        return None, STREAM_NONE
    if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or int(stream) < 0:
        raise ValueError(f"stream: None, 1 (legacy default), 2 (per-thread default) or a stream handle expected (got {stream!r})")
    stream = int(stream)
    if stream in (0, STREAM_LEGACY, STREAM_PER_THREAD):
        return None, stream or STREAM_LEGACY
    return _vp(stream), STREAM_HANDLE


def device_alloc(ctx, nbytes):
    """address of a block of `nbytes` bytes of device memory on the context's GPU (0 for an empty block)"""
    p = _vp()
    check(load().wt_device_alloc(ctx._h, int(nbytes), _c.byref(p)))
    return p.value or 0


def device_free(ctx, ptr):
    check(load().wt_device_free(ctx._h, _vp(ptr)))


def device_copy(ctx, dst, src, nbytes, kind):
    """`nbytes` contiguous bytes dst <- src (addresses), kind COPY_*; complete on return"""
    check(load().wt_device_copy(ctx._h, _vp(dst), _vp(src), int(nbytes), int(kind)))


def batch_load_device(bp, plane, nf, ptr, dtype, strides, f0=0, stream=None):
    """frames f0 .. f0+nf-1 of a plane of the BatchPlan / BatchPlan64 `bp` <- the (nf, H, W) DEVICE array at `ptr` of
    element type `dtype`, `strides` its three strides in bytes: upload's device-to-device form, widening included.
    `stream` (stream_arg's convention): the context's stream first waits for that stream; no host synchronisation.
    (Functions, not methods: the two classes keep the methods they have.)"""
    code = _ELEM_CODES[np.dtype(dtype).str[1:]]
    handle, kind = stream_arg(stream)
    bp._call("load_device", plane, f0, nf, _vp(ptr), code, (_i64 * 3)(*strides), handle, kind)


def batch_store_device(bp, plane, nf, ptr, strides, f0=0, stream=None):
    """frames f0 .. f0+nf-1 of a plane of `bp` -> the (nf, H, W) DEVICE array at `ptr` of the batch's element type:
    download's device-to-device form.  `stream`: that stream then waits for the copy; no host synchronisation."""
    handle, kind = stream_arg(stream)
    bp._call("store_device", plane, f0, nf, _vp(ptr), (_i64 * 3)(*strides), handle, kind)


class _BatchBase:
    """What BatchPlan and BatchPlan64 share, written once: device planes of up to `n` frames of one H x W shape.
    Operations take the number of active frames `nf` (frames 0 .. nf-1); upload / download move a C-contiguous
    (nf, H, W) block.  A subclass names the library's entries (`_prefix`), the element type of its planes (`dtype`)
    and that type in C (`_real`: the transfers, the medians, the per-frame factor and gamma tables; thresholds are
    doubles in both)."""

    _prefix = dtype = _real = None

    def _call(self, name, *args):
        check(getattr(load(), self._prefix + name)(self._h, *args))

    def __init__(self, ctx, n, H, W, family, max_level):
        self._h = _vp()
        self.ctx = ctx
        check(getattr(load(), self._prefix + "create")(ctx._h, n, H, W, family, max_level, _c.byref(self._h)))
        info = (_i64 * 7)()
        self._call("info", info)
        (self.n, self.H, self.W, self.pitch, self.frame_stride, self.max_level, self.family) = [int(v) for v in info]
        _live.add(self)

    def close(self):
        if self._h:
            h, self._h = self._h, _vp()
            check(getattr(load(), self._prefix + "destroy")(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _key(self):
        """what a cached batch must match besides its class and capacity (_StackCache)"""
        return self.H, self.W, self.family, self.max_level

    def _check_frames(self, a):
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f"frames of shape {a.shape[1:]} != batch frame shape {(self.H, self.W)}")

    def upload(self, plane, frames, f0=0):
        a = np.ascontiguousarray(frames, dtype=self.dtype)
        self._check_frames(a)
        self._call("upload", plane, f0, a.shape[0], a.ctypes.data_as(_c.POINTER(self._real)), 0)

    def download(self, plane, nf, out=None, f0=0):
        """(nf, H, W) of the batch's element type; `out` may be any (nf, H, W) view of that type whose frames are
        C-contiguous (e.g. cube[:, s] of an (N, L, H, W) array): the frames land in place, page-locked result blocks
        by default (host_empty)"""
        item = np.dtype(self.dtype).itemsize
        if out is None:
            out = host_empty((nf, self.H, self.W), self.ctx, self.dtype)
        assert out.dtype == self.dtype and out.shape == (nf, self.H, self.W) and out.flags.writeable
        assert out.strides[1:] == (self.W * item, item) and out.strides[0] % item == 0 \
            and out.strides[0] >= self.H * self.W * item
        self._call("download", plane, f0, nf, out.ctypes.data_as(_c.POINTER(self._real)), out.strides[0] // item)
        return out

    def plane_ptr(self, plane):
        """(device pointer of frame 0, frame stride in elements)"""
        p, st = _vp(), _i64()
        self._call("plane_ptr", plane, _c.byref(p), _c.byref(st))
        return p.value, int(st.value)

    def decompose(self, nf, src, level, flags=FLAG_FUSED):
        self._call("decompose", nf, src, level, flags)

    def decompose_bilateral(self, nf, src, level, sigma_b, bilateral_scaling=False, flags=0):
        """Plan.decompose_bilateral / Plan64.decompose_bilateral for frames 0 .. nf-1: one launch of the batched
        march per scale"""
        arr = (_c.c_double * max(level, 1))(*[float(v) for v in sigma_b[:level]])
        self._call("decompose_bilateral", nf, src, level, arr, int(bilateral_scaling), flags)

    def decompose_sum(self, nf, src, level, dst=PLANE_OUT, flags=FLAG_FUSED):
        self._call("decompose_sum", nf, src, level, dst, flags)

    def decompose_pass(self, nf, cur, nxt, s0, ns, flags=FLAG_FUSED):
        self._call("decompose_pass", nf, cur, nxt, s0, ns, flags)

    def decompose_pass_sum(self, nf, cur, nxt, s0, ns, flags, sum_plane, first, last):
        self._call("decompose_pass_sum", nf, cur, nxt, s0, ns, flags, sum_plane, int(first), int(last))

    def abs_median(self, nf, plane):
        """np.median(np.abs(frame)) of `plane` for frames 0 .. nf-1, each in the batch's element type (np.float32 /
        np.float64, as Plan.abs_median / Plan64.abs_median)"""
        m = (self._real * nf)()
        self._call("abs_median", nf, plane, m)
        return [self.dtype(v) for v in m]

    def _map_flags(self, has_map, nf):
        """the arguments of the denoise_sum_map entry after the noise plane: none (`has_map` is the float64 batch's)"""
        return ()

    def denoise_sum(self, nf, count, taus, wgts, soft=True, write_back=False, dst=PLANE_OUT, noise_plane=PLANE_NONE,
                    has_map=None):
        """`taus`: one row of thresholds per active frame (all rows of one length n_den).  `noise_plane`: the plane
        of per-pixel noise maps, one per active frame (ones for a frame with a scalar noise level).  `has_map`, read
        by the float64 batch only: per active frame, whether it has a map (None: all) - a frame without keeps the
        arithmetic of the call without a noise plane"""
        n = len(wgts)
        if len(taus) != nf or any(len(t) != n for t in taus):
            raise ValueError("denoise_sum: one row of len(wgts) thresholds per frame")
        ta = (_c.c_double * max(nf * n, 1))(*[float(t) for row in taus for t in row])
        wa = (_c.c_double * max(n, 1))(*[float(w) for w in wgts])
        if noise_plane != PLANE_NONE:
            self._call("denoise_sum_map", nf, count, dst, n, ta, wa, int(soft), int(write_back), noise_plane,
                       *self._map_flags(has_map, nf))
            return
        self._call("denoise_sum", nf, count, dst, n, ta, wa, int(soft), int(write_back))

    def enhance_sum(self, nf, count, taus, wgts, soft=True, write_back=False, dst=PLANE_OUT):
        """denoise_sum with one row of weights per active frame as well (utils.enhance: a colour image's channels
        are frames with their own sigmas and weights); all rows of one length n_den >= 1"""
        self._call("enhance_sum", nf, count, dst, *_enhance_rows(nf, taus, wgts), int(soft), int(write_back))

    def anscombe(self, nf, src, dst, alpha=1.0, g=0.0, sigma=0.0, inverse=False):
        self._call("anscombe", nf, src, dst, alpha, g, sigma, int(inverse))

    def fill(self, nf, plane, value):
        self._call("fill", nf, plane, value)

    def replicate(self, nf, plane):
        """frame 0 of `plane` -> frames 1 .. nf-1, on the device (a noise map shared by the frames)"""
        self._call("replicate", nf, plane)

    # -- wow (wow_update / wow_scale / reduce / gamma_blend / plane_sum): per-frame parameters are sequences of nf
    # values, the factors and the gamma range in the batch's element type
    @staticmethod
    def _per_frame(values, nf, ctype, what):
        if len(values) != nf:
            raise ValueError(f"{what}: one value per active frame ({nf} frames, {len(values)} values)")
        return (ctype * nf)(*[float(v) for v in values])

    def wow_update(self, nf, plane, taus, soft, factors, gamma_plane=PLANE_NONE, noise_plane=PLANE_NONE):
        """Plan.wow_update / Plan64.wow_update per frame without power plane: taus[f] (0.0: significance one),
        factors[f]; `noise_plane`: the plane of per-pixel noise maps, one per active frame"""
        t = self._per_frame(taus, nf, _c.c_double, "wow_update taus")
        f = self._per_frame(factors, nf, self._real, "wow_update factors")
        if noise_plane != PLANE_NONE:
            self._call("wow_update_map", nf, plane, t, int(soft), f, gamma_plane, noise_plane)
            return
        self._call("wow_update", nf, plane, t, int(soft), f, gamma_plane)

    def wow_scale(self, nf, plane, s, taus, soft, factors, gamma_plane=PLANE_NONE, noise_plane=PLANE_NONE):
        """Plan.wow_scale / Plan64.wow_scale per frame: local power, significance, gamma sum and whitening, in place;
        `noise_plane`: the plane of per-pixel noise maps, one per active frame"""
        t = self._per_frame(taus, nf, _c.c_double, "wow_scale taus")
        f = self._per_frame(factors, nf, self._real, "wow_scale factors")
        if noise_plane != PLANE_NONE:
            self._call("wow_scale_map", nf, plane, s, t, int(soft), f, gamma_plane, noise_plane)
            return
        self._call("wow_scale", nf, plane, s, t, int(soft), f, gamma_plane)

    def reduce(self, nf, plane):
        """[(sum, sumsq, min, max)] of every active frame, fp64 (Plan.reduce's / Plan64.reduce's doubles)"""
        out = (_c.c_double * (4 * nf))()
        self._call("reduce", nf, plane, out)
        return [tuple(out[4 * f:4 * f + 4]) for f in range(nf)]

    def gamma_blend(self, nf, recon, gamma_plane, gmins, gmaxs, inv_gamma, h):
        lo = self._per_frame(gmins, nf, self._real, "gamma_blend gmins")
        hi = self._per_frame(gmaxs, nf, self._real, "gamma_blend gmaxs")
        self._call("gamma_blend", nf, recon, gamma_plane, lo, hi, inv_gamma, h)

    def plane_sum(self, nf, first, count, dst=PLANE_OUT):
        self._call("plane_sum", nf, first, count, dst)


class BatchPlan(_BatchBase):
    """Device planes of up to `n` frames of one H x W shape (wt_batch): _BatchBase's operations in float32, and the
    ones only the float32 batch has - the seeded normal fill and richardson_lucy's PSF and FFT products."""

    _prefix, dtype, _real = "wt_batch_", np.float32, _c.c_float

    def fill_normal(self, nf, plane, seed, first_trial=0):
        """frame f of `plane` <- Plan.fill_normal(plane, seed, first_trial + f), frames 0 .. nf-1 (rng.py: the layout)"""
        self._call("fill_normal", nf, plane, _seed64(seed), _trial32(first_trial))

    # -- richardson_lucy (wt_batch_set_psf / _filter2d / _binary / _mrs_update)
    def set_psf(self, slot, kernel):
        """PSF operand `slot` (0: forward, 1: backward) of the batch <- `kernel`, once per call of the stack function"""
        k = np.ascontiguousarray(kernel, dtype=self.dtype)
        if k.ndim != 2:
            raise ValueError("set_psf kernel must be 2-D")
        self._call("set_psf", slot, k.ctypes.data_as(_c.POINTER(self._real)), k.shape[0], k.shape[1])
        self._psf_shape = getattr(self, "_psf_shape", {})
        self._psf_shape[slot] = k.shape

    def filter2d(self, nf, src, dst, slot, anchor=None, periodic=False):
        """Plan.filter2d per frame with the PSF of `slot`: one launch for frames 0 .. nf-1"""
        kh, kw = getattr(self, "_psf_shape", {}).get(slot, (1, 1))
        ay, ax = (kh // 2, kw // 2) if anchor is None else anchor
        self._call("filter2d", nf, src, dst, slot, ay, ax, 3 if periodic else 0)

    def binary(self, nf, op, a, b, dst):
        self._call("binary", nf, {"sub": 0, "add": 1, "mul": 2, "div": 3, "add_div": 4}[op], a, b, dst)

    def mrs_update(self, nf, plane, mrs_plane, taus, soft, persistent, inv_pow):
        """Plan.mrs_update per frame, scalar noise: taus[f] (0.0: significance one)"""
        t = self._per_frame(taus, nf, _c.c_double, "mrs_update taus")
        self._call("mrs_update", nf, plane, mrs_plane, t, int(soft), int(persistent), float(inv_pow))

    # -- richardson_lucy(fft=True), large PSFs (wt_batch_fft_spectrum / wt_batch_fft_apply)
    def fft_spectrum(self, src):
        """kernel spectrum of the batch <- FFT2 of FRAME 0 of plane src, once per call of the stack function"""
        self._call("fft_spectrum", src)

    def fft_apply(self, nf, src, dst, conj=False):
        """Plan.fft_apply per frame with the batch's one kernel spectrum: six launches for frames 0 .. nf-1"""
        self._call("fft_apply", nf, src, dst, int(conj))


def batch64_fused_ok(family, H, W, level):
    """True when H x W frames of `family` have an all-fused float64 schedule of `level` scales (host logic,
    wt_batch64_fused_ok: what wt64_plan_fused_ok answers for a wt_plan64 of that shape)"""
    ok = _c.c_int(0)
    check(load().wt_batch64_fused_ok(int(family), int(H), int(W), int(level), _c.byref(ok)))
    return bool(ok.value)


def batch64_bilateral_ok(family, H, W, level):
    """True when H x W frames of `family` take the float64 bilateral march per frame and `level` is one of its 1..25
    scales (host logic, wt_batch64_bilateral_ok: Plan64.decompose_bilateral's built-in route, option "stencil64"
    included) - the frames BatchPlan64.decompose_bilateral reproduces bit for bit"""
    ok = _c.c_int(0)
    check(load().wt_batch64_bilateral_ok(int(family), int(H), int(W), int(level), _c.byref(ok)))
    return bool(ok.value)


def batch64_wow_ok(family, H, W, level):
    """True when wow over H x W frames of `family` with `level` scales runs on the float64 batch (host logic,
    wt_batch64_wow_ok: 1..24 scales, fused passes or single-scale stencil passes, option "stencil64" on) - the frames
    BatchPlan64.decompose and BatchPlan64.wow_scale reproduce bit for bit"""
    ok = _c.c_int(0)
    check(load().wt_batch64_wow_ok(int(family), int(H), int(W), int(level), _c.byref(ok)))
    return bool(ok.value)


class BatchPlan64(_BatchBase):
    """Double-precision planes of up to `n` frames of one H x W shape (wt_batch64): _BatchBase's operations for the
    stacks the reference computes in float64.  Integer and big-endian frames cross as they are and are widened on
    the device (device_widens).  It has none of the operations that only the float32 batch has (richardson_lucy's
    four are RLBatchPlan64's; no wt_batch64 entry stands behind the others)."""

    _prefix, dtype, _real = "wt_batch64_", np.float64, _c.c_double

    def upload(self, plane, frames, f0=0):
        a = np.asarray(frames)
        if a.dtype == np.float64 or not device_widens(a.dtype):
            return super().upload(plane, a, f0)
        self._check_frames(a)
        a = np.ascontiguousarray(a)
        code = _ELEM_CODES[a.dtype.str[1:]] | (16 if not a.dtype.isnative and a.itemsize > 1 else 0)
        self._call("upload_elems", plane, f0, a.shape[0], _vp(a.ctypes.data), code)

    @staticmethod
    def _has_map(has_map, nf):
        if len(has_map) != nf:
            raise ValueError(f"denoise_sum has_map: one flag per active frame ({nf} frames, {len(has_map)} flags)")
        return (_c.c_int * nf)(*[int(bool(v)) for v in has_map])

    def _map_flags(self, has_map, nf):
        """one int per active frame, or NULL: every frame has a map"""
        return (None if has_map is None else self._has_map(has_map, nf),)


class RLBatchPlan64(BatchPlan64):
    """A BatchPlan64 with richardson_lucy's operations (wt_batch64_set_psf / _filter2d / _binary / _mrs_update): the
    calls of BatchPlan under the same names and signatures, in float64.  Its first set_psf makes richardson_lucy's planes
    - PLANE_SCRATCH(6 .. 10) and PLANE_SCRATCH(16 + s) - planes of the batch."""

    set_psf = BatchPlan.set_psf
    filter2d = BatchPlan.filter2d
    binary = BatchPlan.binary
    mrs_update = BatchPlan.mrs_update


class _StackCache:
    """A small cache of device stacks that are costly to allocate - objects with `_h` (the live handle), `ctx`, `n` (the
    capacity), `_key()` (what else must match) and `close()`: per context, most recently used last, at most MAX per
    context.  Its own cache, not the plan pool; the batches, the signal stacks and the axis stacks have one each."""

    MAX = 2

    def __init__(self):
        self.lists = {}          # id(ctx) -> [stack], most recently used last

    def acquire(self, cls, ctx, n, *key):
        """a cached `cls` on `ctx` of at least `n` with `_key()` == key, taken out of the cache, else cls(ctx, n, *key)"""
        with _pool_lock:
            lst = self.lists.setdefault(id(ctx), [])
            for i, b in enumerate(lst):
                if type(b) is cls and b._h and b.ctx is ctx and b._key() == key and b.n >= n:
                    return lst.pop(i)
        return cls(ctx, n, *key)

    def release(self, b):
        """a stack that is still open goes (back) into the cache; the oldest of more than MAX is closed"""
        if b is None or not b._h:
            return
        with _pool_lock:
            lst = self.lists.setdefault(id(b.ctx), [])
            lst.append(b)
            while len(lst) > self.MAX:
                lst.pop(0).close()

    def trim(self):
        """Release the device memory of every cached stack."""
        with _pool_lock:
            lst = [b for v in self.lists.values() for b in v]
            self.lists.clear()
        for b in lst:
            b.close()


_batch_cache, _signal_cache, _along_cache = _StackCache(), _StackCache(), _StackCache()


def acquire_batch(ctx, n, H, W, family, max_level):
    """A BatchPlan of at least `n` frames of (H, W, family, max_level) on `ctx`: cached if available, else new."""
    return _batch_cache.acquire(BatchPlan, ctx, n, H, W, family, max_level)


def acquire_batch64(ctx, n, H, W, family, max_level):
    """A BatchPlan64 of at least `n` frames of (H, W, family, max_level) on `ctx`: cached if available, else new
    (the cache of acquire_batch; release with release_batch64)."""
    return _batch_cache.acquire(BatchPlan64, ctx, n, H, W, family, max_level)


def acquire_rl_batch64(ctx, n, H, W, family, max_level):
    """An RLBatchPlan64 of at least `n` frames of (H, W, family, max_level) on `ctx`: cached if available, else new (the
    cache of acquire_batch, which keeps the classes apart; release with release_rl_batch64)."""
    return _batch_cache.acquire(RLBatchPlan64, ctx, n, H, W, family, max_level)


def trim_batches():
    """Release the device memory of every cached BatchPlan (the cache keeps at most two per context)."""
    _batch_cache.trim()


def release_batch(b):
    _batch_cache.release(b)


release_batch64 = release_rl_batch64 = release_batch          # (one cache for every kind of batch)


# ------------------------------------------------------------------------------------------
# stacks of 1-D signals of one length (wt_signals): one workgroup per signal, the scales in LDS
# ------------------------------------------------------------------------------------------
SIGNAL_MAX_LEVEL = 24                     # wt_signals_ok: the per-scale kernels' limit
LINES_ANSCOMBE = 1                        # bit 0 of the `flags` of the wt_signals_..._ex / wt_along_..._ex entries


def signals_ok(family, n_samples, level, itemsize):
    """True when signals of `n_samples` samples of `itemsize` bytes of `family` over `level` scales run on a
    SignalBatch (host logic, wt_signals_ok): a built-in family, 1..24 scales, the two LDS buffers of a signal within
    64 KiB - at most 8192 float32 or 4096 float64 samples"""
    if not isinstance(family, int):
        return False
    return bool(load().wt_signals_ok(int(family), int(n_samples), int(level), int(itemsize)))


def signal_bytes(n_samples, level, itemsize=4, wow=False):
    """device bytes one signal of a SignalBatch takes: the signal, planes 0..level and the sum, at the 16-byte pitch
    (host logic, wt_signals_create); `wow`: and the moments and the two tables of the wow route, 4 * level + 3 doubles
    (wt_signals_moments, wt_signals_wow_sum)"""
    return (level + 3) * _batch_pitch(n_samples, itemsize) * itemsize + (8 * (4 * level + 3) if wow else 0)


def signal_chunks(n, n_samples, level, budget=None, itemsize=4, wow=False):
    """[(first signal, signals)] of a stack of `n` signals, in the manner of batch_chunks: as many signals per chunk
    as `budget` bytes of device memory allow (default BATCH_BYTES; at least one), the last chunk the remainder;
    `wow`: signal_bytes of the wow route, and at most (2^31 - 1) // (level + 1) signals (a workgroup per plane)"""
    if n < 0:
        raise ValueError("negative signal count")
    budget = BATCH_BYTES if budget is None else budget
    cap = ((1 << 31) - 1) // (level + 1) if wow else (1 << 31) - 1
    per = max(1, min(int(budget // signal_bytes(n_samples, level, itemsize, wow)), cap))
    return [(f0, min(per, n - f0)) for f0 in range(0, n, per)]


class _LinesBase:
    """What SignalBatch and AlongBatch share, written once, in the manner of _BatchBase: the handle of a stack of 1-D
    signals of float32 or float64.  A subclass names the library's entries (`_prefix`) and itself with what it holds
    (`_holds`: the head of the element type error)."""

    _prefix = _holds = None

    def _call(self, name, *args):
        check(getattr(load(), self._prefix + name)(self._h, *args))

    def _create(self, n_info, ctx, n, n_samples, family, max_level, dtype, *more):
        """wt_..._create(ctx, n, n_samples, family, max_level, itemsize, *more, &handle); its wt_..._info as ints"""
        self._h = _vp()
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"{self._holds} (got {self.dtype})")
        check(getattr(load(), self._prefix + "create")(ctx._h, n, n_samples, family, max_level, self.dtype.itemsize, *more,
                                                        _c.byref(self._h)))
        info = (_i64 * n_info)()
        self._call("info", info)
        self.level = 0
        _live.add(self)
        return [int(v) for v in info]

    def close(self):
        if self._h:
            h, self._h = self._h, _vp()
            check(getattr(load(), self._prefix + "destroy")(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SignalBatch(_LinesBase):
    """Device memory of up to `n` signals of `n_samples` samples, float32 or float64 (wt_signals).  Operations take the
    number of active signals `nf` (signals 0 .. nf-1); upload / download move C-contiguous blocks of signals."""

    _prefix, _holds = "wt_signals_", "SignalBatch: float32 or float64 signals"

    def __init__(self, ctx, n, n_samples, family, max_level, dtype=np.float32):
        self.n, self.n_samples, self.pitch, self.family, self.max_level, _ = self._create(6, ctx, n, n_samples, family, max_level, dtype)

    def _key(self):
        return self.n_samples, self.family, self.max_level, self.dtype

    def upload(self, signals, f0=0):
        a = np.ascontiguousarray(signals, dtype=self.dtype)
        if a.ndim != 2 or a.shape[1] != self.n_samples:
            raise ValueError(f"signals of shape {a.shape} != (., {self.n_samples})")
        self._call("upload", f0, a.shape[0], _vp(a.ctypes.data))

    def decompose(self, nf, level, anscombe=False):
        """the transform of signals 0 .. nf-1; `anscombe`: of generalized_anscombe(signal), applied as the signals are
        loaded (wt_signals_decompose_ex, flags bit 0) - the same launch"""
        if anscombe:
            self._call("decompose_ex", nf, level, LINES_ANSCOMBE)
        else:
            self._call("decompose", nf, level)
        self.level = level

    def abs_median(self, nf):
        """np.median(np.abs(w_0)) of signals 0 .. nf-1 as an array of the stack's type: one host round trip"""
        out = np.empty(nf, self.dtype)
        self._call("abs_median", nf, _vp(out.ctypes.data))
        return out

    def denoise_sum(self, nf, taus, wgts, soft=True, anscombe=False):
        """Coefficients.denoise + the plane sum of signals 0 .. nf-1: one row of thresholds and one of weights per signal;
        `anscombe`: the inverse transform on every sum before its store (wt_signals_denoise_sum_ex, flags bit 0)"""
        n, ta, wa = _enhance_rows(nf, taus, wgts)
        if anscombe:
            self._call("denoise_sum_ex", nf, n, ta, wa, int(soft), LINES_ANSCOMBE)
        else:
            self._call("denoise_sum", nf, n, ta, wa, int(soft))

    def moments(self, nf):
        """(nf, level + 1, 2) float64: {sum, sum of squares} of every plane of signals 0 .. nf-1 of the last decompose,
        folded in double in a fixed order: one host round trip"""
        out = np.empty((nf, self.level + 1, 2), np.float64)
        self._call("moments", nf, out.ctypes.data_as(_c.POINTER(_c.c_double)))
        return out

    def wow_sum(self, nf, taus, factors, whitening, soft=True, write_planes=False):
        """the per-scale loop of wow + the plane sum of signals 0 .. nf-1: `taus` (nf, level) thresholds (0 =
        significance one), `factors` (nf, level + 1); `write_planes`: the whitened planes replace the planes"""
        ta = np.ascontiguousarray(taus, dtype=np.float64)
        fa = np.ascontiguousarray(factors, dtype=np.float64)
        if ta.shape != (nf, self.level) or fa.shape != (nf, self.level + 1):
            raise ValueError(f"thresholds of shape {ta.shape} and factors of shape {fa.shape} != ({nf}, {self.level}) and "
                             f"({nf}, {self.level + 1})")
        dp = _c.POINTER(_c.c_double)
        self._call("wow_sum", nf, self.level, ta.ctypes.data_as(dp), fa.ctypes.data_as(dp), int(bool(whitening)), int(bool(soft)),
                   int(bool(write_planes)))

    def _target(self, out, shape):
        if out is None:
            return host_empty(shape, self.ctx, self.dtype)
        assert out.dtype == self.dtype and out.shape == shape and out.flags.c_contiguous and out.flags.writeable
        return out

    def download_planes(self, nf, out=None, f0=0):
        """(nf, level + 1, n_samples) of the last decompose"""
        out = self._target(out, (nf, self.level + 1, self.n_samples))
        self._call("download_planes", f0, nf, _vp(out.ctypes.data))
        return out

    def download_sum(self, nf, out=None, f0=0):
        """(nf, n_samples) of the last denoise_sum"""
        out = self._target(out, (nf, self.n_samples))
        self._call("download_sum", f0, nf, _vp(out.ctypes.data))
        return out


def acquire_signals(ctx, n, n_samples, family, max_level, dtype=np.float32):
    """A SignalBatch of at least `n` signals of (n_samples, family, max_level, dtype) on `ctx`: cached if available, else new."""
    return _signal_cache.acquire(SignalBatch, ctx, n, n_samples, family, max_level, np.dtype(dtype))


def release_signals(b):
    _signal_cache.release(b)


def trim_signals():
    """Release the device memory of every cached SignalBatch (the cache keeps at most two per context)."""
    _signal_cache.trim()


# ------------------------------------------------------------------------------------------
# the 1-D transform along an axis that is not the last one (wt_along): an array viewed as (O, N, I), a tile of
# neighbouring signals per workgroup, the scales in LDS
# ------------------------------------------------------------------------------------------
ALONG_MAX_TILE = 256                      # WT_ALONG_MAX_TILE
ALONG_LDS_BYTES = 65536                   # WT_SIGNALS_LDS_BYTES: the two N x TI buffers of a tile (chosen, not measured)
ALONG_MAX_SIGNALS = 1 << 30               # signals of one chunk (wt_along_create)


def along_ok(family, n_samples, n_inner, level, itemsize):
    """True when signals of `n_samples` samples `n_inner` elements apart of `itemsize` bytes of `family` over `level`
    scales run on an AlongBatch (host logic, wt_along_ok): a built-in family, 1..24 scales, n_inner >= 2, and a tile
    with runs of at least 64 bytes within the 64 KiB of LDS - at most 512 samples in float32 and in float64"""
    if not isinstance(family, int):
        return False
    return bool(load().wt_along_ok(int(family), int(n_samples), int(n_inner), int(level), int(itemsize)))


def along_tile(n_samples, itemsize):
    """signals one workgroup takes (host logic, the rule of wt_along.hip): the largest power of two TI with
    2 * n_samples * TI * itemsize <= 64 KiB, at most 256 (0: not even one signal fits).  Never adapted to a narrow
    inner extent: a tile wider than it has idle lanes."""
    if n_samples < 1:
        return 0
    ti = ALONG_MAX_TILE
    while ti and 2 * n_samples * ti * itemsize > ALONG_LDS_BYTES:
        ti >>= 1
    return ti


def along_bytes(n_samples, level, itemsize=4, planes=True):
    """device bytes one signal of an AlongBatch takes (host logic, wt_along_create): the signal, its median and -
    planes - planes 0..level, or - the fused sum - the sum and its rows of the threshold table"""
    if planes:
        return (level + 2) * n_samples * itemsize + itemsize
    return 2 * n_samples * itemsize + itemsize + 2 * level * 8


def along_chunks(O, N, I, level, itemsize=4, budget=None, planes=True):
    """[(first outer index, outer indices, first inner position, inner positions)] of an (O, N, I) array over `budget`
    bytes of device memory (default BATCH_BYTES).  The outer index is split first: as many whole outer slices per chunk
    as fit.  When not even one fits, every outer slice is split along the inner axis in multiples of the tile (at
    least one tile): those chunks move as rows of their inner positions at pitch I."""
    if O < 0 or N < 0 or I < 0:
        raise ValueError("negative size")
    if O == 0 or N == 0 or I == 0:
        return []
    budget = BATCH_BYTES if budget is None else budget
    fit = min(int(budget // along_bytes(N, level, itemsize, planes)), ALONG_MAX_SIGNALS)       # signals of one chunk
    if fit >= I:
        per = fit // I
        return [(o0, min(per, O - o0), 0, I) for o0 in range(0, O, per)]
    tile = max(1, along_tile(N, itemsize))
    ni = max(tile, fit // tile * tile)
    return [(o, 1, i0, min(ni, I - i0)) for o in range(O) for i0 in range(0, I, ni)]


class AlongBatch(_LinesBase):
    """Device memory of chunks of up to `n_signals` signals of `n_samples` samples a stride apart, float32 or float64
    (wt_along).  `planes`: a batch for transforms (decompose / download_planes), else one for the fused thresholded
    sum (denoise / download_sum).  upload takes a (no, n_samples, ni) view of the caller's C-contiguous (O, N, I)
    array - rows of ni elements at pitch I - and the downloads fill views of the same kind."""

    _prefix, _holds = "wt_along_", "AlongBatch: float32 or float64 samples"

    def __init__(self, ctx, n_signals, n_samples, family, max_level, dtype=np.float32, planes=True):
        info = self._create(8, ctx, n_signals, n_samples, family, max_level, dtype, int(bool(planes)))
        self.n, self.n_samples, self.tile, self.family, self.max_level, _, planes, _ = info
        self.planes = bool(planes)
        self.chunk = (0, 0)                  # (outer indices, inner positions) of the last upload

    def _key(self):
        return self.n_samples, self.family, self.max_level, self.dtype, self.planes

    def _rows(self, a, lead=()):
        """pitch in elements of a `lead` + (no, n_samples, ni) block whose rows of ni elements are contiguous and lie
        one pitch apart through the outer index too"""
        no, ni = a.shape[-3], a.shape[-1]
        isz = self.dtype.itemsize
        if a.dtype != self.dtype or a.ndim != len(lead) + 3 or a.shape[-2] != self.n_samples or a.shape[:-3] != tuple(lead):
            raise ValueError(f"a {self.dtype} block of shape {tuple(lead)} + (., {self.n_samples}, .) expected (got {a.dtype} {a.shape})")
        # (numpy keeps any stride for an axis of length one: the one row of a slice then lies where the slices say)
        row = a.strides[-2] if self.n_samples > 1 else a.strides[-3] if no > 1 else ni * isz
        pitch = row // isz
        if (ni > 1 and a.strides[-1] != isz) or row % isz or pitch < ni \
                or (no > 1 and a.strides[-3] != self.n_samples * row):
            raise ValueError("rows of contiguous elements at one pitch expected")
        return pitch

    def upload(self, block):
        pitch = self._rows(block)
        no, _, ni = block.shape
        self._call("upload", no, ni, _vp(block.ctypes.data), pitch)
        self.chunk, self.level = (no, ni), 0

    def decompose(self, level):
        self._call("decompose", level)
        self.level = level

    def abs_median(self, anscombe=False):
        """np.median(np.abs(w_0)) of every signal of the chunk, (no, ni) of the stack's type: one host round trip;
        `anscombe`: of generalized_anscombe(chunk) (wt_along_abs_median_ex, flags bit 0)"""
        out = np.empty(self.chunk, self.dtype)
        if anscombe:
            self._call("abs_median_ex", _vp(out.ctypes.data), LINES_ANSCOMBE)
        else:
            self._call("abs_median", _vp(out.ctypes.data))
        return out

    def denoise(self, level, taus, wgts, soft=True, anscombe=False):
        """the fused transform + Coefficients.denoise + plane sum of the chunk: `taus` one row of thresholds per signal
        ((no * ni, n_den) doubles, 0 = significance one), `wgts` the one row of weights; `anscombe`: the forward
        transform at the load and the inverse at the store of the same launch (wt_along_denoise_ex, flags bit 0)"""
        ta = np.ascontiguousarray(taus, dtype=np.float64)
        wa = np.ascontiguousarray(wgts, dtype=np.float64)
        n_den = wa.shape[0]
        if ta.shape != (self.chunk[0] * self.chunk[1], n_den):
            raise ValueError(f"thresholds of shape {ta.shape} != ({self.chunk[0] * self.chunk[1]}, {n_den})")
        if anscombe:
            self._call("denoise_ex", level, n_den, ta.ctypes.data_as(_dp), wa.ctypes.data_as(_dp), int(soft), LINES_ANSCOMBE)
        else:
            self._call("denoise", level, n_den, ta.ctypes.data_as(_dp), wa.ctypes.data_as(_dp), int(soft))

    def download_planes(self, out):
        """the planes of the last decompose into `out`: a (level + 1, no, n_samples, ni) view"""
        pitch = self._rows(out, (self.level + 1,))
        if out.shape[1::2] != self.chunk or not out.flags.writeable:
            raise ValueError(f"a writable block of the chunk {self.chunk} expected (got {out.shape})")
        self._call("download_planes", _vp(out.ctypes.data), pitch, out.strides[0] // self.dtype.itemsize)
        return out

    def download_sum(self, out):
        """the sum of the last denoise into `out`: a (no, n_samples, ni) view"""
        pitch = self._rows(out)
        if out.shape[0::2] != self.chunk or not out.flags.writeable:
            raise ValueError(f"a writable block of the chunk {self.chunk} expected (got {out.shape})")
        self._call("download_sum", _vp(out.ctypes.data), pitch)
        return out


def acquire_along(ctx, n_signals, n_samples, family, max_level, dtype=np.float32, planes=True):
    """An AlongBatch of at least `n_signals` signals of (n_samples, family, max_level, dtype, planes) on `ctx`: cached if
    available, else new."""
    return _along_cache.acquire(AlongBatch, ctx, n_signals, n_samples, family, max_level, np.dtype(dtype), bool(planes))


def release_along(b):
    _along_cache.release(b)


def trim_along():
    """Release the device memory of every cached AlongBatch (the cache keeps at most two per context)."""
    _along_cache.trim()


# ------------------------------------------------------------------------------------------
# plan pool: hipMalloc/hipFree of a dozen multi-hundred-MiB planes costs milliseconds, far more
# than the transform itself; plans of recently used geometries are kept for reuse.
# ------------------------------------------------------------------------------------------
_POOL_MAX_BYTES = int(os.environ.get("WATROO_HIP_POOL_BYTES", str(16 << 30)))
_pool = []            # [(key, plan)] most recently released last


def _plan_bytes(plan):
    """Device bytes a pooled plan holds: the library's own count for float32 plans (planes, the
    bounce plane of host transfers, idle chunks), an estimate for float64 plans."""
    if isinstance(plan, Plan) and plan._h:
        return plan.memory()[0]
    return (plan.nrows + 2 * plan.halo) * plan.pitch * 8 * (plan.max_level + 1 + 2 + 4)


_pool_lock = threading.RLock()      # plan pool and default contexts are shared by host threads


_dp = _c.POINTER(_c.c_double)


class Plan64:
    """Double-precision planes of one image: wt_plan64, the float64 engine (the reference computes
    float64 / promoted inputs in float64, ref wavelets.py:297,319-320).  Same plane ids and, for the
    operators it has, the same method names as ``Plan``; taps are always given (the built-in
    families pass theirs).  Standard decomposition without bilateral filtering, Coefficients
    operators, convolution, sdev_loc, Anscombe."""

    dtype = np.float64
    custom = True            # generic kernels with run-time taps: no fused passes
    rank, nranks, row0, halo = 0, 1, 0, 0

    def __init__(self, ctx, H, W, taps, max_level):
        self._h = _vp()
        self.ctx = ctx
        self.family = tuple(float(t) for t in taps)
        arr = (_c.c_double * len(self.family))(*self.family)
        check(load().wt64_plan_create(ctx._h, H, W, max_level, arr, len(self.family),
                                      _c.byref(self._h)))
        self.H, self.W, self.nrows, self.max_level = H, W, H, max_level
        self.pitch = (W + 1) // 2 * 2
        _live.add(self)

    def close(self):
        if self._h:
            load().wt64_plan_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shape(self):
        return (self.H, self.W)

    _INT_CODES = _ELEM_CODES          # (emptied by tools/bench_int_input.py to time the host promotion)
    device_widens = staticmethod(device_widens)

    def upload(self, plane, host):
        """plane <- host image as float64.  Integer and big-endian images (what the reference recasts to
        float64 first, ref wavelets.py:297, 319-320) cross PCIe as they are and are widened on the device."""
        src = _elem_source(np.asarray(host), self.shape) if self._INT_CODES else None
        if src is not None:
            check(load().wt64_upload_int(self._h, plane, _vp(src[0]), src[1], src[2]))
            return
        host = np.ascontiguousarray(host, dtype=np.float64)
        if host.shape != self.shape:
            raise ValueError(f"image shape {host.shape} != plan shape {self.shape}")
        check(load().wt64_upload(self._h, plane, host.ctypes.data_as(_dp), host.shape[1]))

    def download(self, plane, out=None):
        if out is None:
            out = host_empty(self.shape, self.ctx, np.float64)
        assert out.dtype == np.float64 and out.shape == self.shape and out.strides[1] == 8
        check(load().wt64_download(self._h, plane, out.ctypes.data_as(_dp), out.strides[0] // 8))
        return out

    def set_border(self, border):
        check(load().wt64_plan_set_border(self._h, int(border)))

    _BUILTIN = {(0.25, 0.5, 0.25): TRIANGLE, (0.0625, 0.25, 0.375, 0.25, 0.0625): B3SPLINE}

    @property
    def fused_family(self):
        """TRIANGLE / B3SPLINE when the taps are a built-in family's (fused passes), else None"""
        return self._BUILTIN.get(self.family)

    def fused_ok(self, level):
        """True when the whole schedule of `level` scales runs as fused passes (wt64_plan_fused_ok)."""
        ok = _c.c_int(0)
        check(load().wt64_plan_fused_ok(self._h, level, _c.byref(ok)))
        return bool(ok.value)

    def decompose(self, src, level, flags=0):
        check(load().wt64_decompose_ex(self._h, src, level, 0, flags & FLAG_MEDIAN_HIST))

    def decompose_pass(self, cur, nxt, s0, ns, flags=FLAG_FUSED):
        check(load().wt64_decompose_pass(self._h, cur, nxt, s0, ns, flags & FLAG_MEDIAN_HIST))

    def decompose_pass_sum(self, cur, nxt, s0, ns, flags, sum_plane, first, last):
        check(load().wt64_decompose_pass_sum(self._h, cur, nxt, s0, ns, sum_plane, int(first), int(last)))

    def decompose_sum(self, src, level, dst=PLANE_OUT, flags=0):
        """Transform + np.sum(planes, axis=0) -> dst; True when the sum rode in the fused passes."""
        fused = _c.c_int(0)
        check(load().wt64_decompose_sum(self._h, src, level, dst, _c.byref(fused)))
        return bool(fused.value)

    def decompose3d(self, src, level, depth):
        check(load().wt64_decompose(self._h, src, level, depth))

    def decompose_cube(self, src, level, depth):
        """decompose3d's planes, bit for bit, with one launch per scale (the float64 cube engine, cubes.py)"""
        check(load().wt64_decompose_cube(self._h, src, level, depth))

    def wow_cube_scale(self, plane, s, depth, tau, soft, noise_plane, factor, gamma_plane):
        """binary("mul") + smooth3d + wow_update of one scale of a cube, bit for bit, in one launch (wt64_wow_cube_scale)"""
        check(load().wt64_wow_cube_scale(self._h, plane, s, depth, float(tau), int(soft), noise_plane, float(factor), gamma_plane))

    def smooth(self, src, dst, s, square_input=False, flags=0):
        check(load().wt64_smooth(self._h, src, dst, s, int(square_input), 0))

    def smooth3d(self, src, dst, s, depth):
        check(load().wt64_smooth(self._h, src, dst, s, 0, depth))

    def local_variance(self, src, dst, s, f1=1.0, f2=1.0, take_sqrt=False, flags=0):
        check(load().wt64_local_variance(self._h, src, dst, s, f1, f2, int(take_sqrt), 0))

    def local_variance3d(self, src, dst, s, depth, f1=1.0, f2=1.0):
        check(load().wt64_local_variance(self._h, src, dst, s, f1, f2, 0, depth))

    def bilateral_conv(self, src, var, dst, s, flags=0):
        check(load().wt64_bilateral_conv(self._h, src, var, dst, s, 0,
                                         int(bool(flags & FLAG_TAPS_REVERSED))))

    def bilateral3d_conv(self, src, var, dst, s, depth):
        check(load().wt64_bilateral_conv(self._h, src, var, dst, s, depth, 0))

    def decompose_bilateral(self, src, level, sigma_b, bilateral_scaling=False, flags=0):
        arr = (_c.c_double * max(level, 1))(*[float(v) for v in sigma_b[:level]])
        check(load().wt64_decompose_bilateral(self._h, src, level, arr, int(bilateral_scaling)))

    def copy_window_from(self, src_plan, src_plane, dst_plane, sy, sx, dy, dx, rows, cols):
        check(load().wt64_copy_window(src_plan._h, src_plane, self._h, dst_plane, sy, sx, dy, dx,
                                      rows, cols))

    def crop_from(self, src_plan, src_plane, dst_plane, y0, x0):
        self.copy_window_from(src_plan, src_plane, dst_plane, y0, x0, 0, 0, self.H, self.W)

    def abs_median(self, plane):
        m = _c.c_double(0)
        check(load().wt64_abs_median(self._h, plane, _c.byref(m)))
        return np.float64(m.value)

    def significance(self, src, dst, tau, soft=True, noise_plane=PLANE_NONE):
        check(load().wt64_significance(self._h, src, dst, tau, 1.0, int(soft), noise_plane, 0))

    def denoise(self, plane, tau, weight=1.0, soft=True, noise_plane=PLANE_NONE):
        check(load().wt64_significance(self._h, plane, plane, tau, weight, int(soft), noise_plane, 1))

    def wow_update(self, plane, power_plane, tau, soft, noise_plane, factor, gamma_plane):
        check(load().wt64_wow_update(self._h, plane, power_plane, float(tau), int(soft),
                                     noise_plane, float(factor), gamma_plane))

    def wow_scale(self, plane, s, tau, soft, noise_plane, factor, gamma_plane, flags=0):
        """local power conv_s(c^2) + the wow update of one scale, in place (wt64_wow_scale)"""
        check(load().wt64_wow_scale(self._h, plane, s, float(tau), int(soft), noise_plane, float(factor), gamma_plane))

    def gamma_blend(self, recon, gamma_plane, gmin, gmax, inv_gamma, h):
        check(load().wt64_gamma_blend(self._h, recon, gamma_plane, gmin, gmax, inv_gamma, h))

    def fill(self, plane, value):
        check(load().wt64_fill_plane(self._h, plane, value))

    def reduce(self, plane):
        out = (_c.c_double * 4)()
        check(load().wt64_reduce(self._h, plane, out))
        return tuple(out)

    def denoise_sum(self, n, taus, wgts, soft, noise_plane=PLANE_NONE, write_back=True, dst=PLANE_OUT):
        """Coefficients.denoise over the first len(taus) planes fused with the plane sum of planes
        0..n-1 -> dst (wt64_denoise_sum); tau <= 0: no threshold on that plane (weight only)."""
        k = len(taus)
        t = (_c.c_double * max(k, 1))(*[float(v) for v in taus])
        w = (_c.c_double * max(k, 1))(*[float(v) for v in wgts])
        check(load().wt64_denoise_sum(self._h, 0, n, dst, k, t, w, int(soft), noise_plane, int(write_back)))

    def plane_sum(self, first, count, dst=PLANE_OUT):
        check(load().wt64_plane_sum(self._h, first, count, dst))

    def plane_sum_early(self, count, dst=PLANE_OUT):
        done = _c.c_int(0)
        check(load().wt64_plane_sum_early(self._h, count, dst, _c.byref(done)))
        return bool(done.value)

    def plane_sum_resume(self, first, count, dst=PLANE_OUT):
        check(load().wt64_plane_sum_resume(self._h, first, count, dst))

    def binary(self, op, a, b, dst):
        code = {"add": 0, "sub": 1, "mul": 2, "div": 3, "add_div": 4}[op]
        check(load().wt64_binary(self._h, code, a, b, dst))

    def taps_conv(self, src, var, dst, offsets, weights, center_weight=None, depth=0, pad_mode=0,
                  fill_value=0.0, dilation=1):
        offs = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        wts = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        assert len(offs) == len(wts)
        check(load().wt64_taps_conv_ex(self._h, src, var, dst, offs.ctypes.data_as(_c.POINTER(_c.c_int32)),
                                       wts.ctypes.data_as(_dp), len(wts),
                                       0.0 if center_weight is None else float(center_weight),
                                       int(center_weight is not None), depth, pad_mode, float(fill_value),
                                       int(dilation)))

    def axis_filter(self, src, dst, axis, offsets, weights, depth=0, pad_mode=0, fill_value=0.0, dilation=1):
        offs = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
        wts = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        assert len(offs) == len(wts)
        check(load().wt64_axis_filter(self._h, src, dst, axis, offs.ctypes.data_as(_c.POINTER(_c.c_int32)), wts.ctypes.data_as(_dp),
                                      len(wts), depth, pad_mode, float(fill_value), int(dilation)))

    def variance_from_moments(self, mean, meansq, dst, f1=1.0, f2=1.0, take_sqrt=False):
        check(load().wt64_variance_from_moments(self._h, mean, meansq, dst, f1, f2, int(take_sqrt)))

    def copy(self, src, dst):
        self.copy_window_from(self, src, dst, 0, 0, 0, 0, self.H, self.W)

    def fft_spectrum(self, src):
        check(load().wt64_fft_spectrum(self._h, src))

    def fft_apply(self, src, dst, conj=False):
        check(load().wt64_fft_apply(self._h, src, dst, int(conj)))

    def filter2d(self, src, dst, kernel, flags=0, anchor=None, periodic=False):
        k = np.ascontiguousarray(kernel, dtype=np.float64)
        if k.ndim != 2:
            raise ValueError("filter2d kernel must be 2-D")
        ay, ax = (k.shape[0] // 2, k.shape[1] // 2) if anchor is None else anchor
        check(load().wt64_filter2d(self._h, src, dst, k.ctypes.data_as(_dp), k.shape[0], k.shape[1],
                                   ay, ax, 3 if periodic else 0))

    def mrs_update(self, plane, mrs_plane, tau, soft, noise_plane, persistent, inv_pow):
        check(load().wt64_mrs_update(self._h, plane, mrs_plane, float(tau), int(soft), noise_plane,
                                     int(persistent), float(inv_pow)))

    def anscombe(self, src, dst, alpha=1, g=0, sigma=0, inverse=False):
        check(load().wt64_anscombe(self._h, src, dst, alpha, g, sigma, int(inverse)))


def acquire_plan64(ctx, H, W, taps, max_level):
    """Pooled float64 plan (same pool and eviction rule as the float32 plans)."""
    taps = tuple(float(t) for t in taps)
    key = (id(ctx), H, W, ("f64",) + taps, max_level)
    with _pool_lock:
        for i in range(len(_pool) - 1, -1, -1):
            if _pool[i][0] == key:
                plan = _pool.pop(i)[1]
                if not plan._h:
                    # closed while pooled: a Coefficients object and its plan collected in one pass of the cyclic
                    # garbage collector run both finalizers, in either order (Coefficients.__del__ pools the plan,
                    # Plan.__del__ closes it)
                    continue
                plan.set_border(0)
                return plan
    return Plan64(ctx, H, W, taps, max_level)


_COLD_FIRST_USE = not os.environ.get("WATROO_HIP_NO_COLD_PLANS")


def acquire_plan(ctx, H, W, family, max_level):
    """A whole-image plan for (H, W, family, max_level): pooled if available, else new.

    Plans made HERE - for the numpy-to-numpy calls of the API - keep their planes on plain hipMalloc (round 5).
    Mapping planes over scattered physical chunks makes the fused passes ~20 % faster, 0.1 ms
    per transform at 8192^2, and costs ~16 ms when a plan is created and first used: worth it for device-resident
    loops over a `_lib.Plan` (bench.py's metric: input already in HBM), not for calls that move the image over PCIe
    both ways (10 ms at 8192^2) - and a one-shot `denoise(img)` would pay it in full (section 3.8: first call of a
    process 48 -> 38 ms).  WATROO_HIP_NO_COLD_PLANS=1 restores scattered planes for pooled plans too."""
    key = (id(ctx), H, W, family, max_level)
    with _pool_lock:
        for i in range(len(_pool) - 1, -1, -1):
            if _pool[i][0] == key:
                plan = _pool.pop(i)[1]
                if not plan._h:
                    # closed while pooled: a Coefficients object and its plan collected in one pass of the cyclic
                    # garbage collector run both finalizers, in either order (Coefficients.__del__ pools the plan,
                    # Plan.__del__ closes it)
                    continue
                plan.set_border(0)
                return plan
    if not _COLD_FIRST_USE:
        return Plan(ctx, H, W, family, max_level)
    plan = Plan(ctx, H, W, family, max_level, scatter=0)      # (per plan: no process-wide option is touched)
    plan.cold = True
    return plan


def release_plan(plan):
    """Hand a plan back for reuse (its planes keep stale data; callers re-upload)."""
    if plan is None or not plan._h or plan.nranks != 1:
        return
    evicted = []
    fam = ("f64",) + plan.family if isinstance(plan, Plan64) else plan.family
    if isinstance(plan, Plan):
        try:
            plan.trim()           # idle physical chunks (up to three planes' worth) go back now
        except WatrooHipError:
            # a plan whose chunks cannot be released is not pooled (it would be handed out again with
            # its state unknown): closed here, and the error goes to the caller
            try:
                plan.close()
            except WatrooHipError:
                pass
            raise
    with _pool_lock:
        _pool.append(((id(plan.ctx), plan.H, plan.W, fam, plan.max_level), plan))
        total = sum(_plan_bytes(p) for _, p in _pool)
        while _pool and (total > _POOL_MAX_BYTES or len(_pool) > 8):
            _, old = _pool.pop(0)
            total -= _plan_bytes(old)
            evicted.append(old)
    first_error = None
    for old in evicted:           # every evicted plan is closed, whatever the ones before it did
        try:
            old.close()
        except WatrooHipError as e:
            first_error = first_error or e
    if first_error is not None:
        raise first_error
