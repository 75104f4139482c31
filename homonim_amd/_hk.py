"""
ctypes binding of include/homonim_hk.h (libhomonim_hk.so) -- the thin FFI layer between the Python host code and the
hand-written HIP kernels.  This is the stub a homonim maintainer would add to homonim/kernel_model.py.

There is NO CPU fallback: if the library is missing or no gfx950 device is present, every entry point raises
``DeviceError`` loudly.
"""
import atexit
import ctypes as C
import sys
import weakref
import math
import os
import threading
from typing import Optional, Sequence

import numpy as np

from homonim_amd.errors import DeviceError, IoError

# HOMONIM_AMD_LIB overrides the library path (kernel-variant experiments); the default is the in-tree build.
_LIB_PATH = os.environ.get('HOMONIM_AMD_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib',
                                                               'libhomonim_hk.so')

HK_OK, HK_ERR_ARG, HK_ERR_HIP, HK_ERR_NODEVICE, HK_ERR_UNSUPPORTED, HK_ERR_NOMEM, HK_ERR_ALREADY = 0, -1, -2, -3, -4, -5, -6
MODEL_CODES = {'gain': 0, 'gain-blk-offset': 1, 'gain-offset': 2}
NODATA_NONE, NODATA_NAN, NODATA_VALUE = 0, 1, 2


class FitDesc(C.Structure):
    _fields_ = [
        ('model', C.c_int32), ('kh', C.c_int32), ('kw', C.c_int32), ('find_r2', C.c_int32),
        ('has_r2_thresh', C.c_int32), ('r2_thresh', C.c_float), ('src_nodata_mode', C.c_int32),
        ('src_nodata', C.c_float), ('ref_nodata_mode', C.c_int32), ('ref_nodata', C.c_float),
    ]  # yapf: disable


class IoDesc(C.Structure):
    _fields_ = [('src_dtype', C.c_int32), ('ref_dtype', C.c_int32), ('out_dtype', C.c_int32),
                ('out_has_nodata', C.c_int32), ('out_nodata', C.c_double)]


class SpaceDesc(C.Structure):
    _fields_ = [('down', C.c_double * 4), ('up', C.c_double * 4), ('down_resampling', C.c_int32),
                ('up_resampling', C.c_int32), ('mask_partial', C.c_int32)]


class SrcSpaceDesc(C.Structure):
    _fields_ = [('map', C.c_double * 4), ('resampling', C.c_int32), ('mask_partial', C.c_int32)]


# numpy dtype name -> hk_dtype
DTYPE_CODES = {'float32': 0, 'uint8': 1, 'uint16': 2, 'int16': 3, 'uint32': 4, 'int32': 5, 'float64': 6}


class CrsDesc(C.Structure):
    _fields_ = [('kind', C.c_int32), ('reserved', C.c_int32), ('a', C.c_double), ('inv_f', C.c_double), ('lat0', C.c_double),
                ('lon0', C.c_double), ('k0', C.c_double), ('fe', C.c_double), ('fn', C.c_double)]


class WarpDesc(C.Structure):
    _fields_ = [('src_crs', CrsDesc), ('dst_crs', CrsDesc), ('src_gt', C.c_double * 4), ('dst_gt', C.c_double * 4)]


class AffineWarpDesc(C.Structure):
    _fields_ = [('src_crs', CrsDesc), ('dst_crs', CrsDesc), ('same_crs', C.c_int32), ('reserved', C.c_int32),
                ('src_gt', C.c_double * 6), ('dst_gt', C.c_double * 6)]


class OutWindow(C.Structure):
    _fields_ = [('stride', C.c_int64), ('band_stride', C.c_int64), ('row0', C.c_int32), ('col0', C.c_int32),
                ('rows', C.c_int32), ('cols', C.c_int32), ('param_stride', C.c_int64)]


class InflateLayout(C.Structure):
    """ hk_inflate_layout: the blocks of one GeoTIFF image (the fields of ``tiff.BlockLayout``, in its order) """
    _fields_ = [('sample_bytes', C.c_int32), ('spp', C.c_int32), ('height', C.c_int32), ('width', C.c_int32),
                ('block_w', C.c_int32), ('block_h', C.c_int32), ('tiled', C.c_int32), ('separate', C.c_int32),
                ('predictor', C.c_int32)]


class DevJob(C.Structure):
    _fields_ = [
        ('src', C.c_void_p), ('ref', C.c_void_p), ('gain', C.c_void_p), ('offset', C.c_void_p), ('r2', C.c_void_p),
        ('corr', C.c_void_p), ('norm', C.c_void_p), ('fail_count', C.c_void_p), ('n_bands', C.c_int32),
        ('height', C.c_int32), ('width', C.c_int32), ('stride', C.c_int64), ('band_stride', C.c_int64),
        ('seg_rows', C.c_int32), ('stream', C.c_int32),
        ('out_row0', C.c_int32), ('out_col0', C.c_int32), ('out_rows', C.c_int32), ('out_cols', C.c_int32),
        ('scratch', C.c_void_p), ('scratch_bytes', C.c_uint64),
    ]  # yapf: disable


class TwoGridJob(C.Structure):
    """ hk_two_grid_job: source and reference blocks on different grids, resident on the device (hk_refspace_fit_apply_dev /
    hk_srcspace_fit_apply_dev) """
    _fields_ = [
        ('src', C.c_void_p), ('ref', C.c_void_p), ('corr', C.c_void_p), ('valid', C.c_void_p), ('params', C.c_void_p),
        ('src_stride', C.c_int64), ('src_band_stride', C.c_int64), ('ref_stride', C.c_int64), ('ref_band_stride', C.c_int64),
        ('corr_stride', C.c_int64), ('corr_band_stride', C.c_int64), ('valid_stride', C.c_int64), ('valid_band_stride', C.c_int64),
        ('param_stride', C.c_int64), ('param_band_stride', C.c_int64),
        ('n_bands', C.c_int32), ('n_param_bands', C.c_int32),
        ('src_height', C.c_int32), ('src_width', C.c_int32), ('ref_height', C.c_int32), ('ref_width', C.c_int32),
        ('out_row0', C.c_int32), ('out_col0', C.c_int32), ('out_rows', C.c_int32), ('out_cols', C.c_int32),
        ('par_row0', C.c_int32), ('par_col0', C.c_int32), ('par_rows', C.c_int32), ('par_cols', C.c_int32),
        ('stream', C.c_int32), ('reserved', C.c_int32),
        ('scratch', C.c_void_p), ('scratch_bytes', C.c_uint64),
    ]  # yapf: disable


_P = C.POINTER
_f32p, _f64p, _u64p = _P(C.c_float), _P(C.c_double), _P(C.c_uint64)

# name -> (restype, argtypes); kept in one table so tests can check every symbol of the header is exported
DEFLATE_CHUNK = 16384  # HK_DEFLATE_CHUNK: raw bytes per DEFLATE block of Context.deflate_tiles
ABI_VERSION = 12  # HK_ABI_VERSION of the include/homonim_hk.h these mirrors were written against
# entry points declared in include/homonim_hk_devtools.h (measurement / test aids), the rest in include/homonim_hk.h
DEVTOOLS = ('hk_synth_fill_dev', 'hk_stream_probe_dev', 'hk_debug_stage_stamps', 'hk_r2_certificate_constants', 'hk_debug_staging_counters',
            'hk_debug_build_ledger', 'hk_debug_checksum_dev', 'hk_debug_fail_after_d2h', 'hk_debug_inpaint_plane_dev',
            'hk_debug_cast_plane_dev', 'hk_debug_fit_build')
# HK_FIT_PLANE_*: the planes a fused launch is handed (hk_debug_fit_build)
FIT_PLANES = {'gain': 1, 'offset': 2, 'r2': 4, 'corr': 8, 'fail_count': 16, 'flags': 32, 'offset_in': 64, 'jobs': 128}

SIGNATURES = {
    'hk_abi_version': (C.c_int, []),
    'hk_backend_name': (C.c_char_p, []),
    'hk_dev_job_scratch_bytes': (C.c_uint64, [C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    'hk_block_norm_split_exchange_doubles': (C.c_uint64, [C.c_int32]),
    'hk_block_norm_split_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'hk_comm_unique_id': (C.c_int, [C.c_void_p]),
    'hk_comm_init': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    'hk_comm_destroy': (C.c_int, [C.c_void_p]),
    'hk_comm_info': (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32)]),
    'hk_comm_allreduce_f64_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    'hk_block_norm_split_comm_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), C.c_void_p]),
    'hk_counts_pending': (C.c_int, [_P(C.c_uint64), C.c_int32]),
    'hk_last_error': (C.c_char_p, []),
    'hk_device_count': (C.c_int, [_P(C.c_int)]),
    'hk_device_pci_bus_id': (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    'hk_ctx_create': (C.c_int, [C.c_int, C.c_int, _P(C.c_void_p)]),
    'hk_ctx_destroy': (C.c_int, [C.c_void_p]),
    'hk_ctx_sync': (C.c_int, [C.c_void_p]),
    'hk_block_norm': (C.c_int, [C.c_void_p, _P(FitDesc), _f32p, C.c_int64, _f32p, C.c_int64, C.c_int32, C.c_int32, _f64p]),
    'hk_compare_sums': (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, C.c_float, _f32p, C.c_int64, C.c_int32, C.c_float,
                                  C.c_int32, C.c_int32, _f64p]),
    'hk_param_stats': (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_int32, C.c_int32, _f64p]),
    'hk_param_stats_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                     C.c_int32, C.c_float, C.c_double, C.c_void_p]),
    'hk_overview_count': (C.c_int, [C.c_int32, C.c_int32, _P(C.c_int32)]),
    'hk_overviews': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                               C.c_double, C.c_int32, _P(C.c_void_p), _P(C.c_int64), _P(C.c_int64)]),
    'hk_overviews_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                   C.c_int32, C.c_double, C.c_int32, _P(C.c_void_p), _P(C.c_int64), _P(C.c_int64), C.c_int32]),
    'hk_overviews_valid': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                     _P(C.c_uint8), C.c_int64, C.c_int32, _P(C.c_void_p), _P(C.c_int64), _P(C.c_int64),
                                     _P(C.c_void_p), _P(C.c_int64)]),
    'hk_overviews_valid_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_int64, C.c_int32, _P(C.c_void_p), _P(C.c_int64), _P(C.c_int64),
                                         _P(C.c_void_p), _P(C.c_int64), C.c_int32]),
    'hk_dataset_mask': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                  C.c_int64, _f32p, C.c_int64]),
    'hk_dataset_mask_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                      C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]),
    'hk_fill_planes_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_double,
                                     C.c_int32]),
    'hk_boundless_window_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_int32]),
    'hk_dev_mem_info': (C.c_int, [C.c_void_p, _u64p, _u64p]),
    'hk_deflate_bound': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int64), _P(C.c_int64)]),
    'hk_deflate_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_void_p, C.c_int64, _P(C.c_int64), _P(C.c_int64)]),
    'hk_deflate_tiles_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                       C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]),
    'hk_deflate_tiles_pred': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                        C.c_int32, C.c_void_p, C.c_int64, _P(C.c_int64), _P(C.c_int64), C.c_int32]),
    'hk_deflate_tiles_pred_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                            C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    'hk_inflate_bound': (C.c_int, [_P(InflateLayout), _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
    'hk_inflate_image': (C.c_int, [C.c_void_p, _P(InflateLayout), C.c_void_p, _P(C.c_int64), _P(C.c_int64), C.c_void_p, C.c_int64,
                                   C.c_int64, _P(C.c_int32)]),
    'hk_inflate_image_dev': (C.c_int, [C.c_void_p, _P(InflateLayout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    'hk_lzw_image': (C.c_int, [C.c_void_p, _P(InflateLayout), C.c_void_p, _P(C.c_int64), _P(C.c_int64), C.c_void_p, C.c_int64,
                               C.c_int64, _P(C.c_int32)]),
    'hk_lzw_image_host': (C.c_int, [_P(InflateLayout), C.c_void_p, _P(C.c_int64), _P(C.c_int64), C.c_void_p, C.c_int64, C.c_int64,
                                    _P(C.c_int32)]),
    'hk_lzw_image_dev': (C.c_int, [C.c_void_p, _P(InflateLayout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    'hk_fit': (C.c_int, [C.c_void_p, _P(FitDesc), _f32p, C.c_int64, _f32p, C.c_int64, C.c_int32, C.c_int32, _f64p,
                         _f32p, C.c_int32, _f64p, _u64p]),
    'hk_apply': (C.c_int, [C.c_void_p, _f32p, C.c_int64, _f32p, C.c_int32, C.c_int32, _f32p]),
    'hk_fit_apply': (C.c_int, [C.c_void_p, _P(FitDesc), _f32p, C.c_int64, _f32p, C.c_int64, C.c_int32, C.c_int32,
                               _f64p, _f32p, C.c_int32, _f32p, _f64p, _u64p]),
    'hk_refspace_fit_apply': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SpaceDesc), C.c_void_p, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32,
                                        C.c_void_p, _u64p]),
    'hk_srcspace_fit_apply': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SrcSpaceDesc), C.c_void_p, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32,
                                        C.c_void_p, _u64p]),
    'hk_refspace_fit_apply_valid': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SpaceDesc), C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32,
                                              C.c_void_p, C.c_void_p, _u64p]),
    'hk_srcspace_fit_apply_valid': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SrcSpaceDesc), C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _f32p, C.c_int32,
                                              C.c_void_p, C.c_void_p, _u64p]),
    'hk_refspace_dev_scratch_bytes': (C.c_uint64, [_P(FitDesc), _P(IoDesc), _P(SpaceDesc), _P(TwoGridJob)]),
    'hk_srcspace_dev_scratch_bytes': (C.c_uint64, [_P(FitDesc), _P(IoDesc), _P(SrcSpaceDesc), _P(TwoGridJob)]),
    'hk_refspace_fit_apply_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SpaceDesc), _P(TwoGridJob), _u64p]),
    'hk_srcspace_fit_apply_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), _P(SrcSpaceDesc), _P(TwoGridJob), _u64p]),
    'hk_reproject': (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_double, C.c_double,
                               C.c_double, C.c_double, C.c_int32, _f32p, C.c_int32, C.c_int32, C.c_float]),
    'hk_reproject_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_float,
                                   C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_int64, C.c_int64, C.c_float, C.c_int32]),
    'hk_warp_coords': (C.c_int, [C.c_void_p, _P(WarpDesc), C.c_double, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p, C.c_int64]),
    'hk_warp_coords_dev': (C.c_int, [C.c_void_p, _P(WarpDesc), C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_int32]),
    'hk_reproject_crs': (C.c_int, [C.c_void_p, _P(WarpDesc), _f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                   C.c_double, C.c_double, C.c_int32, _f32p, C.c_int32, C.c_int32, C.c_float]),
    'hk_reproject_crs_dev': (C.c_int, [C.c_void_p, _P(WarpDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                       C.c_int32, C.c_float, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int64, C.c_int64, C.c_float, C.c_int32]),
    'hk_warp_coords_affine': (C.c_int, [C.c_void_p, _P(AffineWarpDesc), C.c_double, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p,
                                        C.c_int64]),
    'hk_warp_coords_affine_dev': (C.c_int, [C.c_void_p, _P(AffineWarpDesc), C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_int64, C.c_int32]),
    'hk_reproject_affine': (C.c_int, [C.c_void_p, _P(AffineWarpDesc), _f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      C.c_double, C.c_double, C.c_int32, _f32p, C.c_int32, C.c_int32, C.c_float]),
    'hk_reproject_affine_dev': (C.c_int, [C.c_void_p, _P(AffineWarpDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                          C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int64, C.c_int64, C.c_float, C.c_int32]),
    'hk_partial_mask': (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, C.c_float, _f32p, C.c_int32, _f32p, C.c_int64,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, _P(C.c_uint8)]),
    'hk_fit_apply_io': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.c_int32, C.c_int32, _f64p, _f32p, C.c_int32, C.c_void_p, _f64p, _u64p]),
    'hk_fit_apply_block': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_int32, _f64p, C.c_void_p, C.c_int32, C.c_void_p, _P(OutWindow), _f64p, _u64p]),
    'hk_fit_apply_block_valid': (C.c_int, [C.c_void_p, _P(FitDesc), _P(IoDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_int32, C.c_int32, _f64p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, _P(OutWindow),
                                           _f64p, _u64p]),
    'hk_host_alloc': (C.c_int, [C.c_void_p, C.c_size_t, _P(C.c_void_p)]),
    'hk_host_free': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hk_host_register': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'hk_host_unregister': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hk_dev_alloc': (C.c_int, [C.c_void_p, C.c_size_t, _P(C.c_void_p)]),
    'hk_dev_free': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hk_memcpy_h2d': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    'hk_memcpy_d2h': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    'hk_memset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]),
    'hk_fit_apply_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob)]),
    'hk_inpaint_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), _P(C.c_uint64)]),
    'hk_fail_counts_async': (C.c_int, [C.c_void_p, _P(DevJob), _P(C.c_uint64), C.c_void_p]),
    'hk_inpaint_dev_counts': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), _P(C.c_uint64), _P(C.c_uint64)]),
    'hk_event_sync': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hk_r2_certificate_constants': (C.c_int, [C.c_float, _P(C.c_double), _P(C.c_double), _P(C.c_float), _P(C.c_float)]),
    'hk_block_norm_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), C.c_void_p]),
    'hk_block_norm_batch_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), C.c_int32, C.c_void_p]),
    'hk_fit_apply_batch_dev': (C.c_int, [C.c_void_p, _P(FitDesc), _P(DevJob), C.c_int32]),
    'hk_fail_counts_batch_async': (C.c_int, [C.c_void_p, _P(DevJob), C.c_int32, _P(C.c_uint64), C.c_void_p]),
    'hk_compare_sums_dev': (C.c_int, [C.c_void_p, _P(DevJob), C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_void_p]),
    'hk_synth_fill_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                    C.c_int64, C.c_uint64, C.c_int32, C.c_int32]),
    'hk_stream_probe_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    'hk_event_create': (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    'hk_event_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hk_event_record': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    'hk_stream_wait_event': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    'hk_event_elapsed_ms': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_float)]),
    'hk_stream_sync': (C.c_int, [C.c_void_p, C.c_int32]),
    'hk_selftest': (C.c_int, [C.c_void_p]),
    'hk_debug_stage_stamps': (C.c_int, [C.c_void_p, _P(C.c_uint64), C.c_int32]),
    'hk_debug_staging_counters': (C.c_int, [_P(C.c_uint64), C.c_int32]),
    'hk_debug_build_ledger': (C.c_int, [C.c_char_p, C.c_size_t, _P(C.c_size_t), C.c_int32]),
    'hk_debug_fit_build': (C.c_int, [_P(FitDesc), C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_char_p, C.c_size_t]),
    'hk_debug_fail_after_d2h': (C.c_int, [C.c_int32]),
    'hk_debug_checksum_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P(C.c_uint64)]),
    'hk_debug_inpaint_plane_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32,
                                             C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    'hk_debug_cast_plane_dev': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_double, C.c_int32]),
}  # yapf: disable

MASK_BITS, MASK_ALPHA = 0, 1   # HK_MASK_BITS, HK_MASK_ALPHA: the mask_kind of hk_dataset_mask / hk_dataset_mask_dev
PARAM_STATS_N = 10    # values per band of hk_param_stats / hk_param_stats_dev
COMM_ID_BYTES = 128   # HK_COMM_ID_BYTES = sizeof(ncclUniqueId)


def r2_certificate_constants(thresh: float):
    """ (pass_below, fail_above, kappa, kappa_fail) of the r2-mask decision for `thresh` (hk_r2_certificate_constants; host-only). """
    pb, fa, k, kf = C.c_double(), C.c_double(), C.c_float(), C.c_float()
    _check(load_library().hk_r2_certificate_constants(C.c_float(thresh), C.byref(pb), C.byref(fa), C.byref(k), C.byref(kf)))
    return pb.value, fa.value, k.value, kf.value


def refspace_dev_scratch_bytes(desc: FitDesc, space: SpaceDesc, job: TwoGridJob, io: Optional[IoDesc] = None) -> int:
    """ hk_refspace_dev_scratch_bytes (host arithmetic, no device): the scratch of one hk_refspace_fit_apply_dev call, 0 if refused """
    return int(load_library().hk_refspace_dev_scratch_bytes(C.byref(desc), C.byref(io) if io is not None else None, C.byref(space),
                                                            C.byref(job)))


def srcspace_dev_scratch_bytes(desc: FitDesc, space: SrcSpaceDesc, job: TwoGridJob, io: Optional[IoDesc] = None) -> int:
    """ hk_srcspace_dev_scratch_bytes: the same for hk_srcspace_fit_apply_dev """
    return int(load_library().hk_srcspace_dev_scratch_bytes(C.byref(desc), C.byref(io) if io is not None else None, C.byref(space),
                                                            C.byref(job)))


def overview_count(height: int, width: int) -> int:
    """ Number of internal overviews of a raster of this shape (hk_overview_count; host-only). """
    n = C.c_int32(0)
    _check(load_library().hk_overview_count(int(height), int(width), C.byref(n)))
    return int(n.value)


def overview_shapes(height: int, width: int, n_levels: int):
    """ [(ceil(height / 2^m), ceil(width / 2^m)) for m = 1..n_levels] """
    return [(-(-int(height) // (1 << m)), -(-int(width) // (1 << m))) for m in range(1, int(n_levels) + 1)]


def deflate_bound(dtype, n_bands: int, height: int, width: int, tile: int):
    """ -> (number of tiles, bytes that always hold their zlib streams) of ``Context.deflate_tiles`` (hk_deflate_bound; no device
    needed): per tile 2 + sum over its chunks of (chunk + 5) + 6, rounded up to even. """
    n_tiles, cap = C.c_int64(), C.c_int64()
    _check(load_library().hk_deflate_bound(DTYPE_CODES[np.dtype(dtype).name], n_bands, height, width, int(tile), C.byref(n_tiles),
                                           C.byref(cap)))
    return n_tiles.value, cap.value


# HK_INFLATE_*: the status of a block of Context.inflate_image_packed
(INFLATE_OK, INFLATE_TRUNCATED, INFLATE_BAD_HEADER, INFLATE_BAD_BLOCK, INFLATE_BAD_STORED, INFLATE_BAD_CODE, INFLATE_BAD_SYMBOL,
 INFLATE_FAR, INFLATE_OVERRUN, INFLATE_SHORT, INFLATE_ADLER) = range(11)


def _inflate_layout(layout) -> InflateLayout:
    """ a ``tiff.BlockLayout`` (or anything with its fields, or an InflateLayout) as the C struct """
    if isinstance(layout, InflateLayout):
        return layout
    return InflateLayout(*[int(getattr(layout, name)) for name, _ in InflateLayout._fields_])


def inflate_bound(layout):
    """ -> (number of blocks, raw bytes of a full block, bytes of device scratch of ``Context.inflate_image_dev``) for the
    blocks of an image (hk_inflate_bound; no device needed). """
    n_blocks, raw, work = C.c_int64(), C.c_int64(), C.c_int64()
    _check(load_library().hk_inflate_bound(C.byref(_inflate_layout(layout)), C.byref(n_blocks), C.byref(raw), C.byref(work)))
    return n_blocks.value, raw.value, work.value


# HK_LZW_*: the status of a block of Context.lzw_image_packed / lzw_image_host_packed
LZW_OK, LZW_TRUNCATED, LZW_OLD_STYLE, LZW_BAD_FIRST, LZW_BAD_CODE, LZW_SHORT = range(6)


def _packed_blocks(streams, offsets, sizes, lay):
    """ the arguments of the block-image calls checked and as arrays: -> (uint8 buffer, int64 offsets, int64 sizes, out, status) """
    n_blocks, _, _ = inflate_bound(lay)
    buf = np.frombuffer(streams, np.uint8) if isinstance(streams, (bytes, bytearray, memoryview)) else np.ascontiguousarray(streams, np.uint8)
    offsets, sizes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(sizes, np.int64)
    if offsets.shape != (n_blocks,) or sizes.shape != (n_blocks,):
        raise ValueError(f'{offsets.size} offsets and {sizes.size} sizes for {n_blocks} blocks')
    if n_blocks and ((offsets < 0).any() or (sizes < 0).any() or (offsets + sizes > buf.size).any()):
        raise ValueError('a stream lies outside the buffer')
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)   # (every stream is empty: a pointer all the same)
    out = np.empty((lay.spp, lay.height, lay.width), np.dtype(f'u{lay.sample_bytes}'))
    return buf, offsets, sizes, out, np.zeros(n_blocks, np.int32)


def _blocks_image(fn, handle, streams, offsets, sizes, layout, strict):
    """ the block-image entry point ``fn`` of the context ``handle`` (None: the host decoder) -> (array, status per block) """
    lay = _inflate_layout(layout)
    buf, offsets, sizes, out, status = _packed_blocks(streams, offsets, sizes, lay)
    rc = fn(*(() if handle is None else (handle,)), C.byref(lay), buf.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(_P(C.c_int64)),
            sizes.ctypes.data_as(_P(C.c_int64)), out.ctypes.data_as(C.c_void_p), lay.width, lay.height * lay.width,
            status.ctypes.data_as(_P(C.c_int32)))
    if rc == HK_ERR_ARG and status.any():
        if strict:
            raise IoError(load_library().hk_last_error().decode('utf-8', 'replace'))
        return out, status
    _check(rc)
    return out, status


def _pack_streams(streams):
    """ a list of ``bytes`` as one buffer, every stream at a multiple of 16: -> (buffer, offsets, sizes) """
    sizes = np.array([len(s) for s in streams], np.int64)
    padded = (sizes + 15) // 16 * 16
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64) if len(sizes) else np.zeros(0, np.int64)
    buf = np.zeros(int(padded.sum()), np.uint8)
    for o, s in zip(offsets.tolist(), streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return buf, offsets, sizes


def lzw_image_host_packed(streams, offsets, sizes, layout, strict: bool = True):
    """ ``Context.lzw_image_packed`` on the calling thread (hk_lzw_image_host: the kernel's decoder compiled for the host; no
    context, no device): the same arguments, the same (array, status per block), the same ``IoError``. """
    return _blocks_image(load_library().hk_lzw_image_host, None, streams, offsets, sizes, layout, strict)


def lzw_image_host(streams, layout) -> np.ndarray:
    """ What ``tiff.read_tiff`` takes as ``lzw``, without a device: the LZW streams of an image's blocks (a list of ``bytes``, in
    the file's block order) -> its (spp, height, width) array of uint8 / 16 / 32 / 64, decoded by the library on this thread.
    ``IoError`` names the first block whose stream is refused, and why. """
    return lzw_image_host_packed(*_pack_streams(streams), layout, strict=True)[0]


# The TIFF predictors the block decoders undo, as ``tiff.read_tiff`` asks a hook: 3, the floating-point predictor, goes only to a
# hook that says so in its ``predictors`` (a hook without the attribute knows 1 and 2).
PREDICTORS = (1, 2, 3)
lzw_image_host_packed.predictors = lzw_image_host.predictors = PREDICTORS


def block_decoders(inflate, get_context=None):
    """ The ``inflate`` option of ``RasterFuse`` / ``ParamStats`` -> (inflater, lzw) as ``tiff.read_tiff`` takes them: 'host' -- zlib
    on the reading thread (no inflater) and the library's host LZW decoder; 'device' -- ``inflate_image`` / ``lzw_image`` of
    ``get_context()``, which is called only then (None: the option is only checked).  All of them undo predictors 1, 2 and 3. """
    if inflate not in ('host', 'device'):
        raise ValueError(f"`inflate` must be 'host' or 'device', not {inflate!r}")
    if inflate == 'device' and get_context is not None:
        ctx = get_context()
        return ctx.inflate_image, ctx.lzw_image
    return None, lzw_image_host


def comm_unique_id() -> bytes:
    """ A fresh communicator id (hk_comm_unique_id = ncclGetUniqueId): rank 0 calls this and distributes the bytes. """
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _check(load_library().hk_comm_unique_id(buf))
    return bytes(buf)


_lib = None
_lib_lock = threading.Lock()
# page-lock registrations made through Context.pin: (address, bytes) -> [users, registered by us]
_pins = {}
_pin_lock = threading.Lock()


def lib_path() -> str:
    return _LIB_PATH


def load_library():
    """ dlopen libhomonim_hk.so and declare every prototype.  Raises DeviceError if it has not been built. """
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise DeviceError(
                    f'{_LIB_PATH} not found: build it with `python -m homonim_amd.build` (needs hipcc). '
                    'homonim_amd has no CPU fallback.'
                )
            lib = C.CDLL(_LIB_PATH)
            try:
                lib.hk_abi_version.restype = C.c_int
                found = lib.hk_abi_version()
            except AttributeError:
                found = None
            if found != ABI_VERSION:   # struct layouts differ between versions and carry no size field: do not call further
                raise DeviceError(f'{_LIB_PATH} has ABI version {found}, this binding needs {ABI_VERSION}: rebuild it with '
                                  '`python -m homonim_amd.build`')
            for name, (restype, argtypes) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    return _lib


def _check(rc: int):
    if rc == HK_OK:
        return
    msg = load_library().hk_last_error().decode('utf-8', 'replace')
    if rc == HK_ERR_ARG:
        raise ValueError(msg)
    raise DeviceError(f'libhomonim_hk error {rc}: {msg}')


def nodata_code(nodata):
    """ RasterArray.nodata -> (mode, value) of the C ABI. """
    if nodata is None:
        return NODATA_NONE, 0.0
    nodata = float(nodata)
    if math.isnan(nodata):
        return NODATA_NAN, float('nan')
    return NODATA_VALUE, nodata


def out_nodata_code(out_dtype, out_nodata):
    """ Output nodata -> (out_has_nodata, out_nodata) of hk_io_desc.  None, and NaN for a float dtype: masked pixels keep NaN;
    NaN for an integer dtype: 0.  Any other value must survive the cast to ``out_dtype`` as RasterArray._convert_array_dtype
    demands (homonim/raster_array.py:357-358): an integer of the type's range for an integer type, no overflow for float32;
    the library refuses the same with HK_ERR_ARG (hk_api.hip validate_out_nodata). """
    out_dtype = np.dtype(out_dtype)
    if out_nodata is None:
        return 0, 0.0
    value = float(out_nodata)
    if math.isnan(value):
        return (0, 0.0) if out_dtype.kind == 'f' else (1, 0.0)
    if out_dtype.kind == 'f':
        ok = math.isinf(value) or out_dtype.itemsize == 8 or abs(value) < float.fromhex('0x1.ffffffp127')
    else:
        info = np.iinfo(out_dtype)
        ok = math.isfinite(value) and value == math.floor(value) and info.min <= value <= info.max
    if not ok:
        raise ValueError(f"'nodata' value: {out_nodata} cannot be safely cast to '{out_dtype.name}'")
    return 1, value


def _io_desc(src: np.ndarray, ref: np.ndarray, out_dtype: np.dtype, out_nodata) -> IoDesc:
    return make_io_desc(src.dtype, ref.dtype, out_dtype, out_nodata)


def make_desc(model: str, kernel_shape, find_r2: bool, r2_inpaint_thresh: Optional[float], src_nodata, ref_nodata):
    d = FitDesc()
    d.model = MODEL_CODES[str(getattr(model, 'value', model))]
    d.kh, d.kw = int(kernel_shape[0]), int(kernel_shape[1])
    d.find_r2 = int(bool(find_r2))
    d.has_r2_thresh = int(r2_inpaint_thresh is not None)
    d.r2_thresh = float(r2_inpaint_thresh) if r2_inpaint_thresh is not None else 0.0
    d.src_nodata_mode, d.src_nodata = nodata_code(src_nodata)
    d.ref_nodata_mode, d.ref_nodata = nodata_code(ref_nodata)
    return d


class DeviceRaster:
    """ A raster that lies in device memory: what ``RefSpaceModel.fit_apply_dev`` / ``SrcSpaceModel.fit_apply_dev`` take for their
    inputs and outputs.  ``dptr``: device address of the first pixel of band 0; ``shape``: (bands, height, width); ``stride`` /
    ``band_stride``: elements of ``dtype`` between rows / between bands (default: packed).  Inputs also carry their grid:
    ``transform`` (Affine), ``crs`` and ``nodata``.  The memory is the caller's (``Context.dev_alloc``). """

    def __init__(self, dptr: int, dtype, shape, stride: Optional[int] = None, band_stride: Optional[int] = None, transform=None,
                 crs=None, nodata=None):
        self.dptr, self.dtype = int(dptr), np.dtype(dtype)
        if len(shape) != 3:
            raise ValueError('`shape` must be (bands, height, width)')
        self.shape = tuple(int(v) for v in shape)
        self.stride = int(stride) if stride is not None else self.shape[2]
        self.band_stride = int(band_stride) if band_stride is not None else self.shape[1] * self.stride
        self.transform, self.crs, self.nodata = transform, crs, nodata

    @property
    def res(self):
        """ (x, y) pixel size, as ``RasterArray.res`` """
        return abs(self.grid_transform.a), abs(self.grid_transform.e)

    @property
    def grid_transform(self):
        """ the transform of an input raster; ValueError where it was not given """
        if self.transform is None:
            raise ValueError('a DeviceRaster that is an input (`src`, `ref`) needs its `transform`')
        return self.transform


def make_space_desc(down, up, down_resampling: int, up_resampling: int, mask_partial: bool) -> SpaceDesc:
    sp = SpaceDesc()
    for i in range(4):
        sp.down[i], sp.up[i] = float(down[i]), float(up[i])
    sp.down_resampling, sp.up_resampling, sp.mask_partial = int(down_resampling), int(up_resampling), int(bool(mask_partial))
    return sp


def make_srcspace_desc(mapping, resampling: int, mask_partial: bool) -> SrcSpaceDesc:
    sp = SrcSpaceDesc()
    for i in range(4):
        sp.map[i] = float(mapping[i])
    sp.resampling, sp.mask_partial = int(resampling), int(bool(mask_partial))
    return sp


def make_two_grid_job(src: DeviceRaster, ref: DeviceRaster, corr: DeviceRaster, params: Optional[DeviceRaster] = None,
                      valid: Optional[DeviceRaster] = None, window=None, param_window=None, stream: int = 0, scratch: int = 0,
                      scratch_bytes: int = 0) -> TwoGridJob:
    """ hk_two_grid_job from device rasters.  ``corr`` / ``valid`` / ``params``: ``dptr`` is the place of the window's first pixel of
    band 0 in the caller's raster (``params``: of parameter 0 of band 0; its ``band_stride`` separates consecutive planes, which are
    ordered parameter-major: plane p * n_bands + b) and ``shape[0]`` of ``params`` is n_param_bands * n_bands.  ``window`` /
    ``param_window``: (row0, col0, rows, cols) of the source block / of the parameter grid, None for the whole. """
    j = TwoGridJob()
    j.src, j.ref, j.corr = src.dptr or None, ref.dptr or None, corr.dptr or None
    j.valid = (valid.dptr or None) if valid is not None else None
    j.params = (params.dptr or None) if params is not None else None
    j.src_stride, j.src_band_stride, j.ref_stride, j.ref_band_stride = src.stride, src.band_stride, ref.stride, ref.band_stride
    j.corr_stride, j.corr_band_stride = corr.stride, corr.band_stride
    if valid is not None:
        j.valid_stride, j.valid_band_stride = valid.stride, valid.band_stride
    j.n_bands = src.shape[0]
    if params is not None:
        j.param_stride, j.param_band_stride = params.stride, params.band_stride
        j.n_param_bands = params.shape[0] // max(j.n_bands, 1)
    j.src_height, j.src_width, j.ref_height, j.ref_width = src.shape[1], src.shape[2], ref.shape[1], ref.shape[2]
    if window is not None:
        j.out_row0, j.out_col0, j.out_rows, j.out_cols = (int(v) for v in window)
    if param_window is not None:
        j.par_row0, j.par_col0, j.par_rows, j.par_cols = (int(v) for v in param_window)
    j.stream, j.reserved = int(stream), 0
    j.scratch, j.scratch_bytes = (int(scratch) or None), int(scratch_bytes)
    return j


def make_io_desc(src_dtype, ref_dtype, out_dtype, out_nodata=None) -> IoDesc:
    """ hk_io_desc from the three dtypes and the output nodata (``out_nodata_code``) """
    return IoDesc(DTYPE_CODES[np.dtype(src_dtype).name], DTYPE_CODES[np.dtype(ref_dtype).name], DTYPE_CODES[np.dtype(out_dtype).name],
                  *out_nodata_code(out_dtype, out_nodata))


def make_warp_desc(src_def, src_transform, dst_def, dst_transform) -> WarpDesc:
    """ hk_warp_desc from two CRS definitions (homonim_amd.crs.CrsDef) and the axis-aligned geo-transforms of their grids. """
    w = WarpDesc()
    for desc, d in ((w.src_crs, src_def), (w.dst_crs, dst_def)):
        desc.kind, desc.reserved = int(d.kind), 0
        desc.a, desc.inv_f, desc.lat0, desc.lon0, desc.k0, desc.fe, desc.fn = (float(v) for v in d[1:])
    for gt, t in ((w.src_gt, src_transform), (w.dst_gt, dst_transform)):
        if t.b or t.d:
            raise NotImplementedError('re-projection between rotated / sheared grids is not built')
        gt[0], gt[1], gt[2], gt[3] = float(t.c), float(t.a), float(t.f), float(t.e)
    return w


def make_affine_warp_desc(src_def, src_transform, dst_def, dst_transform) -> AffineWarpDesc:
    """ hk_affine_warp_desc from the geo-transforms of two grids, rotated and sheared ones included, and their CRS definitions
    (homonim_amd.crs.CrsDef).  Both definitions None: the grids share one CRS, whatever it is (``same_crs``). """
    if (src_def is None) != (dst_def is None):
        raise ValueError('give both CRS definitions, or neither for two grids of one CRS')
    w = AffineWarpDesc()
    w.same_crs, w.reserved = int(src_def is None), 0
    if src_def is not None:
        for desc, d in ((w.src_crs, src_def), (w.dst_crs, dst_def)):
            desc.kind, desc.reserved = int(d.kind), 0
            desc.a, desc.inv_f, desc.lat0, desc.lon0, desc.k0, desc.fe, desc.fn = (float(v) for v in d[1:])
    for gt, t in ((w.src_gt, src_transform), (w.dst_gt, dst_transform)):
        gt[0], gt[1], gt[2], gt[3], gt[4], gt[5] = float(t.a), float(t.b), float(t.c), float(t.d), float(t.e), float(t.f)
    return w


def _as_f32_2d(a: np.ndarray, name: str) -> np.ndarray:
    if a.ndim != 2:
        raise ValueError(f'`{name}` must be 2-D')
    if a.dtype != np.float32 or a.strides[1] != 4 or a.strides[0] % 4 != 0 or a.strides[0] < a.shape[1] * 4:
        a = np.ascontiguousarray(a, dtype=np.float32)
    return a


def _as_2d_native(a: np.ndarray, name: str) -> np.ndarray:
    """ 2-D raster in one of the dtypes the device converts itself (DTYPE_CODES); rows may be strided. """
    if a.ndim != 2:
        raise ValueError(f'`{name}` must be 2-D')
    if a.dtype.name not in DTYPE_CODES:
        a = a.astype(np.float32)
    it = a.dtype.itemsize
    if a.strides[1] != it or a.strides[0] % it != 0 or a.strides[0] < a.shape[1] * it:
        a = np.ascontiguousarray(a)
    return a


def _unit_column_stride(arr: np.ndarray):
    """ a (bands, h, w) raster as the strided entry points take it (unit column stride), copied if it is not: -> (array, itemsize) """
    it = arr.dtype.itemsize
    if arr.strides[2] != it or arr.strides[1] % it or arr.strides[1] < arr.shape[2] * it or arr.strides[0] % it or arr.strides[0] < 0:
        arr = np.ascontiguousarray(arr)
    return arr, it


def _ptr(a: np.ndarray, typ=_f32p):
    return a.ctypes.data_as(typ)


_live_contexts = weakref.WeakSet()


@atexit.register
def _close_live_contexts():
    """ Contexts still open when the interpreter exits are destroyed HERE -- while the library, the HIP runtime and this module
    are all intact -- instead of from garbage collection during shutdown. """
    for c in list(_live_contexts):
        try:
            c.close()
        except Exception:
            pass


class Context:
    """ One GPU context (hk_ctx): a device + a pool of streams.  Thread-safe; share it between worker threads. """

    def __init__(self, device: int = 0, n_streams: int = 4):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.hk_ctx_create(int(device), int(n_streams), C.byref(h))
        if rc != HK_OK:
            raise DeviceError(
                f"cannot create a GPU context on device {device}: {self._lib.hk_last_error().decode('utf-8', 'replace')}"
            )
        self._h = h
        self.device = device
        self.n_streams = n_streams
        _live_contexts.add(self)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.hk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        # never during interpreter shutdown: by then the order in which the runtime's own objects die is not ours to rely on (a
        # context that is still open is closed by the atexit hook below, before any teardown starts)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def selftest(self):
        _check(self._lib.hk_selftest(self._h))

    def sync(self):
        _check(self._lib.hk_ctx_sync(self._h))

    # -- host-pointer calls (numpy in / numpy out) --------------------------------------------------------------------
    def block_norm(self, desc: FitDesc, src: np.ndarray, ref: np.ndarray) -> np.ndarray:
        src, ref = _as_f32_2d(src, 'src'), _as_f32_2d(ref, 'ref')
        norm = np.zeros(2, np.float64)
        _check(self._lib.hk_block_norm(self._h, C.byref(desc), _ptr(src), src.strides[0] // 4, _ptr(ref),
                                       ref.strides[0] // 4, src.shape[0], src.shape[1], _ptr(norm, _f64p)))
        return norm

    def compare_sums(self, src: np.ndarray, src_nodata, ref: np.ndarray, ref_nodata) -> np.ndarray:
        """ float64[7] = [sum s, sum r, sum s^2, sum r^2, sum s*r, sum (r-s)^2, N] over the jointly valid pixels
        (homonim/compare.py:243-255) """
        src, ref = _as_f32_2d(src, 'src'), _as_f32_2d(ref, 'ref')
        if src.shape != ref.shape:
            raise ValueError('`src` and `ref` shapes differ')
        sums = np.zeros(7, np.float64)
        (sm, sv), (rm, rv) = nodata_code(src_nodata), nodata_code(ref_nodata)
        _check(self._lib.hk_compare_sums(self._h, _ptr(src), src.strides[0] // 4, sm, sv, _ptr(ref), ref.strides[0] // 4,
                                         rm, rv, src.shape[0], src.shape[1], _ptr(sums, _f64p)))
        return sums

    def param_stats(self, plane: np.ndarray, nodata=float('nan'), thresh: Optional[float] = None) -> np.ndarray:
        """ float64[10] = [min, max, sum x, sum x^2, N, N(x < thresh), col_min, row_min, col_max, row_max] over the valid
        pixels of one 2-D float32 raster in host memory (homonim/stats.py:217-229, :135-173; hk_param_stats).  ``thresh``
        None counts nothing. """
        plane = _as_f32_2d(plane, 'plane')
        stats = np.zeros(PARAM_STATS_N, np.float64)
        mode, value = nodata_code(nodata)
        _check(self._lib.hk_param_stats(self._h, _ptr(plane), plane.strides[0] // 4, mode, value,
                                        float('nan') if thresh is None else float(thresh), plane.shape[0], plane.shape[1],
                                        _ptr(stats, _f64p)))
        return stats

    def overviews(self, array: np.ndarray, nodata, n_levels: int, valid: Optional[np.ndarray] = None):
        """ Average overviews of a (bands, h, w) or (h, w) raster of any DTYPE_CODES dtype in host memory: ``n_levels`` arrays
        of the same rank and dtype, level m of shape (ceil(h / 2^m), ceil(w / 2^m)), each the clipped 2 x 2 mean of the
        valid pixels of the level before it (hk_overviews; all levels from one pass over the raster on the device).  Rows and
        bands may be strided (unit column stride); anything else is copied first.
        ``valid``: an (h, w) uint8 or bool validity plane of the raster, valid where not 0, in place of ``nodata`` (which is then
        not read): the masked build (hk_overviews_valid) -- a cell without a valid pixel gives 0 / NaN -- and the return value
        becomes ``(levels, level_valids)``, level_valids[m - 1] the (h_m, w_m) uint8 validity of level m, 255 / 0. """
        arr = np.asarray(array)
        squeeze = arr.ndim == 2
        if squeeze:
            arr = arr[None]
        if arr.ndim != 3 or arr.size == 0:
            raise ValueError('`array` must be a non-empty 2-D or 3-D raster')
        if arr.dtype.name not in DTYPE_CODES:
            raise ValueError(f"unsupported dtype '{arr.dtype}'")
        arr, it = _unit_column_stride(arr)
        nb, h, w = arr.shape
        n_levels = int(n_levels)
        if valid is not None:
            valid = np.asarray(valid)
            if valid.shape != (h, w) or valid.dtype not in (np.uint8, np.bool_):
                raise ValueError(f'`valid` must be a uint8 or bool plane of the raster\'s shape {(h, w)}, not {valid.dtype} {valid.shape}')
            if not 1 <= n_levels <= 31:
                raise ValueError(f'`n_levels` must lie in 1..31, not {n_levels}')
            valid = valid.view(np.uint8)
            if valid.strides[1] != 1 or valid.strides[0] < w:
                valid = np.ascontiguousarray(valid)
        if n_levels < 1:
            return []
        outs = [np.empty((nb, lh, lw), arr.dtype) for lh, lw in overview_shapes(h, w, n_levels)]
        ptrs = (C.c_void_p * n_levels)(*[o.ctypes.data for o in outs])
        strides = (C.c_int64 * n_levels)(*[o.shape[2] for o in outs])
        bstrides = (C.c_int64 * n_levels)(*[o.shape[1] * o.shape[2] for o in outs])
        head = (self._h, arr.ctypes.data_as(C.c_void_p), DTYPE_CODES[arr.dtype.name], nb, h, w, arr.strides[1] // it,
                arr.strides[0] // it if nb > 1 else 0)
        levels = lambda: [o[0] for o in outs] if squeeze else outs   # noqa: E731
        if valid is None:
            mode, value = nodata_code(nodata)
            _check(self._lib.hk_overviews(*head, mode, value, n_levels, ptrs, strides, bstrides))
            return levels()
        vouts = [np.empty(o.shape[1:], np.uint8) for o in outs]
        vptrs = (C.c_void_p * n_levels)(*[o.ctypes.data for o in vouts])
        vstrides = (C.c_int64 * n_levels)(*[o.shape[1] for o in vouts])
        _check(self._lib.hk_overviews_valid(*head, valid.ctypes.data_as(_P(C.c_uint8)), valid.strides[0], n_levels, ptrs, strides,
                                            bstrides, vptrs, vstrides))
        return levels(), vouts

    def dataset_mask(self, array: np.ndarray, mask: Optional[np.ndarray] = None, alpha: Optional[np.ndarray] = None) -> np.ndarray:
        """ The per-dataset mask of a GeoTIFF applied to its bands (hk_dataset_mask): a (bands, h, w) or (h, w) raster of any
        DTYPE_CODES dtype in host memory -> float32 of the same shape, ``float32(array)`` where the pixel is valid and NaN
        (0x7FC00000) elsewhere, every band alike.  Exactly one of ``mask``: the packed bits of an internal mask as
        ``tiff.TiffRaster.mask`` holds them, (h, ceil(w / 8)) uint8, most significant bit first, 1 = valid; ``alpha``: an (h, w)
        plane of the raster's dtype, which must be uint8 or uint16, valid where it is not 0 (it may be a band of a larger array:
        rows may be strided).  Rows of ``array`` may be strided (unit column stride); anything else is copied first. """
        arr = np.asarray(array)
        squeeze = arr.ndim == 2
        if squeeze:
            arr = arr[None]
        if arr.ndim != 3 or arr.size == 0:
            raise ValueError('`array` must be a non-empty 2-D or 3-D raster')
        if arr.dtype.name not in DTYPE_CODES:
            raise ValueError(f"unsupported dtype '{arr.dtype}'")
        if (mask is None) == (alpha is None):
            raise ValueError('exactly one of `mask` and `alpha` must be given')
        nb, h, w = arr.shape
        it = arr.dtype.itemsize
        # (the host entry takes the bands one behind the other: band stride = height x row stride)
        if arr.strides[2] != it or arr.strides[1] % it or arr.strides[1] < w * it or (nb > 1 and arr.strides[0] != h * arr.strides[1]):
            arr = np.ascontiguousarray(arr)
        if mask is not None:
            kind, m = MASK_BITS, np.asarray(mask)
            if m.dtype != np.uint8 or m.shape != (h, (w + 7) // 8):
                raise ValueError(f'`mask` must be uint8 of shape {(h, (w + 7) // 8)}: the packed bits of a {h} x {w} mask, not '
                                 f'{m.dtype} of shape {m.shape}')
            mit = 1
        else:
            kind, m = MASK_ALPHA, np.asarray(alpha)
            if arr.dtype.name not in ('uint8', 'uint16'):
                raise ValueError(f"an alpha band masks uint8 and uint16 rasters, not '{arr.dtype}'")
            if m.dtype != arr.dtype or m.shape != (h, w):
                raise ValueError(f'`alpha` must be {arr.dtype} of shape {(h, w)}, not {m.dtype} of shape {m.shape}')
            mit = it
        if m.strides[1] != mit or m.strides[0] % mit or m.strides[0] < m.shape[1] * mit:
            m = np.ascontiguousarray(m)
        out = np.empty((nb, h, w), np.float32)
        _check(self._lib.hk_dataset_mask(self._h, arr.ctypes.data_as(C.c_void_p), DTYPE_CODES[arr.dtype.name], nb, h, w,
                                         arr.strides[1] // it, m.ctypes.data_as(C.c_void_p), kind, m.strides[0] // mit, _ptr(out), w))
        return out[0] if squeeze else out

    def deflate_tiles_packed(self, array: np.ndarray, tile: int, predictor: int = 1):
        """ ``deflate_tiles`` as the library returns it: (uint8 array of the streams, int64 offsets [n_tiles + 1], int64 sizes
        [n_tiles]) -- tile t's stream is ``out[offsets[t]:offsets[t] + sizes[t]]``; offsets are even and ``offsets[-1]`` is the
        number of bytes used.  ``predictor``: 1 goes through hk_deflate_tiles as ever, anything else through
        hk_deflate_tiles_pred. """
        arr = np.asarray(array)
        if arr.ndim == 2:
            arr = arr[None]
        if arr.ndim != 3 or arr.size == 0:
            raise ValueError('`array` must be a non-empty 2-D or 3-D raster')
        if arr.dtype.name == 'int8':   # (the bytes are what is compressed: the signedness of a sample does not enter)
            arr = arr.view(np.uint8)
        if arr.dtype.name not in DTYPE_CODES:
            raise ValueError(f"unsupported dtype '{arr.dtype}'")
        if arr.dtype.byteorder == '>':
            arr = arr.astype(arr.dtype.newbyteorder('<'))
        arr, it = _unit_column_stride(arr)
        nb, h, w = arr.shape
        code, tile = DTYPE_CODES[arr.dtype.name], int(tile)
        n_tiles, cap = C.c_int64(), C.c_int64()
        _check(self._lib.hk_deflate_bound(code, nb, h, w, tile, C.byref(n_tiles), C.byref(cap)))
        out = np.empty(cap.value, np.uint8)
        offsets, sizes = np.empty(n_tiles.value + 1, np.int64), np.empty(n_tiles.value, np.int64)
        args = (self._h, arr.ctypes.data_as(C.c_void_p), code, nb, h, w, arr.strides[1] // it, arr.strides[0] // it if nb > 1 else 0,
                tile, out.ctypes.data_as(C.c_void_p), cap.value, offsets.ctypes.data_as(_P(C.c_int64)),
                sizes.ctypes.data_as(_P(C.c_int64)))
        if predictor == 1:
            _check(self._lib.hk_deflate_tiles(*args))
        else:
            _check(self._lib.hk_deflate_tiles_pred(*args, int(predictor)))
        return out, offsets, sizes

    def deflate_tiles(self, array: np.ndarray, tile: int, predictor: int = 1) -> list:
        """ One zlib stream per ``tile`` x ``tile`` tile of a (bands, h, w) or (h, w) raster in host memory, made on the device
        (hk_deflate_tiles; the stream format: include/homonim_hk.h): ``bytes`` objects in the order band, tile row, tile column,
        edge tiles zero-padded, samples little-endian -- what ``tiff.write_tiff`` takes as ``compressor``.  Any dtype
        ``write_tiff`` accepts; rows and bands may be strided (unit column stride), anything else is copied first.
        ``predictor``: the TIFF predictor (tag 317) applied to every padded tile row before it is coded (hk_deflate_tiles_pred):
        1 none, 2 horizontal differencing (integer dtypes), 3 the floating-point predictor (float32 / float64); a predictor the
        dtype does not take is a ``ValueError``. """
        out, offsets, sizes = self.deflate_tiles_packed(array, tile, predictor)
        return [out[o:o + n].tobytes() for o, n in zip(offsets[:-1].tolist(), sizes.tolist())]

    def inflate_image_packed(self, streams, offsets, sizes, layout, strict: bool = True):
        """ The image of ``layout`` (a ``tiff.BlockLayout``) from the zlib streams of its blocks, inflated, un-predicted and put
        in place on the device (hk_inflate_image): block b's stream is ``streams[offsets[b]:offsets[b] + sizes[b]]`` (``streams``:
        bytes or a uint8 array).  -> (array (spp, height, width) of uint8 / 16 / 32 / 64, int32 status per block).  A block whose
        stream is refused has a status other than 0 (``INFLATE_*``) and unspecified pixels; ``strict``: it raises ``IoError``
        naming the first such block instead. """
        return _blocks_image(self._lib.hk_inflate_image, self._h, streams, offsets, sizes, layout, strict)

    def inflate_image(self, streams, layout) -> np.ndarray:
        """ What ``tiff.read_tiff`` takes as ``inflater``: the zlib streams of an image's blocks (a list of ``bytes``, in the
        file's block order) -> its (spp, height, width) array of uint8 / 16 / 32 / 64, inflated on the device
        (``inflate_image_packed``).  ``IoError`` names the first block whose stream is refused, and why. """
        return self.inflate_image_packed(*_pack_streams(streams), layout, strict=True)[0]

    def lzw_image_packed(self, streams, offsets, sizes, layout, strict: bool = True):
        """ ``inflate_image_packed`` for the LZW streams (TIFF compression 5) of an image's blocks (hk_lzw_image): the same
        arguments and results; the statuses are ``LZW_*``. """
        return _blocks_image(self._lib.hk_lzw_image, self._h, streams, offsets, sizes, layout, strict)

    def lzw_image(self, streams, layout) -> np.ndarray:
        """ What ``tiff.read_tiff`` takes as ``lzw``: the LZW streams of an image's blocks (a list of ``bytes``, in the file's
        block order) -> its (spp, height, width) array of uint8 / 16 / 32 / 64, decoded on the device (``lzw_image_packed``).
        ``IoError`` names the first block whose stream is refused, and why. """
        return self.lzw_image_packed(*_pack_streams(streams), layout, strict=True)[0]

    # (what ``tiff.read_tiff`` looks at before it hands a predictor-3 image to a hook)
    inflate_image_packed.predictors = inflate_image.predictors = lzw_image_packed.predictors = lzw_image.predictors = PREDICTORS

    def fit_apply(self, desc: FitDesc, src: np.ndarray, ref: np.ndarray, n_param_bands: int, want_params: bool,
                  want_corr: bool, norm_in: Optional[np.ndarray] = None, out_params: Optional[np.ndarray] = None,
                  out_corr: Optional[np.ndarray] = None, out_dtype: str = 'float32', out_nodata: Optional[float] = None):
        """
        -> (params | None, corr | None, norm, r2_fail_count).

        ``src`` / ``ref`` may be float32 or any dtype of DTYPE_CODES (converted on the device as rasterio would on
        read); ``out_dtype`` / ``out_nodata`` convert the corrected block on the device as the reference does on write
        (round half-to-even, clip, masked pixels -> ``out_nodata``).  ``out_params`` / ``out_corr`` let the caller
        supply (e.g. pinned) C-contiguous output arrays.
        """
        src, ref = _as_2d_native(src, 'src'), _as_2d_native(ref, 'ref')
        if src.shape != ref.shape:
            raise ValueError("'ref_ra' and 'src_ra' must have the same CRS, transform and shape")
        h, w = src.shape
        out_dtype = np.dtype(out_dtype)
        if out_dtype.name not in DTYPE_CODES:
            raise ValueError(f'unsupported output dtype {out_dtype}')
        params = corr = None
        if want_params:
            params = out_params if out_params is not None else np.empty((n_param_bands, h, w), np.float32)
            assert params.shape == (n_param_bands, h, w) and params.dtype == np.float32 and params.flags['C_CONTIGUOUS']
        if want_corr:
            corr = out_corr if out_corr is not None else np.empty((h, w), out_dtype)
            assert corr.shape == (h, w) and corr.dtype == out_dtype and corr.flags['C_CONTIGUOUS']
        norm = np.zeros(2, np.float64)
        fail = C.c_uint64(0)
        nin = None
        if norm_in is not None:
            nin = np.ascontiguousarray(norm_in, dtype=np.float64)
        io = _io_desc(src, ref, out_dtype, out_nodata)
        vp = C.c_void_p
        _check(self._lib.hk_fit_apply_io(
            self._h, C.byref(desc), C.byref(io), src.ctypes.data_as(vp), src.strides[0] // src.dtype.itemsize,
            ref.ctypes.data_as(vp), ref.strides[0] // ref.dtype.itemsize, h, w,
            _ptr(nin, _f64p) if nin is not None else None, _ptr(params) if want_params else None, n_param_bands,
            corr.ctypes.data_as(vp) if want_corr else None, _ptr(norm, _f64p), C.byref(fail)))
        return params, corr, norm, int(fail.value)

    def fit_apply_block(self, desc: FitDesc, src: np.ndarray, ref: np.ndarray, window, corr_dst: Optional[np.ndarray],
                        params_dst: Optional[np.ndarray] = None, norm_in: Optional[np.ndarray] = None,
                        out_nodata: Optional[float] = None, valid_dst: Optional[np.ndarray] = None):
        """
        One block of RasterFuse.process (homonim/fuse.py:295-319) in one call: fit + apply on the read-block
        ``src`` / ``ref`` (2-D views, any dtype of DTYPE_CODES), and the window ``(row0, col0, rows, cols)`` of it -- the
        out-block -- written straight into ``corr_dst`` (2-D view of the caller's corrected raster where the out-block
        belongs, any DTYPE_CODES dtype, unit column stride) and ``params_dst`` (3-D view, float32).  With page-locked
        arrays (``pin`` / ``pinned_empty``) the transfers are asynchronous.  -> (norm, r2_fail_count)
        ``valid_dst``: a (rows, cols) uint8 view, unit column stride, that receives the window's validity -- 255 where the float32
        corrected value is not NaN, 0 where it is (hk_fit_apply_block_valid).  It needs ``corr_dst``, and its rows lie as many BYTES
        apart as ``corr_dst``'s lie elements: both are windows of rasters of one width.
        """
        src, ref = _as_2d_native(src, 'src'), _as_2d_native(ref, 'ref')
        if src.shape != ref.shape:
            raise ValueError("'ref_ra' and 'src_ra' must have the same CRS, transform and shape")
        h, w = src.shape
        row0, col0, rows, cols = (int(v) for v in window)
        vp = C.c_void_p
        n_param = 0
        stride = band_stride = 0
        out_dtype = np.dtype(np.float32)
        pstride = 0
        if corr_dst is not None:
            if corr_dst.shape != (rows, cols) or corr_dst.strides[1] != corr_dst.dtype.itemsize or \
                    corr_dst.strides[0] % corr_dst.dtype.itemsize or corr_dst.strides[0] < cols * corr_dst.dtype.itemsize:
                raise ValueError('`corr_dst` must be a (rows, cols) view of the window with unit column stride')
            out_dtype = corr_dst.dtype
            stride = corr_dst.strides[0] // corr_dst.dtype.itemsize
        if params_dst is not None:
            if params_dst.dtype != np.float32 or params_dst.ndim != 3 or params_dst.shape[1:] != (rows, cols) or \
                    params_dst.strides[2] != 4 or params_dst.strides[1] % 4 or params_dst.strides[0] % 4 or \
                    params_dst.strides[1] < 4 * cols or params_dst.strides[0] < 0:
                raise ValueError('`params_dst` must be a float32 (bands, rows, cols) view of the window with unit column stride')
            n_param = params_dst.shape[0]
            pstride = params_dst.strides[1] // 4  # its own row stride: the corrected and parameter rasters need not share one
            band_stride = params_dst.strides[0] // 4
            if corr_dst is None:
                stride = pstride
        if out_dtype.name not in DTYPE_CODES:
            raise ValueError(f'unsupported output dtype {out_dtype}')
        if valid_dst is not None:
            if corr_dst is None:
                raise ValueError('`valid_dst` needs `corr_dst`: validity is that of the corrected block')
            if valid_dst.dtype != np.uint8 or valid_dst.shape != (rows, cols) or valid_dst.strides[1] != 1 or \
                    (rows > 1 and valid_dst.strides[0] != stride):
                raise ValueError('`valid_dst` must be a uint8 (rows, cols) view of the window with unit column stride whose rows '
                                 f'lie {stride} bytes apart, `corr_dst`\'s row stride in elements')
        io = _io_desc(src, ref, out_dtype, out_nodata)
        win = OutWindow(stride, band_stride, row0, col0, rows, cols, pstride)
        norm = np.zeros(2, np.float64)
        fail = C.c_uint64(0)
        nin = np.ascontiguousarray(norm_in, dtype=np.float64) if norm_in is not None else None
        head = (self._h, C.byref(desc), C.byref(io), src.ctypes.data_as(vp), src.strides[0] // src.dtype.itemsize,
                ref.ctypes.data_as(vp), ref.strides[0] // ref.dtype.itemsize, h, w, _ptr(nin, _f64p) if nin is not None else None,
                params_dst.ctypes.data_as(vp) if params_dst is not None else None, n_param,
                corr_dst.ctypes.data_as(vp) if corr_dst is not None else None)
        tail = (C.byref(win), _ptr(norm, _f64p), C.byref(fail))
        if valid_dst is None:
            _check(self._lib.hk_fit_apply_block(*head, *tail))
        else:
            _check(self._lib.hk_fit_apply_block_valid(*head, valid_dst.ctypes.data_as(vp), *tail))
        return norm, int(fail.value)

    def apply(self, src: np.ndarray, params: np.ndarray) -> np.ndarray:
        src = _as_f32_2d(src, 'src')
        params = np.ascontiguousarray(params[:2], dtype=np.float32)
        if params.shape[-2:] != src.shape:
            raise ValueError("'param_ra' and 'src_ra' must have the same CRS, transform and shape")
        out = np.empty(src.shape, np.float32)
        _check(self._lib.hk_apply(self._h, _ptr(src), src.strides[0] // 4, _ptr(params), src.shape[0], src.shape[1],
                                  _ptr(out)))
        return out

    def refspace_fit_apply(self, desc: FitDesc, src: np.ndarray, ref: np.ndarray, down, up, down_resampling: int,
                           up_resampling: int, mask_partial: bool, n_param_bands: int, want_params: bool,
                           out_dtype: str = 'float32', out_nodata: Optional[float] = None,
                           out_corr: Optional[np.ndarray] = None, want_valid: bool = False):
        """ hk_refspace_fit_apply: RefSpaceModel.fit + apply of one block pair on different grids, all on the device.
        -> (params on the reference grid | None, corrected on the source grid, r2_fail_count), and with ``want_valid``
        (hk_refspace_fit_apply_valid) a fourth: the uint8 validity of the corrected block, 255 where its float32 value is not NaN """
        src, ref = _as_2d_native(src, 'src'), _as_2d_native(ref, 'ref')
        out_dtype = np.dtype(out_dtype)
        io = _io_desc(src, ref, out_dtype, out_nodata)
        sp = make_space_desc(down, up, down_resampling, up_resampling, mask_partial)
        params = np.empty((n_param_bands, *ref.shape), np.float32) if want_params else None
        corr = out_corr if out_corr is not None else np.empty(src.shape, out_dtype)
        assert corr.shape == src.shape and corr.dtype == out_dtype and corr.flags['C_CONTIGUOUS']
        fail = C.c_uint64(0)
        vp = C.c_void_p
        head = (self._h, C.byref(desc), C.byref(io), C.byref(sp), src.ctypes.data_as(vp), src.strides[0] // src.dtype.itemsize,
                src.shape[0], src.shape[1], ref.ctypes.data_as(vp), ref.strides[0] // ref.dtype.itemsize, ref.shape[0],
                ref.shape[1], _ptr(params) if want_params else None, n_param_bands, corr.ctypes.data_as(vp))
        if not want_valid:
            _check(self._lib.hk_refspace_fit_apply(*head, C.byref(fail)))
            return params, corr, int(fail.value)
        valid = np.empty(src.shape, np.uint8)
        _check(self._lib.hk_refspace_fit_apply_valid(*head, valid.ctypes.data_as(vp), C.byref(fail)))
        return params, corr, int(fail.value), valid

    def srcspace_fit_apply(self, desc: FitDesc, src: np.ndarray, ref: np.ndarray, mapping, resampling: int, mask_partial: bool,
                           n_param_bands: int, want_params: bool, out_dtype: str = 'float32',
                           out_nodata: Optional[float] = None, out_corr: Optional[np.ndarray] = None, want_valid: bool = False):
        """ hk_srcspace_fit_apply: SrcSpaceModel.fit + KernelModel.apply of one block pair on different grids, all on the device.
        ``mapping``: reference <- source grid as ``reproject`` takes it, both factors positive.  ``src`` / ``ref`` may be float32 or
        any dtype of DTYPE_CODES.  -> (params on the source grid | None, corrected on the source grid, r2_fail_count), and with
        ``want_valid`` (hk_srcspace_fit_apply_valid) a fourth: the uint8 validity of the corrected block, 255 where its float32 value
        is not NaN """
        src, ref = _as_2d_native(src, 'src'), _as_2d_native(ref, 'ref')
        out_dtype = np.dtype(out_dtype)
        if out_dtype.name not in DTYPE_CODES:
            raise ValueError(f'unsupported output dtype {out_dtype}')
        io = _io_desc(src, ref, out_dtype, out_nodata)
        sp = make_srcspace_desc(mapping, resampling, mask_partial)
        params = np.empty((n_param_bands, *src.shape), np.float32) if want_params else None
        corr = out_corr if out_corr is not None else np.empty(src.shape, out_dtype)
        assert corr.shape == src.shape and corr.dtype == out_dtype and corr.flags['C_CONTIGUOUS']
        fail = C.c_uint64(0)
        vp = C.c_void_p
        head = (self._h, C.byref(desc), C.byref(io), C.byref(sp), src.ctypes.data_as(vp), src.strides[0] // src.dtype.itemsize,
                src.shape[0], src.shape[1], ref.ctypes.data_as(vp), ref.strides[0] // ref.dtype.itemsize, ref.shape[0],
                ref.shape[1], _ptr(params) if want_params else None, n_param_bands, corr.ctypes.data_as(vp))
        if not want_valid:
            _check(self._lib.hk_srcspace_fit_apply(*head, C.byref(fail)))
            return params, corr, int(fail.value)
        valid = np.empty(src.shape, np.uint8)
        _check(self._lib.hk_srcspace_fit_apply_valid(*head, valid.ctypes.data_as(vp), C.byref(fail)))
        return params, corr, int(fail.value), valid

    def _two_grid_dev(self, entry, desc: FitDesc, sp, job: TwoGridJob, io: Optional[IoDesc]) -> np.ndarray:
        counts = np.zeros(max(int(job.n_bands), 1), np.uint64)
        _check(entry(self._h, C.byref(desc), C.byref(io) if io is not None else None, C.byref(sp), C.byref(job),
                     counts.ctypes.data_as(_u64p)))
        return counts[:max(int(job.n_bands), 0)]

    def refspace_fit_apply_dev(self, desc: FitDesc, down, up, down_resampling: int, up_resampling: int, mask_partial: bool,
                               job: TwoGridJob, io: Optional[IoDesc] = None) -> np.ndarray:
        """ hk_refspace_fit_apply_dev: ``refspace_fit_apply`` of every band of a device-resident job, queued on ``job.stream``; the
        windows of the corrected, validity and parameter planes go to their places in the caller's device rasters.  -> the per-band
        r2-mask failure counts (uint64; all 0 unless gain-offset runs with an r2 threshold, the one case in which the call waits). """
        return self._two_grid_dev(self._lib.hk_refspace_fit_apply_dev, desc,
                                  make_space_desc(down, up, down_resampling, up_resampling, mask_partial), job, io)

    def srcspace_fit_apply_dev(self, desc: FitDesc, mapping, resampling: int, mask_partial: bool, job: TwoGridJob,
                               io: Optional[IoDesc] = None) -> np.ndarray:
        """ hk_srcspace_fit_apply_dev: ``srcspace_fit_apply`` of every band of a device-resident job (see ``refspace_fit_apply_dev``) """
        return self._two_grid_dev(self._lib.hk_srcspace_fit_apply_dev, desc, make_srcspace_desc(mapping, resampling, mask_partial),
                                  job, io)

    def refspace_dev_scratch_bytes(self, desc: FitDesc, down, up, down_resampling: int, up_resampling: int, mask_partial: bool,
                                   job: TwoGridJob, io: Optional[IoDesc] = None) -> int:
        """ hk_refspace_dev_scratch_bytes: the size of ``job.scratch`` for this call, 0 for arguments the entry would refuse """
        return refspace_dev_scratch_bytes(desc, make_space_desc(down, up, down_resampling, up_resampling, mask_partial), job, io)

    def srcspace_dev_scratch_bytes(self, desc: FitDesc, mapping, resampling: int, mask_partial: bool, job: TwoGridJob,
                                   io: Optional[IoDesc] = None) -> int:
        return srcspace_dev_scratch_bytes(desc, make_srcspace_desc(mapping, resampling, mask_partial), job, io)

    def reproject(self, src: np.ndarray, src_nodata, mapping, dst_shape, resampling: int, dst_fill: float) -> np.ndarray:
        """ hk_reproject: (bands, h, w) or (h, w) float32 -> same rank on the destination grid. """
        arr = np.ascontiguousarray(src, dtype=np.float32)
        squeeze = arr.ndim == 2
        if squeeze:
            arr = arr[None]
        nb, sh, sw = arr.shape
        dh, dw = int(dst_shape[0]), int(dst_shape[1])
        out = np.empty((nb, dh, dw), np.float32)
        mode, val = nodata_code(src_nodata)
        kx, ox, ky, oy = [float(v) for v in mapping]
        _check(self._lib.hk_reproject(self._h, _ptr(arr), nb, sh, sw, mode, val, kx, ox, ky, oy, int(resampling),
                                      _ptr(out), dh, dw, float(dst_fill)))
        return out[0] if squeeze else out

    def warp_coords(self, warp: WarpDesc, shape, offset=(0.5, 0.5), out=None):
        """ hk_warp_coords: the continuous source pixel coordinates ``(x, y)`` (float64 planes of ``shape``) of the destination
        positions (row + offset[0], col + offset[1]) -- offset 0.5: pixel centres; offset 0 on a (h + 1, w + 1) lattice: corners.
        These are the coordinates ``reproject_crs`` uses.  ``out``: an (x, y) pair of float64 planes to fill, rows may be padded. """
        return self._warp_coords(self._lib.hk_warp_coords, warp, shape, offset, out)

    def _warp_coords(self, entry, warp, shape, offset, out):
        h, w = int(shape[0]), int(shape[1])
        x, y = out if out is not None else (np.empty((h, w), np.float64), np.empty((h, w), np.float64))
        for a in (x, y):
            if a.dtype != np.float64 or a.shape != (h, w) or a.strides[1] != 8 or a.strides[0] % 8:
                raise ValueError('coordinate planes must be float64 arrays of `shape` with contiguous rows')
        if x.strides[0] != y.strides[0]:
            raise ValueError('the two coordinate planes must share their row stride')
        _check(entry(self._h, C.byref(warp), float(offset[0]), float(offset[1]), h, w, _ptr(x, _f64p), _ptr(y, _f64p),
                     x.strides[0] // 8))
        return x, y

    def warp_coords_affine(self, warp: AffineWarpDesc, shape, offset=(0.5, 0.5), out=None):
        """ hk_warp_coords_affine: ``warp_coords`` between rotated / sheared grids; the coordinates ``reproject_affine`` uses. """
        return self._warp_coords(self._lib.hk_warp_coords_affine, warp, shape, offset, out)

    def warp_coords_affine_dev(self, warp: AffineWarpDesc, shape, x_dptr: int, y_dptr: int, stride: int, offset=(0.5, 0.5),
                               stream: int = 0):
        """ hk_warp_coords_affine_dev: the same into device planes (asynchronous). """
        _check(self._lib.hk_warp_coords_affine_dev(self._h, C.byref(warp), float(offset[0]), float(offset[1]), int(shape[0]),
                                                   int(shape[1]), C.c_void_p(x_dptr), C.c_void_p(y_dptr), int(stride), int(stream)))

    def warp_coords_dev(self, warp: WarpDesc, shape, x_dptr: int, y_dptr: int, stride: int, offset=(0.5, 0.5), stream: int = 0):
        """ hk_warp_coords_dev: the same into device planes (asynchronous). """
        _check(self._lib.hk_warp_coords_dev(self._h, C.byref(warp), float(offset[0]), float(offset[1]), int(shape[0]),
                                            int(shape[1]), C.c_void_p(x_dptr), C.c_void_p(y_dptr), int(stride), int(stream)))

    def reproject_crs(self, src: np.ndarray, src_nodata, warp: WarpDesc, scale, dst_shape, resampling: int,
                      dst_fill: float) -> np.ndarray:
        """ hk_reproject_crs: (bands, h, w) or (h, w) float32 -> same rank on a destination grid of another CRS; ``scale`` =
        (kx, ky), source pixels per destination pixel; all bands in one device call. """
        return self._reproject_warp(self._lib.hk_reproject_crs, src, src_nodata, warp, scale, dst_shape, resampling, dst_fill)

    def _reproject_warp(self, entry, src, src_nodata, warp, scale, dst_shape, resampling, dst_fill):
        arr = np.ascontiguousarray(src, dtype=np.float32)
        squeeze = arr.ndim == 2
        if squeeze:
            arr = arr[None]
        nb, sh, sw = arr.shape
        dh, dw = int(dst_shape[0]), int(dst_shape[1])
        out = np.empty((nb, dh, dw), np.float32)
        mode, val = nodata_code(src_nodata)
        _check(entry(self._h, C.byref(warp), _ptr(arr), nb, sh, sw, mode, val, float(scale[0]), float(scale[1]), int(resampling),
                     _ptr(out), dh, dw, float(dst_fill)))
        return out[0] if squeeze else out

    def reproject_affine(self, src: np.ndarray, src_nodata, warp: AffineWarpDesc, scale, dst_shape, resampling: int,
                         dst_fill: float) -> np.ndarray:
        """ hk_reproject_affine: ``reproject_crs`` between rotated / sheared grids, in one CRS or across two. """
        return self._reproject_warp(self._lib.hk_reproject_affine, src, src_nodata, warp, scale, dst_shape, resampling, dst_fill)

    def reproject_affine_dev(self, warp: AffineWarpDesc, src_dptr: int, n_bands: int, src_shape, src_stride: int,
                             src_band_stride: int, src_nodata, scale, resampling: int, dst_dptr: int, dst_shape, dst_stride: int,
                             dst_band_stride: int, dst_fill: float, stream: int = 0):
        """ hk_reproject_affine_dev: device rasters, strides in elements (asynchronous). """
        mode, val = nodata_code(src_nodata)
        _check(self._lib.hk_reproject_affine_dev(
            self._h, C.byref(warp), C.c_void_p(src_dptr), int(n_bands), int(src_shape[0]), int(src_shape[1]), int(src_stride),
            int(src_band_stride), mode, val, float(scale[0]), float(scale[1]), int(resampling), C.c_void_p(dst_dptr),
            int(dst_shape[0]), int(dst_shape[1]), int(dst_stride), int(dst_band_stride), float(dst_fill), int(stream)))

    def reproject_crs_dev(self, warp: WarpDesc, src_dptr: int, n_bands: int, src_shape, src_stride: int, src_band_stride: int,
                          src_nodata, scale, resampling: int, dst_dptr: int, dst_shape, dst_stride: int, dst_band_stride: int,
                          dst_fill: float, stream: int = 0):
        """ hk_reproject_crs_dev: device rasters, strides in elements (asynchronous). """
        mode, val = nodata_code(src_nodata)
        _check(self._lib.hk_reproject_crs_dev(
            self._h, C.byref(warp), C.c_void_p(src_dptr), int(n_bands), int(src_shape[0]), int(src_shape[1]), int(src_stride),
            int(src_band_stride), mode, val, float(scale[0]), float(scale[1]), int(resampling), C.c_void_p(dst_dptr),
            int(dst_shape[0]), int(dst_shape[1]), int(dst_stride), int(dst_band_stride), float(dst_fill), int(stream)))

    def reproject_dev(self, src_dptr: int, n_bands: int, src_shape, src_stride: int, src_band_stride: int, src_nodata, mapping,
                      resampling: int, dst_dptr: int, dst_shape, dst_stride: int, dst_band_stride: int, dst_fill: float,
                      stream: int = 0):
        """ hk_reproject_dev: ``reproject`` on device rasters, strides in elements (asynchronous). """
        mode, val = nodata_code(src_nodata)
        kx, ox, ky, oy = [float(v) for v in mapping]
        _check(self._lib.hk_reproject_dev(
            self._h, C.c_void_p(src_dptr), int(n_bands), int(src_shape[0]), int(src_shape[1]), int(src_stride),
            int(src_band_stride), mode, val, kx, ox, ky, oy, int(resampling), C.c_void_p(dst_dptr), int(dst_shape[0]),
            int(dst_shape[1]), int(dst_stride), int(dst_band_stride), float(dst_fill), int(stream)))

    def partial_mask(self, in_arr: np.ndarray, in_nodata, params: np.ndarray, kernel_shape, src: Optional[np.ndarray] = None,
                     want_params: bool = False, want_corr: bool = False, want_mask: bool = False, coverage: bool = False):
        """ mask_partial on a shared grid (hk_partial_mask) -> (masked params | None, corrected | None, mask | None).
        ``coverage``: ``in_arr`` is a coverage fraction (a mask re-projected with `average`), valid where >= 1. """
        in_arr = _as_f32_2d(in_arr, 'in')
        params = np.ascontiguousarray(params, dtype=np.float32)
        if params.ndim != 3 or params.shape[-2:] != in_arr.shape:
            raise ValueError("'param_ra' and 'src_ra' must have the same CRS, transform and shape")
        h, w = in_arr.shape
        if src is not None:
            src = _as_f32_2d(src, 'src')
        mode, val = (3, 0.0) if coverage else nodata_code(in_nodata)
        p_out = np.empty_like(params) if want_params else None
        c_out = np.empty((h, w), np.float32) if want_corr else None
        m_out = np.empty((h, w), np.uint8) if want_mask else None
        _check(self._lib.hk_partial_mask(
            self._h, _ptr(in_arr), in_arr.strides[0] // 4, mode, val, _ptr(params), params.shape[0],
            _ptr(src) if src is not None else None, (src.strides[0] // 4) if src is not None else 0, h, w,
            int(kernel_shape[0]), int(kernel_shape[1]), _ptr(p_out) if want_params else None,
            _ptr(c_out) if want_corr else None, m_out.ctypes.data_as(_P(C.c_uint8)) if want_mask else None))
        return p_out, c_out, m_out

    # -- pinned host memory (async H2D / D2H) ----------------------------------------------------------------------------
    def pinned_empty(self, shape, dtype=np.float32) -> np.ndarray:
        """ A numpy array in page-locked host memory: copies to / from it overlap with kernels of other calls.  The
        memory is released when the array (and every view of it) is garbage collected. """
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        _check(self._lib.hk_host_alloc(self._h, max(nbytes, 1), C.byref(p)))
        lib, addr = self._lib, p.value

        class _Owner:
            def __del__(self_inner):
                if sys.is_finalizing():  # the process is going away: its page-locked memory goes with it
                    return
                try:
                    lib.hk_host_free(None, C.c_void_p(addr))  # page-locked memory outlives the context it came from
                except Exception:
                    pass

        buf = (C.c_byte * max(nbytes, 1)).from_address(addr)
        buf._owner = _Owner()
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def pin(self, arr: np.ndarray) -> bool:
        """ Page-lock an existing C-contiguous array in place (hipHostRegister); undo with ``unpin``.  Registrations are
        counted per address range across the process: concurrent users of one array (two ``RasterFuse.process`` calls on
        the same source raster) share one registration and the last ``unpin`` removes it.  Memory that is page-locked
        already by somebody else (``pinned_empty``, an enclosing registration) is left as it is.  -> whether the range is
        page-locked now. """
        if not arr.flags['C_CONTIGUOUS']:
            raise ValueError('only C-contiguous arrays can be page-locked in place')
        key = (arr.ctypes.data, arr.nbytes)
        with _pin_lock:
            ent = _pins.get(key)
            if ent is not None:
                ent[0] += 1
                return True
            rc = self._lib.hk_host_register(self._h, C.c_void_p(key[0]), key[1])
            if rc == HK_ERR_ALREADY:
                _pins[key] = [1, False]   # not ours to unregister
                return True
            _check(rc)
            _pins[key] = [1, True]
            return True

    def unpin(self, arr: np.ndarray):
        key = (arr.ctypes.data, arr.nbytes)
        with _pin_lock:
            ent = _pins.get(key)
            if ent is None:
                return
            ent[0] -= 1
            if ent[0] > 0:
                return
            del _pins[key]
            if ent[1]:
                _check(self._lib.hk_host_unregister(self._h, C.c_void_p(key[0])))

    def stream_probe_dev(self, a_dptr: int, b_dptr: int, out_dptr: int, nbytes: int, stream: int = 0):
        """ One launch of the flat 2-read 1-write float4 stream out = a + b over three device buffers (hk_stream_probe_dev). """
        _check(self._lib.hk_stream_probe_dev(self._h, C.c_void_p(a_dptr), C.c_void_p(b_dptr), C.c_void_p(out_dptr), nbytes, stream))

    def checksum_dev(self, plane_dptr: int, stride: int, height: int, width: int, stream: int = 0) -> int:
        """ Sum of the 32-bit patterns of a height x width window of a device-resident float32 plane, modulo 2^64
        (hk_debug_checksum_dev: exact and order-free; synchronises the stream). """
        out = C.c_uint64(0)
        _check(self._lib.hk_debug_checksum_dev(self._h, C.c_void_p(plane_dptr), stride, height, width, stream, C.byref(out)))
        return int(out.value)

    def inpaint_plane_dev(self, plane_dptr: int, flags_dptr: Optional[int], gain_dptr: Optional[int], r2_dptr: Optional[int],
                          thresh: float, height: int, width: int, stride: int, mode: int = 0, stream: int = 0):
        """ The in-painting step alone on device-resident planes (hk_debug_inpaint_plane_dev; synchronises the stream). """
        vp = lambda p: C.c_void_p(p) if p else None   # noqa: E731
        _check(self._lib.hk_debug_inpaint_plane_dev(self._h, vp(plane_dptr), vp(flags_dptr), vp(gain_dptr), vp(r2_dptr),
                                                    float(thresh), int(height), int(width), int(stride), int(mode), int(stream)))

    def inpaint_plane(self, plane: np.ndarray, flags: Optional[np.ndarray] = None, gain: Optional[np.ndarray] = None,
                      r2: Optional[np.ndarray] = None, thresh: Optional[float] = None, mode: int = 0,
                      stride: Optional[int] = None, pad_value: Optional[float] = None, pad_flag: Optional[int] = None) -> np.ndarray:
        """ Test aid: in-paint the targets of a 2-D float32 ``plane`` from its sources, the in-painting step of the gain-offset
        model on its own.  The mask is ``flags`` (uint8: 1 source, 0 target, 2 neither) or ``gain`` / ``r2`` / ``thresh``
        (source = (r2 > thresh) & (gain > 0)).  ``mode``: see hk_debug_inpaint_plane_dev.  ``stride`` (elements, default: the
        width rounded up to 4) is the row pitch of every plane on the device; the padding holds ``pad_value`` (planes) and
        ``pad_flag`` (flags), zero by default.  -> the filled height x width plane. """
        if flags is not None and (gain is not None or r2 is not None or thresh is not None):
            raise ValueError('give either `flags` or `gain` / `r2` / `thresh`')
        if flags is None and (gain is None or r2 is None or thresh is None):
            raise ValueError('without `flags`, all of `gain`, `r2` and `thresh` are needed')
        plane = np.ascontiguousarray(plane, np.float32)
        if plane.ndim != 2 or plane.size == 0:
            raise ValueError('`plane` must be a non-empty 2-D raster')
        h, w = plane.shape
        stride = (w + 3) // 4 * 4 if stride is None else int(stride)
        if stride < w:
            raise ValueError(f'stride {stride} is less than the width {w}')

        def padded(a, dtype, name, pad):
            a = np.asarray(a)
            if a.shape != (h, w):
                raise ValueError(f'`{name}` must have the shape of `plane`')
            out = np.full((h, stride), 0 if pad is None else pad, dtype)
            out[:, :w] = a
            return out

        if flags is not None:
            hosts = [padded(plane, np.float32, 'plane', pad_value), padded(flags, np.uint8, 'flags', pad_flag), None, None]
        else:
            hosts = [padded(plane, np.float32, 'plane', pad_value), None, padded(gain, np.float32, 'gain', pad_value),
                     padded(r2, np.float32, 'r2', pad_value)]
        dptrs = [None] * 4
        try:
            for i, a in enumerate(hosts):
                if a is not None:
                    dptrs[i] = self.dev_alloc(a.nbytes)
                    self.h2d(dptrs[i], a)
            self.inpaint_plane_dev(dptrs[0], dptrs[1], dptrs[2], dptrs[3], 0.0 if flags is not None else thresh, h, w, stride, mode)
            out = np.empty((h, stride), np.float32)
            self.d2h(out, dptrs[0])
        finally:
            for p in dptrs:
                if p:
                    self.dev_free(p)
        return np.ascontiguousarray(out[:, :w])

    def cast_plane_dev(self, to_typed: bool, dtype, src_dptr: int, src_stride: int, dst_dptr: int, dst_stride: int, height: int,
                       width: int, has_nodata: bool = False, nodata: float = 0.0, stream: int = 0):
        """ One dtype conversion of hk_convert.hip alone on device-resident planes (hk_debug_cast_plane_dev; synchronises the
        stream).  ``dtype``: a name of DTYPE_CODES or an hk_dtype code. """
        code = dtype if isinstance(dtype, int) else DTYPE_CODES[np.dtype(dtype).name]
        vp = lambda p: C.c_void_p(p) if p else None   # noqa: E731
        _check(self._lib.hk_debug_cast_plane_dev(self._h, int(bool(to_typed)), code, vp(src_dptr), int(src_stride), vp(dst_dptr),
                                                 int(dst_stride), int(height), int(width), int(bool(has_nodata)), float(nodata),
                                                 int(stream)))

    def _cast_plane(self, to_typed, array, dst_dtype, dtype, has_nodata, nodata, stride, dst_stride, sentinel, full):
        if array.ndim != 2 or array.size == 0:
            raise ValueError('`array` must be a non-empty 2-D raster')
        h, w = array.shape
        stride = (w + 3) // 4 * 4 if stride is None else int(stride)
        dst_stride = stride if dst_stride is None else int(dst_stride)
        if stride < w or dst_stride < w:
            raise ValueError(f'stride {min(stride, dst_stride)} is less than the width {w}')
        src = np.zeros((h, stride), array.dtype)   # the padding of the source rows is zero
        src[:, :w] = array
        out = np.empty((h, dst_stride), dst_dtype)
        out.view(np.uint8)[...] = sentinel
        dptrs = [None, None]
        try:
            dptrs[0], dptrs[1] = self.dev_alloc(src.nbytes), self.dev_alloc(out.nbytes)
            self.h2d(dptrs[0], src)
            self.h2d(dptrs[1], out)
            self.cast_plane_dev(to_typed, dtype, dptrs[0], stride, dptrs[1], dst_stride, h, w, has_nodata, nodata)
            self.d2h(out, dptrs[1])
        finally:
            for p in dptrs:
                if p:
                    self.dev_free(p)
        return out if full else np.ascontiguousarray(out[:, :w])

    def cast_in_plane(self, array: np.ndarray, stride: Optional[int] = None, dst_stride: Optional[int] = None, sentinel: int = 0xA5,
                      full: bool = False) -> np.ndarray:
        """ Test aid: a 2-D raster of an integer type of DTYPE_CODES or of float64 converted to float32 by the device's input
        conversion alone (cast_in_kernel: what RasterArray.from_rio_dataset's read with out_dtype float32 gives).  ``stride`` /
        ``dst_stride`` (elements; default: the width rounded up to 4, and ``stride``) are the row pitches of the source and
        the destination plane on the device; the source's padding holds zero, every byte of the destination holds ``sentinel``
        before the call.  -> the height x width result, or with ``full`` the whole height x dst_stride plane. """
        array = np.asarray(array)
        if array.dtype.name not in DTYPE_CODES or array.dtype == np.float32:
            raise ValueError(f"no input conversion from dtype '{array.dtype}'")
        return self._cast_plane(False, array, np.float32, array.dtype, False, 0.0, stride, dst_stride, sentinel, full)

    def cast_out_plane(self, array_f32: np.ndarray, dtype, nodata, stride: Optional[int] = None, dst_stride: Optional[int] = None,
                       sentinel: int = 0xA5, full: bool = False) -> np.ndarray:
        """ Test aid: a 2-D float32 raster converted to ``dtype`` by the device's output conversion alone (cast_out_kernel:
        RasterArray._convert_array_dtype -- round half to even, clip, NaN -> ``nodata``); ``nodata`` as ``fit_apply`` takes
        ``out_nodata``.  Strides, padding, ``sentinel`` and ``full`` as for ``cast_in_plane``. """
        dtype = np.dtype(dtype)
        if dtype.name not in DTYPE_CODES:
            raise ValueError(f'unsupported output dtype {dtype}')
        has, value = out_nodata_code(dtype, nodata)
        return self._cast_plane(True, np.asarray(array_f32, np.float32), dtype, dtype, has, value, stride, dst_stride, sentinel, full)

    # -- device-resident helpers (bench / streaming) ------------------------------------------------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self._lib.hk_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, dptr: int):
        _check(self._lib.hk_dev_free(self._h, C.c_void_p(dptr)))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _check(self._lib.hk_memcpy_h2d(self._h, C.c_void_p(dptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def d2h(self, arr: np.ndarray, dptr: int, nbytes: Optional[int] = None):
        assert arr.flags['C_CONTIGUOUS']
        _check(self._lib.hk_memcpy_d2h(self._h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr),
                                       arr.nbytes if nbytes is None else nbytes))

    def memset(self, dptr: int, value: int, nbytes: int):
        _check(self._lib.hk_memset(self._h, C.c_void_p(dptr), value, nbytes))

    def block_norm_split_phase(self, desc: FitDesc, job: DevJob, phase: int, world_size: int, xchg_dev: int, norm_dev: int):
        """ Queue phase 0..5 of the split-block statistics on this rank's slab (see homonim_amd/split_norm.py). """
        _check(self._lib.hk_block_norm_split_dev(self._h, C.byref(desc), C.byref(job), phase, world_size,
                                                 C.c_void_p(xchg_dev), C.c_void_p(norm_dev)))

    def split_exchange_doubles(self, n_bands: int) -> int:
        return int(self._lib.hk_block_norm_split_exchange_doubles(n_bands))

    # -- the library's own RCCL communicator (one per context; the split-block statistics are its one user) ------------
    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        """ Join the RCCL communicator named by ``unique_id`` (``comm_unique_id()`` of rank 0, handed over by the launcher;
        ``homonim_amd.dist.init_comm`` does that).  Collective: returns when every rank has joined. """
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f'the communicator id has {COMM_ID_BYTES} bytes')
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._lib.hk_comm_init(self._h, buf, rank, world_size))

    def comm_destroy(self):
        _check(self._lib.hk_comm_destroy(self._h))

    def comm_info(self):
        """ -> (rank, world_size) of the context's communicator; (-1, 0) without one. """
        r, w = C.c_int32(-1), C.c_int32(0)
        _check(self._lib.hk_comm_info(self._h, C.byref(r), C.byref(w)))
        return int(r.value), int(w.value)

    def comm_allreduce_f64_dev(self, buf_dptr: int, count: int, stream: int = 0):
        _check(self._lib.hk_comm_allreduce_f64_dev(self._h, C.c_void_p(buf_dptr), count, stream))

    def block_norm_split_comm_dev(self, desc: FitDesc, job: DevJob, norm_dev: int):
        """ Split-block statistics of this rank's slab over the context's communicator: six phases + five RCCL all-reduces
        queued on the job's stream (hk_block_norm_split_comm_dev; asynchronous, collective). """
        _check(self._lib.hk_block_norm_split_comm_dev(self._h, C.byref(desc), C.byref(job), C.c_void_p(norm_dev)))

    def job_scratch_bytes(self, job: DevJob) -> int:
        """ Size of the optional DevJob.scratch (gain-offset with an r2 threshold: the in-painting's inputs). """
        return int(self._lib.hk_dev_job_scratch_bytes(job.n_bands, job.height, job.stride, job.band_stride))

    def fit_apply_dev(self, desc: FitDesc, job: DevJob):
        _check(self._lib.hk_fit_apply_dev(self._h, C.byref(desc), C.byref(job)))

    def counts_pending(self, counts: np.ndarray) -> bool:
        """ Do the counters of a launch (``fail_counts_async``) call for its second half, ``inpaint_dev_counts``?  (failing
        pixels in some band: hk_counts_pending) """
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        return bool(self._lib.hk_counts_pending(c.ctypes.data_as(_P(C.c_uint64)), int(c.size)))

    def fail_counts_async(self, job: DevJob, host_counts: np.ndarray, ready_event: int):
        """ Queue the copy of the job's failure counters into a PINNED uint64 array, their clearing and `ready_event`. """
        assert host_counts.dtype == np.uint64 and host_counts.flags['C_CONTIGUOUS']
        _check(self._lib.hk_fail_counts_async(self._h, C.byref(job), host_counts.ctypes.data_as(_P(C.c_uint64)),
                                              C.c_void_p(ready_event)))

    def event_sync(self, ev: int):
        _check(self._lib.hk_event_sync(self._h, C.c_void_p(ev)))

    def inpaint_dev_counts(self, desc: FitDesc, job: DevJob, counts: np.ndarray) -> int:
        """ In-paint the bands whose count (host array, from fail_counts_async) is non-zero; only queues work. """
        n = C.c_uint64(0)
        counts = np.ascontiguousarray(counts, np.uint64)
        _check(self._lib.hk_inpaint_dev_counts(self._h, C.byref(desc), C.byref(job), counts.ctypes.data_as(_P(C.c_uint64)),
                                               C.byref(n)))
        return int(n.value)

    def inpaint_dev(self, desc: FitDesc, job: DevJob) -> int:
        """ In-paint the bands of a device-resident job whose r2 mask has failures; returns the failure count. """
        n = C.c_uint64(0)
        _check(self._lib.hk_inpaint_dev(self._h, C.byref(desc), C.byref(job), C.byref(n)))
        return int(n.value)

    def block_norm_dev(self, desc: FitDesc, job: DevJob, norm_dptr: int):
        _check(self._lib.hk_block_norm_dev(self._h, C.byref(desc), C.byref(job), C.c_void_p(norm_dptr)))

    @staticmethod
    def job_array(jobs) -> 'C.Array':
        """ The jobs of a batched launch as one contiguous ctypes array (build it once, pass it to every step). """
        if isinstance(jobs, C.Array):
            return jobs
        arr = (DevJob * len(jobs))()
        for i, j in enumerate(jobs):
            C.memmove(C.byref(arr, i * C.sizeof(DevJob)), C.byref(j), C.sizeof(DevJob))
        return arr

    def block_norm_batch_dev(self, desc: FitDesc, jobs, norm_dptr: int):
        """ The block statistics of many device-resident jobs in one launch per kernel stage (hk_block_norm_batch_dev):
        job 0's n_bands x 2 float64 first, then job 1's ... into `norm_dptr`; all on jobs[0].stream. """
        arr = self.job_array(jobs)
        _check(self._lib.hk_block_norm_batch_dev(self._h, C.byref(desc), arr, len(arr), C.c_void_p(norm_dptr)))

    def fit_apply_batch_dev(self, desc: FitDesc, jobs):
        """ Many device-resident jobs as ONE fused launch on jobs[0].stream (hk_fit_apply_batch_dev); every job reads its own
        ``norm`` pointer and, with an r2 threshold, is finished by its own ``inpaint_dev*`` call. """
        arr = self.job_array(jobs)
        _check(self._lib.hk_fit_apply_batch_dev(self._h, C.byref(desc), arr, len(arr)))

    def fail_counts_batch_async(self, jobs, host_counts: np.ndarray, ready_event: int):
        """ ``fail_counts_async`` for the jobs of a batch: all their counters, job after job, into one PINNED uint64 array. """
        arr = self.job_array(jobs)
        assert host_counts.dtype == np.uint64 and host_counts.flags['C_CONTIGUOUS']
        assert host_counts.size >= sum(j.n_bands for j in arr)
        _check(self._lib.hk_fail_counts_batch_async(self._h, arr, len(arr), host_counts.ctypes.data_as(_P(C.c_uint64)),
                                                    C.c_void_p(ready_event)))

    def debug_stage_stamps(self, reset: bool = True) -> np.ndarray:
        """ Stage counters of a -DHK_STAMPS build of the fused kernel (hk_debug_stage_stamps; zeros in the shipped build). """
        out = (C.c_uint64 * 16)()
        _check(self._lib.hk_debug_stage_stamps(self._h, out, 1 if reset else 0))
        return np.array(list(out), dtype=np.uint64)

    def compare_sums_dev(self, job: DevJob, src_nodata, ref_nodata, sums_dptr: int):
        (sm, sv), (rm, rv) = nodata_code(src_nodata), nodata_code(ref_nodata)
        _check(self._lib.hk_compare_sums_dev(self._h, C.byref(job), sm, sv, rm, rv, C.c_void_p(sums_dptr)))

    def param_stats_dev(self, planes_dptr: int, n_bands: int, height: int, width: int, stride: int, band_stride: int,
                        stats_dptr: int, nodata=float('nan'), thresh: Optional[float] = None, stream: int = 0):
        """ Queue the statistics of ``n_bands`` device-resident float32 planes in one launch: ``n_bands`` x 10 float64 into
        ``stats_dptr`` (hk_param_stats_dev; asynchronous). """
        mode, value = nodata_code(nodata)
        _check(self._lib.hk_param_stats_dev(self._h, C.c_void_p(planes_dptr), n_bands, height, width, stride, band_stride,
                                            stream, mode, value, float('nan') if thresh is None else float(thresh),
                                            C.c_void_p(stats_dptr)))

    def overviews_dev(self, planes_dptr: int, dtype: str, n_bands: int, height: int, width: int, stride: int, band_stride: int,
                      nodata, out_dptrs: Sequence[int], out_strides: Sequence[int], out_band_strides: Sequence[int],
                      stream: int = 0):
        """ Queue the average overviews of ``n_bands`` device-resident planes of dtype ``dtype``: level m = 1..len(out_dptrs)
        into ``out_dptrs[m - 1]`` (strides in elements; hk_overviews_dev; asynchronous). """
        n = len(out_dptrs)
        mode, value = nodata_code(nodata)
        _check(self._lib.hk_overviews_dev(self._h, C.c_void_p(planes_dptr), DTYPE_CODES[np.dtype(dtype).name], n_bands, height,
                                          width, stride, band_stride, mode, value, n, (C.c_void_p * n)(*out_dptrs),
                                          (C.c_int64 * n)(*out_strides), (C.c_int64 * n)(*out_band_strides), stream))

    def overviews_valid_dev(self, planes_dptr: int, dtype: str, n_bands: int, height: int, width: int, stride: int, band_stride: int,
                            valid_dptr: int, valid_stride: int, out_dptrs: Sequence[int], out_strides: Sequence[int],
                            out_band_strides: Sequence[int], out_valid_dptrs: Sequence[int], out_valid_strides: Sequence[int],
                            stream: int = 0):
        """ ``overviews_dev`` under the device-resident uint8 validity plane ``valid_dptr`` (valid where not 0, ``valid_stride`` bytes
        between rows) in place of a nodata value; level m's own validity (255 / 0) goes to ``out_valid_dptrs[m - 1]``
        (hk_overviews_valid_dev; asynchronous). """
        n = len(out_dptrs)
        if len(out_valid_dptrs) != n or len(out_valid_strides) != n:
            raise ValueError(f'{len(out_valid_dptrs)} validity planes for {n} levels')
        _check(self._lib.hk_overviews_valid_dev(self._h, C.c_void_p(planes_dptr), DTYPE_CODES[np.dtype(dtype).name], n_bands, height,
                                                width, stride, band_stride, C.c_void_p(valid_dptr), valid_stride, n,
                                                (C.c_void_p * n)(*out_dptrs), (C.c_int64 * n)(*out_strides),
                                                (C.c_int64 * n)(*out_band_strides), (C.c_void_p * n)(*out_valid_dptrs),
                                                (C.c_int64 * n)(*out_valid_strides), stream))

    def dataset_mask_dev(self, planes_dptr: int, dtype: str, n_bands: int, height: int, width: int, stride: int, band_stride: int,
                         mask_dptr: int, mask_kind: int, mask_stride: int, out_dptr: int, out_stride: int, out_band_stride: int,
                         stream: int = 0):
        """ Queue the per-dataset mask of ``n_bands`` device-resident planes of dtype ``dtype``: float32 planes into ``out_dptr``
        (``mask_kind``: MASK_BITS -- packed rows, ``mask_stride`` in bytes -- or MASK_ALPHA -- a plane of ``dtype``, ``mask_stride``
        in elements; the other strides in elements; hk_dataset_mask_dev; asynchronous). """
        _check(self._lib.hk_dataset_mask_dev(self._h, C.c_void_p(planes_dptr), DTYPE_CODES[np.dtype(dtype).name], n_bands, height,
                                             width, stride, band_stride, C.c_void_p(mask_dptr), int(mask_kind), mask_stride,
                                             C.c_void_p(out_dptr), out_stride, out_band_stride, stream))

    def fill_planes_dev(self, planes_dptr: int, dtype, n_bands: int, height: int, width: int, stride: int, band_stride: int, value,
                        stream: int = 0):
        """ Queue the typed prefill of ``n_bands`` device-resident planes of dtype ``dtype`` (strides in elements): ``value`` -- NaN
        allowed for the float types -- into ``width`` samples of every row, nothing into the row padding (hk_fill_planes_dev;
        asynchronous). """
        _check(self._lib.hk_fill_planes_dev(self._h, C.c_void_p(planes_dptr), DTYPE_CODES[np.dtype(dtype).name], n_bands, height, width,
                                            stride, band_stride, float(value), stream))

    def boundless_window_dev(self, raster: 'DeviceRaster', window, out_dptr: int, out_stride: Optional[int] = None,
                             out_band_stride: Optional[int] = None, stream: int = 0) -> 'DeviceRaster':
        """ Queue the window ``(row_off, col_off, height, width)`` of a device-resident raster -- it may hang over the raster or miss it
        -- into ``out_dptr``, all bands in one launch (hk_boundless_window_dev; asynchronous): what ``RasterFuse._read_boundless``
        gives on the host.  A window inside the raster is a copy in the raster's dtype under the raster's nodata.  One that reaches
        beyond it: a raster with a numeric nodata gives a window of its own dtype with the nodata outside; one without a nodata
        value, or with NaN, gives float32 with NaN outside.  -> the window as a ``DeviceRaster`` with that dtype and nodata (grid
        and CRS are not set). """
        row_off, col_off, height, width = (int(v) for v in window)
        mode, value = nodata_code(raster.nodata)
        inside = row_off >= 0 and col_off >= 0 and row_off + height <= raster.shape[1] and col_off + width <= raster.shape[2]
        to_float = mode != NODATA_VALUE and not inside
        if inside:   # (no fill is written)
            mode, value = NODATA_VALUE, 0.0
        elif not to_float:   # the fill as numpy.full puts it into an array of the raster's dtype
            value = float(np.full((), raster.nodata, raster.dtype))
        out = DeviceRaster(out_dptr, np.float32 if to_float else raster.dtype, (raster.shape[0], height, width), out_stride,
                           out_band_stride, nodata=float('nan') if to_float else raster.nodata)
        _check(self._lib.hk_boundless_window_dev(self._h, C.c_void_p(raster.dptr), DTYPE_CODES[raster.dtype.name], raster.shape[0],
                                                 raster.shape[1], raster.shape[2], raster.stride, raster.band_stride, row_off, col_off,
                                                 height, width, mode, 0.0 if to_float else value, C.c_void_p(out_dptr), out.stride,
                                                 out.band_stride, stream))
        return out

    def mem_info(self):
        """ -> (free, total) bytes of the context's device as the runtime reports them (hk_dev_mem_info) """
        free, total = C.c_uint64(), C.c_uint64()
        _check(self._lib.hk_dev_mem_info(self._h, C.byref(free), C.byref(total)))
        return int(free.value), int(total.value)

    def deflate_tiles_dev(self, planes_dptr: int, dtype: str, n_bands: int, height: int, width: int, stride: int, band_stride: int,
                          tile: int, out_dptr: int, out_capacity: int, offsets_dptr: int, sizes_dptr: int, stream: int = 0,
                          predictor: int = 1):
        """ Queue the zlib streams of the tiles of ``n_bands`` device-resident planes of dtype ``dtype`` (strides in elements):
        the streams into ``out_dptr`` (``deflate_bound`` bytes), ``n_tiles + 1`` int64 offsets into ``offsets_dptr``, ``n_tiles``
        int64 sizes into ``sizes_dptr`` (hk_deflate_tiles_dev; asynchronous).  ``predictor``: as in ``deflate_tiles``; other
        than 1 the call is hk_deflate_tiles_pred_dev. """
        args = (self._h, C.c_void_p(planes_dptr), DTYPE_CODES[np.dtype(dtype).name], n_bands, height, width, stride, band_stride,
                tile, C.c_void_p(out_dptr), out_capacity, C.c_void_p(offsets_dptr), C.c_void_p(sizes_dptr), stream)
        if predictor == 1:
            _check(self._lib.hk_deflate_tiles_dev(*args))
        else:
            _check(self._lib.hk_deflate_tiles_pred_dev(*args, int(predictor)))

    def inflate_image_dev(self, layout, streams_dptr: int, offsets_dptr: int, sizes_dptr: int, work_dptr: int, out_dptr: int,
                          stride: int, band_stride: int, status_dptr: int, stream: int = 0):
        """ Queue the inflation of an image's blocks from device-resident streams (``n_blocks`` int64 offsets and sizes) into the
        raster at ``out_dptr`` (strides in elements) and ``n_blocks`` int32 statuses at ``status_dptr``; ``work_dptr``:
        ``inflate_bound``'s scratch bytes (hk_inflate_image_dev; asynchronous). """
        _check(self._lib.hk_inflate_image_dev(self._h, C.byref(_inflate_layout(layout)), C.c_void_p(streams_dptr), C.c_void_p(offsets_dptr),
                                              C.c_void_p(sizes_dptr), C.c_void_p(work_dptr), C.c_void_p(out_dptr), stride, band_stride,
                                              C.c_void_p(status_dptr), stream))

    def lzw_image_dev(self, layout, streams_dptr: int, offsets_dptr: int, sizes_dptr: int, work_dptr: int, out_dptr: int,
                      stride: int, band_stride: int, status_dptr: int, stream: int = 0):
        """ ``inflate_image_dev`` for device-resident LZW streams (hk_lzw_image_dev; asynchronous): the statuses are ``LZW_*``. """
        _check(self._lib.hk_lzw_image_dev(self._h, C.byref(_inflate_layout(layout)), C.c_void_p(streams_dptr), C.c_void_p(offsets_dptr),
                                          C.c_void_p(sizes_dptr), C.c_void_p(work_dptr), C.c_void_p(out_dptr), stride, band_stride,
                                          C.c_void_p(status_dptr), stream))

    inflate_image_dev.predictors = lzw_image_dev.predictors = PREDICTORS

    def synth_fill_dev(self, src_dptr, ref_dptr, n_bands, height, width, stride, band_stride, seed=0, nodata_variant=0,
                       stream=0):
        _check(self._lib.hk_synth_fill_dev(self._h, C.c_void_p(src_dptr), C.c_void_p(ref_dptr), n_bands, height, width,
                                           stride, band_stride, seed, nodata_variant, stream))

    def event(self) -> int:
        e = C.c_void_p()
        _check(self._lib.hk_event_create(self._h, C.byref(e)))
        return e.value

    def event_destroy(self, ev: int):
        self._lib.hk_event_destroy(self._h, C.c_void_p(ev))

    def event_record(self, ev: int, stream: int = 0):
        _check(self._lib.hk_event_record(self._h, C.c_void_p(ev), stream))

    def stream_wait_event(self, stream: int, ev: int):
        """ Work queued on `stream` after this call waits (on the device) for `ev` (hk_stream_wait_event). """
        _check(self._lib.hk_stream_wait_event(self._h, stream, C.c_void_p(ev)))

    def event_elapsed_ms(self, start: int, stop: int) -> float:
        ms = C.c_float(0)
        _check(self._lib.hk_event_elapsed_ms(self._h, C.c_void_p(start), C.c_void_p(stop), C.byref(ms)))
        return float(ms.value)

    def stream_sync(self, stream: int = 0):
        _check(self._lib.hk_stream_sync(self._h, stream))


_default_ctx = None
_default_lock = threading.Lock()


def default_context() -> Context:
    """ Process-wide context on the device named by HOMONIM_AMD_DEVICE (else LOCAL_RANK, else 0). """
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            dev = int(os.environ.get('HOMONIM_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))
            _default_ctx = Context(dev, n_streams=int(os.environ.get('HOMONIM_AMD_STREAMS', '4')))
    return _default_ctx


_ctx_cache = {}


def get_context(device: int, n_streams: int = 4) -> Context:
    """ Process-wide cached context per (device, n_streams): creating one costs stream + slab allocations. """
    with _default_lock:
        key = (int(device), int(n_streams))
        ctx = _ctx_cache.get(key)
        if ctx is None or ctx.handle is None:
            ctx = _ctx_cache[key] = Context(*key)
    return ctx


def device_count() -> int:
    n = C.c_int(0)
    load_library().hk_device_count(C.byref(n))
    return int(n.value)


def staging_counters(reset: bool = False):
    """ (copies queued straight from / to page-locked caller arrays, chunks through the pinned staging ring) since the process
    started or the last reset (hk_debug_staging_counters; test aid). """
    out = (C.c_uint64 * 2)()
    _check(load_library().hk_debug_staging_counters(out, 1 if reset else 0))
    return int(out[0]), int(out[1])


def debug_fail_after_d2h(on: bool):
    """ Fault injection of the test-suite (hk_debug_fail_after_d2h): host-pointer fits fail behind their queued result copies. """
    _check(load_library().hk_debug_fail_after_d2h(1 if on else 0))


def build_ledger(reset: bool = False) -> dict:
    """ {kernel build: launches since the library was loaded or the last reset} for EVERY kernel build in the library, launched or
    not (hk_debug_build_ledger; test aid -- tests/conftest.py keeps the ledger of which builds met the oracle).  Records of one name
    (a kernel with several launch sites) are added up.  No device call: works without a GPU. """
    lib = load_library()
    need = C.c_size_t(0)
    _check(lib.hk_debug_build_ledger(None, 0, C.byref(need), 0))
    buf = C.create_string_buffer(int(need.value) + 4096)   # (room for nothing: records only appear when the library is loaded)
    _check(lib.hk_debug_build_ledger(buf, len(buf), C.byref(need), 1 if reset else 0))
    out = {}
    for line in buf.value.decode().splitlines():
        name, _, count = line.rpartition('\t')
        out[name] = out.get(name, 0) + int(count)
    return out


def fit_build(desc, shape, planes, phase: int = 0, force_ring=None, force_general: bool = False) -> str:
    """ The ledger name of the build of the fused kernel a launch gets (hk_debug_fit_build; test aid, no device): ``shape`` =
    (bands, height, width) of the job, ``planes`` = names out of FIT_PLANES, ``phase`` 0 the one launch / 1 the certificate build /
    2 its list launch.  ValueError where the launch has no build. """
    name = C.create_string_buffer(88)
    bits = sum(FIT_PLANES[p] for p in planes)
    _check(load_library().hk_debug_fit_build(C.byref(desc), int(shape[1]), int(shape[2]), int(shape[0]), bits, int(phase),
                                             -1 if force_ring is None else int(force_ring), int(bool(force_general)), name, len(name)))
    return name.value.decode()


def device_pci_bus_id(device: int) -> str:
    """ PCI bus address of HIP device ``device`` as sysfs spells it, e.g. '0000:c1:00.0' (homonim_amd/topology.py). """
    buf = C.create_string_buffer(32)
    _check(load_library().hk_device_pci_bus_id(int(device), buf, 32))
    return buf.value.decode()
