""" hk_srcspace_fit_apply: SrcSpaceModel.fit + KernelModel.apply of a block pair on two grids in one call (kernel_model.py:506-535,
:442-463), and the footprint kernel that reads the typed reference pixels once (hk_resample.hip footprint_typed_kernel).

The fused call is held to (1) the sequence of public calls it replaces, bit for bit, (2) the oracle composed from
oracle_np.reproject / fit / full_coverage_mask / apply, within what tests/test_gpu_parity.py holds the proc_crs=src path to
(test_src_space_fit_apply_honours_mask_partial: the same NaN pattern, corrected values within 1e-5 relative), (3) itself on float32
copies of typed blocks, (4) itself across the block seams of RasterFuse.process, and (5) its own argument checks.

Shapes: the smallest at which this can go wrong -- a 9 x 300 source (one row of workgroups, crossed at column 256) and 24 x 40;
references 3 x and 2.5 x finer, finer along one axis only, and 2 x coarser (proc_crs=src forced onto a finer source: cubic_spline
up-sampling, the branch that does not take the footprint kernel); every reference starts inside the source's first pixel and ends
inside its last, so the outer footprints hang over the plane's edge. """
import functools
import warnings

import numpy as np
import pytest

from homonim_amd import Affine, CRS, KernelModel, Model, RasterArray, SrcSpaceModel, _hk
from homonim_amd.enums import Resampling
from homonim_amd.errors import DeviceError
from homonim_amd.fuse import RasterFuse, convert_dtype
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

KERNEL = (3, 5)
SRC_RES = 30.
# name -> (source shape, reference pixel size (x, y), reference origin inside the source's first pixel in reference pixels (x, y),
#          reference shape)
PAIRS = {
    'wide-3x': ((9, 300), (10., 10.), (0.7, 0.9), (26, 898)),
    'wide-2.5x': ((9, 300), (12., 12.), (0.7, 0.4), (22, 749)),
    'small-2.5x': ((24, 40), (12., 12.), (0.7, 0.9), (59, 99)),
    'small-x-only': ((24, 40), (10., 30.), (0.7, 0.3), (24, 119)),
    'small-2x-coarser': ((24, 40), (60., 60.), (0.25, 0.25), (13, 21)),
}
MODELS = {
    'gain': (Model.gain, None), 'gain-blk-offset': (Model.gain_blk_offset, None), 'gain-offset': (Model.gain_offset, None),
    'gain-offset-inpaint': (Model.gain_offset, 0.25),
}
NODATA = {'nan': float('nan'), 'numeric': 0., 'none': None}


@pytest.fixture(scope='module')
def ctx():
    c = _hk.default_context()
    c.selftest()
    return c


def _transforms(pair):
    _, (rx, ry), (fx, fy), _ = PAIRS[pair]
    src_tf = Affine(SRC_RES, 0., 1000., 0., -SRC_RES, 5000.)
    ref_tf = Affine(rx, 0., 1000. + fx * rx, 0., -ry, 5000. - fy * ry)
    return src_tf, ref_tf


@functools.lru_cache(maxsize=None)
def _pair(pair, nodata_key):
    """ (src array, ref array, mapping reference <- source) of a pair: positive data with a smooth gain / offset between them, a
    stretch of the reference that is noise (fails the r2 mask), and holes in the reference cut along the source's footprints: one
    footprint entirely invalid, one half invalid, a cluster wider than the kernel; a few holes in the source too. """
    (sh, sw), _, _, (rh, rw) = PAIRS[pair]
    src_tf, ref_tf = _transforms(pair)
    kx, ox, ky, oy = onp.grid_mapping(tuple(ref_tf)[:6], tuple(src_tf)[:6])
    rng = np.random.default_rng(sum(map(ord, pair)))
    src = rng.uniform(50., 200., (sh, sw)).astype(np.float32)
    yy, xx = np.mgrid[0:rh, 0:rw].astype(np.float64)
    # the reference follows the source pixel under it
    si = np.clip(np.floor((yy + 0.5 - oy) / ky).astype(int), 0, sh - 1)
    sj = np.clip(np.floor((xx + 0.5 - ox) / kx).astype(int), 0, sw - 1)
    gain = 1.2 + 0.3 * np.sin(sj / 17.) * np.cos(si / 5.)
    ref = (gain * src[si, sj] + 20. + rng.normal(0., 1., (rh, rw))).astype(np.float32)
    noise = (sj >= 30) & (sj < 36)
    ref[noise] = rng.uniform(50., 250., int(noise.sum())).astype(np.float32)

    def foot(i0, i1, j0, j1):   # the reference pixels touched by source rows [i0, i1) x columns [j0, j1)
        r0, r1 = int(np.floor(ky * i0 + oy)), int(np.ceil(ky * i1 + oy))
        c0, c1 = int(np.floor(kx * j0 + ox)), int(np.ceil(kx * j1 + ox))
        return max(r0, 0), min(r1, rh), max(c0, 0), min(c1, rw)

    nodata = NODATA[nodata_key]
    if nodata is not None:
        r0, r1, c0, c1 = foot(2, 3, 5, 6)          # one footprint entirely invalid
        ref[r0:r1, c0:c1] = nodata
        r0, r1, c0, c1 = foot(4, 5, 12, 13)        # one half invalid
        ref[r0:r1, c0:max((c0 + c1) // 2, c0 + 1)] = nodata
        r0, r1, c0, c1 = foot(3, 7, 18, 25)        # a cluster wider than the kernel
        ref[r0:r1, c0:c1] = nodata
        src[1, 9] = src[6, 33] = src[5:7, 2] = nodata
    return src, ref, (kx, ox, ky, oy)


def _rasters(pair, nodata_key, src=None, ref=None):
    s, r, _ = _pair(pair, nodata_key)
    src_tf, ref_tf = _transforms(pair)
    nodata = NODATA[nodata_key]
    return (RasterArray((s if src is None else src).copy(), CRS(), src_tf, nodata=nodata),
            RasterArray((r if ref is None else ref).copy(), CRS(), ref_tf, nodata=nodata))


def _model(cls, model_key, mask_partial, find_r2=False):
    model, thresh = MODELS[model_key]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return cls(model, KERNEL, find_r2=find_r2, mask_partial=mask_partial, r2_inpaint_thresh=thresh)


def _resampling(pair):
    return Resampling.cubic_spline if pair == 'small-2x-coarser' else Resampling.average


@functools.lru_cache(maxsize=None)
def _fused(pair, nodata_key, model_key, mask_partial):
    src_ra, ref_ra = _rasters(pair, nodata_key)
    corr_ra, param_ra = _model(SrcSpaceModel, model_key, mask_partial).fit_apply(src_ra, ref_ra, want_params=True)
    assert corr_ra.transform == src_ra.transform and param_ra.transform == src_ra.transform
    return corr_ra.array, param_ra.array


def _todays_sequence(ctx, pair, nodata_key, model_key, mask_partial, src_ra, ref_ra, out_dtype='float32', out_nodata=float('nan'),
                     find_r2=False):
    """ ref_ra.reproject -> KernelModel.fit -> mask -> KernelModel.apply -> convert_dtype, from the public pieces """
    km = _model(KernelModel, model_key, mask_partial, find_r2)
    ref_us_ra = ref_ra.reproject(**src_ra.proj_profile, resampling=_resampling(pair), context=ctx)       # kernel_model.py:520
    param_ra = km.fit(src_ra.copy(), ref_us_ra)
    if mask_partial:                                                                                     # :526-531, :375-409
        cover_ra = ref_ra.mask_ra.reproject(**param_ra.proj_profile, nodata=None, resampling=Resampling.average, context=ctx)
        _, _, mask = ctx.partial_mask(cover_ra.array, None, param_ra.array[:2], KERNEL, want_mask=True, coverage=True)
        param_ra.mask = mask.astype(bool)
    else:
        param_ra.mask = src_ra.mask                                                                      # :533
    corr = km.apply(src_ra, param_ra).array
    if np.dtype(out_dtype) != np.float32 or not (out_nodata is None or np.isnan(out_nodata)):
        corr = convert_dtype(corr, str(np.dtype(out_dtype)), out_nodata)
    return corr, param_ra.array


CASES = [(p, n, m, mp) for p in PAIRS for n in NODATA for m in MODELS for mp in (False, True)]
_ids = lambda v: {True: 'partial', False: 'whole'}.get(v, v) if isinstance(v, (bool, str)) else None   # noqa: E731


# -- 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair, nodata_key, model_key, mask_partial', CASES, ids=_ids)
def test_fused_call_equals_todays_sequence(ctx, pair, nodata_key, model_key, mask_partial):
    corr, params = _fused(pair, nodata_key, model_key, mask_partial)
    exp_corr, exp_params = _todays_sequence(ctx, pair, nodata_key, model_key, mask_partial, *_rasters(pair, nodata_key))
    assert corr.dtype == exp_corr.dtype and params.shape == exp_params.shape
    assert np.array_equal(params, exp_params, equal_nan=True)
    assert np.array_equal(corr, exp_corr, equal_nan=True)
    assert np.isfinite(params[0]).any() or mask_partial


# -- 2 -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_on_source_grid(pair, nodata_key):
    """ the reference block on the source grid, and the coverage fraction of its valid mask there """
    src, ref, mapping = _pair(pair, nodata_key)
    nodata = NODATA[nodata_key]
    ref_us = onp.reproject(ref, nodata, mapping, src.shape, dst_nodata=np.nan, resampling=_resampling(pair).name)
    cover = onp.reproject(onp.mask_of(ref, nodata).astype(np.float32), None, mapping, src.shape, dst_nodata=None,
                          resampling='average')
    return ref_us, cover


@pytest.mark.parametrize('pair, nodata_key, model_key, mask_partial', CASES, ids=_ids)
def test_fused_call_matches_the_oracle(pair, nodata_key, model_key, mask_partial):
    src, _, _ = _pair(pair, nodata_key)
    nodata = NODATA[nodata_key]
    ref_us, cover = _oracle_on_source_grid(pair, nodata_key)
    model, thresh = MODELS[model_key]
    exp_params, _ = onp.fit(model.value, src, nodata, ref_us, np.nan, KERNEL, False, thresh)
    exp_params = exp_params.copy()
    if mask_partial:
        exp_params[:, ~onp.full_coverage_mask(cover >= 1, exp_params, KERNEL)] = np.nan
    else:
        exp_params[:, ~onp.mask_of(src, nodata)] = np.nan
    exp_corr = onp.apply(src, exp_params)
    corr, params = _fused(pair, nodata_key, model_key, mask_partial)
    assert (np.isnan(params) == np.isnan(exp_params)).all() and (np.isnan(corr) == np.isnan(exp_corr)).all()
    ok = ~np.isnan(exp_corr)
    if ok.any():
        assert np.max(np.abs(corr[ok] - exp_corr[ok]) / np.maximum(np.abs(exp_corr[ok]), 1e-6)) < 1e-5


# -- 3 -------------------------------------------------------------------------------------------------------------------------------
def _typed_case(ctx, ref_dtype, src_dtype, out_dtype, out_nodata, mask_partial):
    """ the same call on typed blocks and on their float32 casts (+ host convert_dtype) """
    src, ref, _ = _pair('small-2.5x', 'numeric')
    src_t, ref_t = np.round(src).astype(src_dtype), np.round(ref).astype(ref_dtype)   # (values 0 .. 470: every dtype but uint8 ...)
    if np.dtype(ref_dtype) == np.uint8:
        ref_t = np.round(ref / 2).astype(ref_dtype)                                   # (... which takes them halved)
    km = _model(SrcSpaceModel, 'gain-blk-offset', mask_partial, find_r2=True)
    corr_ra, param_ra = km.fit_apply(*_rasters('small-2.5x', 'numeric', src_t, ref_t), want_params=True, out_dtype=out_dtype,
                                     out_nodata=out_nodata)
    exp_ra, exp_param_ra = km.fit_apply(*_rasters('small-2.5x', 'numeric', src_t.astype(np.float32), ref_t.astype(np.float32)),
                                        want_params=True)
    exp_corr = exp_ra.array
    if np.dtype(out_dtype) != np.float32:
        exp_corr = convert_dtype(exp_corr, out_dtype, out_nodata)
    assert corr_ra.array.dtype == np.dtype(out_dtype)
    assert np.array_equal(param_ra.array, exp_param_ra.array, equal_nan=True)
    assert np.array_equal(corr_ra.array, exp_corr, equal_nan=True)
    assert np.isfinite(exp_param_ra.array[0]).sum() > 50
    # ... and the float32 call is the public sequence (so the typed one is)
    seq_corr, seq_params = _todays_sequence(ctx, 'small-2.5x', 'numeric', 'gain-blk-offset', mask_partial,
                                            *_rasters('small-2.5x', 'numeric', src_t.astype(np.float32), ref_t.astype(np.float32)),
                                            find_r2=True)
    assert np.array_equal(exp_ra.array, seq_corr, equal_nan=True) and np.array_equal(exp_param_ra.array, seq_params, equal_nan=True)


@pytest.mark.parametrize('mask_partial', [False, True], ids=_ids)
@pytest.mark.parametrize('ref_dtype', sorted(_hk.DTYPE_CODES))
def test_typed_reference_equals_its_float32_cast(ctx, ref_dtype, mask_partial):
    _typed_case(ctx, ref_dtype, 'float32', 'float32', float('nan'), mask_partial)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'int16'])
def test_typed_source_and_output_equal_their_float32_casts(ctx, dtype):
    _typed_case(ctx, 'uint16', dtype, dtype, 0, True)


def test_cast_output_and_parameters_leave_one_small_call_together(ctx):
    """ A 12 x 20 source and a 6 x 10 reference, uint16 output with an output nodata AND the parameters asked for: the cast-out branch
    and the parameter branch of the call's tail in one call.  The parameters and the float32 call are held to the oracle as in (2),
    the uint16 block to the float32 call converted on the host as in (3). """
    rng = np.random.default_rng(12)
    src = rng.uniform(50., 200., (12, 20)).astype(np.float32)
    ref = (1.25 * src.reshape(6, 2, 10, 2).mean(axis=(1, 3)) + 20. + rng.normal(0., 1., (6, 10))).astype(np.float32)
    src[3, 4] = src[8, 15:17] = ref[4, 7] = 0.
    mapping, kernel = (.5, 0., .5, 0.), (3, 3)
    desc = _hk.make_desc('gain-offset', kernel, True, None, 0., 0.)
    code = onp.RESAMPLING_CODES['cubic_spline']
    params, corr, _ = ctx.srcspace_fit_apply(desc, src, ref, mapping, code, False, 3, True, out_dtype='uint16', out_nodata=65535)
    params32, corr32, _ = ctx.srcspace_fit_apply(desc, src, ref, mapping, code, False, 3, True)
    ref_us = onp.reproject(ref, 0., mapping, src.shape, dst_nodata=np.nan, resampling='cubic_spline')
    exp_params, _ = onp.fit('gain-offset', src, 0., ref_us, np.nan, kernel, True, None)
    exp_params = exp_params.copy()
    exp_params[:, ~onp.mask_of(src, 0.)] = np.nan
    exp_corr = onp.apply(src, exp_params)
    assert (np.isnan(params32) == np.isnan(exp_params)).all() and (np.isnan(corr32) == np.isnan(exp_corr)).all()
    ok = ~np.isnan(exp_corr)
    assert ok.sum() > 0.9 * ok.size
    assert np.max(np.abs(corr32[ok] - exp_corr[ok]) / np.maximum(np.abs(exp_corr[ok]), 1e-6)) < 1e-5
    assert params.shape == (3, 12, 20) and np.array_equal(params, params32, equal_nan=True)
    assert corr.dtype == np.uint16 and np.array_equal(corr, convert_dtype(corr32, 'uint16', 65535))
    assert (corr == 65535).sum() == np.isnan(corr32).sum() >= 3


# -- 4 -------------------------------------------------------------------------------------------------------------------------------
def test_raster_fuse_process_across_blocks(ctx):
    """ RasterFuse.process(proc_crs=src) on a uint16 pair cut into blocks with halos: the blocks travel in the rasters' own dtype,
    the corrected raster comes back as uint16 -- equal, seams included, to the float32 rasters' result converted on the host. """
    rng = np.random.default_rng(77)
    sh, sw = 70, 90
    src = rng.integers(200, 3000, (sh, sw)).astype(np.uint16)
    src_tf = Affine(30., 0., 1000., 0., -30., 5000.)
    ref_tf = Affine(10., 0., 1000. - 30., 0., -10., 5000. + 30.)         # 3 x finer, one source pixel wider all round
    rh, rw = 3 * (sh + 2), 3 * (sw + 2)
    up = np.kron(np.pad(src, 1, mode='edge').astype(np.float64), np.ones((3, 3)))
    ref = np.round(1.3 * up + 100. + rng.normal(0., 20., (rh, rw))).astype(np.uint16)
    src[10:12, 20:23] = 0
    ref[60:75, 100:130] = 0
    ref[150, 40] = 0
    block_config = dict(threads=1, max_block_mem=0.02)
    kw = dict(model=Model.gain_blk_offset, kernel_shape=(5, 5), param_filename=True, model_config=dict(mask_partial=True),
              block_config=block_config)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        rf = RasterFuse(src, ref, src_nodata=0, ref_nodata=0, proc_crs='src', crs=CRS(), transform=src_tf, ref_transform=ref_tf)
        from homonim_amd import utils
        assert len(list(rf.block_pairs(overlap=utils.overlap_for_kernel((5, 5)), max_block_mem=block_config['max_block_mem']))) >= 4
        corr, params = rf.process(out_profile=dict(dtype='uint16', nodata=0), **kw)
        rf32 = RasterFuse(src.astype(np.float32), ref.astype(np.float32), src_nodata=0, ref_nodata=0, proc_crs='src', crs=CRS(),
                          transform=src_tf, ref_transform=ref_tf)
        exp_corr, exp_params = rf32.process(**kw)
    assert corr.dtype == np.uint16 and params.shape == (3, sh, sw)
    assert np.array_equal(params, exp_params, equal_nan=True)
    assert np.array_equal(corr, convert_dtype(exp_corr, 'uint16', 0))
    assert (corr != 0).sum() > 0.5 * corr.size


# -- 5 -------------------------------------------------------------------------------------------------------------------------------
def test_c_boundary_refuses_bad_arguments(ctx):
    """ Nothing is launched: the checks come first.  The library's statuses keep their Python classes (include/homonim_hk.h):
    HK_ERR_UNSUPPORTED, the flipped mapping, is a DeviceError; HK_ERR_ARG, the other two, a ValueError. """
    src, ref, mapping = _pair('small-2.5x', 'nan')
    desc = _hk.make_desc('gain', KERNEL, False, None, np.nan, np.nan)
    with pytest.raises(DeviceError, match='flipped or degenerate grid mapping'):
        ctx.srcspace_fit_apply(desc, src, ref, (-mapping[0], *mapping[1:]), 5, False, 2, True)
    with pytest.raises(ValueError, match='n_param_bands must be 2'):
        ctx.srcspace_fit_apply(desc, src, ref, mapping, 5, False, 3, True)
    lib, vp = ctx._lib, _hk.C.c_void_p
    space = _hk.SrcSpaceDesc(tuple(mapping), 5, 0)
    corr = np.empty(src.shape, np.float32)
    rc = lib.hk_srcspace_fit_apply(ctx.handle, _hk.C.byref(desc), None, _hk.C.byref(space), src.ctypes.data_as(vp), src.shape[1] - 1,
                                   src.shape[0], src.shape[1], ref.ctypes.data_as(vp), ref.shape[1], ref.shape[0], ref.shape[1],
                                   None, 2, corr.ctypes.data_as(vp), None)
    assert rc == _hk.HK_ERR_ARG
    with pytest.raises(ValueError, match='row stride smaller than width'):
        _hk._check(rc)
