""" Re-projection between CRSs on the device (hk_warp.hip) through the C ABI and the public classes.

* coordinates: ``Context.warp_coords`` against the 40-digit mpmath evaluation of the same CRS definitions (tests/_crs_mp.py), below
  1e-6 m, converted to source pixels -- centres and corners of a 97 x 131 lattice, four CRS pairs;
* re-samplers, what they are held to: the exact statement of tests/_resample_exact.py (rational arithmetic from GDAL's rule, sharing
  no formula with the kernels) on the device's own coordinate planes -- all five methods, tap and convolution form, unit scale, up
  and 3:1 down, on 24 x 36 sources: identical nodata pattern, nearest bit for bit, the rest inside the enclosure stated there; no
  pixel is exempt;
* re-samplers, large shapes: the same planes fed to the numpy restatement (tests/_warp_reference.py, itself held to the exact
  statement by tests/test_resample_exact_cpu.py and pinned to the oracle by tests/test_warp_reference_cpu.py): bit for bit for
  nearest / bilinear / cubic / cubic_spline, the project's lanczos bar (same NaN pattern, < 1e-6 relative: the device's ``sin``
  differs from the host's in the last bit) for lanczos;
* a geometry check that does not go through the restatement: a plane in UTM coordinates must come back as the same plane of the
  exactly transformed pixel centres;
* the pipeline: ``RasterFuse`` / ``RasterCompare`` on files of two CRSs equal the same classes on the hand-warped pair;
* refusals. """
import math
import os
import warnings

import numpy as np
import pytest

import _crs_mp
import _resample_exact as rx
import _warp_reference as wr
from conftest import assert_same_f32
from homonim_amd import (Affine, CRS, DeviceError, Model, RasterArray, RasterCompare, RasterFuse, RefSpaceModel, Resampling,
                         SrcSpaceModel, _hk, crs)
from homonim_amd.errors import ImageFormatWarning
from homonim_amd.geo import suggested_warp_grid
from homonim_amd.raster_array import warp_scale
from homonim_amd.tiff import read_tiff, write_tiff
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

TM25 = CRS('unnamed [1024=1; 1025=1; 2048=4326; 2054=9102; 2057=6378137.0; 2059=298.257223563; 3072=32767; 3074=32767; '
           '3075=1; 3076=9001; 3080=25.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]')    # the reference's test rasters
UTM35S, WGS84 = CRS('EPSG:32735'), CRS('EPSG:4326')
M_PER_DEG = math.radians(1.) * 6.4e6
BAR_M = 1e-6
SENTINEL = 0x5A
SRC_SHAPE = (80, 120)
# the corner of the reference's test rasters in each CRS, and a pixel of about 30 m
TM_TF, UTM_TF, GEO_TF = (Affine(30., 0., -60390., 0., -30., -3722700.), Affine(30., 0., 254000., 0., -30., 6278000.),
                         Affine(0.0003, 0., 24.35, 0., -0.0003, -33.55))


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


class Case:
    """ a source grid, a destination grid in another CRS, and what the warp needs of the two """

    def __init__(self, src_crs, src_tf, dst_crs, dst_tf, dst_shape, src_shape=SRC_SHAPE):
        self.src_crs, self.src_tf, self.src_shape = src_crs, src_tf, src_shape
        self.dst_crs, self.dst_tf, self.dst_shape = dst_crs, dst_tf, tuple(dst_shape)
        self.src_def, self.dst_def = crs.parse(src_crs), crs.parse(dst_crs)
        self.warp = _hk.make_warp_desc(self.src_def, src_tf, self.dst_def, dst_tf)
        self.scale = warp_scale(dst_crs, dst_tf, self.dst_shape, src_crs, src_tf)


def _scaled(tf, k):
    return Affine(tf.a * k, 0., tf.c, 0., tf.e * k, tf.f)


def _grown(tf, shape, n):
    return Affine(tf.a, 0., tf.c - n * tf.a, 0., tf.e, tf.f - n * tf.e), (shape[0] + 2 * n, shape[1] + 2 * n)


def _inside(src_crs, src_tf, dst_crs, res, shape):
    """ a dst_crs grid of `shape` and pixel `res` centred on the source's centre """
    xc, yc = src_tf.c + src_tf.a * SRC_SHAPE[1] / 2, src_tf.f + src_tf.e * SRC_SHAPE[0] / 2
    x, y = crs.transform_coords(src_crs, dst_crs, xc, yc)
    return Affine(res, 0., float(x) - res * shape[1] / 2, 0., -res, float(y) + res * shape[0] / 2)


def make_case(name):
    if name == 'unit':        # 30 m Transverse Mercator -> 30 m UTM: scale ~ 1; the suggested grid overhangs the (rotated) source
        return Case(TM25, TM_TF, UTM35S, *suggested_warp_grid(TM25, TM_TF, SRC_SHAPE, UTM35S))
    if name == 'up6':         # 30 m -> 5 m, inside the source
        return Case(TM25, TM_TF, UTM35S, _inside(TM25, TM_TF, UTM35S, 5., (97, 131)), (97, 131))
    if name == 'down3':       # 10 m -> 30 m: the stretched kernels
        tf, (h, w) = suggested_warp_grid(TM25, _scaled(TM_TF, 1 / 3), SRC_SHAPE, UTM35S)
        return Case(TM25, _scaled(TM_TF, 1 / 3), UTM35S, _scaled(tf, 3.), (h // 3 + 2, w // 3 + 2))
    if name == 'overhang':    # a destination that overhangs the source by 7 pixels and more on all four sides
        tf, shape = suggested_warp_grid(TM25, TM_TF, SRC_SHAPE, UTM35S)
        return Case(TM25, TM_TF, UTM35S, *_grown(tf, shape, 7))
    if name == 'utm-geo':
        return Case(UTM35S, UTM_TF, WGS84, *suggested_warp_grid(UTM35S, UTM_TF, SRC_SHAPE, WGS84))
    if name == 'geo-utm':
        return Case(WGS84, GEO_TF, UTM35S, *suggested_warp_grid(WGS84, GEO_TF, SRC_SHAPE, UTM35S))
    raise KeyError(name)


CASES = ('unit', 'up6', 'down3', 'overhang', 'utm-geo', 'geo-utm')


def source(nodata, seed=14, bands=1):
    """ onp.synth_pair sources (positive: the relative bar of lanczos is meaningful), 'frame+holes' """
    out = []
    for b in range(bands):
        a, _ = onp.synth_pair(*SRC_SHAPE, seed + b, 'frame+holes')
        if nodata is not None and not np.isnan(nodata):
            a[np.isnan(a)] = nodata
        out.append(a)
    return out[0] if bands == 1 else np.stack(out)


def check_band(got, exp, resampling, what):
    if resampling == 'lanczos':     # tests/test_gpu_parity.py:1647-1650
        assert (np.isnan(got) == np.isnan(exp)).all(), what
        ok = ~np.isnan(exp)
        assert np.max(np.abs(got[ok] - exp[ok]) / np.abs(exp[ok])) < 1e-6, what
    else:
        assert_same_f32(got, exp, what)


# -- 1. coordinates ---------------------------------------------------------------------------------------------------------------
def _coords_padded(ctx, warp, shape, offset, pad=5):
    """ Context.warp_coords into planes with spare pitch; the slack must come back untouched """
    h, w = shape
    stores = [np.empty((h, w + pad), np.float64) for _ in range(2)]
    for s in stores:
        s.view(np.uint8)[...] = SENTINEL
    x, y = ctx.warp_coords(warp, shape, offset, out=(stores[0][:, :w], stores[1][:, :w]))
    for s in stores:
        assert (s[:, w:].view(np.uint8) == SENTINEL).all(), 'a coordinate plane was written outside its width'
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


COORD_PAIRS = {   # name: (source CRS, source geo-transform, destination CRS, destination geo-transform)
    'tm25-from-utm35s': (TM25, TM_TF, UTM35S, UTM_TF), 'utm35s-from-tm25': (UTM35S, UTM_TF, TM25, TM_TF),
    'utm35s-from-wgs84': (UTM35S, UTM_TF, WGS84, GEO_TF), 'wgs84-from-utm35s': (WGS84, GEO_TF, UTM35S, UTM_TF),
}


@pytest.mark.oracle
@pytest.mark.parametrize('pair', list(COORD_PAIRS))
def test_warp_coords_against_mpmath(ctx, pair):
    """ centres (offset 0.5) and corners (offset 0 on a lattice one larger) of a 97 x 131 destination grid: the device's source pixel
    coordinates against the exact transformation of the same destination positions, below 1e-6 m """
    src_crs, src_tf, dst_crs, dst_tf = COORD_PAIRS[pair]
    c = Case(src_crs, src_tf, dst_crs, dst_tf, (97, 131))
    m_per_unit = M_PER_DEG if c.src_def.is_geographic else 1.
    worst = 0.
    for what, shape, off in (('centres', (97, 131), 0.5), ('corners', (98, 132), 0.)):
        gx, gy = _coords_padded(ctx, c.warp, shape, (off, off))
        assert np.isfinite(gx).all() and np.isfinite(gy).all()
        rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        X, Y = dst_tf.c + (cols + off) * dst_tf.a, dst_tf.f + (rows + off) * dst_tf.e     # as the device forms them
        exact = _crs_mp.transform_many(tuple(c.dst_def), tuple(c.src_def), X.ravel(), Y.ravel())
        with _crs_mp.mp.workdps(_crs_mp.DPS):
            exact_px = [((ex - src_tf.c) / src_tf.a, (ey - src_tf.f) / src_tf.e) for ex, ey in exact]
        err = _crs_mp.max_error(gx.ravel(), gy.ravel(), exact_px, abs(src_tf.a) * m_per_unit, abs(src_tf.e) * m_per_unit)
        print(f'[warp_coords] {pair} {what}: largest error {err:.3e} m ({err / (abs(src_tf.a) * m_per_unit):.3e} source pixels)')
        worst = max(worst, err)
        assert err < BAR_M, f'{pair} {what}: {err} m'
    print(f'[warp_coords] {pair}: largest error {worst:.3e} m')


def test_warp_coords_dev_equals_the_host_entry_point(ctx):
    c = make_case('unit')
    h, w = c.dst_shape
    x, y = ctx.warp_coords(c.warp, c.dst_shape)
    stride = w + 3
    store = np.empty((2, h, stride), np.float64)
    store.view(np.uint8)[...] = SENTINEL
    d = ctx.dev_alloc(store.nbytes)
    try:
        ctx.h2d(d, store)
        ctx.warp_coords_dev(c.warp, c.dst_shape, d, d + h * stride * 8, stride)
        ctx.stream_sync(0)
        ctx.d2h(store, d)
    finally:
        ctx.dev_free(d)
    assert (store[:, :, w:].view(np.uint8) == SENTINEL).all()
    assert np.array_equal(store[0, :, :w], x, equal_nan=True) and np.array_equal(store[1, :, :w], y, equal_nan=True)


# -- 2. re-samplers ---------------------------------------------------------------------------------------------------------------
def _resample_case(ctx, case_name, resampling, nodata):
    c = make_case(case_name)
    src = source(nodata)
    got = ctx.reproject_crs(src, nodata, c.warp, c.scale, c.dst_shape, onp.RESAMPLING_CODES[resampling], np.nan)
    sx, sy = ctx.warp_coords(c.warp, c.dst_shape)
    exp = wr.warp_resample(src, nodata, sx, sy, c.scale[0], c.scale[1], dst_nodata=np.nan, resampling=resampling)
    check_band(got, exp, resampling, f'{case_name} {resampling} nodata {nodata}')
    return c, got, sx, sy


@pytest.mark.oracle
@pytest.mark.parametrize('resampling', wr.MODES)
@pytest.mark.parametrize('case_name', CASES)
def test_warp_resamplers_equal_the_restatement_on_the_devices_coordinates(ctx, case_name, resampling):
    c, got, sx, sy = _resample_case(ctx, case_name, resampling, np.nan)
    inside = (sx >= 0) & (sx < SRC_SHAPE[1]) & (sy >= 0) & (sy < SRC_SHAPE[0])
    assert np.isnan(got[~inside]).all()          # dst_fill where the destination has no source
    assert (~np.isnan(got)).sum() > 0.3 * inside.sum()
    if case_name in ('unit', 'overhang', 'down3', 'utm-geo', 'geo-utm'):
        assert (~inside).any()                   # ... and these grids do overhang it
    if case_name == 'overhang':
        assert not inside[:7].any() and not inside[-7:].any() and not inside[:, :7].any() and not inside[:, -7:].any()
    if case_name == 'up6':
        assert 0.16 < c.scale[0] < 0.17 and 0.16 < c.scale[1] < 0.17
    if case_name == 'down3':
        assert 2.9 < c.scale[0] < 3.1 and 2.9 < c.scale[1] < 3.1


@pytest.mark.oracle
@pytest.mark.parametrize('resampling', wr.MODES)
@pytest.mark.parametrize('case_name', ['unit', 'down3', 'up6'])
@pytest.mark.parametrize('nodata', [None, -9999.], ids=['none', 'number'])
def test_warp_resamplers_nodata_none_and_number(ctx, case_name, resampling, nodata):
    _resample_case(ctx, case_name, resampling, nodata)


@pytest.mark.oracle
@pytest.mark.parametrize('resampling', wr.MODES)
def test_three_bands_on_a_pitched_layout(ctx, resampling):
    """ hk_reproject_crs_dev: 3 bands, rows and planes with slack on both sides; every band against the restatement, the slack
    untouched, and the host entry point gives the same bits """
    c = make_case('unit')
    src = source(np.nan, seed=20, bands=3)
    nb, sh, sw = src.shape
    dh, dw = c.dst_shape
    s_store = np.full((nb, sh + 2, sw + 3), np.float32(7.), np.float32)
    s_store[:, :sh, :sw] = src
    d_store = np.empty((nb, dh + 1, dw + 5), np.float32)
    d_store.view(np.uint8)[...] = SENTINEL
    code = onp.RESAMPLING_CODES[resampling]
    d_src, d_dst = ctx.dev_alloc(s_store.nbytes), ctx.dev_alloc(d_store.nbytes)
    try:
        ctx.h2d(d_src, s_store)
        ctx.h2d(d_dst, d_store)
        ctx.reproject_crs_dev(c.warp, d_src, nb, (sh, sw), s_store.shape[2], s_store.shape[1] * s_store.shape[2], np.nan, c.scale,
                              code, d_dst, (dh, dw), d_store.shape[2], d_store.shape[1] * d_store.shape[2], np.nan)
        ctx.stream_sync(0)
        ctx.d2h(d_store, d_dst)
    finally:
        ctx.dev_free(d_src)
        ctx.dev_free(d_dst)
    got = np.ascontiguousarray(d_store[:, :dh, :dw])
    slack = d_store.copy()
    slack[:, :dh, :dw].view(np.uint8)[...] = SENTINEL
    assert (slack.view(np.uint8) == SENTINEL).all(), 'the destination was written outside its height x width'
    sx, sy = ctx.warp_coords(c.warp, c.dst_shape)
    for b in range(nb):
        exp = wr.warp_resample(src[b], np.nan, sx, sy, c.scale[0], c.scale[1], dst_nodata=np.nan, resampling=resampling)
        check_band(got[b], exp, resampling, f'band {b} {resampling}')
    host = ctx.reproject_crs(src, np.nan, c.warp, c.scale, c.dst_shape, code, np.nan)
    assert_same_f32(host, got, f'host against device entry point, {resampling}')


# -- 2b. re-samplers against the exact statement ------------------------------------------------------------------------------------
SMALL_SHAPE = (24, 36)
SMALL_CASES = ('unit', 'up', 'down3', 'utm-geo')


def small_case(name):
    """ the WARP_AXIS path on a 24 x 36 source: grids small enough for rational arithmetic at every pixel """
    if name == 'unit':        # 30 m Transverse Mercator -> 30 m UTM, the suggested grid and 2 pixels more on every side
        return Case(TM25, TM_TF, UTM35S, *_grown(*suggested_warp_grid(TM25, TM_TF, SMALL_SHAPE, UTM35S), 2), src_shape=SMALL_SHAPE)
    if name == 'up':          # 30 m -> 12 m about the source's centre: 0.4 source pixels per pixel, the tap form
        xc, yc = TM_TF.c + TM_TF.a * SMALL_SHAPE[1] / 2, TM_TF.f + TM_TF.e * SMALL_SHAPE[0] / 2
        x, y = crs.transform_coords(TM25, UTM35S, xc, yc)
        return Case(TM25, TM_TF, UTM35S, Affine(12., 0., float(x) - 12. * 28, 0., -12., float(y) + 12. * 20), (40, 56),
                    src_shape=SMALL_SHAPE)
    if name == 'down3':       # 10 m -> 30 m: the stretched kernels
        tf, (h, w) = suggested_warp_grid(TM25, _scaled(TM_TF, 1 / 3), SMALL_SHAPE, UTM35S)
        return Case(TM25, _scaled(TM_TF, 1 / 3), UTM35S, _scaled(tf, 3.), (h // 3 + 2, w // 3 + 2), src_shape=SMALL_SHAPE)
    if name == 'utm-geo':
        return Case(UTM35S, UTM_TF, WGS84, *suggested_warp_grid(UTM35S, UTM_TF, SMALL_SHAPE, WGS84), src_shape=SMALL_SHAPE)
    raise KeyError(name)


def small_source(nodata, seed=14):
    a, _ = onp.synth_pair(*SMALL_SHAPE, seed, 'frame+holes')
    if not np.isnan(nodata):
        a[np.isnan(a)] = nodata
    return a


@pytest.mark.oracle
@pytest.mark.parametrize('nodata', [np.nan, -9999.], ids=['nan', 'number'])
@pytest.mark.parametrize('resampling', wr.MODES)
@pytest.mark.parametrize('case_name', SMALL_CASES)
def test_warp_resamplers_inside_the_exact_enclosure(ctx, case_name, resampling, nodata):
    """ hk_warp.hip held DIRECTLY to the exact statement of tests/_resample_exact.py on the device's own coordinate planes, which
    are arbitrary doubles: identical nodata pattern, bit-equal for nearest, inside the enclosure for the rest; the guards of the
    statement make a case that would exempt a pixel fail as mis-designed.  The exact side is computed once per (case, method) and
    serves both nodata variants and the bands of the second one. """
    c = small_case(case_name)
    assert max(c.dst_shape) <= 60
    src = small_source(nodata)
    code = onp.RESAMPLING_CODES[resampling]
    got = ctx.reproject_crs(src, nodata, c.warp, c.scale, c.dst_shape, code, np.nan)
    sx, sy = ctx.warp_coords(c.warp, c.dst_shape)
    inside = (sx >= 0) & (sx < SMALL_SHAPE[1]) & (sy >= 0) & (sy < SMALL_SHAPE[0])
    res = rx.enclosure_failures_at(got, src, nodata, sx, sy, c.scale[0], c.scale[1], resampling)
    rx.assert_held(res, f'device warp {case_name} {resampling} nodata {nodata}', 0.3 * inside.sum())
    if case_name == 'unit':       # overhangs the source on all four sides
        assert not inside[:2].any() and not inside[-2:].any() and not inside[:, :2].any() and not inside[:, -2:].any()
        assert 0.99 < c.scale[0] < 1.01 and 0.99 < c.scale[1] < 1.01
    if case_name == 'up':
        assert 0.39 < c.scale[0] < 0.41 and 0.39 < c.scale[1] < 0.41 and not rx.uses_conv('bilinear', *c.scale)
    if case_name == 'down3':
        assert (~inside).any() and 2.9 < c.scale[0] < 3.1 and 2.9 < c.scale[1] < 3.1 and rx.uses_conv('bilinear', *c.scale)
    if not np.isnan(nodata):      # three bands in one call, the first and the last the same raster
        other = small_source(nodata, seed=15)
        three = ctx.reproject_crs(np.stack([src, other, src]), nodata, c.warp, c.scale, c.dst_shape, code, np.nan)
        for b in (0, 2):
            res = rx.enclosure_failures_at(three[b], src, nodata, sx, sy, c.scale[0], c.scale[1], resampling)
            rx.assert_held(res, f'device warp {case_name} {resampling} band {b} of three', 0.3 * inside.sum())
        assert not np.array_equal(three[1], three[0], equal_nan=True)


@pytest.mark.oracle
def test_reproject_dev_gives_the_bits_of_reproject(ctx):
    """ hk_reproject_dev is hk_reproject on device rasters (the baseline of tools/warp_timing.py) """
    src = source(np.nan)
    mapping, shape = (0.45, -0.5, 0.45, -0.5), (180, 270)
    exp = ctx.reproject(src, np.nan, mapping, shape, 1, np.nan)
    assert_same_f32(exp, onp.reproject(src, np.nan, mapping, shape, dst_nodata=np.nan, resampling='bilinear'), 'hk_reproject')
    out = np.empty(shape, np.float32)
    d_src, d_dst = ctx.dev_alloc(src.nbytes), ctx.dev_alloc(out.nbytes)
    try:
        ctx.h2d(d_src, src)
        ctx.reproject_dev(d_src, 1, src.shape, src.shape[1], src.size, np.nan, mapping, 1, d_dst, shape, shape[1], out.size, np.nan)
        ctx.stream_sync(0)
        ctx.d2h(out, d_dst)
    finally:
        ctx.dev_free(d_src)
        ctx.dev_free(d_dst)
    assert_same_f32(out, exp, 'hk_reproject_dev')


# -- 3. geometry, independent of the restatement ----------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('resampling', ['bilinear', 'cubic', 'cubic_spline'])
def test_a_plane_comes_back_as_the_plane_of_the_exactly_transformed_centres(ctx, resampling):
    """ source: f = c + a E + b N sampled as float32 on a UTM 35S grid, a = b = 1e-2 / m, abs(f) < 2048.  These kernels reproduce
    planes, so every interior pixel of a Transverse Mercator (lon0 25) grid must equal c + a E(p) + b N(p) with (E, N) the exact
    transform of its centre, within 2 ulp of max abs(f) in float32 (2.4e-4): the sample's rounding and the output's.  2 ulp is a
    2.4 cm shift: a mistaken half-pixel convention or an axis swap cannot pass. """
    a_, b_ = 1e-2, 1e-2
    sh, sw = SRC_SHAPE
    rows, cols = np.mgrid[0:sh, 0:sw].astype(np.float64)
    e0, n0 = UTM_TF.c, UTM_TF.f
    c_ = 1000. - a_ * e0 - b_ * n0
    plane = (c_ + a_ * (UTM_TF.c + (cols + 0.5) * UTM_TF.a) + b_ * (UTM_TF.f + (rows + 0.5) * UTM_TF.e)).astype(np.float32)
    assert np.abs(plane).max() < 2048
    src_ra = RasterArray(plane, UTM35S, UTM_TF, nodata=None)
    shape = (60, 90)
    dst_tf = _inside(UTM35S, UTM_TF, TM25, 20., shape)
    got = src_ra.reproject(crs=TM25, transform=dst_tf, shape=shape, resampling=resampling, nodata=np.nan, context=ctx).array
    assert got.shape == shape and not np.isnan(got).any()      # interior: every tap of every pixel lies inside the source
    r, cl = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    X, Y = dst_tf.c + (cl + 0.5) * dst_tf.a, dst_tf.f + (r + 0.5) * dst_tf.e
    exact = _crs_mp.transform_many(tuple(crs.parse(TM25)), tuple(crs.parse(UTM35S)), X.ravel(), Y.ravel())
    exp = np.array([float(c_ + a_ * e + b_ * n) for e, n in exact]).reshape(shape)
    # and the taps did lie inside
    px, py = (np.array([float(e) for e, _ in exact]) - UTM_TF.c) / UTM_TF.a, (np.array([float(n) for _, n in exact]) - UTM_TF.f) / UTM_TF.e
    assert px.min() > 2.5 and px.max() < sw - 2.5 and py.min() > 2.5 and py.max() < sh - 2.5
    tol = 2 * np.spacing(np.float32(np.abs(plane).max()))
    err = np.abs(got.astype(np.float64) - exp).max()
    print(f'[plane] {resampling}: largest error {err:.3e} against 2 ulp = {tol:.3e}')
    assert err <= tol


# -- 4. the pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pair_files(tmp_path_factory):
    """ src.tif: 3 bands, 5 m, Transverse Mercator lon0 25 (the reference rasters' key-list label); ref.tif: 30 m, EPSG:32735,
    covering it with a margin -- onp.synth_pair data, both label families read from files """
    d = tmp_path_factory.mktemp('warp_pair')
    sh, sw = 520, 648
    src_tf = Affine(5., 0., -60000., 0., -5., -3723000.)
    src = np.stack([onp.synth_pair(sh, sw, 30 + b, 'frame+holes')[0] for b in range(3)])
    cols, rows = np.array([0., sw, sw, 0.]), np.array([0., 0., sh, sh])
    xs, ys = crs.transform_coords(TM25, UTM35S, src_tf.c + cols * src_tf.a, src_tf.f + rows * src_tf.e)
    left, top = math.floor(xs.min() / 30.) * 30. - 300., math.ceil(ys.max() / 30.) * 30. + 300.
    rw, rh = int((xs.max() - left) / 30.) + 12, int((top - ys.min()) / 30.) + 12
    ref_tf = Affine(30., 0., left, 0., -30., top)
    ref = np.stack([onp.synth_pair(rh, rw, 40 + b, 'frame+holes')[1] for b in range(3)])
    src_fn, ref_fn = os.path.join(d, 'src.tif'), os.path.join(d, 'ref.tif')
    write_tiff(src_fn, src, src_tf, TM25, float('nan'))
    write_tiff(ref_fn, ref, ref_tf, UTM35S, float('nan'))
    assert read_tiff(src_fn).crs == TM25 and read_tiff(ref_fn).crs == UTM35S
    return dict(dir=str(d), src=src_fn, ref=ref_fn, src_tf=src_tf, ref_tf=ref_tf)


def _hand_warped(files, proc_crs):
    """ the pair brought to one CRS by hand through the public API, as utils.same_orientation_crs picks the image """
    s, r = read_tiff(files['src']), read_tiff(files['ref'])
    src_ra = RasterArray(s.array, s.crs, s.transform, nodata=s.nodata)
    ref_ra = RasterArray(r.array, r.crs, r.transform, nodata=r.nodata)
    if proc_crs == 'src':
        return src_ra.reproject(crs=r.crs, resampling=Resampling.bilinear), ref_ra
    return src_ra, ref_ra.reproject(crs=s.crs, resampling=Resampling.bilinear)


@pytest.mark.oracle
@pytest.mark.parametrize('model', ['gain-blk-offset', 'gain-offset'])
@pytest.mark.parametrize('proc_crs', ['ref', 'src'])
def test_raster_fuse_on_two_crss_equals_the_hand_warped_pair(ctx, pair_files, proc_crs, model):
    tag = f'{proc_crs}_{model}'
    corr_fn, param_fn = (os.path.join(pair_files['dir'], f'{kind}_{tag}.tif') for kind in ('corr', 'param'))
    kwargs = dict(model=model, kernel_shape=(5, 5), build_ovw=True, overwrite=True)
    with pytest.warns(ImageFormatWarning, match='re-projected to the same CRS: src.tif and ref.tif'):
        fuse = RasterFuse(pair_files['src'], pair_files['ref'], proc_crs=proc_crs)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        corr, params = fuse.process(corr_fn, param_filename=param_fn, **kwargs)
        src_ra, ref_ra = _hand_warped(pair_files, proc_crs)
        hand = RasterFuse(src_ra, ref_ra, proc_crs=proc_crs)
        exp_corr, exp_params = hand.process(os.path.join(pair_files['dir'], f'hand_corr_{tag}.tif'),
                                            param_filename=os.path.join(pair_files['dir'], f'hand_param_{tag}.tif'), **kwargs)
    assert fuse.proc_crs.name == proc_crs
    assert_same_f32(corr, exp_corr, 'corrected')
    assert_same_f32(params, exp_params, 'parameters')
    assert (~np.isnan(corr)).mean() > 0.5 and (~np.isnan(params)).mean() > 0.3
    # the corrected file is on the source's grid: the source file's own for proc_crs=ref, the warped source's for proc_crs=src
    written = read_tiff(corr_fn)
    assert_same_f32(written.array, corr, 'corrected file')
    assert crs.same_crs(written.crs, src_ra.crs) and written.crs == (TM25 if proc_crs == 'ref' else UTM35S)
    for got, exp in zip(written.transform, src_ra.transform):
        assert got == exp
    if proc_crs == 'ref':
        assert written.transform == pair_files['src_tf'] and corr.shape == (3, 520, 648)
    assert_same_f32(read_tiff(param_fn).array, params, 'parameter file')
    from homonim_amd import read_tiff_overviews
    ovw, hand_ovw = read_tiff_overviews(corr_fn), read_tiff_overviews(os.path.join(pair_files['dir'], f'hand_corr_{tag}.tif'))
    assert len(ovw) == len(hand_ovw) >= 1
    for a, b in zip(ovw, hand_ovw):
        assert_same_f32(np.asarray(a), np.asarray(b), 'overview')


@pytest.mark.oracle
def test_proc_crs_auto_resolves_before_the_warp(ctx, pair_files):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert RasterFuse(pair_files['src'], pair_files['ref']).proc_crs.name == 'ref'     # 5 m source, 30 m reference
        # swapped: a 30 m "source" inside a 5 m "reference" that does not cover it
        from homonim_amd.errors import ImageContentError
        with pytest.raises(ImageContentError, match='does not cover'):
            RasterFuse(pair_files['ref'], pair_files['src'])


@pytest.mark.oracle
@pytest.mark.parametrize('proc_crs', ['ref', 'src'])
def test_raster_compare_on_two_crss_equals_the_hand_warped_pair(ctx, pair_files, proc_crs):
    with pytest.warns(ImageFormatWarning, match='re-projected to the same CRS'):
        cmp = RasterCompare(pair_files['src'], pair_files['ref'], proc_crs=proc_crs)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = cmp.process()
        exp = RasterCompare(*_hand_warped(pair_files, proc_crs), proc_crs=proc_crs).process()
    assert got == exp and got['Mean']['n'] > 1000


# -- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_refused(ctx):
    a = RasterArray(source(np.nan), TM25, TM_TF)
    b = RasterArray(source(np.nan), UTM35S, UTM_TF)
    for mode in ('average', 'mode', 'max', 'min', 'med', 'q1', 'q3', 'sum', 'rms'):
        with pytest.raises(NotImplementedError, match=mode):
            a.reproject(crs=UTM35S, resampling=mode, context=ctx)
    c = make_case('unit')
    with pytest.raises(DeviceError, match='footprint'):        # and at the C boundary
        ctx.reproject_crs(a.array, np.nan, c.warp, c.scale, c.dst_shape, int(Resampling.average), np.nan)
    airy = CRS('OSGB [1024=1; 2057=6377563.396; 2059=299.3249646; 3075=1; 3080=-2.0; 3081=49.0; 3082=400000.0; 3083=-100000.0; '
               '3092=0.9996012717]')
    with pytest.raises(NotImplementedError, match='ellipsoid'):
        a.reproject(crs=airy, resampling='bilinear', context=ctx)
    w = _hk.make_warp_desc(crs.parse(airy), TM_TF, crs.parse(UTM35S), UTM_TF)
    with pytest.raises(DeviceError, match='ellipsoid'):
        ctx.warp_coords(w, (4, 4))
    with pytest.raises(NotImplementedError, match='EPSG:3857'):
        a.reproject(crs=CRS('EPSG:3857'), resampling='bilinear', context=ctx)
    with pytest.raises(NotImplementedError, match='EPSG:3857'):
        RasterArray(a.array, CRS('EPSG:3857'), TM_TF).reproject(crs=UTM35S, resampling='bilinear', context=ctx)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(NotImplementedError, match='EPSG:3857'):
            RasterFuse(a, RasterArray(b.array, CRS('EPSG:3857'), UTM_TF))
    for model in (RefSpaceModel(Model.gain, (3, 3)), SrcSpaceModel(Model.gain, (3, 3))):
        model.context = ctx
        with pytest.raises(NotImplementedError, match=r'reproject\(crs='):
            model.fit(a, b)
        with pytest.raises(NotImplementedError, match=r'reproject\(crs='):
            model.fit_apply(a, b)
    # unknown CRSs behave as before: equal labels work
    same = RasterArray(a.array, CRS('EPSG:3857'), TM_TF).reproject(crs=CRS('epsg:3857'), transform=_scaled(TM_TF, 0.5),
                                                                   shape=(160, 240), resampling='bilinear', context=ctx)
    assert same.shape == (160, 240)
