""" Rotated and sheared rasters on the device (hk_warp.hip, the affine builds) through the C ABI and the public classes.

* coordinates within one CRS: ``Context.warp_coords_affine`` against exact rational arithmetic on the five grid pairs of
  tests/_rotated_grids.py, under the bar stated there; across two CRSs against the 40-digit evaluation (tests/_crs_mp.py) composed
  with the exact affines, below the project's 1e-6 m;
* re-samplers, what they are held to: the exact statement of tests/_resample_exact.py (rational arithmetic from GDAL's rule, sharing
  no formula with the kernels) on the device's own coordinate planes -- all five methods on both affine paths, unit scale, up and
  3:1 down, on 24 x 36 sources: identical nodata pattern, nearest bit for bit, the rest inside the enclosure stated there; no pixel
  is exempt;
* re-samplers, large shapes and workgroup boundaries: the same planes fed to the numpy restatement (tests/_warp_reference.py, itself
  held to the exact statement by tests/test_resample_exact_cpu.py): bit for bit for nearest / bilinear / cubic / cubic_spline, the
  project's lanczos bar for lanczos;
* exact turns: a raster stored turned by 90 / 180 / 270 degrees, south-up or not, comes back bit for bit;
* the device entry points equal the host ones, three bands equal three single bands;
* the pipeline: ``RasterFuse`` / ``RasterCompare`` on rotated GeoTIFFs equal the same classes on the hand-warped rasters;
* refusals at the C boundary.

The one-CRS cases run under the label EPSG:3857, which homonim_amd/crs.py cannot define: that path needs no CRS mathematics. """
import math
import os
import warnings

import numpy as np
import pytest

import _crs_mp
import _resample_exact as rx
import _rotated_grids as rg
import _warp_reference as wr
from conftest import assert_same_f32
from homonim_amd import Affine, CRS, DeviceError, RasterArray, RasterCompare, RasterFuse, Resampling, _hk, crs
from homonim_amd.errors import ImageFormatWarning
from homonim_amd.geo import suggested_warp_grid
from homonim_amd.raster_array import warp_scale
from homonim_amd.tiff import read_tiff, write_tiff
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

TM25 = CRS('unnamed [1024=1; 1025=1; 2048=4326; 2054=9102; 2057=6378137.0; 2059=298.257223563; 3072=32767; 3074=32767; '
           '3075=1; 3076=9001; 3080=25.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]')
UTM35S, WGS84, WEB = CRS('EPSG:32735'), CRS('EPSG:4326'), CRS('EPSG:3857')
M_PER_DEG = math.radians(1.) * 6.4e6
BAR_M = 1e-6
SENTINEL = 0x5A
SRC_SHAPE = (80, 120)
UNIT_SHAPE = (83, 271)     # crosses a workgroup boundary in both directions and ends in a partial tile, for every tile shape tried
X0, Y0 = 254000., 6278000.


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


class Case:
    """ a source grid, a destination grid, either of them rotated or sheared, in one CRS or two, and what the warp needs of them """

    def __init__(self, src_crs, src_tf, dst_crs, dst_tf, dst_shape, src_shape=SRC_SHAPE):
        self.src_crs, self.src_tf, self.src_shape = src_crs, src_tf, src_shape
        self.dst_crs, self.dst_tf, self.dst_shape = dst_crs, dst_tf, tuple(dst_shape)
        self.same = crs.same_crs(src_crs, dst_crs)
        self.src_def, self.dst_def = (None, None) if self.same else (crs.parse(src_crs), crs.parse(dst_crs))
        self.warp = _hk.make_affine_warp_desc(self.src_def, src_tf, self.dst_def, dst_tf)
        self.scale = warp_scale(dst_crs, dst_tf, self.dst_shape, src_crs, src_tf)


def _centred(src_tf, res, shape, src_shape=SRC_SHAPE):
    """ the north-up grid of `shape` and pixel `res` centred on the source's centre """
    xc, yc = src_tf * (src_shape[1] / 2, src_shape[0] / 2)
    return Affine(res, 0., xc - res * shape[1] / 2, 0., -res, yc + res * shape[0] / 2)


def _grown(tf, shape, n):
    return Affine(tf.a, 0., tf.c - n * tf.a, 0., tf.e, tf.f - n * tf.e), (shape[0] + 2 * n, shape[1] + 2 * n)


ROT30 = rg.rotated(X0, Y0, 30., 30.)
TM_ROT30 = rg.rotated(-60390., -3722700., 30., 30.)


def make_case(name):
    if name == 'rot30':           # unit scale, a destination wider than the turned source
        return Case(WEB, ROT30, WEB, _centred(ROT30, 30., UNIT_SHAPE), UNIT_SHAPE)
    if name == 'rot30-down3':     # onto a grid three times coarser: the stretched kernels
        return Case(WEB, ROT30, WEB, _centred(ROT30, 90., (45, 85)), (45, 85))
    if name == 'rot90':
        tf = rg.rotated(X0, Y0, 90., 30.)
        return Case(WEB, tf, WEB, _centred(tf, 30., UNIT_SHAPE), UNIT_SHAPE)
    if name == 'sheared':
        tf = Affine(30., 3., X0, -2., -30., Y0)
        return Case(WEB, tf, WEB, _centred(tf, 30., UNIT_SHAPE), UNIT_SHAPE)
    if name == 'rotated-dst':     # a north-up source onto a destination turned by 15 degrees
        tf = Affine(30., 0., X0, 0., -30., Y0)
        xc, yc = tf * (SRC_SHAPE[1] / 2, SRC_SHAPE[0] / 2)
        dst = Affine.translation(xc, yc) * Affine.rotation(15.) * Affine.scale(30., -30.) * Affine.translation(-UNIT_SHAPE[1] / 2,
                                                                                                          -UNIT_SHAPE[0] / 2)
        return Case(WEB, tf, WEB, dst, UNIT_SHAPE)
    if name == 'overhang':        # the turned source's own bounding box and 7 pixels more on every side
        return Case(WEB, ROT30, WEB, *_grown(*suggested_warp_grid(WEB, ROT30, SRC_SHAPE, WEB), 7))
    if name == 'two-crs':         # a turned Transverse Mercator source onto the suggested UTM grid
        return Case(TM25, TM_ROT30, UTM35S, *suggested_warp_grid(TM25, TM_ROT30, SRC_SHAPE, UTM35S))
    if name == 'two-crs-up2':     # 30 m -> 15 m: the un-stretched bilinear and cubic_spline builds, whatever the two scale factors
        x, y = crs.transform_coords(TM25, UTM35S, *(TM_ROT30 * (SRC_SHAPE[1] / 2, SRC_SHAPE[0] / 2)))
        return Case(TM25, TM_ROT30, UTM35S, Affine(15., 0., float(x) - 15. * UNIT_SHAPE[1] / 2, 0., -15., float(y) + 15. * UNIT_SHAPE[0] / 2),
                    UNIT_SHAPE)
    if name == 'two-crs-down3':
        tf, (h, w) = suggested_warp_grid(TM25, TM_ROT30, SRC_SHAPE, UTM35S)
        return Case(TM25, TM_ROT30, UTM35S, Affine(tf.a * 3, 0., tf.c, 0., tf.e * 3, tf.f), (h // 3 + 2, w // 3 + 2))
    raise KeyError(name)


CASES = ('rot30', 'rot30-down3', 'rot90', 'sheared', 'rotated-dst', 'overhang', 'two-crs', 'two-crs-up2', 'two-crs-down3')


def source(nodata, seed=14, bands=1, shape=SRC_SHAPE):
    """ onp.synth_pair sources (positive: the relative bar of lanczos is meaningful), 'frame+holes' """
    out = []
    for b in range(bands):
        a, _ = onp.synth_pair(*shape, seed + b, 'frame+holes')
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


def _coords_padded(ctx, warp, shape, offset, pad=5):
    """ Context.warp_coords_affine into planes with spare pitch; the slack must come back untouched """
    h, w = shape
    stores = [np.empty((h, w + pad), np.float64) for _ in range(2)]
    for s in stores:
        s.view(np.uint8)[...] = SENTINEL
    x, y = ctx.warp_coords_affine(warp, shape, offset, out=(stores[0][:, :w], stores[1][:, :w]))
    for s in stores:
        assert (s[:, w:].view(np.uint8) == SENTINEL).all(), 'a coordinate plane was written outside its width'
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


# -- 1. coordinates, one CRS --------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('pair', list(rg.PAIRS))
def test_affine_coords_against_exact_rational_arithmetic(ctx, pair):
    src_tf, dst_tf = rg.PAIRS[pair]
    warp = _hk.make_affine_warp_desc(None, src_tf, None, dst_tf)
    worst = 0.
    for what, shape, off in rg.LATTICES:
        gx, gy = _coords_padded(ctx, warp, shape, (off, off))
        assert np.isfinite(gx).all() and np.isfinite(gy).all()
        err, bar = rg.max_error(pair, shape, off, gx, gy), rg.bar(pair, shape, off)
        print(f'[warp_coords_affine] {pair} {what}: largest error {err:.3e} source pixels, bar {bar:.3e} ({err / bar:.3f} of it)')
        worst = max(worst, err)
        assert err <= bar, f'{pair} {what}: {err} > {bar}'
        nx, ny = rg.coords_np(src_tf, dst_tf, shape, off)     # and the numpy statement of the same expressions, to the bit
        assert np.array_equal(gx, nx) and np.array_equal(gy, ny), f'{pair} {what}: not the stated association'
    print(f'[warp_coords_affine] {pair}: largest error {worst:.3e} source pixels')
    if pair == '90deg-1m':
        assert worst == 0.


# -- 2. coordinates, two CRSs -------------------------------------------------------------------------------------------------------
TWO_CRS_PAIRS = {   # name: (source CRS, source geo-transform, destination CRS, destination geo-transform)
    'rot30-tm25-to-utm35s': (TM25, TM_ROT30, UTM35S, Affine(30., 0., 254000., 0., -30., 6278000.)),
    'wgs84-to-rot15-utm35s': (WGS84, Affine(0.0003, 0., 24.35, 0., -0.0003, -33.55), UTM35S, rg.rotated(254000., 6278000., 15., 30.)),
}


@pytest.mark.oracle
@pytest.mark.parametrize('pair', list(TWO_CRS_PAIRS))
def test_affine_coords_across_crss_against_mpmath(ctx, pair):
    """ centres of a 35 x 263 destination grid (more than one tile in both directions, for every tile shape tried) and corners of a small lattice: the device's
    source pixel coordinates against the exact CRS transformation of the destination positions, taken through the exact source
    affine """
    src_crs, s, dst_crs, d = TWO_CRS_PAIRS[pair]
    c = Case(src_crs, s, dst_crs, d, (35, 263))
    m_per_unit = M_PER_DEG if c.src_def.is_geographic else 1.
    px_m = [v * m_per_unit for v in (math.hypot(s.a, s.d), math.hypot(s.b, s.e))]
    for what, shape, off in (('centres', (35, 263), 0.5), ('corners', (7, 41), 0.)):
        gx, gy = _coords_padded(ctx, c.warp, shape, (off, off))
        assert np.isfinite(gx).all() and np.isfinite(gy).all()
        rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        X, Y = (d.c + (cols + off) * d.a) + (rows + off) * d.b, (d.f + (cols + off) * d.d) + (rows + off) * d.e   # as the device
        exact = _crs_mp.transform_many(tuple(c.dst_def), tuple(c.src_def), X.ravel(), Y.ravel())
        with _crs_mp.mp.workdps(_crs_mp.DPS):
            mpf = _crs_mp.mp.mpf
            sa, sb, sc, sd, se, sf = (mpf(v) for v in s[:6])
            det = sa * se - sb * sd
            exact_px = [(((ex - sc) * se - (ey - sf) * sb) / det, ((ey - sf) * sa - (ex - sc) * sd) / det) for ex, ey in exact]
        err = _crs_mp.max_error(gx.ravel(), gy.ravel(), exact_px, px_m[0], px_m[1])
        print(f'[warp_coords_affine] {pair} {what}: largest error {err:.3e} m')
        assert err < BAR_M, f'{pair} {what}: {err} m'


# -- 3. re-samplers -----------------------------------------------------------------------------------------------------------------
def _resample_case(ctx, case_name, resampling, nodata):
    c = make_case(case_name)
    src = source(nodata)
    fill = 0. if nodata is None else np.nan
    got = ctx.reproject_affine(src, nodata, c.warp, c.scale, c.dst_shape, onp.RESAMPLING_CODES[resampling], fill)
    sx, sy = ctx.warp_coords_affine(c.warp, c.dst_shape)
    exp = wr.warp_resample(src, nodata, sx, sy, c.scale[0], c.scale[1], dst_nodata=fill, resampling=resampling)
    check_band(got, exp, resampling, f'{case_name} {resampling} nodata {nodata}')
    return c, got, sx, sy


@pytest.mark.oracle
@pytest.mark.parametrize('resampling', wr.MODES)
@pytest.mark.parametrize('case_name', CASES)
def test_affine_resamplers_equal_the_restatement_on_the_devices_coordinates(ctx, case_name, resampling):
    c, got, sx, sy = _resample_case(ctx, case_name, resampling, np.nan)
    inside = (sx >= 0) & (sx < SRC_SHAPE[1]) & (sy >= 0) & (sy < SRC_SHAPE[0])
    assert np.isnan(got[~inside]).all()          # dst_fill where the destination has no source
    assert (~inside).any() and (~np.isnan(got)).sum() > 0.3 * inside.sum()
    if case_name == 'overhang':
        assert not inside[:7].any() and not inside[-7:].any() and not inside[:, :7].any() and not inside[:, -7:].any()
    expected = 3. if case_name.endswith('down3') else 0.5 if case_name.endswith('up2') else 1.
    tol = 0.02 if case_name == 'sheared' else 1e-3 if case_name.startswith('two-crs') else 1e-12
    assert abs(c.scale[0] / expected - 1.) < tol and abs(c.scale[1] / expected - 1.) < tol


@pytest.mark.oracle
@pytest.mark.parametrize('nodata', [None, -9999.], ids=['none', 'number'])
def test_bilinear_at_30_degrees_with_nodata_none_and_number(ctx, nodata):
    _resample_case(ctx, 'rot30', 'bilinear', nodata)


# -- 3b. re-samplers against the exact statement --------------------------------------------------------------------------------------
SMALL_SHAPE = (24, 36)
SMALL_CASES = ('rot30', 'rot30-up', 'rot30-down3', 'sheared', 'rotated-dst', 'two-crs', 'two-crs-up', 'two-crs-down3')


def small_case(name):
    """ WARP_AFFINE_SAME and WARP_AFFINE on a 24 x 36 source: grids small enough for rational arithmetic at every pixel.  The source
    turned by 30 degrees spans 43.2 x 38.8 pixels of its own size """
    def centred(tf, res, shape, shift=(0., 0.)):
        d = _centred(tf, res, shape, SMALL_SHAPE)
        return Case(WEB, tf, WEB, Affine(d.a, 0., d.c + shift[0], 0., d.e, d.f + shift[1]), shape, src_shape=SMALL_SHAPE)
    if name == 'rot30':           # unit scale, wider than the turned source
        return centred(ROT30, 30., (36, 52))
    if name == 'rot30-up':        # 0.4 source pixels per pixel: the tap form of bilinear and cubic_spline
        return centred(ROT30, 12., (40, 56))
    if name == 'rot30-down3':     # three times coarser, 48 x 54 source pixels: overhangs the turned source on all sides
        return centred(ROT30, 90., (16, 18))
    if name == 'sheared':         # off the lattice on which this shear's coordinates are whole numbers (guard 2 of the statement)
        return centred(Affine(30., 3., X0, -2., -30., Y0), 30., (30, 44), shift=(7.3, -4.1))
    if name == 'rotated-dst':     # a north-up source onto a destination turned by 15 degrees
        tf, shape = Affine(30., 0., X0, 0., -30., Y0), (30, 44)
        xc, yc = tf * (SMALL_SHAPE[1] / 2, SMALL_SHAPE[0] / 2)
        dst = Affine.translation(xc, yc) * Affine.rotation(15.) * Affine.scale(30., -30.) * Affine.translation(-shape[1] / 2,
                                                                                                          -shape[0] / 2)
        return Case(WEB, tf, WEB, dst, shape, src_shape=SMALL_SHAPE)
    tf, (h, w) = suggested_warp_grid(TM25, TM_ROT30, SMALL_SHAPE, UTM35S)
    if name == 'two-crs':         # a turned Transverse Mercator source onto the suggested UTM grid
        return Case(TM25, TM_ROT30, UTM35S, tf, (h, w), src_shape=SMALL_SHAPE)
    if name == 'two-crs-up':      # 30 m -> 12 m about the source's centre
        x, y = crs.transform_coords(TM25, UTM35S, *(TM_ROT30 * (SMALL_SHAPE[1] / 2, SMALL_SHAPE[0] / 2)))
        return Case(TM25, TM_ROT30, UTM35S, Affine(12., 0., float(x) - 12. * 28, 0., -12., float(y) + 12. * 20), (40, 56),
                    src_shape=SMALL_SHAPE)
    if name == 'two-crs-down3':
        return Case(TM25, TM_ROT30, UTM35S, Affine(tf.a * 3, 0., tf.c, 0., tf.e * 3, tf.f), (h // 3 + 2, w // 3 + 2),
                    src_shape=SMALL_SHAPE)
    raise KeyError(name)


@pytest.mark.oracle
@pytest.mark.parametrize('nodata', [np.nan, -9999.], ids=['nan', 'number'])
@pytest.mark.parametrize('resampling', wr.MODES)
@pytest.mark.parametrize('case_name', SMALL_CASES)
def test_affine_resamplers_inside_the_exact_enclosure(ctx, case_name, resampling, nodata):
    """ the affine builds of hk_warp.hip held DIRECTLY to the exact statement of tests/_resample_exact.py on the device's own
    coordinate planes, which are arbitrary doubles: identical nodata pattern, bit-equal for nearest, inside the enclosure for the
    rest; the guards of the statement make a case that would exempt a pixel fail as mis-designed.  The exact side is computed once
    per (case, method) and serves both nodata variants. """
    c = small_case(case_name)
    assert max(c.dst_shape) <= 60 and c.same == (not case_name.startswith('two-crs'))
    src = source(nodata, shape=SMALL_SHAPE)
    got = ctx.reproject_affine(src, nodata, c.warp, c.scale, c.dst_shape, onp.RESAMPLING_CODES[resampling], np.nan)
    sx, sy = ctx.warp_coords_affine(c.warp, c.dst_shape)
    inside = (sx >= 0) & (sx < SMALL_SHAPE[1]) & (sy >= 0) & (sy < SMALL_SHAPE[0])
    res = rx.enclosure_failures_at(got, src, nodata, sx, sy, c.scale[0], c.scale[1], resampling)
    rx.assert_held(res, f'device affine {case_name} {resampling} nodata {nodata}', 0.3 * inside.sum())
    if not case_name.endswith('-up'):
        assert (~inside).any()
    if case_name == 'rot30-down3':      # overhangs the source on all four sides
        assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any()
    expected = 3. if case_name.endswith('down3') else 0.4 if case_name.endswith('-up') else 1.
    tol = 0.02 if case_name == 'sheared' else 1e-3 if case_name.startswith('two-crs') else 1e-12
    assert abs(c.scale[0] / expected - 1.) < tol and abs(c.scale[1] / expected - 1.) < tol
    assert rx.uses_conv('bilinear', *c.scale) == (max(c.scale) > 1 + 1e-9)


# -- 4. exact turns -----------------------------------------------------------------------------------------------------------------
def _turned(data, tf, quarter_turns, south_up):
    """ `data` on the north-up grid `tf` as a file would hold it after np.rot90 (and a flip of the rows): the stored array and the
    geo-transform that puts every stored pixel where it was """
    arr, t = data, tf
    for _ in range(quarter_turns):
        w = arr.shape[-1]
        arr, t = np.rot90(arr, axes=(-2, -1)), t * Affine(0., -1., float(w), 1., 0., 0.)   # column = w - stored row, row = stored column
    if south_up:
        arr, t = arr[..., ::-1, :], t * Affine(1., 0., 0., 0., -1., float(arr.shape[-2]))
    return np.ascontiguousarray(arr), t


NORTH_UP = Affine(1., 0., X0, 0., -1., Y0)


@pytest.mark.oracle
@pytest.mark.parametrize('south_up', [False, True], ids=['north-up', 'south-up'])
@pytest.mark.parametrize('quarter_turns', [1, 2, 3], ids=['90', '180', '270'])
@pytest.mark.parametrize('resampling', ['nearest', 'bilinear'])
def test_an_exact_turn_comes_back_bit_for_bit(ctx, resampling, quarter_turns, south_up):
    """ integer origin, pixel 1.0: every coordinate is an exact half-integer, so both methods must return the very samples """
    data = source(np.nan, seed=17, shape=UNIT_SHAPE)
    arr, tf = _turned(data, NORTH_UP, quarter_turns, south_up)
    assert arr.shape == (UNIT_SHAPE if quarter_turns == 2 else UNIT_SHAPE[::-1])
    back = RasterArray(arr, WEB, tf).reproject(transform=NORTH_UP, shape=UNIT_SHAPE, resampling=resampling, nodata=np.nan, context=ctx)
    assert_same_f32(back.array, data, f'{quarter_turns} quarter turns, south-up {south_up}, {resampling}')
    assert (~np.isnan(data)).mean() > 0.5


# -- 5. entry points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('case_name', ['rot30', 'two-crs'])
def test_the_device_entry_points_equal_the_host_ones(ctx, case_name):
    """ hk_warp_coords_affine_dev and hk_reproject_affine_dev on planes with slack equal the host entry points (which test 3 holds
    to the restatement); three bands in one call equal three calls of one band """
    c = make_case(case_name)
    h, w = c.dst_shape
    x, y = ctx.warp_coords_affine(c.warp, c.dst_shape)
    stride = w + 3
    store = np.empty((2, h, stride), np.float64)
    store.view(np.uint8)[...] = SENTINEL
    src = source(np.nan, seed=20, bands=3)
    nb, sh, sw = src.shape
    s_store = np.full((nb, sh + 2, sw + 3), np.float32(7.), np.float32)
    s_store[:, :sh, :sw] = src
    d_store = np.empty((nb, h + 1, w + 5), np.float32)
    d_store.view(np.uint8)[...] = SENTINEL
    d_xy, d_src, d_dst = ctx.dev_alloc(store.nbytes), ctx.dev_alloc(s_store.nbytes), ctx.dev_alloc(d_store.nbytes)
    try:
        ctx.h2d(d_xy, store)
        ctx.h2d(d_src, s_store)
        ctx.h2d(d_dst, d_store)
        ctx.warp_coords_affine_dev(c.warp, c.dst_shape, d_xy, d_xy + h * stride * 8, stride)
        ctx.reproject_affine_dev(c.warp, d_src, nb, (sh, sw), s_store.shape[2], s_store.shape[1] * s_store.shape[2], np.nan, c.scale,
                                 1, d_dst, (h, w), d_store.shape[2], d_store.shape[1] * d_store.shape[2], np.nan)
        ctx.stream_sync(0)
        ctx.d2h(store, d_xy)
        ctx.d2h(d_store, d_dst)
    finally:
        for d in (d_xy, d_src, d_dst):
            ctx.dev_free(d)
    assert (store[:, :, w:].view(np.uint8) == SENTINEL).all()
    assert np.array_equal(store[0, :, :w], x, equal_nan=True) and np.array_equal(store[1, :, :w], y, equal_nan=True)
    got = np.ascontiguousarray(d_store[:, :h, :w])
    slack = d_store.copy()
    slack[:, :h, :w].view(np.uint8)[...] = SENTINEL
    assert (slack.view(np.uint8) == SENTINEL).all(), 'the destination was written outside its height x width'
    host = ctx.reproject_affine(src, np.nan, c.warp, c.scale, c.dst_shape, 1, np.nan)
    assert_same_f32(host, got, 'host against device entry point')
    for b in range(nb):
        assert_same_f32(ctx.reproject_affine(src[b], np.nan, c.warp, c.scale, c.dst_shape, 1, np.nan), host[b], f'band {b} alone')
    assert (~np.isnan(host)).mean() > 0.1


# -- 6. the pipeline ----------------------------------------------------------------------------------------------------------------
def _covering_ref(src_crs, src_tf, src_shape, ref_crs, seed, bands):
    """ a 30 m north-up reference in `ref_crs` that covers the source with a margin """
    sh, sw = src_shape
    xs, ys = zip(*(src_tf * p for p in ((0., 0.), (sw, 0.), (sw, sh), (0., sh))))
    xs, ys = np.array(xs), np.array(ys)
    if not crs.same_crs(src_crs, ref_crs):
        xs, ys = crs.transform_coords(src_crs, ref_crs, xs, ys)
    left, top = math.floor(xs.min() / 30.) * 30. - 300., math.ceil(ys.max() / 30.) * 30. + 300.
    rw, rh = int((xs.max() - left) / 30.) + 12, int((top - ys.min()) / 30.) + 12
    ref = np.stack([onp.synth_pair(rh, rw, seed + b, 'frame+holes')[1] for b in range(bands)])
    return ref, Affine(30., 0., left, 0., -30., top)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """ rot30.tif: 2 bands, 5 m, turned by 30 degrees, label EPSG:3857; ref.tif: 30 m north-up in the same CRS, covering it;
    tm_rot30.tif / utm_ref.tif: the same in Transverse Mercator lon0 25 against EPSG:32735;
    turn90.tif / plain.tif / plain_ref.tif: a raster stored turned by 90 degrees, the same raster north-up, and their reference """
    d = str(tmp_path_factory.mktemp('rotated'))
    out = dict(dir=d)
    shape, bands = (200, 260), 2
    src = np.stack([onp.synth_pair(*shape, 30 + b, 'frame+holes')[0] for b in range(bands)])
    for tag, src_crs, ref_crs, tf in (('one', WEB, WEB, rg.rotated(X0, Y0, 30., 5.)),
                                      ('two', TM25, UTM35S, rg.rotated(-60000., -3723000., 30., 5.))):
        ref, ref_tf = _covering_ref(src_crs, tf, shape, ref_crs, 40, bands)
        out[f'{tag}_src'], out[f'{tag}_ref'] = os.path.join(d, f'{tag}_rot30.tif'), os.path.join(d, f'{tag}_ref.tif')
        write_tiff(out[f'{tag}_src'], src, tf, src_crs, float('nan'), rotated=True)
        write_tiff(out[f'{tag}_ref'], ref, ref_tf, ref_crs, float('nan'))
    plain_tf = Affine(5., 0., X0, 0., -5., Y0)
    turned, turned_tf = _turned(src, plain_tf, 1, False)
    ref, ref_tf = _covering_ref(WEB, plain_tf, shape, WEB, 50, bands)
    out.update(turn90=os.path.join(d, 'turn90.tif'), plain=os.path.join(d, 'plain.tif'), plain_ref=os.path.join(d, 'plain_ref.tif'))
    write_tiff(out['turn90'], turned, turned_tf, WEB, float('nan'), rotated=True)
    write_tiff(out['plain'], src, plain_tf, WEB, float('nan'))
    write_tiff(out['plain_ref'], ref, ref_tf, WEB, float('nan'))
    return out


def _ra(fn):
    t = read_tiff(fn)
    return RasterArray(t.array, t.crs, t.transform, nodata=t.nodata)


def _north_up_by_hand(ra):
    tf, shape = suggested_warp_grid(ra.crs, ra.transform, ra.shape, ra.crs)
    return ra.reproject(transform=tf, shape=shape, resampling=Resampling.bilinear)


def _process(fuse, d, tag, model):
    return fuse.process(os.path.join(d, f'corr_{tag}.tif'), param_filename=os.path.join(d, f'param_{tag}.tif'), model=model,
                        kernel_shape=(5, 5), overwrite=True)


@pytest.mark.oracle
@pytest.mark.parametrize('model', ['gain-blk-offset', 'gain-offset'])
def test_raster_fuse_on_a_rotated_file_equals_the_hand_warped_raster(ctx, files, model):
    with warnings.catch_warnings():
        warnings.simplefilter('error', ImageFormatWarning)      # rotation alone warns of nothing
        fuse = RasterFuse(files['one_src'], files['one_ref'])
    hand_src = _north_up_by_hand(_ra(files['one_src']))
    assert hand_src.transform.b == 0 and hand_src.transform.e < 0 and hand_src.shape != (200, 260)
    corr, params = _process(fuse, files['dir'], f'one_{model}', model)
    exp_corr, exp_params = _process(RasterFuse(hand_src, _ra(files['one_ref'])), files['dir'], f'one_hand_{model}', model)
    assert_same_f32(corr, exp_corr, 'corrected')
    assert_same_f32(params, exp_params, 'parameters')
    assert (~np.isnan(corr)).mean() > 0.3 and (~np.isnan(params)).mean() > 0.2
    written = read_tiff(os.path.join(files['dir'], f'corr_one_{model}.tif'))      # north-up, on the warped source's grid
    assert tuple(written.transform) == tuple(hand_src.transform) and written.crs == WEB
    assert_same_f32(written.array, corr, 'corrected file')


@pytest.mark.oracle
@pytest.mark.parametrize('model', ['gain-blk-offset', 'gain-offset'])
def test_raster_fuse_on_a_quarter_turned_file_equals_the_unrotated_pair(ctx, files, model):
    corr, params = _process(RasterFuse(files['turn90'], files['plain_ref']), files['dir'], f'turn_{model}', model)
    exp_corr, exp_params = _process(RasterFuse(files['plain'], files['plain_ref']), files['dir'], f'plain_{model}', model)
    assert_same_f32(corr, exp_corr, 'corrected')
    assert_same_f32(params, exp_params, 'parameters')
    assert corr.shape == (2, 200, 260) and (~np.isnan(corr)).mean() > 0.3


@pytest.mark.oracle
def test_raster_compare_on_a_rotated_file_equals_the_hand_warped_raster(ctx, files):
    got = RasterCompare(files['one_src'], files['one_ref']).process()
    exp = RasterCompare(_north_up_by_hand(_ra(files['one_src'])), _ra(files['one_ref'])).process()
    assert got == exp and got['Mean']['n'] > 1000


@pytest.mark.oracle
@pytest.mark.parametrize('proc_crs', ['src', 'ref'])
def test_a_rotated_source_and_a_reference_in_another_crs(ctx, files, proc_crs):
    """ proc_crs=src: the source goes from its rotated grid into the reference's CRS in ONE warp; proc_crs=ref: the reference is
    warped into the source's CRS, and the source goes north-up there """
    with pytest.warns(ImageFormatWarning, match='re-projected to the same CRS'):
        fuse = RasterFuse(files['two_src'], files['two_ref'], proc_crs=proc_crs)
    src_ra, ref_ra = _ra(files['two_src']), _ra(files['two_ref'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if proc_crs == 'src':
            hand = RasterFuse(src_ra.reproject(crs=ref_ra.crs, resampling=Resampling.bilinear), ref_ra, proc_crs=proc_crs)
        else:
            hand = RasterFuse(_north_up_by_hand(src_ra), ref_ra.reproject(crs=src_ra.crs, resampling=Resampling.bilinear),
                              proc_crs=proc_crs)
        corr, params = _process(fuse, files['dir'], f'two_{proc_crs}', 'gain-blk-offset')
        exp_corr, exp_params = _process(hand, files['dir'], f'two_hand_{proc_crs}', 'gain-blk-offset')
    assert fuse.proc_crs.name == proc_crs
    assert_same_f32(corr, exp_corr, 'corrected')
    assert_same_f32(params, exp_params, 'parameters')
    assert (~np.isnan(corr)).mean() > 0.3 and (~np.isnan(params)).mean() > 0.2


# -- 7. refusals at the C boundary ----------------------------------------------------------------------------------------------------
def test_the_c_boundary_refuses_what_is_not_built(ctx):
    c = make_case('rot30')
    src = source(np.nan)
    with pytest.raises(DeviceError, match='footprint'):
        ctx.reproject_affine(src, np.nan, c.warp, c.scale, c.dst_shape, int(Resampling.average), np.nan)
    flat = _hk.make_affine_warp_desc(None, Affine(30., 15., X0, -30., -15., Y0), None, c.dst_tf)      # det = 0
    with pytest.raises(ValueError, match='degenerate'):        # HK_ERR_ARG: an unusable descriptor
        ctx.warp_coords_affine(flat, (4, 4))
    with pytest.raises(ValueError, match='degenerate'):
        ctx.reproject_affine(src, np.nan, flat, (1., 1.), (4, 4), 1, np.nan)
    for bad in (float('nan'), float('inf')):
        w = _hk.make_affine_warp_desc(None, Affine(30., 3., bad, 0., -30., Y0), None, c.dst_tf)
        with pytest.raises(ValueError, match='finite'):
            ctx.warp_coords_affine(w, (4, 4))
    airy = CRS('OSGB [1024=1; 2057=6377563.396; 2059=299.3249646; 3075=1; 3080=-2.0; 3081=49.0; 3082=400000.0; 3083=-100000.0; '
               '3092=0.9996012717]')
    w = _hk.make_affine_warp_desc(crs.parse(airy), ROT30, crs.parse(UTM35S), c.dst_tf)
    with pytest.raises(DeviceError, match='ellipsoid'):
        ctx.warp_coords_affine(w, (4, 4))
    with pytest.raises(NotImplementedError, match='EPSG:3857'):      # two CRSs need both defined, rotated or not
        RasterArray(src, WEB, ROT30).reproject(crs=UTM35S, resampling='bilinear', context=ctx)
