""" The generic re-samplers of hk_resample.hip (resample_kernel, resample_conv_kernel) through hk_reproject.

* every method of RESAMPLING_CODES held DIRECTLY to the exact statement of tests/_resample_exact.py -- rational arithmetic written
  from GDAL's rule, sharing no formula with the kernel or with oracle_np --: the tap form up-sampling, the convolution form (cubic,
  lanczos, stretched bilinear / cubic / cubic_spline) up, down and one axis each, nearest, and the nine footprint methods on a source
  with ties; identical nodata pattern, the exact-valued methods to the bit, the others inside the enclosure stated there
  (``1/2 ulp32 + 2^-40 A``; lanczos absolute, on signed sources); no pixel exempt (a case that breaks a guard of the statement fails
  as mis-designed);
* the edges, against oracle_np.reproject bit for bit (lanczos: the project's bar, same nodata pattern and 1e-6 relative, the
  device's ``sin`` differs from the host's in the last bit): several bands in one call, sources of one to nine pixels for every built
  method up and down, destinations wholly and partly outside the source, a numeric fill value, numeric nodata, destinations of one row
  and of one column. """
import numpy as np
import pytest

import _resample_exact as rx
from conftest import assert_same_f32
from homonim_amd import _hk
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

CODES = onp.RESAMPLING_CODES
METHODS = sorted(CODES, key=CODES.get)


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def _same(got, exp, method, what):
    if method != 'lanczos':
        return assert_same_f32(got, exp, what)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    fill_g, fill_e = np.isnan(got), np.isnan(exp)
    assert (fill_g == fill_e).all(), f'{what}: nodata pattern'
    ok = ~fill_e
    assert (np.abs(got[ok] - exp[ok]) <= 1e-6 * np.abs(exp[ok])).all(), what


def _both(ctx, src, nodata, mapping, dst_shape, method, fill=np.nan):
    got = ctx.reproject(src, nodata, mapping, dst_shape, CODES[method], fill)
    exp = onp.reproject(src, nodata, mapping, dst_shape, dst_nodata=fill, resampling=method)
    return got, exp


def _hold(ctx, method, mapping, dst_shape, nodata, src_shape):
    src = rx.source(src_shape, nodata)
    got = ctx.reproject(src, nodata, mapping, dst_shape, CODES[method], np.nan)
    res = rx.enclosure_failures(got, src, nodata, mapping, dst_shape, method)
    print(f'{method} {mapping}: {res["n_valid"]} valued pixels, worst error {res["worst"]:.3f} of the bound, '
          f'{len(res["pattern"])} pattern and {len(res["value"])} value failures')
    assert not res['pattern'], f'{method} {mapping}: nodata pattern departs from the rule at {res["pattern"][:5]}'
    assert not res['value'], f'{method} {mapping}: outside the enclosure at {res["value"][:5]}'
    assert res['n_valid'] > 0.4 * dst_shape[0] * dst_shape[1]


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.UP_CASES)
@pytest.mark.parametrize('method', ['bilinear', 'cubic_spline'])
def test_device_upsamplers_inside_the_exact_enclosure(ctx, method, mapping, dst_shape, nodata):
    _hold(ctx, method, mapping, dst_shape, nodata, (13, 21))


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.DOWN_CASES)
def test_device_average_inside_the_exact_enclosure(ctx, mapping, dst_shape, nodata):
    _hold(ctx, 'average', mapping, dst_shape, nodata, rx.AVG_SHAPE)


def _hold_res(res, what, n_min):
    rx.assert_held(res, f'device {what}', n_min)


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('half', [0, 1])
@pytest.mark.parametrize('method', METHODS)
def test_every_method_inside_the_exact_enclosure(ctx, method, nodata, half):
    """ every method of RESAMPLING_CODES on every dyadic case the statement holds it on (in two halves, which keeps each test
    short): the convolution form (cubic and lanczos at every scale, the stretched bilinear / cubic / cubic_spline, one axis up and
    one down), nearest, and the footprint methods on a source with ties.  Signed sources throughout, lanczos included: its
    enclosure is absolute.  The exact side is computed once for both nodata variants. """
    cases = rx.scaled_cases(method)[half::2]
    assert cases
    for mapping, dst_shape, build in cases:
        src = build(nodata)
        got = ctx.reproject(src, nodata, mapping, dst_shape, CODES[method], np.nan)
        _hold_res(rx.enclosure_failures(got, src, nodata, mapping, dst_shape, method), f'{method} {mapping} nodata {nodata}',
                  0.4 * dst_shape[0] * dst_shape[1])


@pytest.mark.parametrize('method', METHODS)
def test_every_method_with_a_numeric_fill(ctx, method):
    """ dst_fill = -9999 where the rule gives nothing: the pattern is read off the fill value, the values are held as before """
    mapping, dst_shape, build = rx.scaled_cases(method)[-1]
    src = build(np.nan)
    got = ctx.reproject(src, np.nan, mapping, dst_shape, CODES[method], -9999.)
    assert not np.isnan(got).any() and (got == -9999.).any()
    _hold_res(rx.enclosure_failures(got, src, np.nan, mapping, dst_shape, method, fill=-9999.), f'{method} {mapping} fill -9999',
              0.4 * dst_shape[0] * dst_shape[1])


# -- edges -----------------------------------------------------------------------------------------------------------
def _for(method, a):
    """ lanczos is held to a RELATIVE bar, which says nothing of a sum that cancels: it gets the field's magnitude (as the project's
    other lanczos tests use positive rasters); every other method keeps the signs """
    return (np.abs(a) + np.float32(0.05)).astype(np.float32) if method == 'lanczos' else a


def _field(shape, seed=3, method=None):
    """ a few repeated values among random ones, so that the rank-order methods have ties to break """
    rng = np.random.default_rng(seed)
    a = rng.normal(0.2, 1., shape).astype(np.float32)
    a[rng.random(shape) < 0.15] = np.float32(0.5)
    return _for(method, a)


@pytest.mark.parametrize('method, mapping, dst_shape', [('cubic_spline', (.375, -.25, .375, .125), (36, 58)),
                                                         ('average', (2.5, -1.25, 2.5, .375), (6, 9)),
                                                         ('lanczos', (1.5, .125, .75, -.25), (20, 12)),
                                                         ('med', (2., 0., 3., .5), (5, 10))])
def test_three_bands_in_one_call(ctx, method, mapping, dst_shape):
    """ band strides of source and destination: every band of a three-band call equals its single-band call and the oracle """
    src = _for(method, np.stack([rx.source(), _field((13, 21), 8), -rx.source() * np.float32(1.5)]))
    src[1, 2:5, 10:12] = np.nan
    got = ctx.reproject(src, np.nan, mapping, dst_shape, CODES[method], np.nan)
    assert got.shape == (3, *dst_shape)
    for b in range(3):
        alone, exp = _both(ctx, src[b], np.nan, mapping, dst_shape, method)
        assert_same_f32(got[b], alone, f'{method} band {b} of three vs alone')
        _same(got[b], exp, method, f'{method} band {b}')
    assert not np.array_equal(got[0], got[1], equal_nan=True)


@pytest.mark.parametrize('method', METHODS)
def test_sources_of_a_few_pixels(ctx, method):
    """ 1 x 1 to 3 x 3 sources, up (0.4 source pixels per destination pixel) and down (1.6), the destination reaching past the source on
    every side: every tap rule meets both edges of the plane at once """
    for shape in ((1, 1), (1, 7), (5, 1), (2, 2), (3, 3)):
        src = _field(shape, 10 + shape[0] * shape[1], method)
        if shape == (3, 3):
            src[1, 1] = np.nan
        for k, o in ((.4, -.3), (1.6, -.8)):
            dst_shape = (int(np.ceil((shape[0] + 1.) / k)), int(np.ceil((shape[1] + 1.) / k)))
            got, exp = _both(ctx, src, np.nan, (k, o, k, o), dst_shape, method)
            _same(got, exp, method, f'{method} source {shape} k {k}')
            assert np.isfinite(exp).any()


@pytest.mark.parametrize('method', METHODS)
def test_destination_outside_the_source(ctx, method):
    src = _field((9, 14), method=method)
    src[3:5, 6:9] = np.nan
    # wholly outside, far off and just off the corner: nothing but fill
    for mapping in ((1., 100., 1., 100.), (.5, -40., .5, 3.), (2., 14., 2., 9.)):
        got = ctx.reproject(src, np.nan, mapping, (6, 8), CODES[method], np.nan)
        assert np.isnan(got).all(), f'{method} {mapping}'
    # partly outside on all four sides, up and down
    for mapping, dst_shape in (((.5, -3., .5, -2.25), (30, 44)), ((2., -5., 1.5, -3.5), (11, 13))):
        got, exp = _both(ctx, src, np.nan, mapping, dst_shape, method)
        _same(got, exp, method, f'{method} partly outside {mapping}')
        for edge in (exp[0], exp[-1], exp[:, 0], exp[:, -1]):
            assert np.isnan(edge).all()
        assert np.isfinite(exp).sum() > 0.2 * exp.size


@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cubic', 'cubic_spline', 'average', 'mode', 'max', 'sum'])
def test_numeric_fill_and_numeric_nodata(ctx, method):
    """ dst_fill = -9999 where nothing lands; nodata 7.5 in the source, which is not the fill """
    src = _field((12, 17), 4)
    src[4:7, 3:8] = np.float32(7.5)
    src[0, :2] = np.float32(7.5)
    for mapping, dst_shape in (((.5, -1.5, .5, -1.), (28, 40)), ((2.5, -3.75, 2., -2.5), (8, 9))):
        got, exp = _both(ctx, src, 7.5, mapping, dst_shape, method, fill=-9999.)
        assert not np.isnan(exp).any() and (exp == -9999.).any() and (exp != -9999.).sum() > 0.25 * exp.size
        if method in ('nearest', 'mode', 'max'):
            assert not (exp == 7.5).any()
        assert_same_f32(got, exp, f'{method} {mapping} fill -9999, nodata 7.5')


@pytest.mark.parametrize('method', ['nearest', 'bilinear', 'cubic_spline', 'average', 'lanczos'])
@pytest.mark.parametrize('dst_shape', [(1, 257), (17, 1)])
def test_destinations_of_one_row_and_of_one_column(ctx, method, dst_shape):
    """ 257 columns: a second block of one lane; one column: a block of one lane in every row """
    src = _field((23, 300), 6, method)
    src[:, 100:104] = np.nan
    k = (1.25 if method in ('average', 'lanczos') else .75)
    mapping = (k * 300. / 257. if dst_shape[1] > 1 else k, .5, k, 1.)
    mapping = tuple(float(np.float32(v)) for v in mapping)
    got, exp = _both(ctx, src, np.nan, mapping, dst_shape, method)
    _same(got, exp, method, f'{method} destination {dst_shape}')
    assert np.isfinite(exp).sum() > 0.5 * exp.size
