""" oracle_np.reproject and tests/_warp_reference.py held to the exact statement of tests/_resample_exact.py: identical nodata pattern
and every pixel inside the enclosure stated there (bit-equal for the exact-valued methods), for every method of the scaled path on
dyadic grids and for the five point methods on per-pixel coordinates that are not dyadic, NaN and numeric nodata.  The device
kernels are held bit for bit to these two elsewhere, and to the same statement directly in tests/test_gpu_resample_exact.py,
tests/test_gpu_warp.py and tests/test_gpu_rotated.py; the statement itself is checked here against hand-worked pixels. """
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import _resample_exact as rx
import _warp_reference as wr
from oracle import oracle_np as onp


def test_the_statement_on_hand_worked_pixels():
    src = np.arange(1, 13, dtype=np.float32).reshape(3, 4)   # rows 1..4, 5..8, 9..12
    src[1, 2] = np.nan
    # bilinear, 2x up-sampling: destination (2, 2) has its centre at source (1.25, 1.25): taps rows 0, 1 x columns 0, 1, d = 3/4
    v, a, w = rx.exact(src, np.nan, (.5, 0., .5, 0.), (6, 8), 'bilinear')
    assert w[2, 2] == 1 and v[2, 2] == Fr(1, 16) * 1 + Fr(3, 16) * 2 + Fr(3, 16) * 5 + Fr(9, 16) * 6 and a[2, 2] == v[2, 2]
    # destination (2, 3): centre (1.25, 1.75), taps columns 1, 2 with d = 1/4; (1, 2) is nodata and dropped -> renormalised
    assert w[2, 3] == 1 - Fr(3, 4) * Fr(1, 4)
    assert v[2, 3] == (Fr(3, 16) * 2 + Fr(1, 16) * 3 + Fr(9, 16) * 6) / w[2, 3]
    # destination (2, 5): centre (1.25, 2.75) lies in the nodata pixel -> nodata whatever its taps hold
    assert v[2, 5] is None and w[2, 5] is None
    # destination (0, 0): centre (0.25, 0.25), taps -1 and 0 on both axes: only (0, 0) is inside, weight 9/16
    assert w[0, 0] == Fr(9, 16) and v[0, 0] == 1
    # cubic_spline at d = 1/2: weights 1/48, 23/48, 23/48, 1/48
    assert [t[1] for t in rx._line_weights('cubic_spline', Fr(1), Fr(0), 1)[0][1]] == [Fr(1, 6), Fr(2, 3), Fr(1, 6), 0]
    assert [t[1] for t in rx._line_weights('cubic_spline', Fr(1), Fr(1, 2), 1)[0][1]] == [Fr(1, 48), Fr(23, 48), Fr(23, 48), Fr(1, 48)]
    # average, 2.5:1 from -0.5: column 0 covers [-0.5, 2] -> clipped [0, 2]; column 1 covers [2, 4.5] -> clipped [2, 4], share 1 each
    v, a, w = rx.exact(src, np.nan, (2.5, -.5, 3., 0.), (1, 2), 'average')
    assert w[0, 0] == 6 and v[0, 0] == Fr(1 + 2 + 5 + 6 + 9 + 10, 6)
    assert w[0, 1] == 5 and v[0, 1] == Fr(3 + 4 + 8 + 11 + 12, 5)
    # average with partial shares: footprint rows [0.5, 2], columns [1.5, 3] -> shares (1/2, 1) x (1/2, 1), the nodata pixel dropped
    v, a, w = rx.exact(src, np.nan, (1.5, 1.5, 1.5, .5), (1, 1), 'average')
    assert w[0, 0] == Fr(1, 4) + Fr(1, 2) + Fr(1, 2)
    assert v[0, 0] == (Fr(1, 4) * 2 + Fr(1, 2) * 3 + Fr(1, 2) * 6) / w[0, 0] == 4 and a[0, 0] == 5
    # footprint wholly outside the plane, however close: nodata
    v, _, _ = rx.exact(src, np.nan, (2., -2.5, 2., 0.), (1, 1), 'average')
    assert v[0, 0] is None
    with pytest.raises(ValueError):
        rx.exact(src, np.nan, (.3, 0., .5, 0.), (2, 2), 'bilinear')


def _weights(method, s, k):
    """ the convolution form's (source index, weight) list on one axis, and the guard notes it left """
    notes = []
    return rx._axis_conv(method, Fr(s), Fr(k), notes)[1], notes


def test_the_convolution_form_on_hand_worked_pixels():
    # cubic (a = -1/2) un-stretched at s = 1: origin 0, d = 1/2, taps -1 .. 2 at x = -3/2, -1/2, 1/2, 3/2
    #   f(1/2) = 3/16 - 10/16 + 1 = 9/16;  f(3/2) = -27/16 + 90/16 - 6 + 2 = -1/16
    taps, _ = _weights('cubic', 1, 1)
    assert taps == [(-1, Fr(-1, 16)), (0, Fr(9, 16)), (1, Fr(9, 16)), (2, Fr(-1, 16))]
    # cubic at k = 2, s = 1: scale 1/2, x = (t - 1/2) / 2 = +-1/4, 3/4, 5/4, 7/4 for t = -3 .. 4 (|x| < 2 and no further):
    #   f(1/4) = 3/128 - 20/128 + 1 = 111/128;  f(3/4) = 81/128 - 180/128 + 1 = 29/128
    #   f(5/4) = -125/128 + 500/128 - 5 + 2 = -9/128;  f(7/4) = -343/128 + 980/128 - 7 + 2 = -3/128;  they sum to 2 = k
    taps, notes = _weights('cubic', 1, 2)
    k2 = [Fr(v, 128) for v in (-3, -9, 29, 111, 111, 29, -9, -3)]
    assert taps == list(zip(range(-3, 5), k2)) and sum(k2) == 2 and not notes
    # the tent at k = 2, s = 1: x = +-1/4, 3/4 for t = -1 .. 2: 1/4, 3/4, 3/4, 1/4, summing to 2
    taps, _ = _weights('bilinear', 1, 2)
    assert taps == [(-1, Fr(1, 4)), (0, Fr(3, 4)), (1, Fr(3, 4)), (2, Fr(1, 4))]
    # ... and the stretched B-spline there: 2/3 - 1/16 + 1/128 = 235/384;  2/3 - 9/16 + 27/128 = 121/384;  (3/4)^3 / 6 = 27/384;
    # (1/4)^3 / 6 = 1/384;  twice their sum is 768/384 = 2
    taps, _ = _weights('cubic_spline', 1, 2)
    assert [w for _, w in taps] == [Fr(v, 384) for v in (1, 27, 121, 235, 235, 121, 27, 1)]
    # a whole stretched bilinear pixel: 2:1 over rows 1..4, 5..8, 9..12 with (1, 2) nodata; destination (0, 0) has its centre at
    # (1, 1): rows and columns -1 .. 2 weigh 1/4, 3/4, 3/4, 1/4, of which -1 is outside
    src = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    src[1, 2] = np.nan
    v, a, w = rx.exact(src, np.nan, (2., 0., 2., 0.), (1, 2), 'bilinear')
    q, h = Fr(1, 4), Fr(3, 4)
    assert w[0, 0] == (h + h + q) ** 2 - h * q == Fr(46, 16)
    assert v[0, 0] == (h * (h * 1 + h * 2 + q * 3) + h * (h * 5 + h * 6) + q * (h * 9 + h * 10 + q * 11)) / w[0, 0] == Fr(203, 46)
    assert a[0, 0] == Fr(203, 16)                               # sum(|w| |v|) / min(|W|, 1), and W > 1
    # destination (0, 1): centre (1, 3): the centre pixel (1, 3) = 8 is valid; columns 1 .. 4 weigh 1/4, 3/4, 3/4, 1/4, column 4 outside
    assert w[0, 1] == (h + h + q) * (q + h + h) - h * h
    # lanczos: sinc(x) sinc(x / 3).  x = 1/2: 1 * (1/2) / (pi/2 * pi/6) = 6 / pi^2;  x = 3/2: (-1) * 1 / (3 pi/2 * pi/2) = -4 / (3 pi^2);
    # x = 3: zero, and the tap is not kept
    import mpmath as mp
    with mp.workdps(70):
        six, four = (Fr(int(mp.floor(v * mp.mpf(10) ** 55)), 10 ** 55) for v in (6 / mp.pi ** 2, 4 / (3 * mp.pi ** 2)))
    assert abs(rx.kernel('lanczos', Fr(1, 2)) - six) < Fr(1, 10 ** 40)
    assert abs(rx.kernel('lanczos', Fr(-3, 2)) + four) < Fr(1, 10 ** 40)
    assert rx.kernel('lanczos', Fr(3)) == 0 and rx.kernel('lanczos', Fr(0)) == 1
    taps, _ = _weights('lanczos', Fr(1, 2), 1)                  # d = 0: x = t, only |t| < 3 is support
    assert [t for t, _ in taps] == [-2, -1, 0, 1, 2] and [w for _, w in taps] == [0, 0, 1, 0, 0]
    taps, _ = _weights('lanczos', 1, 1)                         # d = 1/2: x = -5/2 .. 5/2, six taps
    assert [t for t, _ in taps] == [-2, -1, 0, 1, 2, 3] and taps[2][1] == taps[3][1] == rx.kernel('lanczos', Fr(1, 2))
    # guard 3: a stretched tap a hair inside the support edge is a mis-designed case, one exactly on it is not
    # (s = 1/2: d = 0 and tap 4 sits at x = 2 exactly; s = 1/2 + 2^-40 moves it to 2 - 2^-41)
    assert _weights('cubic', Fr(1, 2) + Fr(1, 2 ** 40), 2)[1] and not _weights('cubic', Fr(1, 2), 2)[1]


def test_a_cubic_pixel_whose_kept_weights_cancel_is_nodata():
    """ 2:1 cubic at the centre of an 8 x 8 source: both axes have taps t = -3 .. 4 with weights (-3, -9, 29, 111, 111, 29, -9, -3) / 128,
    the centre pixel is t = (1, 1) with 111 * 111 = 12321 (in units of 1 / 16384).  Kept besides it: the eight pixels of 111 * -9 = -999,
    six of 111 * -3 = -333, seven of 29 * -9 = -261, six of 29 * -3 = -87 and two of -3 * -3 = 9:
    12321 - 7992 - 1998 - 1827 - 522 + 18 = 0.  W = 0, below 1e-6 in magnitude: nodata, though the centre pixel is valid.  One more
    pixel kept and the value is back. """
    kept = [(-3, -3), (-3, -1), (-3, 0), (-3, 1), (-3, 2), (-3, 4), (-2, -1), (-2, 0), (-2, 1), (-2, 2), (-1, -3), (-1, -2), (-1, 3),
            (-1, 4), (0, -3), (0, -2), (0, 3), (0, 4), (1, -3), (1, -2), (1, 3), (1, 4), (2, -3), (2, -2), (2, 3), (2, 4), (3, -1),
            (3, 0), (3, 1), (1, 1)]
    a = dict(zip(range(-3, 5), (-3, -9, 29, 111, 111, 29, -9, -3)))
    assert sum(a[ty] * a[tx] for ty, tx in kept) == 0
    rng = np.random.default_rng(5)
    src = np.full((8, 8), np.nan, np.float32)
    for ty, tx in kept:
        src[ty + 3, tx + 3] = np.float32(rng.normal(0.2, 1.))
    mapping = (2., 3., 2., 3.)          # the one destination pixel has its centre at (4, 4): origin 3, d = 1/2
    v, _, w = rx.exact(src, np.nan, mapping, (1, 1), 'cubic')
    assert w[0, 0] == 0 and v[0, 0] is None and not np.isnan(src[4, 4])
    got = onp.reproject(src, np.nan, mapping, (1, 1), dst_nodata=np.nan, resampling='cubic')
    assert np.isnan(got[0, 0])
    src[3, 3] = np.float32(1.5)         # t = (0, 0), weight 111 * 111
    v, _, w = rx.exact(src, np.nan, mapping, (1, 1), 'cubic')
    assert w[0, 0] == Fr(12321, 16384) and v[0, 0] is not None
    res = rx.enclosure_failures(onp.reproject(src, np.nan, mapping, (1, 1), dst_nodata=np.nan, resampling='cubic'), src, np.nan,
                                mapping, (1, 1), 'cubic')
    assert not res['pattern'] and not res['value']


def test_the_footprint_methods_on_hand_worked_pixels():
    src = np.arange(1, 13, dtype=np.float32).reshape(3, 4)   # rows 1..4, 5..8, 9..12
    src[1, 2] = np.nan
    # partial shares: footprint rows [0.5, 2], columns [1.5, 3] -> shares (1/2, 1) x (1/2, 1) over 2, 3 / 6, nodata
    part = (1.5, 1.5, 1.5, .5)
    v, a, w = rx.exact(src, np.nan, part, (1, 1), 'sum')
    assert w[0, 0] == Fr(5, 4) and v[0, 0] == Fr(1, 4) * 2 + Fr(1, 2) * 3 + Fr(1, 2) * 6 == 5 and a[0, 0] == 5
    v, _, _ = rx.exact(src, np.nan, part, (1, 1), 'rms')     # the SQUARE: (4/4 + 9/2 + 36/2) / (5/4)
    assert v[0, 0] == (Fr(1, 4) * 4 + Fr(1, 2) * 9 + Fr(1, 2) * 36) / Fr(5, 4) == Fr(94, 5)
    assert [rx.exact(src, np.nan, part, (1, 1), m)[0][0, 0] for m in ('max', 'min', 'med', 'q1', 'q3')] == [6, 2, 3, 2, 6]
    # a footprint inside ONE source pixel: 2x up-sampling, destination (0, 1) covers rows [0, 0.5], columns [0.5, 1] of pixel
    # (0, 0) = 1: it weighs 1, not its share 1/4
    v, a, w = rx.exact(src, np.nan, (.5, 0., .5, 0.), (6, 8), 'sum')
    assert v[0, 1] == 1 and w[0, 1] == 1 and v[5, 7] == 12 and v[2, 5] is None
    assert rx.exact(src, np.nan, (.5, 0., .5, 0.), (6, 8), 'rms')[0][5, 7] == 144
    # one axis inside a single pixel (row 0 alone: weight 1), the other with shares 1/2, 1 over columns 1, 2: 2/2 + 3
    v, _, w = rx.exact(src, np.nan, (1.5, 1.5, .5, 0.), (1, 1), 'sum')
    assert v[0, 0] == 4 and w[0, 0] == Fr(3, 2)
    # mode: in row-major order 5, 7, 7, 5 -- 7 is the first to reach two; 5 occurs first and last, and is the smaller
    tie = np.array([[5, 7], [7, 5]], np.float32)
    assert rx.exact(tie, np.nan, (2., 0., 2., 0.), (1, 1), 'mode')[0][0, 0] == 7
    assert onp.reproject(tie, np.nan, (2., 0., 2., 0.), (1, 1), resampling='mode')[0, 0] == 7
    # ... and 7, 5, 5, 7: 5 reaches two first, 7 occurs last and is the larger
    assert rx.exact(np.array([[7, 5], [5, 7]], np.float32), np.nan, (2., 0., 2., 0.), (1, 1), 'mode')[0][0, 0] == 5
    # all different: the first
    assert rx.exact(np.array([[3, 9], [1, 4]], np.float32), np.nan, (2., 0., 2., 0.), (1, 1), 'mode')[0][0, 0] == 3
    # the quantiles: element max(0, ceil(q n - 1)) of the sorted values
    #   n = 1: 0, 0, 0;  n = 2: med ceil(0) = 0, q1 ceil(-1/2) = 0, q3 ceil(1/2) = 1;  n = 4: 1, 0, 2;  n = 5: ceil(3/2) = 2, ceil(1/4) = 1, ceil(11/4) = 3
    for row, exp in (([7], (7, 7, 7)), ([4, 2], (2, 2, 4)), ([8, 1, 6, 3], (3, 1, 6)), ([9, 2, 7, 4, 5], (5, 4, 7))):
        one = np.array([row], np.float32)
        got = tuple(rx.exact(one, np.nan, (float(len(row)), 0., 1., 0.), (1, 1), m)[0][0, 0] for m in ('med', 'q1', 'q3'))
        assert got == exp, (row, got)
        for m, e in zip(('med', 'q1', 'q3'), exp):
            assert onp.reproject(one, np.nan, (float(len(row)), 0., 1., 0.), (1, 1), resampling=m)[0, 0] == e
    # nearest: the pixel under the centre; destination (0, 1) of a 1.5:1 grid has its centre at (0.75, 2.25) -> (0, 2) = 3
    v, _, _ = rx.exact(src, np.nan, (1.5, 0., 1.5, 0.), (2, 3), 'nearest')
    assert v[0, 1] == 3 and v[1, 1] == 11 and v[1, 2] == 12
    # ... a nodata pixel under the centre and a centre outside the plane give nodata
    v, _, _ = rx.exact(src, np.nan, (1., 0., 1., 0.), (4, 5), 'nearest')
    assert v[1, 2] is None and v[1, 1] == 6 and v[3, 0] is None and v[0, 4] is None


def _hold_res(res, what, n_min):
    rx.assert_held(res, f'oracle {what}', n_min)


def _hold_all(method, mapping, dst_shape, nodata, src):
    got = onp.reproject(src, nodata, mapping, dst_shape, dst_nodata=np.nan, resampling=method)
    _hold_res(rx.enclosure_failures(got, src, nodata, mapping, dst_shape, method), f'{method} {mapping}',
              0.4 * dst_shape[0] * dst_shape[1])


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.UP_CASES)
@pytest.mark.parametrize('method', ['nearest', 'cubic', 'lanczos'])
def test_oracle_point_methods_on_the_upsampling_cases(method, mapping, dst_shape, nodata):
    _hold_all(method, mapping, dst_shape, nodata, rx.source((13, 21), nodata))


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.STRETCH_CASES)
@pytest.mark.parametrize('method', ['bilinear', 'cubic', 'cubic_spline', 'lanczos'])
def test_oracle_convolution_form_inside_the_exact_enclosure(method, mapping, dst_shape, nodata):
    assert rx.uses_conv(method, mapping[0], mapping[2]) == (method in ('cubic', 'lanczos') or max(mapping[0], mapping[2]) > 1)
    _hold_all(method, mapping, dst_shape, nodata, rx.source((13, 21), nodata))


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.DOWN_CASES)
@pytest.mark.parametrize('method', ['bilinear', 'cubic', 'cubic_spline', 'lanczos'])
def test_oracle_convolution_form_on_the_downsampling_cases(method, mapping, dst_shape, nodata):
    """ up to 4 source pixels per pixel on an axis, destinations that start and end outside the plane """
    assert rx.uses_conv(method, mapping[0], mapping[2])
    _hold_all(method, mapping, dst_shape, nodata, rx.source(rx.AVG_SHAPE, nodata))


def test_every_method_has_its_cases():
    for method in rx.ALL_METHODS:
        cases = rx.scaled_cases(method)
        assert len(cases) >= 4
        assert (method in rx.CONV_R) == all((m, s) in [(m, s) for m, s, _ in cases] for m, s in rx.STRETCH_CASES)


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.DOWN_CASES + (rx.UP_FOOT_CASE,))
@pytest.mark.parametrize('method', ['nearest', 'max', 'min', 'sum', 'rms', 'mode', 'med', 'q1', 'q3', 'average'])
def test_oracle_footprint_methods_on_a_source_with_ties(method, mapping, dst_shape, nodata):
    _hold_all(method, mapping, dst_shape, nodata, rx.source_with_ties(rx.AVG_SHAPE, nodata))


def turned_planes(src_shape, dst_shape, degrees, k):
    """ the source coordinates of a destination grid turned by `degrees` about the source's centre, k source pixels per pixel: the
    cosine and sine are whatever doubles they are, so no coordinate is dyadic """
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    v, u = np.mgrid[0:dst_shape[0], 0:dst_shape[1]].astype(np.float64)
    u, v = u + 0.5 - dst_shape[1] / 2, v + 0.5 - dst_shape[0] / 2
    return src_shape[1] / 2 + k * (c * u - s * v), src_shape[0] / 2 + k * (s * u + c * v)


WARP_SRC = (24, 36)
WARP_CASES = {'turn30': ((30, 44), 30., 1.), 'turn30-down3': ((12, 16), 30., 3.), 'turn15-up': ((40, 50), 15., .4)}


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('method', rx.POINT_METHODS)
@pytest.mark.parametrize('case', list(WARP_CASES))
def test_warp_restatement_inside_the_exact_enclosure(case, method, nodata):
    dst_shape, degrees, k = WARP_CASES[case]
    src, _ = onp.synth_pair(*WARP_SRC, 14, 'frame+holes')
    if not np.isnan(nodata):
        src[np.isnan(src)] = nodata
    sx, sy = turned_planes(WARP_SRC, dst_shape, degrees, k)
    got = wr.warp_resample(src, nodata, sx, sy, k, k, dst_nodata=np.nan, resampling=method)
    inside = (sx >= 0) & (sx < WARP_SRC[1]) & (sy >= 0) & (sy < WARP_SRC[0])
    assert (~inside).any() == (case != 'turn15-up')      # the two coarser grids overhang the source on all sides
    _hold_res(rx.enclosure_failures_at(got, src, nodata, sx, sy, k, k, method), f'{case} {method}', 0.3 * inside.sum())


def _hold(method, mapping, dst_shape, nodata, src_shape):
    src = rx.source(src_shape, nodata)
    got = onp.reproject(src, nodata, mapping, dst_shape, dst_nodata=np.nan, resampling=method)
    res = rx.enclosure_failures(got, src, nodata, mapping, dst_shape, method)
    print(f'{method} {mapping}: {res["n_valid"]} valued pixels, worst error {res["worst"]:.3f} of the bound, '
          f'{len(res["pattern"])} pattern and {len(res["value"])} value failures')
    assert not res['pattern'], f'{method} {mapping}: nodata pattern departs from the rule at {res["pattern"][:5]}'
    assert not res['value'], f'{method} {mapping}: outside the enclosure at {res["value"][:5]}'
    assert res['n_valid'] > 0.4 * dst_shape[0] * dst_shape[1]


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.UP_CASES)
@pytest.mark.parametrize('method', ['bilinear', 'cubic_spline'])
def test_oracle_upsamplers_inside_the_exact_enclosure(method, mapping, dst_shape, nodata):
    _hold(method, mapping, dst_shape, nodata, (13, 21))


@pytest.mark.parametrize('nodata', [np.nan, -9999.])
@pytest.mark.parametrize('mapping, dst_shape', rx.DOWN_CASES)
def test_oracle_average_inside_the_exact_enclosure(mapping, dst_shape, nodata):
    _hold('average', mapping, dst_shape, nodata, rx.AVG_SHAPE)
