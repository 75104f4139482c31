""" oracle_np.reproject held to the exact statement of tests/_resample_exact.py: identical nodata pattern and every pixel inside
``1/2 ulp32 + 2^-40 A`` of the exact value, for bilinear and cubic_spline (up-sampling) and average (down-sampling), NaN and numeric
nodata.  The device kernels are held bit for bit to this oracle elsewhere, and to the same statement directly in
tests/test_gpu_resample_exact.py; the statement itself is checked here against hand-worked pixels. """
from fractions import Fraction as Fr

import numpy as np
import pytest

import _resample_exact as rx
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
