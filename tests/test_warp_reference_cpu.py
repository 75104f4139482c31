""" tests/_warp_reference.py -- the numpy restatement of the warp re-samplers on per-pixel coordinate planes -- pinned to the
existing oracle: on planes built as ``kx * (j + .5) + ox`` it must equal ``oracle_np.reproject`` bit for bit.  Every mapping and
shape ``test_more_device_resamplers_equal_oracle`` (tests/test_gpu_parity.py) uses for these methods, nodata None, NaN and a
number.  Lanczos included: both sides use the host's ``sin``. """
import numpy as np
import pytest

import _warp_reference as wr
from conftest import assert_same_f32
from oracle import oracle_np as onp

CASES = [
    ('bilinear', (2.2, 0.3, 1.9, -0.4), (40, 55)), ('cubic_spline', (3.0, 0., 3.0, 0.), (27, 40)),
    ('cubic', (.45, -.5, .45, -.5), (180, 270)), ('cubic', (2.5, 0.2, 2.5, 0.1), (30, 45)), ('cubic', (1., 0., 1., 0.), (80, 120)),
    ('lanczos', (.5, 0., .5, 0.), (160, 240)), ('lanczos', (2.0, 0., 2.0, 0.), (40, 60)),
    ('bilinear', (1.5, 0., .5, 0.), (160, 80)),
    # the up-sampling builds of bilinear / cubic_spline and nearest (tests/test_gpu_parity.py covers them elsewhere); grids that
    # overhang the source
    ('bilinear', (.45, -.5, .45, -.5), (180, 270)), ('cubic_spline', (.3, -2., .35, -1.5), (250, 420)),
    ('nearest', (2.2, 0.3, 1.9, -0.4), (40, 55)), ('nearest', (.45, -.5, .45, -.5), (180, 270)),
]


@pytest.mark.parametrize('resampling, mapping, dst_shape', CASES)
@pytest.mark.parametrize('nodata', [None, np.nan, -9999.], ids=['none', 'nan', 'number'])
def test_restatement_equals_the_oracle_on_affine_planes(resampling, mapping, dst_shape, nodata):
    src, _ = onp.synth_pair(80, 120, 14, 'frame+holes' if nodata is not None else 'none')
    if nodata is not None and not np.isnan(nodata):
        src[np.isnan(src)] = nodata
    sx, sy = wr.affine_planes(mapping, dst_shape)
    for dst_nodata in (np.nan, None):
        got = wr.warp_resample(src, nodata, sx, sy, mapping[0], mapping[2], dst_nodata=dst_nodata, resampling=resampling)
        exp = onp.reproject(src, nodata, mapping, dst_shape, dst_nodata=dst_nodata, resampling=resampling)
        assert_same_f32(got, exp, f'{resampling} {mapping} nodata {nodata} -> {dst_nodata}')
    assert np.isfinite(exp[exp == exp]).all()


def test_unusable_coordinates_are_no_data():
    src, _ = onp.synth_pair(20, 30, 3, 'none')
    sx, sy = wr.affine_planes((1., 0., 1., 0.), (20, 30))
    sx[2, 3], sy[4, 5], sx[6, 7], sy[8, 9] = np.nan, np.inf, -1e300, 1e15
    for resampling in wr.MODES:
        out = wr.warp_resample(src, None, sx, sy, 1., 1., dst_nodata=-1., resampling=resampling)
        assert out[2, 3] == out[4, 5] == out[6, 7] == out[8, 9] == -1.
        assert (out != -1.).sum() == out.size - 4
    with pytest.raises(NotImplementedError):
        wr.warp_resample(src, None, sx, sy, 1., 1., resampling='average')
