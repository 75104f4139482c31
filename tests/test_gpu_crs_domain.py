""" warp_coord() of hk_warp.hip over the domain families of tests/_crs_domain.py -- both hemispheres and the equator, zones 1 and 60
and the antimeridian, 84 degrees to the poles and beyond, 6 to 90 degrees from the central meridian, Airy / a sphere / a latitude
of origin at a pole, rotated grids -- through ``Context.warp_coords`` and ``Context.warp_coords_affine``:

* the device's source pixel coordinates against the 40-digit reference in ground metres, below the bar the family module derives
  from the HOST statement's measured error (1e-6 m everywhere but at the one place outside the series' useful range);
* NaN in both planes exactly where the contract gives it, position for position, and exactly where the host statement has it;
* on two families (rows beyond the pole; rows that cross 90 degrees from the central meridian) ``Context.reproject_crs`` under nearest
  and bilinear: the fill value exactly where the device's own planes are NaN or outside the source, the numpy restatement
  (tests/_warp_reference.py) on those planes bit for bit elsewhere, and at least a third of the positions with an image inside.

The reference is computed once per process (``_crs_domain.reference``) and shared by every test here. """
import numpy as np
import pytest

import _crs_domain as dom
import _warp_reference as wr
from conftest import assert_same_f32
from homonim_amd import CRS, _hk, crs
from homonim_amd.geo import is_rotated
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

SENTINEL = 0x5A
FILL = -9999.


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


@pytest.fixture(scope='module')
def reference():
    return dom.reference()


def _descriptor(case):
    """ the case as the package hands it to the device: hk_affine_warp_desc for rotated / sheared grids, hk_warp_desc otherwise """
    s, d = dom.definition(case.src), dom.definition(case.dst)
    if is_rotated(case.dst_tf) or is_rotated(case.src_tf):
        return _hk.make_affine_warp_desc(s, case.src_tf, d, case.dst_tf), True
    return _hk.make_warp_desc(s, case.src_tf, d, case.dst_tf), False


def _coords_padded(ctx, case, shape, offset, pad=5):
    """ the device's coordinate planes, written into planes with spare pitch; the slack must come back untouched """
    warp, affine = _descriptor(case)
    h, w = shape
    stores = [np.empty((h, w + pad), np.float64) for _ in range(2)]
    for s in stores:
        s.view(np.uint8)[...] = SENTINEL
    entry = ctx.warp_coords_affine if affine else ctx.warp_coords
    x, y = entry(warp, shape, (offset, offset), out=(stores[0][:, :w], stores[1][:, :w]))
    for s in stores:
        assert (s[:, w:].view(np.uint8) == SENTINEL).all(), 'a coordinate plane was written outside its width'
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


@pytest.mark.parametrize('family', dom.FAMILIES)
def test_warp_coords_over_the_domain(ctx, reference, family):
    """ per case of the family, centres and (where the case asks) corners: NaN where the rule gives it and where the host statement
    has it, in both planes; finite elsewhere; the error against the reference below the case's bar """
    worst_of_family = 0.
    for case in (c for c in dom.cases() if c.family == family):
        assert is_rotated(case.dst_tf) == (family == 'rotated')
        worst = 0.
        for what, shape, off in dom.lattices(case):
            gx, gy = _coords_padded(ctx, case, shape, off)
            bad = dom.expected_nan(case, what, shape, off)
            assert np.array_equal(np.isnan(gx), bad) and np.array_equal(np.isnan(gy), bad), f'{case.name} {what}: NaN pattern'
            hx, hy = crs.transform_coords(CRS(case.dst), CRS(case.src), *dom.positions(case, shape, off))
            assert np.array_equal(np.isnan(hx), np.isnan(gx)) and np.array_equal(np.isnan(hy), np.isnan(gy)), \
                f'{case.name} {what}: device and host statement disagree on what has no image'
            assert np.isfinite(gx[~bad]).all() and np.isfinite(gy[~bad]).all(), f'{case.name} {what}'
            worst = max(worst, dom.ground_error(case, what, gx, gy, bad, pixels=True))
        bar = dom.bar_of(case)
        print(f'[crs domain, device] {family} {case.name}: largest error {worst:.3e} m (host statement {case.host:.3e} m, '
              f'bar {bar:.3e} m)')
        assert worst < bar, f'{case.name}: {worst} m against {bar} m'
        if bar == dom.BAR_M:
            worst_of_family = max(worst_of_family, worst)
    print(f'[crs domain, device] {family}: largest error {worst_of_family:.3e} m over the cases held to {dom.BAR_M:.0e} m')


def test_the_far_side_of_a_source_that_ends_at_180(ctx, reference):
    """ 'utm60-180->wgs84-ending-at-180': positions beyond the antimeridian are longitude -180 + d, a column 360 / step to the left
    of the plane -- finite, far outside, not NaN -- and the positions short of it lie inside the plane """
    c = dom.case('utm60-180->wgs84-ending-at-180')
    col, row = _coords_padded(ctx, c, c.shape, 0.5)
    exact_lon = np.array([float(p[0]) for p in reference[(c.name, 'centres')][0]]).reshape(c.shape)
    far = exact_lon < 0
    assert far.any() and (~far).any() and np.isfinite(col).all() and np.isfinite(row).all()
    assert (np.abs(col[far] - dom.FAR_SIDE_COLUMN) < 2 * dom.SRC_SHAPE[1]).all()
    assert ((col[~far] > 0) & (col[~far] < dom.SRC_SHAPE[1])).all()


@pytest.fixture(scope='module')
def small_source():
    """ 24 x 36, positive, no nodata: a destination pixel is then the fill value for its coordinate's sake alone """
    a, _ = onp.synth_pair(*dom.SRC_SHAPE, 14, 'none')
    assert a.shape == dom.SRC_SHAPE and np.isfinite(a).all() and (a > 0).all()
    return a


@pytest.mark.parametrize('resampling', ['nearest', 'bilinear'])
@pytest.mark.parametrize('name', dom.RESAMPLED)
def test_resamplers_where_part_of_the_grid_has_no_image(ctx, small_source, name, resampling):
    """ the fill value exactly where the device's own coordinate planes are NaN or outside the source plane; the restatement on
    those planes, bit for bit, elsewhere; and not trivially all fill: at least a third of the positions with an image lie inside """
    case = dom.case(name)
    warp, affine = _descriptor(case)
    assert not affine
    scale = dom.tap_scale(case)        # <= 1 on both axes: the tap form, warp_kernel<0 / 1, WARP_AXIS>
    got = ctx.reproject_crs(small_source, None, warp, scale, case.shape, onp.RESAMPLING_CODES[resampling], FILL)
    sx, sy = ctx.warp_coords(warp, case.shape)
    no_image = np.isnan(sx)
    assert np.array_equal(no_image, np.isnan(sy)) and no_image.any() and not no_image.all()
    assert np.array_equal(no_image, dom.expected_nan(case, 'centres', case.shape, 0.5))
    with np.errstate(invalid='ignore'):
        cx, cy = np.floor(sx + 1e-10), np.floor(sy + 1e-10)       # the source pixel under the centre, as rs_centre takes it
        inside = ~no_image & (cx >= 0) & (cx < dom.SRC_SHAPE[1]) & (cy >= 0) & (cy < dom.SRC_SHAPE[0])
    assert np.array_equal(got == np.float32(FILL), ~inside), f'{name} {resampling}: the fill value is not where the planes say'
    assert (~inside & ~no_image).any(), 'the case is meant to have positions with an image outside the plane as well'
    assert 3 * inside.sum() >= (~no_image).sum()
    exp = wr.warp_resample(small_source, None, sx, sy, scale[0], scale[1], dst_nodata=FILL, resampling=resampling)
    assert_same_f32(got, exp, f'{name} {resampling}')
    # and the values are the source's, from many of its pixels (the 13 positions on the pole share one)
    under = small_source[cy[inside].astype(int), cx[inside].astype(int)]
    assert len(np.unique(under)) >= 10
    if resampling == 'nearest':
        assert np.array_equal(got[inside], under)
