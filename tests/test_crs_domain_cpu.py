""" The host statement of the CRS transformation (``crs.transform_coords``, float64 numpy) over the domain families of
tests/_crs_domain.py: its error against the 40-digit reference in ground metres, and the exact NaN pattern of the contract, position
for position.  Every definition of the families can be written as a label ``crs.parse`` reads (3081 = +-90 included), so every case
goes through ``transform_coords`` and none needs ``crs._TM`` directly.

This is also where the figures of ``_crs_domain.HOST_M`` come from: the test prints the host error and the bar of every case. """
import numpy as np
import pytest

import _crs_domain as dom
from homonim_amd import CRS, crs


def _host(case, shape, offset):
    X, Y = dom.positions(case, shape, offset)
    return crs.transform_coords(CRS(case.dst), CRS(case.src), X, Y)


def test_the_module_stays_within_its_budget():
    points = sum(shape[0] * shape[1] for c in dom.cases() for _, shape, _ in dom.lattices(c))
    assert points < 4000
    assert {c.family for c in dom.cases()} == set(dom.FAMILIES)
    assert all(c.shape[0] <= 9 and c.shape[1] <= 13 for c in dom.cases())
    # every bar is the project's, or four times a host figure that is above it
    assert all(dom.bar_of(c) == (dom.BAR_M if c.host <= dom.BAR_M else 4 * c.host) for c in dom.cases())


@pytest.mark.parametrize('family', dom.FAMILIES)
def test_host_statement_over_the_domain(family):
    """ per case of the family: NaN exactly where the rule gives it and in both coordinates, finite elsewhere, and the error against
    the reference below the case's bar; the recorded host figure is what this measures (within the factor of the bar) """
    for case in (c for c in dom.cases() if c.family == family):
        worst = 0.
        for what, shape, off in dom.lattices(case):
            gx, gy = _host(case, shape, off)
            bad = dom.expected_nan(case, what, shape, off)
            if dom.definition(case.dst).is_geographic:      # the rule at 40 digits is the rule as the code forms it
                assert np.array_equal(bad, dom.float64_nan(case, shape, off)), f'{case.name} {what}: a position on the 90 degree line'
            assert np.array_equal(np.isnan(gx), bad) and np.array_equal(np.isnan(gy), bad), f'{case.name} {what}: NaN pattern'
            assert np.isfinite(gx[~bad]).all() and np.isfinite(gy[~bad]).all(), f'{case.name} {what}'
            worst = max(worst, dom.ground_error(case, what, gx, gy, bad, pixels=False))
        bar = dom.bar_of(case)
        print(f'[crs domain, host] {family} {case.name}: largest error {worst:.3e} m, recorded {case.host:.3e} m, bar {bar:.3e} m')
        assert worst < bar, f'{case.name}: {worst} m against {bar} m'
        assert worst <= dom.BAR_M or worst > case.host / 4, f'{case.name}: the recorded host figure {case.host} is stale ({worst})'


def test_the_lattices_reach_what_they_are_there_for():
    """ the design of the cases, from the reference: the equator, the antimeridian, the poles and the 90 degree line do lie where
    the case table says """
    ref = dom.reference()
    lat = lambda name: np.array([float(p[1]) for p in ref[(name, 'centres')][1]]).reshape(dom.case(name).shape)
    lon = lambda name: np.array([float(p[0]) for p in ref[(name, 'centres')][1]]).reshape(dom.case(name).shape)
    for name in ('utm35s-equator->utm35n', 'utm35n-equator->utm35s'):
        assert lat(name).min() < 0 < lat(name).max()
    assert dom.case('utm35s-equator->utm35n').dst_tf.f > 9e6 > 1e6 > dom.case('utm35n-equator->utm35s').dst_tf.f
    # longitudes either side of the antimeridian; the geographic lattice writes them above 180
    for name in ('utm01-180->utm60', 'utm60-180->utm01', 'utm60-180->wgs84-ending-at-180'):
        assert (lon(name) > 179.9).any() and (lon(name) < -179.9).any()
    X, _ = dom.positions(dom.case('wgs84-above-180->utm01'), dom.MAX_LATTICE, 0.5)
    assert X.min() < 179.91 and X.max() > 180.09
    # exactly 90 and beyond
    for name, rows in (('wgs84-top-row-90->utm33n', {0: 90.}), ('wgs84-row-beyond-90->utm33n', {0: 90.25, 1: 90.}),
                       ('wgs84-rows-to-beyond--90->utm33s', {3: -90., 4: -90.25})):
        c = dom.case(name)
        _, Y = dom.positions(c, c.shape, 0.5)
        for row, value in rows.items():
            assert (Y[row] == value).all()
    # the lattice near the pole holds it: latitudes above 89.9995 and longitudes on the far side, 180 degrees from lon0 = 15
    assert lat('utm33n-89.999n->wgs84').max() > 89.9995 and (np.abs(lon('utm33n-89.999n->wgs84')) > 150).any()
    # the row that crosses 90 degrees from lon0 = 15: finite to column 5 (89.8125 degrees), NaN from column 6 (90.0625) on
    c = dom.case('wgs84-crossing-90e->utm33n')
    bad = dom.expected_nan(c, 'centres', c.shape, 0.5)
    assert not bad[:, :6].any() and bad[:, 6:].all()
    X, _ = dom.positions(c, c.shape, 0.5)
    assert X[0, 5] - 15. == 89.8125 and X[0, 6] - 15. == 90.0625
    # the far cases are as far from lon0 = 15 as their names say
    for dist in (6., 30., 60., 89.9):
        for lat_ in (0., 45.):
            for name in (f'wgs84-{dist:g}e-{lat_:g}n->utm33n', f'utm33n-{dist:g}e-{lat_:g}n->wgs84'):
                if (dist, lat_) == (89.9, 0.) and name.startswith('utm33n'):
                    continue       # outside the series' range: the inverse of that grid is no longitude at all (see the case table)
                assert abs(lon(name) - 15. - dist).max() < 0.01 and abs(lat(name) - lat_).max() < 0.01, name
    # rotated lattices are rotated and their sources sheared
    for c in dom.cases():
        if c.family == 'rotated':
            assert c.dst_tf.b and c.dst_tf.d and c.src_tf.b and c.src_tf.d
            assert abs(np.degrees(np.arctan2(c.dst_tf.d, c.dst_tf.a)) - 30.) < 1e-9


def test_the_far_side_of_a_source_that_ends_at_180():
    """ 'utm60-180->wgs84-ending-at-180': the source grid's right edge is longitude 180.  A position beyond it has longitude -180 + d
    by ``_wrap180`` and the reference alike, so its column is 360 / step to the LEFT of the plane: finite and far outside, not NaN
    and not column 36 + d / step """
    c = dom.case('utm60-180->wgs84-ending-at-180')
    gx, gy = _host(c, c.shape, 0.5)
    exact_lon = np.array([float(p[0]) for p in dom.reference()[(c.name, 'centres')][0]]).reshape(c.shape)
    col = (gx - c.src_tf.c) / c.src_tf.a
    far = exact_lon < 0
    assert far.any() and (~far).any() and np.isfinite(col).all()
    assert (np.abs(col[far] - dom.FAR_SIDE_COLUMN) < 2 * dom.SRC_SHAPE[1]).all()
    assert ((col[~far] > 0) & (col[~far] < dom.SRC_SHAPE[1])).all()


def test_wrap180_at_its_edges():
    """ (-180, 180]: 180 stays, -180 and 540 become 180, and one ulp either side goes where it belongs """
    got = crs._wrap180(np.array([180., -180., 540., -540., np.nextafter(180., 181.), np.nextafter(-180., 0.), 0., 360., -360.]))
    assert got.tolist() == [180., 180., 180., 180., np.nextafter(-180., 0.), np.nextafter(-180., 0.), 0., 0., 0.]


@pytest.mark.parametrize('name', dom.RESAMPLED)
def test_the_resampling_cases_are_not_trivial(name):
    """ by the reference: part of the lattice has no image, of the rest some falls outside the 24 x 36 source and at least a third
    inside, and the steps are below one source pixel (the tap form of the re-samplers) """
    c = dom.case(name)
    kx, ky = dom.tap_scale(c)
    assert 0.3 < kx <= 1 and 0.3 < ky <= 1
    bad = dom.expected_nan(c, 'centres', c.shape, 0.5)
    exact, _ = dom.reference()[(name, 'centres')]
    col = (np.array([float(p[0]) for p in exact]).reshape(c.shape) - c.src_tf.c) / c.src_tf.a
    row = (np.array([float(p[1]) for p in exact]).reshape(c.shape) - c.src_tf.f) / c.src_tf.e
    inside = ~bad & (col >= 0) & (col < dom.SRC_SHAPE[1]) & (row >= 0) & (row < dom.SRC_SHAPE[0])
    assert bad.any() and (~bad & ~inside).any() and 3 * inside.sum() >= (~bad).sum()
