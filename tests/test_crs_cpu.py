""" CRS definitions and the host (float64 numpy) coordinate transformation, homonim_amd/crs.py: label parsing, equality by
definition, what unknown CRSs raise, and ``crs.transform_coords`` against a 40-digit mpmath evaluation of the same definitions
(tests/_crs_mp.py).

The bar on coordinates is 1e-6 m (geographic output: 1e-6 m over 6.4e6 m, in radians).  Float64 numpy measures 4.1e-9 m forward
and 2.1e-9 m inverse on this domain -- about 2 ulp of a 1e7 m coordinate; the bar is about 250 times that and 2e-7 of the smallest
pixel of the fixtures (5 m). """
import math

import numpy as np
import pytest

import _crs_mp
from homonim_amd import CRS, crs
from homonim_amd.geo import Affine, suggested_warp_grid

TM25_LABEL = ('unnamed [1024=1; 1025=1; 2048=4326; 2054=9102; 2057=6378137.0; 2059=298.257223563; 3072=32767; 3074=32767; '
              '3075=1; 3076=9001; 3080=25.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]')   # the reference's test rasters
TM25, UTM35S, WGS84 = CRS(TM25_LABEL), CRS('EPSG:32735'), CRS('EPSG:4326')
UTM35S_KEYS = CRS('UTM 35S [1024=1; 1025=1; 2048=4326; 2054=9102; 2057=6378137.0; 2059=298.257223563; 3072=32767; 3075=1; '
                  '3076=9001; 3080=27.0; 3081=0.0; 3082=500000.0; 3083=10000000.0; 3092=0.9996]')
AIRY_TM = CRS('OSGB [1024=1; 2057=6377563.396; 2059=299.3249646; 3075=1; 3080=-2.0; 3081=49.0; 3082=400000.0; 3083=-100000.0; '
              '3092=0.9996012717]')
AIRY_GEO = CRS('Airy [1024=2; 2054=9102; 2057=6377563.396; 2059=299.3249646]')
BAR_M = 1e-6
BAR_DEG = math.degrees(1e-6 / 6.4e6)


def test_the_three_label_families_parse():
    assert crs.parse(WGS84) == crs.CrsDef(crs.GEOGRAPHIC, 6378137.0, 298.257223563)
    assert crs.parse('epsg:4326') == crs.parse(WGS84)
    assert crs.parse(UTM35S) == crs.CrsDef(crs.TMERC, 6378137.0, 298.257223563, 0., 27., 0.9996, 500000., 10000000.)
    assert crs.parse(CRS('EPSG:32601')) == crs.CrsDef(crs.TMERC, 6378137.0, 298.257223563, 0., -177., 0.9996, 500000., 0.)
    assert crs.parse(CRS('EPSG:32660')).lon0 == 177.
    assert crs.parse(TM25) == crs.CrsDef(crs.TMERC, 6378137.0, 298.257223563, 0., 25., 1., 0., 0.)
    assert crs.parse(AIRY_TM) == crs.CrsDef(crs.TMERC, 6377563.396, 299.3249646, 49., -2., 0.9996012717, 400000., -100000.)
    assert crs.parse(AIRY_GEO) == crs.CrsDef(crs.GEOGRAPHIC, 6377563.396, 299.3249646)
    # a geographic key list that names EPSG:4326 and no ellipsoid is on WGS84
    assert crs.parse(CRS('[1024=2; 2048=4326]')) == crs.parse(WGS84)


def test_the_labels_tiff_py_reads_from_the_fixture_rasters_parse():
    import os

    from conftest import REPO
    from homonim_amd.tiff import read_tiff_header
    for name in ('ngi_rgb_byte_1.tif', 'landsat8_byte.tif', 'sentinel2_b432_byte.tif'):
        header = read_tiff_header(os.path.join(REPO, 'tests', 'golden', 'rasters', name))
        assert header.crs.to_string() == TM25_LABEL
        assert crs.parse(header.crs) == crs.parse(TM25)


def test_equal_definitions_are_the_same_crs():
    assert crs.same_crs(UTM35S, UTM35S_KEYS) and crs.same_crs(UTM35S_KEYS, UTM35S)
    assert UTM35S != UTM35S_KEYS                      # geo.CRS keeps its label
    assert not crs.same_crs(UTM35S, CRS('EPSG:32635')) and not crs.same_crs(UTM35S, TM25)
    assert crs.same_crs(CRS('anything at all'), CRS('Anything At All'))   # unknown CRSs: by label, as geo.CRS compares
    x, y = crs.transform_coords(UTM35S, UTM35S_KEYS, [254000.], [6278000.])
    assert x[0] == 254000. and y[0] == 6278000.


@pytest.mark.parametrize('label', [
    'EPSG:3857', 'EPSG:32661', 'EPSG:32700', 'EPSG:4269', 'WGS 84 / Pseudo-Mercator', '',
    'x [1024=1; 2048=4326; 3075=7; 3080=25.0]',                                      # another projection method
    'x [1024=1; 2048=4326; 3075=1; 3076=9002; 3080=25.0]',                            # feet
    'x [1024=1; 2048=4326; 3075=1; 3080=25.0; 3088=12.0]',                            # a key the definition does not cover
    'x [1024=1; 2057=6378137.0; 3075=1; 3080=25.0]',                                  # half an ellipsoid
    'x [1024=1; 2048=4267; 3075=1; 3080=25.0]',                                       # a datum named by code only
])
def test_unknown_labels(label):
    assert crs.parse(CRS(label) if label else label) is None
    other = CRS(label or 'nameless')
    with pytest.raises(NotImplementedError) as ex:
        crs.transform_coords(other, UTM35S, [0.], [0.])
    assert other.to_string() in str(ex.value)
    with pytest.raises(NotImplementedError) as ex:
        crs.transform_coords(UTM35S, other, [0.], [0.])
    assert other.to_string() in str(ex.value)
    x, y = np.array([1., 2.]), np.array([3., 4.])
    with pytest.raises(NotImplementedError):          # even onto itself: there is nothing to transform with
        crs.transform_coords(other, other, x, y)


def test_different_ellipsoids_raise():
    with pytest.raises(NotImplementedError, match='ellipsoid'):
        crs.transform_coords(AIRY_TM, UTM35S, [400000.], [100000.])
    with pytest.raises(NotImplementedError, match='ellipsoid'):
        crs.definitions(WGS84, AIRY_GEO)


def _points(seed, lon0):
    rng = np.random.default_rng(seed)
    return lon0 + rng.uniform(-8., 8., 3000), rng.uniform(-84., 84., 3000)


@pytest.mark.parametrize('src, dst, lon0', [(TM25, UTM35S, 26.), (UTM35S, TM25, 26.), (UTM35S, WGS84, 27.), (WGS84, UTM35S, 27.)],
                         ids=['tm25-utm35s', 'utm35s-tm25', 'utm35s-wgs84', 'wgs84-utm35s'])
def test_transform_coords_against_mpmath(src, dst, lon0):
    """ 3000 seeded points, latitude in [-84, 84], longitude within 8 degrees of the central meridian(s) (lon0 = 26 keeps a point
    within 9 degrees of both 25 and 27): the float64 result against the 40-digit one, below 1e-6 m. """
    lon, lat = _points(11, lon0)
    s_def, d_def = crs.parse(src), crs.parse(dst)
    if s_def.is_geographic:
        xs, ys = lon, lat
    else:   # the inputs are float64 coordinates of the source CRS; the reference transforms exactly these
        xs, ys = crs.transform_coords(WGS84, src, lon, lat)
    got_x, got_y = crs.transform_coords(src, dst, xs, ys)
    exact = _crs_mp.transform_many(tuple(s_def), tuple(d_def), xs, ys)
    if d_def.is_geographic:
        err = _crs_mp.max_error(got_x, got_y, exact)
        print(f'{src!r} -> {dst!r}: largest error {err:.3e} degrees = {math.radians(err) * 6.4e6:.3e} m')
        assert err < BAR_DEG
    else:
        err = _crs_mp.max_error(got_x, got_y, exact)
        print(f'{src!r} -> {dst!r}: largest error {err:.3e} m')
        assert err < BAR_M


def test_epsg_guidance_note_example():
    """ EPSG Guidance Note 7-2, Transverse Mercator example: Airy 1830, latitude of origin 49 N, central meridian 2 W, k0
    0.9996012717, FE 400000, FN -100000; 50 30' N 0 30' E -> E 577274.99, N 69740.50.  The published figures come from older
    formulae and differ from the n^6 series (577274.984, 69740.492) by 8 mm: within 0.02 m. """
    e, n = crs.transform_coords(AIRY_GEO, AIRY_TM, [0.5], [50.5])
    assert abs(e[0] - 577274.99) < 0.02 and abs(n[0] - 69740.50) < 0.02
    assert abs(e[0] - 577274.984) < 1e-3 and abs(n[0] - 69740.492) < 1e-3
    lon, lat = crs.transform_coords(AIRY_TM, AIRY_GEO, [577274.99], [69740.50])
    assert abs(lon[0] - 0.5) < 0.02 / 70000 and abs(lat[0] - 50.5) < 0.02 / 111000
    ex, ey = _crs_mp.transform(tuple(crs.parse(AIRY_GEO)), tuple(crs.parse(AIRY_TM)), 0.5, 50.5)
    assert abs(float(ex) - 577274.99) < 0.02 and abs(float(ey) - 69740.50) < 0.02


def test_utm_identities():
    for zone in (1, 31, 35, 60):
        lon0 = 6. * zone - 183.
        e, n = crs.transform_coords(WGS84, CRS(f'EPSG:326{zone:02d}'), [lon0], [0.])
        assert (e[0], n[0]) == (500000., 0.)
        e, n = crs.transform_coords(WGS84, CRS(f'EPSG:327{zone:02d}'), [lon0], [0.])
        assert (e[0], n[0]) == (500000., 10000000.)
    # northing along the central meridian is k0 times the meridian arc: a quarter meridian of WGS84 is 10 001 965.729 m
    e, n = crs.transform_coords(WGS84, CRS('EPSG:32631'), [3.], [90.])
    assert abs(e[0] - 500000.) < 1e-6 and abs(n[0] - 0.9996 * 10001965.729) < 2e-3


def test_round_trip():
    lon, lat = _points(12, 26.)
    for a, b in ((TM25, UTM35S), (UTM35S, WGS84)):
        xs, ys = crs.transform_coords(WGS84, a, lon, lat)
        bx, by = crs.transform_coords(a, b, xs, ys)
        rx, ry = crs.transform_coords(b, a, bx, by)
        assert np.max(np.abs(rx - xs)) < 1e-8 and np.max(np.abs(ry - ys)) < 1e-8


def test_geographic_conventions():
    # longitude differences wrap to (-180, 180]: 183 W is 177 E, the central meridian of zone 60
    e, _ = crs.transform_coords(WGS84, CRS('EPSG:32660'), [-183., 177.], [10., 10.])
    assert e[0] == e[1] == 500000.
    lon, _ = crs.transform_coords(CRS('EPSG:32660'), WGS84, [900000.], [1000000.])
    assert -180. < lon[0] <= 180. and lon[0] < -177.     # east of the antimeridian
    # beyond the poles, and 90 degrees or more from the central meridian: no data
    e, n = crs.transform_coords(WGS84, UTM35S, [27., 27., 118.], [90.5, -91., 0.])
    assert np.isnan(e).all() and np.isnan(n).all()


def test_suggested_warp_grid_onto_the_rasters_own_crs_is_its_own_grid():
    tf, shape = Affine(5.0, 0., -57129.44916219164, 0., -5.0, -3723906.806172144), (1421, 805)
    got_tf, got_shape = suggested_warp_grid(TM25, tf, shape, TM25)
    assert got_shape == shape
    for got, exp in zip((got_tf.a, got_tf.c, got_tf.e, got_tf.f), (tf.a, tf.c, tf.e, tf.f)):
        assert abs(got - exp) <= 1e-9 * abs(exp)
    assert got_tf.b == 0 and got_tf.d == 0
    got_tf, got_shape = suggested_warp_grid(UTM35S, Affine(30., 0., 250000., 0., -30., 6280000.), (454, 267), UTM35S_KEYS)
    assert got_shape == (454, 267) and abs(got_tf.a - 30.) < 3e-8 and abs(got_tf.c - 250000.) < 2.5e-4


def test_suggested_warp_grid_between_crss():
    """ north-up, square pixels of about the source's size, and an extent that holds every transformed outline point """
    tf, shape = Affine(30., 0., -60390., 0., -30., -3722700.), (454, 267)
    got_tf, (h, w) = suggested_warp_grid(TM25, tf, shape, UTM35S)
    assert got_tf.a == -got_tf.e > 0 and got_tf.b == got_tf.d == 0
    assert abs(got_tf.a / 30. - 1.) < 1e-3                # k0 0.9996 against 1, two degrees from the central meridian
    cols, rows = np.array([0., 267., 267., 0.]), np.array([0., 0., 454., 454.])
    xs, ys = crs.transform_coords(TM25, UTM35S, tf.c + cols * tf.a, tf.f + rows * tf.e)
    assert got_tf.c <= xs.min() and got_tf.f >= ys.max()
    assert got_tf.c + (w + 0.5) * got_tf.a >= xs.max() and got_tf.f + (h + 0.5) * got_tf.e <= ys.min()


def test_models_and_footprint_modes_refuse_two_crss_by_name():
    """ (no device needed: the refusals come before any device call) """
    from homonim_amd import Model, RasterArray, RefSpaceModel, SrcSpaceModel
    a = RasterArray(np.ones((8, 8), np.float32), TM25, Affine(30., 0., -60390., 0., -30., -3722700.))
    b = RasterArray(np.ones((8, 8), np.float32), UTM35S, Affine(30., 0., 254000., 0., -30., 6278000.))
    for model in (RefSpaceModel(Model.gain, (3, 3)), SrcSpaceModel(Model.gain, (3, 3))):
        with pytest.raises(NotImplementedError, match=r'reproject\(crs='):
            model.fit(a, b)
    with pytest.raises(NotImplementedError, match=r'reproject\(crs='):
        RefSpaceModel(Model.gain, (3, 3)).fit_apply(a, b)
    with pytest.raises(NotImplementedError, match='average'):
        a.reproject(crs=UTM35S, resampling='average')
    with pytest.raises(NotImplementedError, match='EPSG:3857'):
        a.reproject(crs=CRS('EPSG:3857'), resampling='bilinear')
