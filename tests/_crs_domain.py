""" Domain families for the CRS transformation (homonim_amd/crs.py on the host, warp_coord() of hk_warp.hip on the device): small
lattices at the places where a Transverse Mercator implementation goes wrong -- both hemispheres and the equator, zones 1 and 60
and the antimeridian, 84 degrees to the poles, 6 to 90 degrees from the central meridian, other ellipsoids and origins, rotated
grids -- each held to the 40-digit evaluation of the same definitions (tests/_crs_mp.py).  Pure Python, no GPU: tests/
test_crs_domain_cpu.py applies the families to the host statement, tests/test_gpu_crs_domain.py to the device.

Words.  A case is a warp: a *destination* lattice (positions ``dst_tf`` of pixel centres, offset 0.5, and on a few cases of pixel
corners, offset 0 on a lattice one larger) in the CRS ``dst`` whose every position is taken to the CRS ``src`` of a *source* grid
``src_tf``.  "a -> b" below reads "positions of a, transformed to b".  Definitions are the GeoKey / EPSG labels ``crs.parse`` reads.

What the reference measures.  tests/_crs_mp.py sums the SAME Krueger series to n^6 as the code under test, at 40 digits and term by
term.  The figures here are therefore evaluation error (rounding, summation order, Newton steps, the wrap), not truncation error of
the series: where the series itself is useless (89.9 degrees from the central meridian on the equator) the reference is as far from
the true projection as the code.

The error measure, stated once (``ground_error``): ground metres, never coordinate units.
  * Transverse Mercator source: abs(dx), abs(dy) of the source CRS coordinate (device: pixel error times the source pixel);
  * geographic source: latitude error x M_PER_DEG, longitude error x M_PER_DEG x cos(exact latitude) -- without the cosine a position
    at 89.999 degrees fails for the meridians' convergence, not for the code's error.
Longitudes are compared modulo 360 in every family but 'antimeridian', where the value itself is compared: the wrap is that
family's subject.

The NaN rule (``expected_nan``).  The reference refuses nothing, so the pattern comes from the contract and the reference supplies
the values elsewhere: a geographic position with abs(latitude) > 90 has no image, and neither has a position whose longitude
difference to the central meridian of a Transverse Mercator source, wrapped to (-180, 180], has cos <= 0.  The difference is
taken from the reference's longitude at 40 digits; ``float64_nan`` restates it as the code forms it (float64, from the lattice's own
longitudes) and the CPU test holds the two equal, i.e. no lattice sits within rounding of the 90 degree line.

The bars.  The project's bar is BAR_M = 1e-6 m.  Each case carries ``host``, the error of the host statement (crs.transform_coords)
measured against the reference on a CPU, and its bar follows from it by one rule (``bar_of``): 1e-6 m where the host statement is at
or below it, four times the host figure otherwise -- the factor covers the device's real-arithmetic Clenshaw summation order and the
last bits of its sincos / exp / atanh.  No bar was chosen by looking at the device. """
import functools
import math
from collections import namedtuple

import numpy as np

import _crs_mp
from homonim_amd import CRS, crs
from homonim_amd.geo import Affine, is_rotated

BAR_M = 1e-6
M_PER_DEG = math.radians(1.) * 6.4e6
SRC_SHAPE = (24, 36)
MAX_LATTICE = (9, 13)
FAMILIES = ('hemispheres', 'antimeridian', 'high-latitude', 'far-from-meridian', 'definitions', 'rotated')

WGS84 = 'EPSG:4326'
AIRY_TM = ('OSGB [1024=1; 2057=6377563.396; 2059=299.3249646; 3075=1; 3080=-2.0; 3081=49.0; 3082=400000.0; 3083=-100000.0; '
           '3092=0.9996012717]')
AIRY_GEO = 'Airy [1024=2; 2054=9102; 2057=6377563.396; 2059=299.3249646]'
# a sphere: e = 0, atanh(0), every alpha / beta zero; k0 = 1 and no false origin
SPHERE_TM = 'sphere TM [1024=1; 2057=6371000.0; 2059=0.0; 3075=1; 3080=10.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]'
SPHERE_GEO = 'sphere [1024=2; 2054=9102; 2057=6371000.0; 2059=0.0]'
# 1 / f = 15, about Jupiter's: on WGS84 and Airy ONE Newton step on tau already reaches float64 (e^2 is that small), so the count of
# three shows only on a flatter body -- here one step leaves 6 mm, two are enough
OBLATE_TM = 'oblate TM [1024=1; 2057=6378137.0; 2059=15.0; 3075=1; 3080=10.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]'
OBLATE_GEO = 'oblate [1024=2; 2054=9102; 2057=6378137.0; 2059=15.0]'
# latitude of origin at a pole: crs.parse lets 3081 = +-90 through (abs(lat0) <= 90), so the copysign branch of _TM.__init__ and of
# crs_params (hk_warp.hip) is reached through a label like every other case; large false origins on both
TM_LAT0_N = 'TM lat0 90 [1024=1; 2048=4326; 3075=1; 3080=-45.0; 3081=90.0; 3082=5000000.0; 3083=30000000.0; 3092=0.994]'
TM_LAT0_S = 'TM lat0 -90 [1024=1; 2048=4326; 3075=1; 3080=100.0; 3081=-90.0; 3082=-20000000.0; 3083=4000000.0; 3092=1.0]'

Case = namedtuple('Case', 'name family src dst dst_tf shape src_tf corners host')


def definition(label):
    d = crs.parse(CRS(label))
    assert d is not None, label
    return d


def bar_of(case):
    """ 1e-6 m where the host statement meets it, four times the host statement's measured error otherwise """
    return BAR_M if case.host <= BAR_M else 4. * case.host


# -- grids --------------------------------------------------------------------------------------------------------------------------
def _centred(x, y, px, py, shape):
    return Affine(px, 0., x - px * shape[1] / 2, 0., -py, y + py * shape[0] / 2)


def _geo_lattice(lon, lat, step, shape):
    """ a geographic grid centred on (lon, lat); ``step`` = degrees per pixel (one number or (along longitude, along latitude)),
    binary fractions, so that every position is an exact double wherever lon and lat are """
    sx, sy = step if isinstance(step, tuple) else (step, step)
    return _centred(lon, lat, sx, sy, shape)


def _image(src, dst, x, y, res):
    """ where the grids are put: the reference's image of one point, to a whole pixel.  The code under test places nothing. """
    ex, ey = _crs_mp.transform(tuple(definition(src)), tuple(definition(dst)), x, y)
    return round(float(ex) / res) * res, round(float(ey) / res) * res


def _tm_lattice(tm, geo, lon, lat, res, shape):
    """ a north-up grid of ``tm`` with pixel ``res`` m centred (to a whole pixel) on the image of (lon, lat) """
    return _centred(*_image(geo, tm, lon, lat, res), res, res, shape)


def _source_around(src, dst, dst_tf, shape, res):
    """ a SRC_SHAPE source grid of pixel ``res`` (metres or degrees) centred on the image of the lattice's centre """
    h, w = shape
    if is_rotated(dst_tf):
        xc, yc = dst_tf.c + dst_tf.a * w / 2 + dst_tf.b * h / 2, dst_tf.f + dst_tf.d * w / 2 + dst_tf.e * h / 2
    else:
        xc, yc = dst_tf.c + dst_tf.a * w / 2, dst_tf.f + dst_tf.e * h / 2
    return _centred(*_image(dst, src, xc, yc, res), res, res, SRC_SHAPE)


def _rotated(tf, shape, degrees):
    """ ``tf`` turned by ``degrees`` about the centre of its grid """
    h, w = shape
    xc, yc = tf.c + tf.a * w / 2, tf.f + tf.e * h / 2
    co, si = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    a, b, d, e = tf.a * co, -tf.e * si, tf.a * si, tf.e * co
    return Affine(a, b, xc - a * w / 2 - b * h / 2, d, e, yc - d * w / 2 - e * h / 2)


def _sheared(tf):
    """ a sheared grid on ``tf``'s origin: rows lean by a quarter pixel per row, columns climb an eighth """
    return Affine(tf.a, tf.a / 4, tf.c, tf.a / 8, tf.e, tf.f)


GEO_STEP = 2. ** -12      # degrees: about 27 m
TM_RES = 30.


def _utm(zone, south=False):
    return f'EPSG:32{7 if south else 6}{zone:02d}'


def _far_tm_lattice(dist, lat, shape):
    """ UTM 33N positions ``dist`` degrees east of the central meridian.  At 89.9 degrees on the equator the series has no
    meaningful value (cosh(12 eta) ~ 1e36), so the grid is placed on the leading term eta' = asinh(tan(dist)) alone. """
    if (dist, lat) == (89.9, 0.):
        ka = 0.9996 * 6367449.145823415
        x = 500000. + round(ka * math.asinh(math.tan(math.radians(dist))) / TM_RES) * TM_RES
        return _centred(x, 0., TM_RES, TM_RES, shape)
    return _tm_lattice(_utm(33), WGS84, 15. + dist, lat, TM_RES, shape)


def _far_tm_source(dist, lat):
    """ a UTM 33N source grid under the far geographic lattices; at 89.9 degrees on the equator the coordinates are ~1e26 m and
    any grid does """
    if (dist, lat) == (89.9, 0.):
        return Affine(TM_RES, 0., 45000000., 0., -TM_RES, 0.)
    return _centred(*_image(WGS84, _utm(33), 15. + dist, lat, TM_RES), TM_RES, TM_RES, SRC_SHAPE)


@functools.lru_cache(None)
def cases():
    """ the case table, built on first use (placing the grids asks the reference for some forty points) """
    full, half, mid, small = MAX_LATTICE, (5, 13), (7, 9), (5, 5)
    out = []

    def add(name, src, dst, dst_tf, shape, src_tf=None, corners=False):
        assert shape[0] <= MAX_LATTICE[0] and shape[1] <= MAX_LATTICE[1]
        if src_tf is None:
            src_tf = _source_around(src, dst, dst_tf, shape, GEO_STEP if definition(src).is_geographic else TM_RES)
        out.append(Case(name, family, src, dst, dst_tf, tuple(shape), src_tf, corners, HOST_M[name]))

    family = 'hemispheres'      # fn = 0 next to fn = 1e7, the equator inside a lattice
    add('utm33n-45n->wgs84', WGS84, _utm(33), _tm_lattice(_utm(33), WGS84, 16., 45., TM_RES, full), full, corners=True)
    add('wgs84-45n->utm33n', _utm(33), WGS84, _geo_lattice(16., 45., GEO_STEP, full), full)
    add('utm35s-equator->utm35n', _utm(35), _utm(35, True), _tm_lattice(_utm(35, True), WGS84, 28.5, 0., TM_RES, full), full)
    add('utm35n-equator->utm35s', _utm(35, True), _utm(35), _tm_lattice(_utm(35), WGS84, 28.5, 0., TM_RES, full), full)
    add('utm33s-45s->wgs84', WGS84, _utm(33, True), _tm_lattice(_utm(33, True), WGS84, 14., -45., TM_RES, full), full)
    add('wgs84-45s->utm33s', _utm(33, True), WGS84, _geo_lattice(14., -45., GEO_STEP, full), full)

    family = 'antimeridian'     # zones 1 and 60; the wrap itself (longitudes are compared by value in this family)
    add('utm01-180->utm60', _utm(60), _utm(1), _tm_lattice(_utm(1), WGS84, 180., 10., TM_RES, full), full)
    add('utm60-180->utm01', _utm(1), _utm(60), _tm_lattice(_utm(60), WGS84, 180., 10., TM_RES, full), full)
    # a geographic lattice from 179.9 to 180.1, written as longitudes above 180
    add('wgs84-above-180->utm01', _utm(1), WGS84, _geo_lattice(180., 10., 2. ** -6, full), full, corners=True)
    # a geographic source whose grid ENDS at 180: what lies beyond it is longitude -180 + d, a column 360 / step to the left, far
    # outside the plane -- finite, not NaN (FAR_SIDE_COLUMN)
    add('utm60-180->wgs84-ending-at-180', WGS84, _utm(60), _tm_lattice(_utm(60), WGS84, 180., 10., TM_RES, full), full,
        src_tf=Affine(GEO_STEP, 0., 180. - SRC_SHAPE[1] * GEO_STEP, 0., -GEO_STEP, 10. + SRC_SHAPE[0] * GEO_STEP / 2))

    family = 'high-latitude'    # tau ~ 1e16, hypot(sinh, cos) ~ 0, three Newton steps
    add('utm33n-84n->wgs84', WGS84, _utm(33), _tm_lattice(_utm(33), WGS84, 17., 84., TM_RES, full), full)
    add('wgs84-84n->utm33n', _utm(33), WGS84, _geo_lattice(17., 84., GEO_STEP, full), full)
    # 30 m pixels centred 112 m from the pole: the lattice holds the pole, its upper rows lie beyond it (longitude lon0 + 180)
    add('utm33n-89.999n->wgs84', WGS84, _utm(33), _tm_lattice(_utm(33), WGS84, 15., 89.999, TM_RES, full), full, corners=True)
    add('wgs84-89.999n->utm33n', _utm(33), WGS84, _geo_lattice(17., 89.999, (0.25, 2. ** -16), full), full)
    # 90.125 + (row + 0.5) * -0.25: the top row of centres is exactly 90
    add('wgs84-top-row-90->utm33n', _utm(33), WGS84, Affine(1., 0., 8.5, 0., -0.25, 90.125), half,
        src_tf=Affine(32768., 0., 0., 0., -32768., 10400000.))
    # ... and from 90.375 the top row is 90.25, beyond the pole, the second exactly 90; meridians 8 degrees apart, to 48 degrees
    # either side of lon0: a fan as wide as it is long (a re-sampling case)
    beyond = Affine(8., 0., -37., 0., -0.25, 90.375)
    # the source grids of the two re-sampling cases are plain numbers chosen from the reference (tap_scale says how;
    # tests/test_crs_domain_cpu.py holds the choice to it)
    add('wgs84-row-beyond-90->utm33n', _utm(33), WGS84, beyond, full, src_tf=Affine(32768., 0., 376832., 0., -32768., 10108928.))
    add('utm33s-80s->wgs84', WGS84, _utm(33, True), _tm_lattice(_utm(33, True), WGS84, 13., -80., TM_RES, full), full)
    add('wgs84-80s->utm33s', _utm(33, True), WGS84, _geo_lattice(13., -80., GEO_STEP, full), full)
    # -89.125 + (row + 0.5) * -0.25 on 5 rows: -89.25, -89.5, -89.75, exactly -90, and -90.25 beyond
    add('wgs84-rows-to-beyond--90->utm33s', _utm(33, True), WGS84, Affine(1., 0., 8.5, 0., -0.25, -89.125), half,
        src_tf=Affine(32768., 0., 0., 0., -32768., 400000.))

    family = 'far-from-meridian'    # UTM 33N, lon0 = 15: a raster that overhangs its zone, to the edge of the projection
    for dist in (6., 30., 60., 89.9):
        for lat in (0., 45.):
            add(f'wgs84-{dist:g}e-{lat:g}n->utm33n', _utm(33), WGS84, _geo_lattice(15. + dist, lat, GEO_STEP, small), small,
                src_tf=_far_tm_source(dist, lat))
            add(f'utm33n-{dist:g}e-{lat:g}n->wgs84', WGS84, _utm(33), _far_tm_lattice(dist, lat, small), small,
                src_tf=_centred(15. + dist, lat, GEO_STEP, GEO_STEP, SRC_SHAPE))
    # geographic rows that cross 90 degrees from lon0 = 15: centres at 105.0625 + (col - 6) / 4, no image from column 6 on (a
    # re-sampling case)
    cross = Affine(0.25, 0., 105.0625 - 6.5 * 0.25, 0., -0.25, 30.625)
    add('wgs84-crossing-90e->utm33n', _utm(33), WGS84, cross, half, src_tf=Affine(65536., 0., 8814592., 0., -65536., 10190848.))

    family = 'definitions'
    # OSGB over 49.5 - 61 N, 8 W - 2 E: centres from 8 W by 1.25 degrees and from 60 N down by 1.5
    add('airy->osgb', AIRY_TM, AIRY_GEO, Affine(1.25, 0., -8.625, 0., -1.5, 60.75), mid,
        src_tf=Affine(65536., 0., -200000., 0., -65536., 1300000.))
    add('osgb->airy', AIRY_GEO, AIRY_TM, Affine(75000., 0., -100000., 0., -150000., 1250000.), mid,
        src_tf=Affine(0.5, 0., -9., 0., -0.5, 61.5))
    add('sphere-geo->tm', SPHERE_TM, SPHERE_GEO, _geo_lattice(12., 35., GEO_STEP, small), small)
    add('sphere-tm->geo', SPHERE_GEO, SPHERE_TM, _tm_lattice(SPHERE_TM, SPHERE_GEO, 12., 35., TM_RES, small), small)
    add('oblate-geo->tm', OBLATE_TM, OBLATE_GEO, _geo_lattice(12., 50., GEO_STEP, small), small)
    add('oblate-tm->geo', OBLATE_GEO, OBLATE_TM, _tm_lattice(OBLATE_TM, OBLATE_GEO, 12., 50., TM_RES, small), small)
    add('wgs84->tm-lat0-90', TM_LAT0_N, WGS84, _geo_lattice(-43., 70., GEO_STEP, mid), mid)
    add('tm-lat0-90->wgs84', WGS84, TM_LAT0_N, _tm_lattice(TM_LAT0_N, WGS84, -43., 70., TM_RES, mid), mid)
    add('wgs84->tm-lat0--90', TM_LAT0_S, WGS84, _geo_lattice(102., -30., GEO_STEP, mid), mid)
    add('tm-lat0--90->wgs84', WGS84, TM_LAT0_S, _tm_lattice(TM_LAT0_S, WGS84, 102., -30., TM_RES, mid), mid)

    # two cases of different families with the destination turned by 30 degrees and a sheared source: hk_warp_coords_affine
    family = 'rotated'
    for name in ('utm33n-45n->wgs84', 'utm01-180->utm60'):
        c = next(c for c in out if c.name == name)
        add(name + '-rotated', c.src, c.dst, _rotated(c.dst_tf, mid, 30.), mid, src_tf=_sheared(c.src_tf))
    return tuple(out)


# The host statement's largest error against the reference per case, ground metres: float64 numpy on an x86-64 CPU, as
# tests/test_crs_domain_cpu.py prints it.  The bar of a case follows by bar_of(): 1e-6 m where the figure is at or below 1e-6 m,
# four times the figure otherwise.
HOST_M = {
    # hemispheres: every bar 1e-6 m
    'utm33n-45n->wgs84': 1.8e-9, 'wgs84-45n->utm33n': 2.0e-9, 'utm35s-equator->utm35n': 2.3e-10, 'utm35n-equator->utm35s': 2.3e-10,
    'utm33s-45s->wgs84': 1.6e-9, 'wgs84-45s->utm33s': 2.0e-9,
    # antimeridian: every bar 1e-6 m
    'utm01-180->utm60': 4.6e-9, 'utm60-180->utm01': 4.7e-9, 'wgs84-above-180->utm01': 3.7e-10,
    'utm60-180->wgs84-ending-at-180': 1.6e-9,
    # high latitude, the poles included: every bar 1e-6 m
    'utm33n-84n->wgs84': 2.5e-9, 'wgs84-84n->utm33n': 2.2e-9, 'utm33n-89.999n->wgs84': 2.2e-9, 'wgs84-89.999n->utm33n': 2.2e-9,
    'wgs84-top-row-90->utm33n': 1.7e-9, 'wgs84-row-beyond-90->utm33n': 2.0e-9, 'utm33s-80s->wgs84': 2.2e-9,
    'wgs84-80s->utm33s': 2.5e-9, 'wgs84-rows-to-beyond--90->utm33s': 1.7e-9,
    # far from the central meridian: 1e-6 m to 60 degrees on the equator and to 89.9 degrees at 45 N ...
    'wgs84-6e-0n->utm33n': 2.6e-10, 'utm33n-6e-0n->wgs84': 3.3e-10, 'wgs84-6e-45n->utm33n': 1.8e-9, 'utm33n-6e-45n->wgs84': 8.8e-10,
    'wgs84-30e-0n->utm33n': 1.5e-9, 'utm33n-30e-0n->wgs84': 9.2e-10, 'wgs84-30e-45n->utm33n': 1.4e-9, 'utm33n-30e-45n->wgs84': 1.1e-9,
    'wgs84-60e-0n->utm33n': 2.0e-9, 'utm33n-60e-0n->wgs84': 1.8e-9, 'wgs84-60e-45n->utm33n': 2.0e-9, 'utm33n-60e-45n->wgs84': 1.3e-9,
    'wgs84-89.9e-45n->utm33n': 2.4e-9, 'utm33n-89.9e-45n->wgs84': 1.5e-9, 'wgs84-crossing-90e->utm33n': 3.4e-9,
    # ... but 89.9 degrees from the central meridian ON the equator is outside the series' useful range: eta' = 7.04, the sixth
    # term carries cosh(12 eta') ~ 1e36 and the "easting" is ~1e26 m, so the rounding of the longitude difference alone is worth
    # 2e14 m.  Bar: 4 x 2.145e14 = 8.58e14 m, loose on purpose; finiteness and the NaN rule are asserted as everywhere.
    'wgs84-89.9e-0n->utm33n': 2.145e14,
    # The inverse of a grid placed there is no place on Earth either: sinh(eta') overflows, tau' = 0 and the longitude difference is
    # atan2(+-inf, c) = +-90 degrees, which the reference reaches as well (4e-33 m): finite by saturation.  Bar 1e-6 m.
    'utm33n-89.9e-0n->wgs84': 0.,
    # definitions: every bar 1e-6 m
    'airy->osgb': 2.2e-9, 'osgb->airy': 3.2e-9, 'sphere-geo->tm': 8.1e-10, 'sphere-tm->geo': 7.2e-10, 'oblate-geo->tm': 3.4e-9, 'oblate-tm->geo': 3.1e-9, 'wgs84->tm-lat0-90': 3.5e-9,
    'tm-lat0-90->wgs84': 2.5e-9, 'wgs84->tm-lat0--90': 2.3e-9, 'tm-lat0--90->wgs84': 2.2e-9,
    # rotated: every bar 1e-6 m
    'utm33n-45n->wgs84-rotated': 1.4e-9, 'utm01-180->utm60-rotated': 4.7e-9,
}


def case(name):
    return next(c for c in cases() if c.name == name)


# for 'utm60-180->wgs84-ending-at-180': a position d degrees beyond the antimeridian has longitude -180 + d, i.e. source column
# 36 - (360 - d) / step: about this far to the left of the plane
FAR_SIDE_COLUMN = -360. / GEO_STEP + SRC_SHAPE[1]


# -- lattices -----------------------------------------------------------------------------------------------------------------------
def lattices(case):
    """ [(what, shape, offset)]: centres, and corners on a lattice one larger for the cases that ask for them """
    h, w = case.shape
    return [('centres', (h, w), 0.5)] + ([('corners', (h + 1, w + 1), 0.)] if case.corners else [])


def positions(case, shape, offset):
    """ the lattice's positions in the destination CRS, formed as the device forms them (hk_warp.hip, warp_coord) """
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    t = case.dst_tf
    if is_rotated(t):
        return (t.c + (cols + offset) * t.a) + (rows + offset) * t.b, (t.f + (cols + offset) * t.d) + (rows + offset) * t.e
    return t.c + (cols + offset) * t.a, t.f + (rows + offset) * t.e


# -- the reference, once per process ------------------------------------------------------------------------------------------------
_REFERENCE = {}


def _geographic_of(d):
    return (crs.GEOGRAPHIC, d.a, d.inv_f, 0., 0., 1., 0., 0.)


def reference():
    """ {(case name, what): (exact, lonlat)}: per position the exact source CRS coordinate and the exact (longitude, latitude), mpf
    pairs in row-major order.  Every case in one pool of workers, once. """
    if _REFERENCE:
        return _REFERENCE
    jobs, keys = [], []
    for c in cases():
        s, d = definition(c.src), definition(c.dst)
        for what, shape, off in lattices(c):
            X, Y = positions(c, shape, off)
            pts = [(float(x), float(y)) for x, y in zip(X.ravel(), Y.ravel())]
            jobs.append((tuple(d), tuple(s), pts))
            keys.append((c.name, what, 'exact'))
            if not d.is_geographic and not s.is_geographic:     # the longitudes in between, for the NaN rule
                jobs.append((tuple(d), _geographic_of(d), pts))
                keys.append((c.name, what, 'lonlat'))
    assert sum(len(j[2]) for j in jobs) < 4300      # the lattices and, between two Transverse Mercators, their longitudes
    import multiprocessing
    import os
    with multiprocessing.get_context('spawn').Pool(max(1, min(12, os.cpu_count() or 1))) as pool:
        done = dict(zip(keys, pool.map(_crs_mp._chunk, jobs, chunksize=1)))
    mpf = _crs_mp.mp.mpf
    for c in cases():
        s, d = definition(c.src), definition(c.dst)
        for what, shape, off in lattices(c):
            exact = done[(c.name, what, 'exact')]
            if d.is_geographic:
                X, Y = positions(c, shape, off)
                lonlat = [(mpf(float(x)), mpf(float(y))) for x, y in zip(X.ravel(), Y.ravel())]
            elif s.is_geographic:
                lonlat = exact
            else:
                lonlat = done[(c.name, what, 'lonlat')]
            _REFERENCE[(c.name, what)] = (exact, lonlat)
    return _REFERENCE


# -- the NaN rule -------------------------------------------------------------------------------------------------------------------
def expected_nan(case, what, shape, offset):
    """ True where the contract gives NaN: abs(latitude) > 90 on a geographic destination; cos <= 0 of the longitude difference to a
    Transverse Mercator source's central meridian, wrapped to (-180, 180], from the reference's longitude """
    s, d = definition(case.src), definition(case.dst)
    bad = np.zeros(shape, bool)
    if d.is_geographic:
        bad |= ~(np.abs(positions(case, shape, offset)[1]) <= 90.)
    if not s.is_geographic:
        _, lonlat = reference()[(case.name, what)]
        mp = _crs_mp.mp
        with mp.workdps(_crs_mp.DPS):
            beyond = [mp.cos(mp.radians(_crs_mp.wrap180(lon - mp.mpf(s.lon0)))) <= 0 for lon, _ in lonlat]
        bad |= np.array(beyond, bool).reshape(shape)
    return bad


def float64_nan(case, shape, offset):
    """ the same rule as the code forms it, for a geographic destination: float64, from the lattice's own longitudes """
    s, d = definition(case.src), definition(case.dst)
    assert d.is_geographic
    X, Y = positions(case, shape, offset)
    bad = ~(np.abs(Y) <= 90.)
    if not s.is_geographic:
        diff = X - s.lon0
        diff = diff - 360. * np.floor(diff / 360.)
        diff = np.where(diff > 180., diff - 360., diff)
        bad |= ~(np.cos(np.radians(diff)) > 0.)
    return bad


# -- the error measure --------------------------------------------------------------------------------------------------------------
def ground_error(case, what, got_x, got_y, skip, pixels):
    """ The largest error in ground metres (module docstring) of ``got_x, got_y`` over the positions where ``skip`` is False.
    ``pixels``: the values are continuous source pixel coordinates (the device's) and are first taken through the source
    geo-transform in exact arithmetic, so that nothing is rounded between what the device stored and what is compared; otherwise
    they are source CRS coordinates (the host statement's). """
    s = definition(case.src)
    exact, _ = reference()[(case.name, what)]
    mp = _crs_mp.mp
    t = case.src_tf
    modulo = case.family != 'antimeridian'
    worst = 0.
    with mp.workdps(_crs_mp.DPS):
        a, b, c, d, e, f = (mp.mpf(float(v)) for v in t)
        for gx, gy, (ex, ey), out in zip(np.ravel(got_x), np.ravel(got_y), exact, np.ravel(skip)):
            if out:
                continue
            gx, gy = mp.mpf(float(gx)), mp.mpf(float(gy))
            if pixels:
                gx, gy = c + a * gx + b * gy, f + d * gx + e * gy
            dx, dy = gx - ex, gy - ey
            if s.is_geographic:
                if modulo:
                    dx = dx - 360 * mp.floor(dx / 360 + mp.mpf(1) / 2)
                dx, dy = dx * M_PER_DEG * mp.cos(mp.radians(ey)), dy * M_PER_DEG
            worst = max(worst, float(abs(dx)), float(abs(dy)))
    return worst


# -- the two re-sampling cases --------------------------------------------------------------------------------------------------------
RESAMPLED = ('wgs84-row-beyond-90->utm33n', 'wgs84-crossing-90e->utm33n')    # one high-latitude, one crossing 90 degrees from lon0


def tap_scale(case):
    """ (kx, ky) for a re-sampling case: the mean step between the images of neighbouring positions along a row / a column, in
    source pixels, over the pairs that both have an image (``raster_array.warp_scale`` reads the ends of the central row and column,
    which here have none).  From the reference; at most 1 by the choice of the source grid: its pixel is the largest such step
    rounded up to a power of two, so no axis is down-sampled and the re-samplers run in their tap form.  The grid's left edge lies
    inside the images' bounding box, so that the leftmost images fall outside the plane. """
    exact, _ = reference()[(case.name, 'centres')]
    bad = expected_nan(case, 'centres', case.shape, 0.5)
    px, py = (np.array([float(p[k]) for p in exact]).reshape(case.shape) for k in (0, 1))
    px, py = np.where(bad, np.nan, (px - case.src_tf.c) / case.src_tf.a), np.where(bad, np.nan, (py - case.src_tf.f) / case.src_tf.e)
    kx, ky = (float(np.nanmean(np.hypot(np.diff(px, axis=k), np.diff(py, axis=k)))) for k in (1, 0))
    assert 0. < kx <= 1. and 0. < ky <= 1., (kx, ky)
    return kx, ky
