"""
Coordinate reference system definitions and the transformation between them.

``geo.CRS`` is a label.  This module parses the labels ``tiff.py`` produces into definitions -- kind, ellipsoid, and for a
Transverse Mercator its origin, scale and false origin -- so that rasters of different CRSs can be brought together: the
reference hands such a pair to GDAL (``RasterPairReader`` warns and goes on, homonim/raster_pair.py:160-166;
``utils.same_orientation_crs``, homonim/utils.py:190-209), this package warps on the GPU (hk_warp.hip).

Known labels
  * ``EPSG:4326``;
  * ``EPSG:326zz`` / ``EPSG:327zz``: the WGS84 UTM zones north / south;
  * the GeoKey lists of user-defined CRSs (``name [1024=1; ...; 3075=1; 3080=25.0; ...]``, tiff.py): Transverse Mercator
    (``3075=1``) with keys 3080 / 3081 / 3082 / 3083 / 3092 and the ellipsoid keys 2057 / 2059, and geographic lists (``1024=2``).

Everything else is unknown: such a CRS equals only itself (by label), and a pair with one raises ``NotImplementedError`` naming
it.  There are no datum shifts: two CRSs on different ellipsoids raise ``NotImplementedError`` as well.

Mathematics (public formulae): Transverse Mercator by the Krueger series in the third flattening n to n^6 -- the alpha / beta
coefficients of Karney (2011), "Transverse Mercator with an accuracy of a few nanometers", J. Geodesy 85 -- forward and
inverse; the inverse takes the conformal latitude to the geodetic one by Newton on tau = tan(phi).  Geographic CRSs are degrees,
longitude first; longitude differences wrap to (-180, 180]; abs(latitude) > 90 gives NaN.

``transform_coords`` is the float64 numpy statement of the transformation.  Host code uses it for bounds and grids; pixels are
transformed on the device (``Context.warp_coords`` returns the device's own coordinates).
"""
import math
import re
from typing import NamedTuple, Optional, Tuple

import numpy as np

GEOGRAPHIC, TMERC = 0, 1   # hk_crs_kind of include/homonim_hk.h
WGS84 = (6378137.0, 298.257223563)
# GeoKey ids (GeoTIFF 1.1, annex B)
_K_MODEL, _K_GEOG, _K_ANG_UNITS, _K_SEMI_MAJOR, _K_INV_FLAT = 1024, 2048, 2054, 2057, 2059
_K_PROJ_CT, _K_LIN_UNITS, _K_LON0, _K_LAT0, _K_FE, _K_FN, _K_K0 = 3075, 3076, 3080, 3081, 3082, 3083, 3092
# every key a Transverse Mercator / geographic key list may carry and still be fully described by a CrsDef
_TM_KEYS = {1024, 1025, 2048, 2050, 2054, 2056, 2057, 2059, 3072, 3074, 3075, 3076, 3080, 3081, 3082, 3083, 3092}


class CrsDef(NamedTuple):
    """ What the transformation needs of a CRS; two labels with equal definitions are the same CRS. """
    kind: int      # GEOGRAPHIC / TMERC
    a: float       # ellipsoid: semi-major axis, metres
    inv_f: float   # inverse flattening (0: a sphere)
    lat0: float = 0.   # Transverse Mercator: latitude of origin, degrees
    lon0: float = 0.   # central meridian, degrees
    k0: float = 1.     # scale on the central meridian
    fe: float = 0.     # false easting / northing, metres
    fn: float = 0.

    @property
    def is_geographic(self) -> bool:
        return self.kind == GEOGRAPHIC


def _label(crs) -> str:
    return crs.to_string() if hasattr(crs, 'to_string') else str(crs)


def _parse_keys(body: str) -> Optional[CrsDef]:
    keys = {}
    for item in body.split(';'):
        m = re.fullmatch(r'\s*(\d+)\s*=\s*(\S+)\s*', item)
        if not m:
            return None
        try:
            keys[int(m.group(1))] = float(m.group(2))
        except ValueError:
            return None
    if not set(keys) <= _TM_KEYS:       # a key this module does not understand may change the meaning of the others
        return None
    if keys.get(_K_ANG_UNITS, 9102) != 9102:    # degrees
        return None
    if _K_SEMI_MAJOR in keys and _K_INV_FLAT in keys:
        ellipsoid = (keys[_K_SEMI_MAJOR], keys[_K_INV_FLAT])
    elif keys.get(_K_GEOG) == 4326 and _K_SEMI_MAJOR not in keys and _K_INV_FLAT not in keys:
        ellipsoid = WGS84
    else:
        return None
    if not (ellipsoid[0] > 0 and (ellipsoid[1] == 0 or ellipsoid[1] > 1)):
        return None
    model = keys.get(_K_MODEL)
    if model == 2:
        return CrsDef(GEOGRAPHIC, *ellipsoid)
    if model != 1 or keys.get(_K_PROJ_CT) != 1 or keys.get(_K_LIN_UNITS, 9001) != 9001 or _K_LON0 not in keys:
        return None
    d = CrsDef(TMERC, *ellipsoid, keys.get(_K_LAT0, 0.), keys[_K_LON0], keys.get(_K_K0, 1.), keys.get(_K_FE, 0.),
               keys.get(_K_FN, 0.))
    if not (d.k0 > 0 and abs(d.lat0) <= 90 and all(math.isfinite(v) for v in d)):
        return None
    return d


def parse(crs) -> Optional[CrsDef]:
    """ The definition of a CRS (a ``geo.CRS`` or its label), or None when the label is not one of the known families. """
    label = _label(crs).strip()
    m = re.fullmatch(r'(?i)EPSG:(\d+)', label)
    if m:
        code = int(m.group(1))
        if code == 4326:
            return CrsDef(GEOGRAPHIC, *WGS84)
        zone = code % 100
        if code // 100 in (326, 327) and 1 <= zone <= 60:
            return CrsDef(TMERC, *WGS84, 0., 6. * zone - 183., 0.9996, 500000., 0. if code // 100 == 326 else 10000000.)
        return None
    m = re.fullmatch(r'[^\[\]]*\[([^\[\]]*)\]', label)
    return _parse_keys(m.group(1)) if m else None


def same_crs(a, b) -> bool:
    """ Equal labels (any CRS), or two known labels with equal definitions. """
    if _label(a).strip().lower() == _label(b).strip().lower():
        return True
    da, db = parse(a), parse(b)
    return da is not None and da == db


def definitions(src_crs, dst_crs) -> Tuple[CrsDef, CrsDef]:
    """ The definitions of two CRSs a transformation runs between; ``NotImplementedError`` naming the CRS that is not known,
    or the two ellipsoids when they differ. """
    defs = []
    for crs in (src_crs, dst_crs):
        d = parse(crs)
        if d is None:
            raise NotImplementedError(f"re-projection from / to '{_label(crs)}' is not built: its definition is not known "
                                      '(EPSG:4326, the WGS84 UTM zones EPSG:326zz / 327zz and Transverse Mercator / geographic '
                                      'GeoKey lists are)')
        defs.append(d)
    s, d = defs
    if (s.a, s.inv_f) != (d.a, d.inv_f):
        raise NotImplementedError(f"re-projection between different ellipsoids is not built (no datum shifts): "
                                  f"'{_label(src_crs)}' is on a={s.a!r}, 1/f={s.inv_f!r}, '{_label(dst_crs)}' on a={d.a!r}, "
                                  f'1/f={d.inv_f!r}')
    return s, d


# -- Transverse Mercator (Krueger n-series, Karney 2011 eqs. 35, 36) ---------------------------------------------------------
def _alpha(n):
    n2, n3, n4, n5, n6 = n ** 2, n ** 3, n ** 4, n ** 5, n ** 6
    return (n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800,
            13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360,
            61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440,
            49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600,
            34729 * n5 / 80640 - 3418889 * n6 / 1995840,
            212378941 * n6 / 319334400)


def _beta(n):
    n2, n3, n4, n5, n6 = n ** 2, n ** 3, n ** 4, n ** 5, n ** 6
    return (n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
            n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
            17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
            4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
            4583 * n5 / 161280 - 108847 * n6 / 3991680,
            20648693 * n6 / 638668800)


class _TM:
    """ Constants of one Transverse Mercator definition. """

    def __init__(self, d: CrsDef):
        f = 1. / d.inv_f if d.inv_f else 0.
        n = f / (2. - f)
        self.e = math.sqrt(f * (2. - f))
        self.e2m = (1. - f) ** 2
        self.ka = d.k0 * (d.a / (1. + n) * (1. + n ** 2 / 4. + n ** 4 / 64. + n ** 6 / 256.))
        self.alp, self.bet = _alpha(n), _beta(n)
        self.lon0, self.fe, self.fn = d.lon0, d.fe, d.fn
        if abs(d.lat0) == 90.:
            self.xi0 = math.copysign(math.pi / 2, d.lat0)
        else:
            xip = math.atan(float(self._taup(np.float64(math.tan(math.radians(d.lat0))))))
            self.xi0 = xip + sum(a * math.sin(2 * (j + 1) * xip) for j, a in enumerate(self.alp))

    def _taup(self, tau):
        t1 = np.sqrt(1. + tau * tau)
        sig = np.sinh(self.e * np.arctanh(self.e * tau / t1))
        return tau * np.sqrt(1. + sig * sig) - sig * t1

    @staticmethod
    def _series(c, xi, eta):
        """ sum_j c[j] sin(2 (j + 1) (xi + i eta)) by Clenshaw's recurrence on the complex argument """
        zeta2 = 2. * (xi + 1j * eta)
        a = 2. * np.cos(zeta2)
        y0 = np.zeros_like(a)
        y1 = np.zeros_like(a)
        for cj in reversed(c):
            y0, y1 = a * y0 - y1 + cj, y0
        return np.sin(zeta2) * y0

    def forward(self, lon, lat):
        """ degrees -> (easting, northing); NaN 90 degrees or more from the central meridian and for abs(lat) > 90 """
        dlam = np.radians(_wrap180(lon - self.lon0))
        with np.errstate(all='ignore'):
            tp = self._taup(np.tan(np.radians(lat)))
            sl, cl = np.sin(dlam), np.cos(dlam)
            xip, etap = np.arctan2(tp, cl), np.arcsinh(sl / np.hypot(tp, cl))
            z = self._series(self.alp, xip, etap)
            x = self.fe + self.ka * (etap + z.imag)
            y = self.fn + self.ka * ((xip + z.real) - self.xi0)
        bad = ~(cl > 0.) | ~(np.abs(lat) <= 90.)
        return np.where(bad, np.nan, x), np.where(bad, np.nan, y)

    def inverse(self, x, y):
        """ (easting, northing) -> degrees """
        with np.errstate(all='ignore'):
            xi, eta = (y - self.fn) / self.ka + self.xi0, (x - self.fe) / self.ka
            z = self._series(self.bet, xi, eta)
            xip, etap = xi - z.real, eta - z.imag
            s, c, sh = np.sin(xip), np.cos(xip), np.sinh(etap)
            tp = s / np.hypot(sh, c)
            dlam = np.arctan2(sh, c)
            tau = tp / self.e2m
            for _ in range(3):   # the error squares per step from ~e^2: below 1e-20 after the third
                t1 = np.sqrt(1. + tau * tau)
                tpi = self._taup(tau)
                tau = tau + (tp - tpi) / np.sqrt(1. + tpi * tpi) * (1. + self.e2m * (tau * tau)) / (self.e2m * t1)
        return self.lon0 + np.degrees(dlam), np.degrees(np.arctan(tau))


def _wrap180(d):
    """ a longitude (difference) in degrees brought to (-180, 180] """
    d = np.remainder(np.asarray(d, np.float64), 360.)       # [0, 360)
    return np.where(d > 180., d - 360., d)


def transform_coords(src_crs, dst_crs, xs, ys):
    """
    Coordinates ``(xs, ys)`` of ``src_crs`` in ``dst_crs`` (float64 numpy arrays of the inputs' common shape; geographic
    coordinates are (longitude, latitude) in degrees).  NaN where a point has no image.  Raises ``NotImplementedError`` for an
    unknown CRS or two ellipsoids (``definitions``).
    """
    s, d = definitions(src_crs, dst_crs)
    xs, ys = np.broadcast_arrays(np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    if s == d:
        return xs.copy(), ys.copy()
    if s.is_geographic:
        lon, lat = xs, np.where(np.abs(ys) <= 90., ys, np.nan)
    else:
        lon, lat = _TM(s).inverse(xs, ys)
    if d.is_geographic:
        return np.where(np.isnan(lat), np.nan, _wrap180(lon)), lat + 0. * lon
    return _TM(d).forward(lon, lat)
