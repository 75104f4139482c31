""" 40-digit mpmath evaluation of the CRS definitions homonim_amd/crs.py parses: the reference the float64 transformations (numpy
on the host, hk_warp.hip on the device) are held to.

Written on its own from the published formulae (Karney 2011, "Transverse Mercator with an accuracy of a few nanometers", eqs. 7-9,
11, 19-21, 35, 36): rational coefficients, the series summed term by term with complex sines, Newton run to convergence -- no
Clenshaw recurrence, no fixed iteration count, no code shared with the package.  A definition is the tuple
``(kind, a, inv_f, lat0, lon0, k0, fe, fn)`` with kind 0 = geographic (degrees), 1 = Transverse Mercator.

``transform_many`` spreads the points over worker processes (spawned: they import this module and mpmath only). """
import os
from fractions import Fraction as Fr

import mpmath as mp

DPS = 40
ALPHA = [
    [Fr(1, 2), Fr(-2, 3), Fr(5, 16), Fr(41, 180), Fr(-127, 288), Fr(7891, 37800)],
    [Fr(13, 48), Fr(-3, 5), Fr(557, 1440), Fr(281, 630), Fr(-1983433, 1935360)],
    [Fr(61, 240), Fr(-103, 140), Fr(15061, 26880), Fr(167603, 181440)],
    [Fr(49561, 161280), Fr(-179, 168), Fr(6601661, 7257600)],
    [Fr(34729, 80640), Fr(-3418889, 1995840)],
    [Fr(212378941, 319334400)],
]
BETA = [
    [Fr(1, 2), Fr(-2, 3), Fr(37, 96), Fr(-1, 360), Fr(-81, 512), Fr(96199, 604800)],
    [Fr(1, 48), Fr(1, 15), Fr(-437, 1440), Fr(46, 105), Fr(-1118711, 3870720)],
    [Fr(17, 480), Fr(-37, 840), Fr(-209, 4480), Fr(5569, 90720)],
    [Fr(4397, 161280), Fr(-11, 504), Fr(-830251, 7257600)],
    [Fr(4583, 161280), Fr(-108847, 3991680)],
    [Fr(20648693, 638668800)],
]


def _mpf(v):
    return mp.mpf(v.numerator) / v.denominator if isinstance(v, Fr) else mp.mpf(v)


class TM:
    def __init__(self, d):
        _, a, inv_f, lat0, lon0, k0, fe, fn = d
        f = 1 / mp.mpf(inv_f) if inv_f else mp.mpf(0)
        n = f / (2 - f)
        self.e = mp.sqrt(f * (2 - f))
        self.ka = mp.mpf(k0) * mp.mpf(a) / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64 + n ** 6 / 256)
        self.alp = [sum(_mpf(c) * n ** (j + 1 + k) for k, c in enumerate(row)) for j, row in enumerate(ALPHA)]
        self.bet = [sum(_mpf(c) * n ** (j + 1 + k) for k, c in enumerate(row)) for j, row in enumerate(BETA)]
        self.lon0, self.fe, self.fn = mp.mpf(lon0), mp.mpf(fe), mp.mpf(fn)
        xip = mp.atan(self.taup(mp.tan(mp.radians(mp.mpf(lat0)))))
        self.xi0 = xip + sum(a_ * mp.sin(2 * (j + 1) * xip) for j, a_ in enumerate(self.alp))

    def taup(self, tau):
        sig = mp.sinh(self.e * mp.atanh(self.e * tau / mp.sqrt(1 + tau * tau)))
        return tau * mp.sqrt(1 + sig * sig) - sig * mp.sqrt(1 + tau * tau)

    def forward(self, lon, lat):
        dlam = mp.radians(wrap180(lon - self.lon0))
        tp = self.taup(mp.tan(mp.radians(lat)))
        xip = mp.atan2(tp, mp.cos(dlam))
        etap = mp.asinh(mp.sin(dlam) / mp.hypot(tp, mp.cos(dlam)))
        z = mp.mpc(xip, etap)
        z = z + sum(a_ * mp.sin(2 * (j + 1) * z) for j, a_ in enumerate(self.alp))
        return self.fe + self.ka * z.imag, self.fn + self.ka * (z.real - self.xi0)

    def inverse(self, x, y):
        z = mp.mpc((y - self.fn) / self.ka + self.xi0, (x - self.fe) / self.ka)
        z = z - sum(b_ * mp.sin(2 * (j + 1) * z) for j, b_ in enumerate(self.bet))
        xip, etap = z.real, z.imag
        tp = mp.sin(xip) / mp.hypot(mp.sinh(etap), mp.cos(xip))
        dlam = mp.atan2(mp.sinh(etap), mp.cos(xip))
        e2m = 1 - self.e ** 2
        tau = tp / e2m
        for _ in range(40):
            tpi = self.taup(tau)
            dtau = (tp - tpi) / mp.sqrt(1 + tpi * tpi) * (1 + e2m * tau * tau) / (e2m * mp.sqrt(1 + tau * tau))
            tau += dtau
            if abs(dtau) <= mp.mpf(10) ** (-(DPS - 4)) * max(1, abs(tau)):
                break
        else:
            raise ArithmeticError('Newton on tau did not converge')
        return self.lon0 + mp.degrees(dlam), mp.degrees(mp.atan(tau))


def wrap180(d):
    d = d - 360 * mp.floor(d / 360)     # [0, 360)
    return d - 360 if d > 180 else d


def transform(src_def, dst_def, x, y):
    """ one point; exact inputs (floats are taken at their binary value) """
    with mp.workdps(DPS):
        x, y = mp.mpf(x), mp.mpf(y)
        lon, lat = (x, y) if src_def[0] == 0 else TM(src_def).inverse(x, y)
        if dst_def[0] == 0:
            return wrap180(lon), lat
        return TM(dst_def).forward(lon, lat)


def _chunk(args):
    src_def, dst_def, pts = args
    with mp.workdps(DPS):
        s = None if src_def[0] == 0 else TM(src_def)
        d = None if dst_def[0] == 0 else TM(dst_def)
        out = []
        for x, y in pts:
            x, y = mp.mpf(x), mp.mpf(y)
            lon, lat = (x, y) if s is None else s.inverse(x, y)
            out.append((wrap180(lon), lat) if d is None else d.forward(lon, lat))
        return out


def transform_many(src_def, dst_def, xs, ys, workers=None):
    """ [(X, Y)] as mpf pairs for float64 sequences xs, ys """
    pts = [(float(x), float(y)) for x, y in zip(xs, ys)]
    workers = workers or max(1, min(12, os.cpu_count() or 1))
    if workers == 1 or len(pts) < 400:
        return _chunk((tuple(src_def), tuple(dst_def), pts))
    import multiprocessing
    size = -(-len(pts) // (workers * 4))
    jobs = [(tuple(src_def), tuple(dst_def), pts[k:k + size]) for k in range(0, len(pts), size)]
    with multiprocessing.get_context('spawn').Pool(workers) as pool:
        return [p for part in pool.map(_chunk, jobs) for p in part]


def max_error(got_x, got_y, exact, scale_x=1.0, scale_y=1.0):
    """ the largest abs(got - exact) over both coordinates, each scaled (e.g. metres per degree), as a float """
    with mp.workdps(DPS):
        worst = mp.mpf(0)
        for gx, gy, (ex, ey) in zip(got_x, got_y, exact):
            worst = max(worst, abs(mp.mpf(float(gx)) - ex) * scale_x, abs(mp.mpf(float(gy)) - ey) * scale_y)
        return float(worst)
