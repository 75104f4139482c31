""" Rotated and sheared grid pairs, and the exact statement of the warp's affine coordinate function (hk_warp.hip warp_coord, the
same-CRS path), shared by tests/test_rotated_cpu.py and tests/test_gpu_rotated.py.

The device forms, in float64 and in exactly this association (include/homonim_hk.h, hk_affine_warp_desc):

    X = (c + col * a) + row * b, Y = (f + col * d) + row * e                  destination geo-transform
    u = X - sc, v = Y - sf, col_s = (u * se - v * sb) / det, row_s = (v * sa - u * sd) / det, det = sa * se - sb * sd

``coords_np`` is that statement in numpy; ``exact_lattice`` is the same map in ``fractions.Fraction`` on the float64 coefficients
taken as the rationals they are (exact: the map is affine, so three rationals per coordinate give every lattice point).

The bar, in source pixels: ``8 ulp(M) / p + 8 eps max|coordinate|``.  M is the largest origin magnitude of the two grids: X, Y, u
and v are each rounded at that magnitude or below (two roundings for X, two for Y, one each for u, v: at most 1/2 ulp(M) each, and
each enters a pixel coordinate divided by the source's smaller pixel extent p = |det| / max(hypot(sa, sd), hypot(sb, se))).  The
second term counts the two products, their difference, the quotient and det's own three roundings, each relative to the
coordinate in pixels (eps = 2^-52). """
import functools
import math
from fractions import Fraction

import numpy as np

from homonim_amd import Affine

EPS = 2.0 ** -52
LATTICES = (('centres', (97, 131), 0.5), ('corners', (98, 132), 0.))


def rotated(x0, y0, degrees, pixel, south_up=False):
    """ a grid of square pixels rotated by ``degrees`` about its origin (x0, y0); rows run down unless ``south_up`` """
    return Affine.translation(x0, y0) * Affine.rotation(degrees) * Affine.scale(pixel, pixel if south_up else -pixel)


# name: (source geo-transform, destination geo-transform)
PAIRS = {
    'north-up-from-30deg-0.5m': (rotated(-60400., -3722690., 30., 0.5), Affine(0.5, 0., -60390., 0., -0.5, -3722700.)),
    '90deg-1m': (rotated(254000., 6277870., 90., 1.), Affine(1., 0., 254000., 0., -1., 6278000.)),
    'shear3-and-minus40deg-30m': (Affine(30., 3., 254000., 0., -30., 6278000.), rotated(254600., 6277900., -40., 30.)),
    '15deg-5m-from-minus40deg-south-up-30m': (rotated(253000., 6274000., -40., 30., south_up=True), rotated(254500., 6276500., 15., 5.)),
    '10deg-from-77deg-0.05m': (rotated(-60390., -3722700., 77., 0.05), rotated(-60391., -3722703., 10., 0.05)),
}


def coords_np(src_tf, dst_tf, shape, off):
    """ the device's expressions, operation for operation, on the (row + off, col + off) lattice of ``shape`` -> (col_s, row_s) """
    s, d = src_tf, dst_tf
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    rows, cols = rows + off, cols + off
    X, Y = (d.c + cols * d.a) + rows * d.b, (d.f + cols * d.d) + rows * d.e
    det = s.a * s.e - s.b * s.d
    u, v = X - s.c, Y - s.f
    return (u * s.e - v * s.b) / det, (v * s.a - u * s.d) / det


@functools.lru_cache(maxsize=None)
def exact_lattice(pair, shape, off):
    """ ((x0, x_col, x_row), (y0, y_col, y_row)) as Fractions: the exact source coordinate of lattice point (i, j) is
    x0 + j * x_col + i * x_row, likewise y """
    s, d = ([Fraction(v) for v in tf[:6]] for tf in PAIRS[pair])
    sa, sb, sc, sd, se, sf = s
    da, db, dc, dd, de, df = d
    det = sa * se - sb * sd
    o = Fraction(off)

    def comp(k0, kx, ky):   # k0 + kx * X + ky * Y with X, Y affine in (col, row)
        const = k0 + kx * (dc + o * da + o * db) + ky * (df + o * dd + o * de)
        return const, kx * da + ky * dd, kx * db + ky * de
    x = comp((-sc * se + sf * sb) / det, se / det, -sb / det)
    y = comp((-sf * sa + sc * sd) / det, -sd / det, sa / det)
    return x, y


def max_error(pair, shape, off, gx, gy):
    """ the largest distance, in source pixels and per coordinate, of the float64 planes ``gx, gy`` from the exact lattice """
    (x0, xc, xr), (y0, yc, yr) = exact_lattice(pair, shape, off)
    worst = Fraction(0)
    for i in range(shape[0]):
        ex, ey = x0 + i * xr, y0 + i * yr
        for j in range(shape[1]):
            worst = max(worst, abs(Fraction(float(gx[i, j])) - (ex + j * xc)), abs(Fraction(float(gy[i, j])) - (ey + j * yc)))
    return float(worst)


def max_abs_coord(pair, shape, off):
    """ the largest exact coordinate magnitude on the lattice, in source pixels (an affine map takes its extremes at the corners) """
    (x0, xc, xr), (y0, yc, yr) = exact_lattice(pair, shape, off)
    h, w = shape[0] - 1, shape[1] - 1
    return float(max(abs(c0 + j * cc + i * cr) for c0, cc, cr in ((x0, xc, xr), (y0, yc, yr)) for i in (0, h) for j in (0, w)))


def bar(pair, shape, off):
    s, d = PAIRS[pair]
    m = max(abs(s.c), abs(s.f), abs(d.c), abs(d.f))
    p = abs(s.a * s.e - s.b * s.d) / max(math.hypot(s.a, s.d), math.hypot(s.b, s.e))
    return 8. * float(np.spacing(m)) / p + 8. * EPS * max_abs_coord(pair, shape, off)
