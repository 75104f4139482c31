""" An exact statement of GDAL's warp re-samplers -- all fourteen methods of the scaled path, and the five point methods on PER-PIXEL
source coordinates -- in ``fractions.Fraction`` arithmetic on the float32 inputs, and the enclosure a float64-accumulating
implementation must meet.

Written from GDAL's published rule (gdal/alg/gdalwarpkernel.cpp: GWKResample, GWKCubic, GWKBilinear, GWKBSpline, GWKLanczosSinc,
GWKAverageOrMode), NOT from hk_resample_taps.h, oracle/oracle_np.py or tests/_warp_reference.py: those share one float64 formula,
operation for operation, so a mistake in a weight, a radius, a rank or a renormalisation rule that all of them make passes every
bit-for-bit comparison between them.  This module shares nothing with them but the mapping convention ``src = k * dst + o`` on
continuous coordinates (integers = pixel edges, pixel p covers [p, p + 1)).

Two ways in:
  * ``exact`` / ``enclosure_failures``: a DYADIC mapping, ``k`` and ``o`` multiples of 1/8.  Then ``k * (j + 1/2) + o`` and ``k * j + o``
    are exact in double as well, every ``floor`` in an implementation sees the true value, and the ``1e-10`` nudges implementations
    add before ``floor`` / ``ceil`` can move nothing (the nearest other multiple of 1/16 is 6e-2 away);
  * ``exact_at`` / ``enclosure_failures_at``: float64 coordinate planes ``sx, sy`` taken as the exact rationals they are (two CRSs,
    rotated grids); ``kx, ky`` (source pixels per destination pixel) only choose the form and the stretch.

The rules
---------
nearest: the source pixel ``floor(s)`` under the destination centre, when it is inside the plane and valid.

bilinear / cubic_spline on axes that step at most ``1 + 1e-9`` source pixels per destination pixel (the TAP form), ``s`` per axis:
  * the source pixel ``floor(s)`` under the destination centre must be inside the plane and valid, else nodata;
  * ``i0 = floor(s - 1/2)``, ``d = s - 1/2 - i0``; taps ``i0 + t``, t = 0, 1 (bilinear) or -1, 0, 1, 2 (cubic_spline);
  * weights: bilinear ``1 - d, d``; cubic B-spline ``(1-d)^3/6, ((2-d)^3 - 4(1-d)^3)/6, ((3-d)^3 - 4(2-d)^3 + 6(1-d)^3)/6, d^3/6``;
    the 2-D weight is the product of the two axes' weights;
  * taps outside the plane or invalid are dropped; ``W`` = sum of the kept weights; ``W < 1e-6``: nodata;
  * value = ``sum(w v)`` when ``0.99999 <= W <= 1.00001``, else ``sum(w v) / W``.

cubic and lanczos always, bilinear and cubic_spline when either axis steps more than ``1 + 1e-9`` (the CONVOLUTION form, GWKResample):
  * per axis ``scale = min(1, 1 / k)``; origin and fraction as above; tap ``i0 + t`` (any integer t) has weight ``f((t - d) * scale)``;
  * f, with R its radius: the tent ``1 - |x|`` (R = 1); the cubic convolution kernel with a = -1/2, ``3/2 |x|^3 - 5/2 |x|^2 + 1`` on
    [0, 1] and ``-1/2 |x|^3 + 5/2 |x|^2 - 4 |x| + 2`` on [1, 2] (R = 2); the cubic B-spline ``2/3 - x^2 + |x|^3 / 2`` on [0, 1] and
    ``(2 - |x|)^3 / 6`` on [1, 2] (R = 2); ``sinc(x) sinc(x / 3)``, sinc(x) = sin(pi x) / (pi x) (R = 3); f = 0 for ``|x| >= R``.
    The support is stated by that alone -- every t with ``|(t - d) * scale| < R`` -- and by no radius formula, so that an
    implementation's ``ceil(R / scale)`` is itself under test;
  * the centre pixel ``floor(s)`` must be inside the plane and valid; taps outside the plane or invalid are dropped;
  * ``|W| < 1e-6``: nodata (W may be negative or cancel here); otherwise value = ``sum(w v) / W``, always.
  The three polynomial kernels are exact in Fraction.  The lanczos weight is evaluated with mpmath at 50 digits and converted to the
  Fraction it is; that adds an absolute error below 1e-40 to a weight, 25 orders below anything held here.

The footprint methods, destination pixel (i, j): its footprint ``[k j + o, k (j + 1) + o]`` per axis, clipped to the plane; the pixels
are those that share a positive length with it on both axes, the valid ones taken in row-major order; none: nodata.
  * average: the mean weighted by the shared area;
  * max, min: over those pixels;
  * sum ``sum(w v)`` and rms ``sqrt(sum(w v^2) / sum(w))``: w the product of the per-axis shares, EXCEPT that an axis whose clipped
    footprint touches a single pixel weighs it 1, whatever its share (GDAL's rule);
  * mode: the value whose running count, scanning in row-major order, first reaches the highest count;
  * med, q1, q3: element ``max(0, ceil(q n - 1))`` of the n sorted values, q = 1/2, 1/4, 3/4.

What a result is held to
------------------------
Exact-valued methods (nearest, max, min, mode, med, q1, q3): the identical nodata pattern and the identical float32 value; no
tolerance (the test sources hold no zero, so value and bit pattern are one).

bilinear, cubic_spline, average, cubic, sum: ``|got - exact| <= 1/2 ulp32(got) + 2^-40 * A``, ``A = sum(|w| |v|) / min(|W|, 1)``
(sum: ``A = sum(w |v|)``).  The first term is the one rounding of the float64 result to float32.  The second bounds what float64
evaluation can lose.  In the TAP form:
  * a 1-D B-spline weight is made from about 10 operations on operands of magnitude <= 27 (``(3 - d)^3``); the absolute error of the
    two middle weights is below ``10 * 27 * 2^-53 / 6 < 2^-47``, and as they are >= 1/6 their relative error is below ``2^-44``; the two
    outer weights are a cube and a division, relative error below ``2^-50``.  Bilinear weights (one subtraction) and the overlap
    weights of `average` (two subtractions) do better;
  * a 2-D weight is one more product: relative error below ``2^-43``;
  * the sum runs over at most 16 products (`average`, `sum` at the ratios tested here: at most 5 x 5 = 25); each product and each
    addition rounds once, which adds less than ``27 * 2^-53 < 2^-48`` relative to ``sum(|w| |v|)``; the same holds for ``W``, whose terms
    are all positive;
  * the division by ``W`` carries W's relative error (< 2^-43) over and rounds once more.
  Together: below ``2^-42 * sum(|w| |v|) / W``, so ``2^-40 * A`` has a factor 4 to spare and is still 2^-16 of a float32 ulp of a
  well-conditioned pixel: a wrong tap, weight or rule cannot hide in it.
In the CONVOLUTION form a weight can vanish inside the support, so its error is bounded absolutely, not relatively:
  * the argument ``(t - d) * scale`` costs the division ``1 / k`` and one product: relative error 2^-52, absolute ``|x| 2^-52 <= 2^-51``,
    which a kernel of slope at most 3/2 turns into at most ``2^-50`` of weight;
  * the cubic kernel is about 8 operations on operands <= 8: on [0, 1] (operands <= 2.5) below ``2^-49``, on [1, 2] below
    ``6 * 8 * 2^-53 < 2^-47``, where the kernel itself is below 0.075; the tent is one subtraction; the B-spline, summed from cubes up
    to 64 with coefficients up to 6, stays below ``2^-46``;
  * a 2-D weight is ``wx wy``, with absolute error ``e <= |wx| ey + |wy| ex <= 2^-46``, typically 2^-48;
  * ``sum(w v)`` is then off by at most ``e sum(|v|)`` and ``W`` by ``e n``, over the n kept taps, plus one rounding per product and
    addition, ``2 n 2^-53`` relative to ``sum(|w| |v|)``.  A stretched axis holds ``2 ceil(R k)`` taps whose weights sum to k, so the mean
    2-D weight is ``k^2 / (2 ceil(R k))^2 >= 1 / (4 R^2)``, whatever k: 1/16 for the cubics, 1/4 for the tent.  ``e sum(|v|)`` is thus
    about ``16 e sum(|w| |v|) <= 2^-42 sum(|w| |v|)``, and the rounding term, at the largest steps used here (3 x 3, and 1.5 x 4 with fewer
    taps), ``2 * 144 * 2^-53 < 2^-44``;
  * the division by W carries both over.
  Together below ``2^-41.5 A``: ``2^-40 A`` keeps a factor of about 3 at k = 3, and since the tap count grows as k^2 while the mean
  weight does not fall, a factor of 2 as far as k = 8.  No case here goes beyond k = 4.

rms: with h that bound (``A = sum(w |v|) / min(W, 1)``; every term of ``sum(w v^2)`` is positive, so float64 keeps a relative 2^-47 of
the quotient and of its root, and the root is at most ``sqrt(n) <= 5`` times the mean of |v|):
``max(got - h, 0)^2 <= sum(w v^2) / sum(w) <= (got + h)^2``, decided in rationals, without a square root.

lanczos: ``|got - exact| <= 1/2 ulp32(got) + 2^-40 * B / min(|W|, 1)``,
``B = min(sum_kept(|v|) (1 + |exact|), (sum_kept(|v|) + n |exact|) / 16)`` over the n kept taps.  An implementation forms
``px = fl(pi x)``, ``|px| < 3 pi``, which is off by up to ``|px| 2^-53 + |x| 1.3e-16 < 2^-49.3`` ABSOLUTELY (pi itself is rounded);
``sin`` then returns the sine of that argument to about an ulp.  Near a zero of the sinc (x = 1, 2, 3) the numerator is therefore
known to 2^-48.5 absolutely, not relatively, and is divided by ``px px / 3 >= 3.2``; away from the zeros, and near x = 0 where the
denominator is small, the same errors are relative ones of a weight that is at most 1.  A 1-D weight is thus off by less than 2^-50
in absolute terms, by 2^-49 with the stretch's ``|f'| |x| 2^-52``, and a 2-D weight by ``e < 2^-48``.  Over the n kept taps
``sum(w v)`` is off by ``e sum_kept(|v|)`` and W by ``e n``; each product and addition rounds once, ``(n + 1) 2^-53`` relative to
``sum(|w| |v|) <= sum_kept(|v|)`` and to ``sum(|w|) <= n``; so ``sum(w v) / W`` is off by at most
``(e + (n + 1) 2^-53) (sum_kept(|v|) + n |exact|) / |W|``, and with ``n <= 18 x 18 = 324`` (k = 3) the factor is below 2^-44.5: the second
form of B, with a factor 1.4 in hand against the worst case and some 25 against the typical one (the mean |w| of a stretched
lanczos is 0.04, not 1).  The first form is the bar this project set itself from the float64 restatement's measured margin; it
follows from the same inequality where the kept samples' mean magnitude is at least 2^-8 (``n <= 256 sum_kept(|v|)``), and the
smaller of the two is what holds here.  Both conditions -- ``n <= 324``, and the mean magnitude wherever more than one tap is kept
(one tap returns its sample whatever its weight) -- are CHECKED at every lanczos pixel; a case that misses one is mis-designed.
The weights' magnitudes do not enter the bound at all: it is absolute, and holds where ``sum(w v)`` cancels, which is where the
second form is the smaller.

No pixel is exempt
------------------
Four guards keep a case from exempting pixels; all are conditions on the case, checked on the exact side:
  1. a pixel whose exact ``|W|`` lies within 1e-9 of 1e-6 -- in the tap form also of 0.99999 or 1.00001 -- could legitimately fall on
     either side in float64: the case is MIS-DESIGNED and the enclosure functions raise for it instead of skipping the pixel;
  2. on the per-pixel path, a coordinate with ``s`` or ``s - 1/2`` within 1e-9 of an integer could have its ``floor`` moved by an
     implementation's 1e-10 nudge: mis-designed;
  3. a tap of a stretched axis with ``|(t - d) * scale|`` within 1e-9 of R but not equal to it: mis-designed.  (Equal to R happens on
     dyadic grids; every kernel here is continuous and zero at R, so a float64 argument 2^-52 off gives a weight below 2^-50 where
     the statement gives none, well inside the room derived above.);
  4. the float64 slack term may exceed ``1/2 ulp32(got)`` at no more than 1 % of a case's valued pixels: the enclosure functions return
     the count as ``n_slack_over`` and the tests assert the cap, so that an ill-conditioned case cannot make the enclosure
     meaningless.
"""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

METHODS = ('bilinear', 'cubic_spline', 'average')      # the three stated first; ALL_METHODS holds every one
TAP_METHODS = ('bilinear', 'cubic_spline')
CONV_R = dict(bilinear=1, cubic=2, cubic_spline=2, lanczos=3)
FOOTPRINT_METHODS = ('average', 'max', 'min', 'sum', 'rms', 'mode', 'med', 'q1', 'q3')
POINT_METHODS = ('nearest', 'bilinear', 'cubic', 'cubic_spline', 'lanczos')
EXACT_VALUED = ('nearest', 'max', 'min', 'mode', 'med', 'q1', 'q3')
ALL_METHODS = ('nearest', 'bilinear', 'cubic', 'cubic_spline', 'lanczos') + FOOTPRINT_METHODS
QUANTILE = dict(med=Fr(1, 2), q1=Fr(1, 4), q3=Fr(3, 4))
W_MIN, W_LO, W_HI = Fr(1, 10 ** 6), Fr(99999, 100000), Fr(100001, 100000)
NEAR = Fr(1, 10 ** 9)
STRETCH = 1 + Fr(1, 10 ** 9)
SLACK = Fr(1, 2 ** 40)
COORD_MAX = Fr(10 ** 15)     # a coordinate at or beyond this, or not finite, has no source
SLACK_OVER_CAP = 0.01
LANCZOS_DPS = 50
LANCZOS_MAX_TAPS = 324       # 18 x 18: k = 3 on both axes

# the up-sampling cases of bilinear / cubic_spline: (kx, ox, ky, oy) -> destination shape, over source()
UP_CASES = (((.375, -.25, .375, .125), (36, 58)), ((.5, 0., .25, -.5), (54, 42)), ((1., .5, 1., .5), (13, 21)),
            ((.75, -1.5, 1., .25), (14, 30)))
# the down-sampling cases of average, over source(AVG_SHAPE): aligned 2:1 with a clipped last row and column; 2.5:1 that starts
# outside on the left; 3:1 that starts outside at the top; 1.5 x 4 anisotropic; 2:1 whose first and last destination rows and
# columns lie wholly outside the plane, some by less than one source pixel
AVG_SHAPE = (29, 43)
DOWN_CASES = (((2., 0., 2., 0.), (15, 22)), ((2.5, -1.25, 2.5, .375), (12, 18)), ((3., .5, 3., -1.5), (10, 15)),
              ((1.5, .125, 4., -.25), (8, 29)), ((2., -2.5, 2., -2.5), (18, 25)))
# the stretched cases of the convolution form, over source(): 2:1 aligned; 2.5 x 1.5 that starts outside; one axis up and one down
# (both take the convolution form, the up-sampled one un-stretched); unit scale (cubic and lanczos only differ from the tap form);
# 1.75 x 2.25, where R k is no whole number for any of the radii, so that a radius rounded down loses a tap of every kernel
STRETCH_CASES = (((2., 0., 2., 0.), (7, 11)), ((2.5, -1.25, 1.5, .375), (9, 8)), ((.75, -1.5, 3., .25), (5, 30)),
                 ((1., .5, 1., .5), (13, 21)), ((1.75, .125, 2.25, -.375), (6, 12)))
# an up-sampling footprint case over source(AVG_SHAPE): every footprint lies within one or two source pixels
UP_FOOT_CASE = ((.5, 0., .5, .25), (20, 30))


def source(shape=(13, 21), nodata=np.nan):
    """ N(0.2, 1) float32 with a nodata block, 5 % scattered nodata and a nodata run in the first row. """
    rng = np.random.default_rng(20240607)
    src = rng.normal(0.2, 1., shape).astype(np.float32)
    holes = rng.random(shape) < 0.05
    src[4:7, 5:9] = np.nan
    src[holes] = np.nan
    src[0, :3] = np.nan
    if nodata is None:
        raise ValueError('the exact cases need a nodata value')
    if not np.isnan(nodata):
        assert not (src == np.float32(nodata)).any()
        src = np.where(np.isnan(src), np.float32(nodata), src)
    return src


def source_with_ties(shape=AVG_SHAPE, nodata=np.nan):
    """ source() with 30 % of its pixels at 0.5 and 15 % at -1.25, the nodata pattern kept: the rank-order methods get ties to break and
    `mode` something to decide.  No pixel is zero. """
    src = source(shape, np.nan)
    rng = np.random.default_rng(20240608)
    u = rng.random(shape)
    hole = np.isnan(src)
    src[u < 0.30] = np.float32(0.5)
    src[(u >= 0.30) & (u < 0.45)] = np.float32(-1.25)
    src[hole] = np.nan
    assert not (src == 0).any()
    if not np.isnan(nodata):
        assert not (src == np.float32(nodata)).any()
        src = np.where(np.isnan(src), np.float32(nodata), src)
    return src


def scaled_cases(method):
    """ every dyadic case `method` is held on: [(mapping, destination shape, source builder taking the nodata value)] -- the point
    methods on the up-sampling cases and, those with a convolution form, on the stretched cases over source() and on the
    down-sampling cases over source(AVG_SHAPE); nearest and the footprint methods on the down-sampling and the up-sampling
    footprint case over source_with_ties() """
    plain, ties = functools.partial(source, (13, 21)), functools.partial(source_with_ties, AVG_SHAPE)
    out = []
    if method in POINT_METHODS:
        out += [(m, s, plain) for m, s in UP_CASES]
    if method in CONV_R:
        out += [(m, s, plain) for m, s in STRETCH_CASES] + [(m, s, functools.partial(source, AVG_SHAPE)) for m, s in DOWN_CASES]
    if method in FOOTPRINT_METHODS + ('nearest',):
        out += [(m, s, ties) for m, s in DOWN_CASES + (UP_FOOT_CASE,)]
    return out


def _dyadic(mapping):
    out = tuple(Fr(float(v)) for v in mapping)
    for v in out:
        if (v * 8).denominator != 1:
            raise ValueError(f'mapping {mapping} is not dyadic: every term must be a multiple of 1/8')
    if out[0] <= 0 or out[2] <= 0:
        raise ValueError('flipped or degenerate mapping')
    return out


def _floor(x: Fr) -> int:
    return x.numerator // x.denominator


def _ceil(x: Fr) -> int:
    return -((-x.numerator) // x.denominator)


def uses_conv(method, kx, ky) -> bool:
    """ whether GDAL takes the convolution form (GWKResample) for this method at these steps """
    return method in ('cubic', 'lanczos') or (method in TAP_METHODS and (Fr(kx) > STRETCH or Fr(ky) > STRETCH))


# -- the kernels -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1 << 16)
def _lanczos(x: Fr) -> Fr:
    import mpmath as mp
    if x == 0:
        return Fr(1)
    with mp.workdps(LANCZOS_DPS):
        px = mp.pi * mp.mpf(x.numerator) / mp.mpf(x.denominator)
        w = mp.sin(px) * mp.sin(px / 3) / (px * px / 3)
        sign, man, exp, _ = w._mpf_
    return Fr(-int(man) if sign else int(man)) * Fr(2) ** int(exp)


def kernel(method: str, x: Fr) -> Fr:
    """ f(x) of the convolution form; 0 at and beyond the radius """
    ax = abs(x)
    if ax >= CONV_R[method]:
        return Fr(0)
    if method == 'lanczos' and ax.denominator == 1:
        return Fr(1 if ax == 0 else 0)      # sinc at an integer: exactly so
    if method == 'bilinear':
        return 1 - ax
    if method == 'cubic':
        if ax <= 1:
            return Fr(3, 2) * ax ** 3 - Fr(5, 2) * ax ** 2 + 1
        return -Fr(1, 2) * ax ** 3 + Fr(5, 2) * ax ** 2 - 4 * ax + 2
    if method == 'cubic_spline':
        if ax <= 1:
            return Fr(2, 3) - ax ** 2 + ax ** 3 / 2
        return (2 - ax) ** 3 / 6
    return _lanczos(ax)


def _axis_taps(method, s: Fr):
    """ the tap form on one axis: (centre pixel, [(source index, weight)]) before clipping to the plane """
    i0 = _floor(s - Fr(1, 2))
    d = s - Fr(1, 2) - i0
    if method == 'bilinear':
        taps = [(i0, 1 - d), (i0 + 1, d)]
    else:
        a, b, c = 1 - d, 2 - d, 3 - d
        taps = [(i0 - 1, a ** 3 / 6), (i0, (b ** 3 - 4 * a ** 3) / 6), (i0 + 1, (c ** 3 - 4 * b ** 3 + 6 * a ** 3) / 6),
                (i0 + 2, d ** 3 / 6)]
        assert sum(w for _, w in taps) == 1
    return _floor(s), taps


def _axis_conv(method, s: Fr, k: Fr, notes: list):
    """ the convolution form on one axis: (centre pixel, [(source index, weight)]): every tap inside the support, found by the weight's
    own cut-off ``|x| < R``; guard 3 is noted into `notes` """
    R = CONV_R[method]
    scale = min(Fr(1), 1 / k)
    i0 = _floor(s - Fr(1, 2))
    d = s - Fr(1, 2) - i0
    ts = []
    t = 0
    while (t - d) * scale < R:          # t - d > -1 >= -R / scale: the tap is inside on the other side as well
        ts.append(t)
        t += 1
    hi_out = t
    t = -1
    while (d - t) * scale < R:
        ts.append(t)
        t -= 1
    lo_out = t
    if scale < 1:
        for t in (hi_out - 1, hi_out, lo_out + 1, lo_out):
            gap = abs(abs((t - d) * scale) - R)
            if 0 < gap < NEAR:
                notes.append(f'tap {t} of s = {float(s)!r} lies {float(gap):.1e} from the support edge')
    return _floor(s), [(i0 + t, kernel(method, (t - d) * scale)) for t in sorted(ts)]


def _line_weights(method, k, o, n_dst):
    """ per destination index: (centre pixel, [(source index, weight)]) along one axis, before clipping to the plane """
    return [_axis_taps(method, k * (j + Fr(1, 2)) + o) for j in range(n_dst)]


def _line_conv(method, k, o, n_dst, notes):
    return [_axis_conv(method, k * (j + Fr(1, 2)) + o, k, notes) for j in range(n_dst)]


def _line_overlaps(k, o, n_dst, n_src):
    """ per destination index: [(source index, length it shares with the destination pixel's footprint clipped to [0, n_src])] """
    out = []
    for j in range(n_dst):
        lo, hi = max(k * j + o, Fr(0)), min(k * (j + 1) + o, Fr(n_src))
        taps = []
        p = _floor(lo) if lo < hi else 0
        while lo < hi and p < hi:
            share = min(Fr(p + 1), hi) - max(Fr(p), lo)
            if share > 0:
                taps.append((p, share))
            p += 1
        out.append((None, taps))
    return out


# -- one destination pixel -----------------------------------------------------------------------------------------------------------
def _weighted(vals, sh, sw, ytaps, xtaps):
    """ -> sum(w v), sum(|w| |v|), sum(w), sum(|v|), n over the taps that are inside the plane, valid and of non-zero weight """
    acc = mag = w_all = v_all = Fr(0)
    n = 0
    for a, wy in ytaps:
        if not 0 <= a < sh or wy == 0:
            continue
        for b, wx in xtaps:
            if not 0 <= b < sw or wx == 0 or vals[a][b] is None:
                continue
            w = wx * wy
            acc += w * vals[a][b]
            mag += abs(w) * abs(vals[a][b])
            w_all += w
            v_all += abs(vals[a][b])
            n += 1
    return acc, mag, w_all, v_all, n


def _point_pixel(method, conv, vals, sh, sw, cy, ytaps, cx, xtaps, notes, where):
    """ bilinear / cubic / cubic_spline / lanczos at one destination pixel -> (value, A, W) """
    if not (0 <= cy < sh and 0 <= cx < sw and vals[cy][cx] is not None):
        return None, None, None
    acc, mag, w_all, v_all, n = _weighted(vals, sh, sw, ytaps, xtaps)
    if not conv:
        if w_all < W_MIN:
            return None, None, w_all
        return (acc if W_LO <= w_all <= W_HI else acc / w_all), mag / min(w_all, Fr(1)), w_all
    if abs(w_all) < W_MIN:
        return None, None, w_all
    value = acc / w_all
    if method != 'lanczos':
        return value, mag / min(abs(w_all), Fr(1)), w_all
    if n > LANCZOS_MAX_TAPS or (n > 1 and v_all * 256 < n):
        notes.append(f'{where}: a lanczos pixel keeps {n} samples of mean magnitude {float(v_all / n):.2e}: the bound is not derived for it')
    return value, min(v_all * (1 + abs(value)), (v_all + n * abs(value)) / 16) / min(abs(w_all), Fr(1)), w_all


def _footprint_pixel(method, vals, ytaps, xtaps):
    """ a footprint method at one destination pixel -> (value, A, W); rms: value is the SQUARE, sum(w v^2) / sum(w) """
    pix = [(wy, wx, vals[a][b]) for a, wy in ytaps for b, wx in xtaps if vals[a][b] is not None]     # row-major
    if not pix:
        return None, None, Fr(0)
    vs = [v for _, _, v in pix]
    if method in ('max', 'min'):
        return (max(vs) if method == 'max' else min(vs)), Fr(0), Fr(len(vs))
    if method == 'mode':
        counts, best, best_n = {}, None, 0
        for v in vs:
            counts[v] = counts.get(v, 0) + 1
            if counts[v] > best_n:
                best, best_n = v, counts[v]
        return best, Fr(0), Fr(len(vs))
    if method in QUANTILE:
        return sorted(vs)[max(0, _ceil(QUANTILE[method] * len(vs) - 1))], Fr(0), Fr(len(vs))
    one_y, one_x = len(ytaps) == 1, len(xtaps) == 1
    if method == 'average':
        one_y = one_x = False          # a common factor of all the weights: the mean does not see it
    acc = mag = w_all = Fr(0)
    for wy, wx, v in pix:
        w = (Fr(1) if one_y else wy) * (Fr(1) if one_x else wx)
        acc += w * (v * v if method == 'rms' else v)
        mag += w * abs(v)
        w_all += w
    if method == 'sum':
        return acc, mag, w_all
    return acc / w_all, mag / min(w_all, Fr(1)), w_all


def _valid_samples(src, nodata):
    """ -> (the float32 samples with the invalid ones zeroed, the validity mask) as bytes: what a result is cached on, so that the NaN
    and the numeric-nodata variant of one source share it """
    src = np.ascontiguousarray(src, np.float32)
    mask = ~np.isnan(src)
    if nodata is not None and not np.isnan(nodata):
        mask &= src != np.float32(nodata)
    return np.where(mask, src, np.float32(0)).tobytes(), mask.tobytes(), src.shape


def _values(val_bytes, mask_bytes, shape):
    val, mask = np.frombuffer(val_bytes, np.float32).reshape(shape), np.frombuffer(mask_bytes, bool).reshape(shape)
    return [[Fr(float(val[a, b])) if mask[a, b] else None for b in range(shape[1])] for a in range(shape[0])]


# -- dyadic mappings -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_cached(val_bytes, mask_bytes, shape, mapping, dst_shape, method):
    sh, sw = shape
    dh, dw = dst_shape
    kx, ox, ky, oy = _dyadic(mapping)
    vals = _values(val_bytes, mask_bytes, shape)
    notes = []
    conv = uses_conv(method, kx, ky)
    if method in FOOTPRINT_METHODS:
        rows, cols = _line_overlaps(ky, oy, dh, sh), _line_overlaps(kx, ox, dw, sw)
    elif conv:
        rows, cols = _line_conv(method, ky, oy, dh, notes), _line_conv(method, kx, ox, dw, notes)
    elif method in TAP_METHODS:
        rows, cols = _line_weights(method, ky, oy, dh), _line_weights(method, kx, ox, dw)
    elif method == 'nearest':
        rows = [(_floor(ky * (i + Fr(1, 2)) + oy), None) for i in range(dh)]
        cols = [(_floor(kx * (j + Fr(1, 2)) + ox), None) for j in range(dw)]
    else:
        raise NotImplementedError(method)
    value = np.empty((dh, dw), object)
    amp = np.empty((dh, dw), object)
    wsum = np.empty((dh, dw), object)
    for i, (cy, ytaps) in enumerate(rows):
        for j, (cx, xtaps) in enumerate(cols):
            if method in FOOTPRINT_METHODS:
                value[i, j], amp[i, j], wsum[i, j] = _footprint_pixel(method, vals, ytaps, xtaps)
            elif method == 'nearest':
                ok = 0 <= cy < sh and 0 <= cx < sw and vals[cy][cx] is not None
                value[i, j], amp[i, j], wsum[i, j] = (vals[cy][cx], Fr(0), Fr(1)) if ok else (None, None, None)
            else:
                value[i, j], amp[i, j], wsum[i, j] = _point_pixel(method, conv, vals, sh, sw, cy, ytaps, cx, xtaps, notes, (i, j))
    return value, amp, wsum, ('conv' if conv else 'tap' if method in TAP_METHODS else 'none'), tuple(notes)


def _exact_full(src, nodata, mapping, dst_shape, method):
    return _exact_cached(*_valid_samples(src, nodata), tuple(float(v) for v in mapping), tuple(int(v) for v in dst_shape), method)


def exact(src: np.ndarray, nodata: float, mapping, dst_shape, method: str):
    """ -> (value, A, W): object arrays of Fraction on the destination grid; value and A are None where the rule gives nodata, W is
    None where the centre rule already did.  `rms`: value is the square, ``sum(w v^2) / sum(w)``.  Results are cached: do not write
    into them. """
    return _exact_full(src, nodata, mapping, dst_shape, method)[:3]


# -- per-pixel coordinates -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _exact_at_cached(val_bytes, mask_bytes, shape, sx_bytes, sy_bytes, dst_shape, kx, ky, method):
    if method not in POINT_METHODS:
        raise NotImplementedError(f'{method} on per-pixel coordinates')
    sx, sy = (np.frombuffer(b, np.float64).reshape(dst_shape) for b in (sx_bytes, sy_bytes))
    sh, sw = shape
    dh, dw = dst_shape
    vals = _values(val_bytes, mask_bytes, shape)
    fkx, fky = Fr(kx), Fr(ky)
    if fkx <= 0 or fky <= 0:
        raise ValueError('flipped or degenerate steps')
    conv = uses_conv(method, fkx, fky)
    notes = []
    value = np.empty((dh, dw), object)
    amp = np.empty((dh, dw), object)
    wsum = np.empty((dh, dw), object)
    half = Fr(1, 2)
    for i in range(dh):
        for j in range(dw):
            value[i, j] = amp[i, j] = wsum[i, j] = None
            if not (math.isfinite(sx[i, j]) and math.isfinite(sy[i, j])):
                continue
            x, y = Fr(float(sx[i, j])), Fr(float(sy[i, j]))
            if abs(x) >= COORD_MAX or abs(y) >= COORD_MAX:
                continue
            if not (-2 < x < sw + 2 and -2 < y < sh + 2):
                continue      # the centre pixel lies outside the plane by more than any nudge could mend
            for s in (x, y, x - half, y - half):
                if abs(s - round(s)) < NEAR:
                    notes.append(f'({i}, {j}): coordinate {float(s)!r} lies within 1e-9 of an integer')
            cx, cy = _floor(x), _floor(y)
            if method == 'nearest':
                if 0 <= cy < sh and 0 <= cx < sw and vals[cy][cx] is not None:
                    value[i, j], amp[i, j], wsum[i, j] = vals[cy][cx], Fr(0), Fr(1)
                continue
            if not (0 <= cy < sh and 0 <= cx < sw and vals[cy][cx] is not None):
                continue
            if conv:
                (_, ytaps), (_, xtaps) = _axis_conv(method, y, fky, notes), _axis_conv(method, x, fkx, notes)
            else:
                (_, ytaps), (_, xtaps) = _axis_taps(method, y), _axis_taps(method, x)
            value[i, j], amp[i, j], wsum[i, j] = _point_pixel(method, conv, vals, sh, sw, cy, ytaps, cx, xtaps, notes, (i, j))
    return value, amp, wsum, ('conv' if conv else 'tap' if method in TAP_METHODS else 'none'), tuple(notes)


def _exact_at_full(src, nodata, sx, sy, kx, ky, method):
    sx, sy = np.ascontiguousarray(sx, np.float64), np.ascontiguousarray(sy, np.float64)
    assert sx.shape == sy.shape and sx.ndim == 2
    return _exact_at_cached(*_valid_samples(src, nodata), sx.tobytes(), sy.tobytes(), sx.shape, float(kx), float(ky), method)


def exact_at(src: np.ndarray, nodata, sx: np.ndarray, sy: np.ndarray, kx: float, ky: float, method: str):
    """ nearest / bilinear / cubic / cubic_spline / lanczos at the continuous source coordinates ``sx, sy`` (float64 planes of the
    destination's shape, taken as the exact rationals they are); ``kx, ky`` choose the form and the stretch.  -> (value, A, W) as
    `exact`.  A coordinate that is not finite, or at or beyond 1e15, has no source.  Cached on the valid samples: do not write into
    the result. """
    return _exact_at_full(src, nodata, sx, sy, kx, ky, method)[:3]


# -- the enclosure -----------------------------------------------------------------------------------------------------------------
def _sqrt_fr(q: Fr) -> Fr:
    import mpmath as mp
    with mp.workdps(LANCZOS_DPS):
        r = mp.sqrt(mp.mpf(q.numerator) / mp.mpf(q.denominator))
        sign, man, exp, _ = r._mpf_
    return Fr(int(man)) * Fr(2) ** int(exp)


def _enclose(got, full, method, fill, what):
    value, amp, wsum, form, notes = full
    is_fill = np.isnan(got) if np.isnan(fill) else got == np.float32(fill)
    near, pattern, outside, worst, used, n_over = list(notes), [], [], Fr(0), Fr(0), 0
    thresholds = (W_MIN, W_LO, W_HI) if form == 'tap' else (W_MIN,) if form == 'conv' else ()
    for i in range(got.shape[0]):
        for j in range(got.shape[1]):
            w = wsum[i, j]
            if w is not None and any(abs(abs(w) - t) < NEAR for t in thresholds):
                near.append((i, j, float(w)))
            if (value[i, j] is None) != bool(is_fill[i, j]):
                pattern.append((i, j, float(got[i, j]), None if value[i, j] is None else float(value[i, j])))
                continue
            if value[i, j] is None:
                continue
            g = Fr(float(got[i, j]))
            if method in EXACT_VALUED:
                if g != value[i, j]:
                    outside.append((i, j, float(got[i, j]), float(value[i, j]), float('inf')))
                    worst = max(worst, Fr(10 ** 9))
                continue
            half_ulp = Fr(float(np.spacing(np.abs(got[i, j])))) / 2
            slack = SLACK * amp[i, j]
            n_over += slack > half_ulp
            bound = half_ulp + slack
            if method == 'rms':
                ok = max(g - bound, Fr(0)) ** 2 <= value[i, j] <= (g + bound) ** 2
                err = abs(g - _sqrt_fr(value[i, j]))
            else:
                err = abs(g - value[i, j])
                ok = err <= bound
            worst = max(worst, err / bound)
            if slack > 0:
                used = max(used, (err - half_ulp) / slack)
            if not ok:
                outside.append((i, j, float(got[i, j]), float(value[i, j]), float(err / bound)))
    if near:
        raise AssertionError(f'mis-designed case {method} {what}: {len(near)} pixels break a guard, the first {near[:5]}')
    return dict(pattern=pattern, value=outside, worst=float(worst), slack_used=float(used), n_valid=int(sum(v is not None for v in value.ravel())),
                n_slack_over=int(n_over))


def assert_held(res: dict, what: str, n_min: float):
    """ print the summary line of an enclosure result and assert all it must meet: no pattern or value failure, guard 4, and more
    than `n_min` valued pixels (a case cannot pass by being empty) """
    print(f'[exact] {what}: {res["n_valid"]} valued pixels, worst error {res["worst"]:.3f} of the bound ({res["slack_used"]:.4f} of the float64 slack used), {len(res["pattern"])} pattern and '
          f'{len(res["value"])} value failures, {res["n_slack_over"]} pixels whose slack exceeds half an ulp')
    assert not res['pattern'], f'{what}: nodata pattern departs from the rule at {res["pattern"][:5]}'
    assert not res['value'], f'{what}: outside the enclosure at {res["value"][:5]}'
    assert res['n_slack_over'] <= SLACK_OVER_CAP * res['n_valid'], f'{what}: ill-conditioned case, guard 4'
    assert res['n_valid'] > n_min, f'{what}: only {res["n_valid"]} valued pixels'


def enclosure_failures(got: np.ndarray, src: np.ndarray, nodata: float, mapping, dst_shape, method: str, fill=np.nan):
    """ Hold a float32 result to the exact statement.  -> dict(pattern=[...], value=[...], worst=<largest error in units of the
    bound>, n_valid, n_slack_over): the pixels whose nodata state differs from the rule's, those outside the enclosure (the
    exact-valued methods: those that differ at all), and the number of valued pixels whose float64 slack exceeds half an ulp
    (guard 4: the caller asserts ``n_slack_over <= SLACK_OVER_CAP * n_valid``).  Raises when the case breaks guard 1 or 3 (the case is
    mis-designed: no pixel may be exempt). """
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == tuple(dst_shape), (got.dtype, got.shape)
    return _enclose(got, _exact_full(src, nodata, mapping, dst_shape, method), method, fill, mapping)


def enclosure_failures_at(got: np.ndarray, src: np.ndarray, nodata, sx, sy, kx, ky, method: str, fill=np.nan):
    """ `enclosure_failures` on per-pixel coordinates; raises for guards 1, 2 and 3 """
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(sx), (got.dtype, got.shape)
    return _enclose(got, _exact_at_full(src, nodata, sx, sy, kx, ky, method), method, fill, f'steps ({kx}, {ky})')
