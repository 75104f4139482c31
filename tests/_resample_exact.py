""" An exact statement of three of GDAL's warp re-samplers -- `bilinear`, `cubic_spline` (up-sampling) and `average` -- in
``fractions.Fraction`` arithmetic on the float32 inputs, and the enclosure a float64-accumulating implementation must meet.

Written from GDAL's published rule (gdal/alg/gdalwarpkernel.cpp), NOT from hk_resample.hip or oracle/oracle_np.py: those two share
one float64 formula, operation for operation, so a mistake in a weight or in the renormalisation rule that both make passes every
bit-for-bit comparison between them.  This module shares nothing with them but the mapping convention
``src = k * dst + o`` on continuous coordinates (integers = pixel edges, pixel p covers [p, p + 1)).

Only DYADIC mappings are accepted: ``k`` and ``o`` multiples of 1/8.  Then ``k * (j + 1/2) + o`` and ``k * j + o`` are exact in
double as well, every ``floor`` in an implementation sees the true value, and the ``1e-10`` nudges implementations add before
``floor`` / ``ceil`` can move nothing (the nearest other multiple of 1/16 is 6e-2 away).

The rules
---------
bilinear / cubic_spline, destination pixel (i, j), ``s = k * (j + 1/2) + o`` per axis:
  * the source pixel ``floor(s)`` under the destination centre must be inside the plane and valid, else nodata;
  * ``i0 = floor(s - 1/2)``, ``d = s - 1/2 - i0``; taps ``i0 + t``, t = 0, 1 (bilinear) or -1, 0, 1, 2 (cubic_spline);
  * weights: bilinear ``1 - d, d``; cubic B-spline ``(1-d)^3/6, ((2-d)^3 - 4(1-d)^3)/6, ((3-d)^3 - 4(2-d)^3 + 6(1-d)^3)/6, d^3/6``;
    the 2-D weight is the product of the two axes' weights;
  * taps outside the plane or invalid are dropped; ``W`` = sum of the kept weights; ``W < 1e-6``: nodata;
  * value = ``sum(w v)`` when ``0.99999 <= W <= 1.00001``, else ``sum(w v) / W``.
average, destination pixel (i, j): its footprint ``[k j + o, k (j + 1) + o]`` per axis, clipped to the plane; the value is the mean
  of the valid source pixels weighted by the area each shares with the clipped footprint; no valid pixel with a positive share:
  nodata.

The enclosure
-------------
``|got - exact| <= 1/2 ulp32(got) + 2^-40 * A``, ``A = sum(|w| |v|) / min(W, 1)``.
The first term is the one rounding of the float64 result to float32.  The second bounds what float64 evaluation can lose:
  * a 1-D B-spline weight is made from about 10 operations on operands of magnitude <= 27 (``(3 - d)^3``); the absolute error of the
    two middle weights is below ``10 * 27 * 2^-53 / 6 < 2^-47``, and as they are >= 1/6 their relative error is below ``2^-44``; the two
    outer weights are a cube and a division, relative error below ``2^-50``.  Bilinear weights (one subtraction) and the overlap
    weights of `average` (two subtractions) do better;
  * a 2-D weight is one more product: relative error below ``2^-43``;
  * the sum runs over at most 16 products (`average` at the ratios tested here: at most 5 x 5 = 25); each product and each addition
    rounds once, which adds less than ``27 * 2^-53 < 2^-48`` relative to ``sum(|w| |v|)``; the same holds for ``W``, whose terms are
    all positive;
  * the division by ``W`` carries W's relative error (< 2^-43) over and rounds once more.
Together: below ``2^-42 * sum(|w| |v|) / W``, so ``2^-40 * A`` has a factor 4 to spare and is still 2^-16 of a float32 ulp of a
well-conditioned pixel: a wrong tap, weight or rule cannot hide in it.

No pixel is exempt.  The three thresholds of the rule are decimal, not dyadic: a pixel whose exact ``W`` lies within 1e-9 of one could
legitimately fall on either side in float64, so a case that contains one is MIS-DESIGNED and ``enclosure_failures`` raises for it
instead of skipping the pixel.
"""
import functools
from fractions import Fraction as Fr

import numpy as np

METHODS = ('bilinear', 'cubic_spline', 'average')
W_MIN, W_LO, W_HI = Fr(1, 10 ** 6), Fr(99999, 100000), Fr(100001, 100000)
NEAR = Fr(1, 10 ** 9)
SLACK = Fr(1, 2 ** 40)

# the up-sampling cases of bilinear / cubic_spline: (kx, ox, ky, oy) -> destination shape, over source()
UP_CASES = (((.375, -.25, .375, .125), (36, 58)), ((.5, 0., .25, -.5), (54, 42)), ((1., .5, 1., .5), (13, 21)),
            ((.75, -1.5, 1., .25), (14, 30)))
# the down-sampling cases of average, over source(AVG_SHAPE): aligned 2:1 with a clipped last row and column; 2.5:1 that starts
# outside on the left; 3:1 that starts outside at the top; 1.5 x 4 anisotropic; 2:1 whose first and last destination rows and
# columns lie wholly outside the plane, some by less than one source pixel
AVG_SHAPE = (29, 43)
DOWN_CASES = (((2., 0., 2., 0.), (15, 22)), ((2.5, -1.25, 2.5, .375), (12, 18)), ((3., .5, 3., -1.5), (10, 15)),
              ((1.5, .125, 4., -.25), (8, 29)), ((2., -2.5, 2., -2.5), (18, 25)))


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


def _line_weights(method, k, o, n_dst):
    """ per destination index: (centre pixel, [(source index, weight)]) along one axis, before clipping to the plane """
    out = []
    for j in range(n_dst):
        s = k * (j + Fr(1, 2)) + o
        i0 = _floor(s - Fr(1, 2))
        d = s - Fr(1, 2) - i0
        if method == 'bilinear':
            taps = [(i0, 1 - d), (i0 + 1, d)]
        else:
            a, b, c = 1 - d, 2 - d, 3 - d
            taps = [(i0 - 1, a ** 3 / 6), (i0, (b ** 3 - 4 * a ** 3) / 6), (i0 + 1, (c ** 3 - 4 * b ** 3 + 6 * a ** 3) / 6),
                    (i0 + 2, d ** 3 / 6)]
            assert sum(w for _, w in taps) == 1
        out.append((_floor(s), taps))
    return out


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


@functools.lru_cache(maxsize=None)
def _exact_cached(src_bytes, shape, nodata_key, mapping, dst_shape, method):
    src = np.frombuffer(src_bytes, np.float32).reshape(shape)
    nodata = float('nan') if nodata_key == 'nan' else float(nodata_key)
    valid = ~np.isnan(src) if np.isnan(nodata) else (src != np.float32(nodata)) & ~np.isnan(src)
    sh, sw = shape
    dh, dw = dst_shape
    kx, ox, ky, oy = _dyadic(mapping)
    vals = [[Fr(float(src[a, b])) if valid[a, b] else None for b in range(sw)] for a in range(sh)]
    if method == 'average':
        rows, cols = _line_overlaps(ky, oy, dh, sh), _line_overlaps(kx, ox, dw, sw)
    elif method in ('bilinear', 'cubic_spline'):
        rows, cols = _line_weights(method, ky, oy, dh), _line_weights(method, kx, ox, dw)
    else:
        raise NotImplementedError(method)
    value = np.empty((dh, dw), object)
    amp = np.empty((dh, dw), object)
    wsum = np.empty((dh, dw), object)
    for i, (cy, ytaps) in enumerate(rows):
        for j, (cx, xtaps) in enumerate(cols):
            value[i, j] = amp[i, j] = wsum[i, j] = None
            if method != 'average' and not (0 <= cy < sh and 0 <= cx < sw and valid[cy, cx]):
                continue
            acc = mag = w_all = Fr(0)
            for a, wy in ytaps:
                if not 0 <= a < sh:
                    continue
                for b, wx in xtaps:
                    if not 0 <= b < sw or vals[a][b] is None:
                        continue
                    w = wx * wy
                    acc += w * vals[a][b]
                    mag += abs(w) * abs(vals[a][b])
                    w_all += w
            wsum[i, j] = w_all
            if method == 'average':
                if w_all > 0:
                    value[i, j], amp[i, j] = acc / w_all, mag / min(w_all, Fr(1))
                continue
            if w_all < W_MIN:
                continue
            value[i, j] = acc if W_LO <= w_all <= W_HI else acc / w_all
            amp[i, j] = mag / min(w_all, Fr(1))
    return value, amp, wsum


def exact(src: np.ndarray, nodata: float, mapping, dst_shape, method: str):
    """ -> (value, A, W): object arrays of Fraction on the destination grid; value and A are None where the rule gives nodata, W is
    None where the centre rule already did.  Results are cached: do not write into them. """
    src = np.ascontiguousarray(src, np.float32)
    key = 'nan' if np.isnan(nodata) else repr(float(nodata))
    return _exact_cached(src.tobytes(), src.shape, key, tuple(float(v) for v in mapping), tuple(int(v) for v in dst_shape), method)


def enclosure_failures(got: np.ndarray, src: np.ndarray, nodata: float, mapping, dst_shape, method: str, fill=np.nan):
    """ Hold a float32 result to the exact statement.  -> dict(pattern=[...], value=[...], worst=<largest error in units of the
    bound>): the pixels whose nodata state differs from the rule's, and those outside the enclosure.  Raises when the case holds a
    pixel within 1e-9 of a threshold of the rule (the case is mis-designed: no pixel may be exempt). """
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == tuple(dst_shape), (got.dtype, got.shape)
    value, amp, wsum = exact(src, nodata, mapping, dst_shape, method)
    is_fill = np.isnan(got) if np.isnan(fill) else got == np.float32(fill)
    near, pattern, outside, worst = [], [], [], Fr(0)
    for i in range(got.shape[0]):
        for j in range(got.shape[1]):
            w = wsum[i, j]
            if w is not None and method != 'average' and any(abs(w - t) < NEAR for t in (W_MIN, W_LO, W_HI)):
                near.append((i, j, float(w)))
            if (value[i, j] is None) != bool(is_fill[i, j]):
                pattern.append((i, j, float(got[i, j]), None if value[i, j] is None else float(value[i, j])))
                continue
            if value[i, j] is None:
                continue
            g = Fr(float(got[i, j]))
            bound = Fr(float(np.spacing(np.abs(got[i, j])))) / 2 + SLACK * amp[i, j]
            err = abs(g - value[i, j])
            worst = max(worst, err / bound)
            if err > bound:
                outside.append((i, j, float(got[i, j]), float(value[i, j]), float(err / bound)))
    if near:
        raise AssertionError(f'mis-designed case {method} {mapping}: accumulated weights within 1e-9 of a threshold at {near[:5]}')
    return dict(pattern=pattern, value=outside, worst=float(worst), n_valid=int(sum(v is not None for v in value.ravel())))
