""" numpy restatement of the warp re-samplers (hk_warp.hip): nearest / bilinear / cubic / cubic_spline / lanczos on PER-PIXEL source
coordinates.

``oracle_np.reproject`` states GDAL's warp kernels for an affine mapping ``sx = kx * (j + .5) + ox``.  Across CRSs the only thing
that changes is where ``sx, sy`` come from; this module restates the same arithmetic, operation for operation, with the
coordinates handed in as planes.  It is held to the exact statement of tests/_resample_exact.py (rational arithmetic from GDAL's rule,
no formula shared) on turned grids whose coordinates are arbitrary doubles, all five methods, by
tests/test_resample_exact_cpu.py; tests/test_warp_reference_cpu.py pins it to the oracle bit for bit on affine planes.  The GPU tests
hold the kernels to the exact statement directly on small grids, and feed this module the device's own coordinate planes for the
bit-for-bit comparison at the large ones.  ``kx, ky`` (source pixels per destination pixel) pick the stretched kernels and scale
their support exactly as the oracle's mapping factors do. """
import math

import numpy as np

from oracle import oracle_np as onp

COORD_MAX = 1e15   # a coordinate at or beyond this, or NaN, is "no data" (hk_warp.hip WARP_COORD_MAX)
MODES = ('nearest', 'bilinear', 'cubic', 'cubic_spline', 'lanczos')


def warp_resample(src: np.ndarray, src_nodata, sx: np.ndarray, sy: np.ndarray, kx: float, ky: float, dst_nodata=np.nan,
                  resampling: str = 'bilinear') -> np.ndarray:
    """ One band (2-D float32) re-sampled at the continuous source pixel coordinates ``sx, sy`` (float64 planes of the
    destination's shape; integers = pixel edges). """
    if resampling not in MODES:
        raise NotImplementedError(resampling)
    sh, sw = src.shape
    dh, dw = sx.shape
    valid = onp.mask_of(src, src_nodata)
    srcd = src.astype(np.float64)
    out = np.zeros((dh, dw), np.float64)
    got = np.zeros((dh, dw), bool)
    stretched = kx > 1 + 1e-9 or ky > 1 + 1e-9
    conv = resampling in ('cubic', 'lanczos') or (resampling in ('bilinear', 'cubic_spline') and stretched)
    R = dict(bilinear=1, cubic=2, cubic_spline=2, lanczos=3).get(resampling, 0)
    xs = 1.0 / kx if kx > 1.0 else 1.0
    ys = 1.0 / ky if ky > 1.0 else 1.0
    rx = int(math.ceil(R / xs)) if xs < 1.0 else R
    ry = int(math.ceil(R / ys)) if ys < 1.0 else R
    taps = (0, 1) if resampling == 'bilinear' else (-1, 0, 1, 2)
    for i in range(dh):
        for j in range(dw):
            x, y = float(sx[i, j]), float(sy[i, j])
            if not (abs(x) < COORD_MAX and abs(y) < COORD_MAX):
                continue
            cx, cy = int(math.floor(x + 1e-10)), int(math.floor(y + 1e-10))
            if cx < 0 or cx >= sw or cy < 0 or cy >= sh or not valid[cy, cx]:
                continue   # the source pixel under the destination centre must be valid
            if resampling == 'nearest':
                out[i, j], got[i, j] = srcd[cy, cx], True
                continue
            ix, iy = int(math.floor(x - 0.5)), int(math.floor(y - 0.5))
            dx, dy = x - 0.5 - ix, y - 0.5 - iy
            acc = wacc = 0.0
            if conv:
                for tj in range(1 - ry, ry + 1):
                    a = iy + tj
                    if a < 0 or a >= sh:
                        continue
                    wy = onp._conv_weight(resampling, (tj - dy) * ys)
                    if wy == 0.0:
                        continue
                    for ti in range(1 - rx, rx + 1):
                        b = ix + ti
                        if b < 0 or b >= sw or not valid[a, b]:
                            continue
                        wgt = onp._conv_weight(resampling, (ti - dx) * xs) * wy
                        acc += srcd[a, b] * wgt
                        wacc += wgt
                if not abs(wacc) < 1e-6:
                    out[i, j], got[i, j] = acc / wacc, True
            else:
                wxs = (1 - dx, dx) if resampling == 'bilinear' else onp._bspline_weights(dx)
                wys = (1 - dy, dy) if resampling == 'bilinear' else onp._bspline_weights(dy)
                for tj, wyv in zip(taps, wys):
                    a = iy + tj
                    if a < 0 or a >= sh:
                        continue
                    for ti, wxv in zip(taps, wxs):
                        b = ix + ti
                        if b < 0 or b >= sw or not valid[a, b]:
                            continue
                        wgt = float(wxv) * float(wyv)
                        acc += srcd[a, b] * wgt
                        wacc += wgt
                if wacc < 1e-6:
                    continue
                out[i, j], got[i, j] = (acc / wacc if (wacc < 0.99999 or wacc > 1.00001) else acc), True
    res = out.astype(np.float32)
    res[~got] = 0 if dst_nodata is None else dst_nodata
    return res


def affine_planes(mapping, dst_shape):
    """ The coordinate planes of the oracle's affine mapping, formed as the oracle forms them. """
    kx, ox, ky, oy = mapping
    sx = np.array([[kx * (j + 0.5) + ox for j in range(dst_shape[1])]] * dst_shape[0], np.float64)
    sy = np.array([[ky * (i + 0.5) + oy] * dst_shape[1] for i in range(dst_shape[0])], np.float64)
    return sx, sy
