""" The exact expectations of the internal-mask tests, in numpy (no library code): the average overviews of a raster under a
per-dataset validity mask, and the inputs the GPU and CPU tests share.

THE RULE (include/homonim_hk.h, hk_overviews_valid_dev).  Level m has shape (ceil(h / 2^m), ceil(w / 2^m)).  Its pixel
(i, j) takes the pixels (2i..2i+1, 2j..2j+1) of level m - 1 that lie inside that level AND are valid there.  Float types: the valid
values summed as float64 in row-major order starting from +0, divided by their count in float64, rounded once to the type.  Integer
types: floor((2 S + n) / (2 n)) of the exact sum S of the n valid values.  A cell without a valid pixel gives 0 (integers) or NaN
(floats) and is invalid on level m; every other cell is valid there (255).  A NaN under a valid bit is data and propagates.  Level
m + 1 is formed from level m's values and validity as stored. """
import numpy as np


def _quads(plane: np.ndarray, fill):
    """ the four pixels (row-major) of every 2 x 2 cell of a 2-D plane padded to even sizes with ``fill`` """
    h, w = plane.shape
    p = np.full((h + h % 2, w + w % 2), fill, plane.dtype)
    p[:h, :w] = plane
    return p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]


def masked_overview_levels(array: np.ndarray, valid: np.ndarray, n_levels: int):
    """ -> (levels, level_valids) of a (bands, h, w) or (h, w) raster under the (h, w) validity ``valid`` (valid where not 0):
    levels[m - 1] of the raster's rank and dtype, level_valids[m - 1] (h_m, w_m) uint8, 255 / 0. """
    a = np.asarray(array)
    squeeze = a.ndim == 2
    cur = a[None] if squeeze else a
    v = np.asarray(valid) != 0
    assert v.shape == cur.shape[1:]
    levels, valids = [], []
    for _ in range(n_levels):
        m = _quads(v, False)
        n = sum(x.astype(np.int64) for x in m)
        out = []
        for band in cur:
            q = _quads(band, 0)
            if band.dtype.kind == 'f':
                s = np.zeros(n.shape, np.float64)
                for x, ok in zip(q, m):                      # row-major order; a masked pixel adds +0
                    s = s + np.where(ok, x.astype(np.float64), 0.0)
                with np.errstate(invalid='ignore', divide='ignore'):
                    lv = np.where(n > 0, s / n, np.nan).astype(band.dtype)
            else:
                s = np.zeros(n.shape, np.int64)
                for x, ok in zip(q, m):
                    s = s + np.where(ok, x.astype(np.int64), 0)
                lv = np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0).astype(band.dtype)   # // floors
            out.append(lv)
        cur, v = np.stack(out), n > 0
        levels.append(cur[0] if squeeze else cur)
        valids.append(v.astype(np.uint8) * np.uint8(255))
    return levels, valids


def masked_overview_levels_loop(array: np.ndarray, valid: np.ndarray, n_levels: int):
    """ the same, cell by cell in plain Python on a single (h, w) plane: what ``masked_overview_levels`` is checked against """
    cur, v = np.asarray(array), np.asarray(valid) != 0
    levels, valids = [], []
    for _ in range(n_levels):
        h, w = cur.shape
        oh, ow = (h + 1) // 2, (w + 1) // 2
        lv, ok = np.zeros((oh, ow), cur.dtype), np.zeros((oh, ow), bool)
        for i in range(oh):
            for j in range(ow):
                vals = [cur[y, x] for y in (2 * i, 2 * i + 1) for x in (2 * j, 2 * j + 1) if y < h and x < w and v[y, x]]
                ok[i, j] = bool(vals)
                if cur.dtype.kind == 'f':
                    s = 0.0
                    for x in vals:
                        s += float(x)
                    lv[i, j] = cur.dtype.type(s / len(vals)) if vals else np.nan
                else:
                    s = sum(int(x) for x in vals)
                    lv[i, j] = (2 * s + len(vals)) // (2 * len(vals)) if vals else 0
        cur, v = lv, ok
        levels.append(lv)
        valids.append(ok.astype(np.uint8) * np.uint8(255))
    return levels, valids


def same_bits(got: np.ndarray, exp: np.ndarray) -> bool:
    """ equal shape, dtype and bytes, except that every NaN equals every NaN """
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False
    if got.dtype.kind != 'f':
        return bool((got == exp).all())
    return bool((((got == exp) & (np.signbit(got) == np.signbit(exp))) | ((got != got) & (exp != exp))).all())


def overview_case(dtype, shape, seed: int, bands: int = 2):
    """ A (bands, h, w) raster of ``dtype`` and its (h, w) uint8 validity for the overview tests: a quarter of the pixels invalid at
    random, an all-invalid 2 x 2 cell, a cell valid in one pixel only, an invalid last row and column, garbage under the invalid
    pixels and -- floats -- a NaN under a valid bit. """
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    h, w = shape
    if dt.kind == 'f':
        a = rng.normal(0.0, 1e4, (bands, h, w)).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, (bands, h, w), dtype=dt, endpoint=True)
    valid = (rng.random((h, w)) >= 0.25).astype(np.uint8) * np.uint8(255)
    valid[valid != 0] = rng.integers(1, 255, int((valid != 0).sum()), dtype=np.uint8, endpoint=True)   # valid is "not 0", not 255
    valid[-1, :] = 0
    valid[:, -1] = 0
    if h >= 4 and w >= 6:
        valid[0:2, 0:2] = 0                                   # a cell without a valid pixel
        valid[2:4, 2:4] = 0
        valid[3, 2] = 255                                     # a cell valid in one pixel only
        valid[0:2, 4:6] = 255                                 # a whole cell
        if dt.kind == 'f':
            a[:, 0, 4] = np.nan                               # a NaN under a valid bit is data
    return a, valid


def holed_source(shape, seed: int, bands: int = 1):
    """ A float32 (bands, h, w) source / reference pair on one grid: the source has a NaN frame and holes of 1, 2 and 9 pixels """
    rng = np.random.default_rng(seed)
    h, w = shape
    src = rng.uniform(20.0, 200.0, (bands, h, w)).astype(np.float32)
    ref = (1.1 * src + 5.0 + rng.normal(0, 2.0, src.shape)).astype(np.float32)
    src[:, :2, :] = src[:, -2:, :] = np.nan
    src[:, :, :3] = src[:, :, -3:] = np.nan
    cy, cx = h // 2, w // 2
    src[:, cy, cx] = np.nan                                   # 1 pixel
    src[:, cy // 2, cx // 2:cx // 2 + 2] = np.nan             # 2 pixels
    src[:, cy + cy // 2 - 1:cy + cy // 2 + 2, cx + cx // 2 - 1:cx + cx // 2 + 2] = np.nan   # 9 pixels
    return src, ref
