""" Internal overviews (build_ovw; homonim/fuse.py:152-165) without a GPU: the level rule, the arithmetic, the file format.

``overview_levels`` below restates DESIGN.md 5.3 in numpy, for every sample type; the GPU tests (tests/test_gpu_overviews.py)
compare the kernel with it.  Here it is itself held to the oracle: a factor-2 average overview is
``oracle_np.reproject(level, nodata, (2, 0, 2, 0), ceil-shape, nodata, 'average')``, the restated GDAL warp kernel both published
accuracy tables pin, chained level to level.  Float comparisons are on the bits (a NaN equals a NaN). """
import math
import struct

import numpy as np
import pytest

from conftest import assert_same_f32
from homonim_amd import Affine, CRS, _hk, overview_factors, read_tiff_overviews
from homonim_amd.tiff import read_tiff, write_tiff
from oracle import oracle_np


# -- the restatement ----------------------------------------------------------------------------------------------------------
def level_down(a: np.ndarray, nodata) -> np.ndarray:
    """ One level: pixel (i, j) from the pixels (2i..2i+1, 2j..2j+1) of ``a`` that exist and are valid under ``nodata`` (None: all
    are, a NaN is data; NaN: not NaN; a value: not equal to it).  Floats: float64 sum in row-major order / count, rounded once to
    the dtype; integers: floor((2 S + n) / (2 n)) exactly.  No valid pixel: nodata (0 under None). """
    h, w = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((2 * oh, 2 * ow), a.dtype)
    pad[:h, :w] = a
    valid = np.zeros((2 * oh, 2 * ow), bool)
    valid[:h, :w] = True
    if nodata is not None:
        if math.isnan(nodata):
            if a.dtype.kind == 'f':
                valid &= ~np.isnan(pad)
        else:
            valid &= ~(pad == a.dtype.type(nodata))
    is_float = a.dtype.kind == 'f'
    s = np.zeros((oh, ow), np.float64 if is_float else np.int64)
    n = np.zeros((oh, ow), np.int64)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):   # row-major
        v, m = pad[dy::2, dx::2], valid[dy::2, dx::2]
        with np.errstate(invalid='ignore'):
            s = s + np.where(m, v.astype(s.dtype), 0)
        n += m
    fill = a.dtype.type(0 if nodata is None else nodata)
    with np.errstate(invalid='ignore', divide='ignore'):
        if is_float:
            mean = (s / n).astype(a.dtype)
        else:
            mean = np.floor_divide(2 * s + n, np.maximum(2 * n, 1)).astype(a.dtype)   # numpy's // floors
    return np.where(n > 0, mean, fill).astype(a.dtype)


def overview_levels(a: np.ndarray, nodata, n_levels: int):
    """ levels 1..n_levels of a (h, w) or (bands, h, w) raster, each from the level before it """
    if a.ndim == 3:
        per_band = [overview_levels(b, nodata, n_levels) for b in a]
        return [np.stack([pb[m] for pb in per_band]) for m in range(n_levels)]
    out, cur = [], a
    for _ in range(n_levels):
        cur = level_down(cur, nodata)
        out.append(cur)
    return out


def levels_to_1x1(shape) -> int:
    return max(1, int(math.ceil(math.log2(max(shape)))))


def oracle_levels(a: np.ndarray, nodata, n_levels: int):
    out, cur = [], a
    for _ in range(n_levels):
        shape = ((cur.shape[0] + 1) // 2, (cur.shape[1] + 1) // 2)
        cur = oracle_np.reproject(cur, nodata, (2, 0, 2, 0), shape, nodata, 'average')
        assert cur.dtype == np.float32
        out.append(cur)
    return out


NODATA = {'none': None, 'nan': float('nan'), 'value': -7.0}


def holed(shape, mode: str, seed: int, hole_fraction=0.3) -> np.ndarray:
    """ seeded float32 raster with holes of the mode's nodata; under 'none' the holes are NaN pixels, which are data """
    rng = np.random.default_rng(seed)
    a = rng.normal(100.0, 30.0, shape).astype(np.float32)
    hole = rng.random(shape) < hole_fraction
    a[hole] = np.float32('nan') if NODATA[mode] is None else np.float32(NODATA[mode])
    return a


# -- the level rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, factors', [
    ((511, 4000), []), ((512, 512), [2]), ((1024, 700), [2]), ((1421, 805), [2]), ((16384, 16384), [2, 4, 8, 16, 32, 64]),
    ((2 ** 17, 2 ** 17), [2, 4, 8, 16, 32, 64, 128, 256]),
])
def test_overview_factors_follow_the_reference_rule(shape, factors):
    """ hand-derived from homonim/fuse.py:161-164: n = min(8, int(min(log2(shape))) - 8), factors 2^1 .. 2^n """
    assert overview_factors(shape) == factors
    assert overview_factors((3, *shape)) == factors        # (bands, rows, columns) reads its last two
    assert _hk.overview_count(*shape) == len(factors)      # the C ABI's helper is the same rule


def test_overview_count_equals_the_float_rule_on_many_shapes():
    rng = np.random.default_rng(5)
    sides = np.concatenate([2 ** np.arange(0, 20), 2 ** np.arange(1, 20) - 1, 2 ** np.arange(1, 20) + 1, rng.integers(1, 300000, 200)])
    for h, w in zip(rng.permutation(sides), sides):
        n = min(8, int(np.min(np.log2((int(h), int(w))))) - 8)
        assert len(overview_factors((h, w))) == max(n, 0) == _hk.overview_count(int(h), int(w)), (h, w)


def test_the_binding_has_the_entry_points():
    assert callable(_hk.Context.overviews) and callable(_hk.Context.overviews_dev)
    for name in ('hk_overview_count', 'hk_overviews', 'hk_overviews_dev'):
        assert name in _hk.SIGNATURES


# -- the arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(NODATA))
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (8, 8), (17, 33), (30, 21), (1, 9), (9, 1)])
def test_restatement_equals_the_chained_oracle_bit_for_bit(shape, mode):
    a = holed(shape, mode, seed=shape[0] * 1000 + shape[1])
    n = levels_to_1x1(shape)
    mine, theirs = overview_levels(a, NODATA[mode], n), oracle_levels(a, NODATA[mode], n)
    assert mine[-1].shape == (1, 1)
    for m, (x, y) in enumerate(zip(mine, theirs), 1):
        assert x.shape == (math.ceil(shape[0] / 2 ** m), math.ceil(shape[1] / 2 ** m))
        assert_same_f32(x, y, f'{shape} {mode} level {m}')


def test_restatement_empty_cells_and_propagating_nan():
    nan = np.float32('nan')
    a = np.array([[nan, nan, 1, 2], [nan, nan, nan, 4], [5, 6, 7, 8]], np.float32)
    assert_same_f32(level_down(a, float('nan')), np.array([[nan, 7 / 3], [5.5, 7.5]], np.float32))
    assert_same_f32(level_down(a, None), np.array([[nan, nan], [5.5, 7.5]], np.float32))      # NaN is data
    b = np.where(np.isnan(a), np.float32(9), a)
    assert_same_f32(level_down(b, 9.0), np.array([[9, 7 / 3], [5.5, 7.5]], np.float32))


def test_restatement_integer_rounding_is_half_up_and_exact():
    """ floor((2 S + n) / (2 n)) = floor(mean + 1/2): -0.5 -> 0, -1.5 -> -1, 2.5 -> 3; no wrap at the ends of 32-bit types """
    assert level_down(np.array([[-1, 0]], np.int16), None).tolist() == [[0]]
    assert level_down(np.array([[-2, -1]], np.int32), None).tolist() == [[-1]]
    assert level_down(np.array([[2, 3]], np.uint8), None).tolist() == [[3]]
    assert level_down(np.array([[-3, -4], [-4, -3]], np.int16), None).tolist() == [[-3]]       # -3.5 -> -3
    assert level_down(np.array([[1, 2], [2, 0]], np.uint8), 0).tolist() == [[2]]               # 5/3 = 1.67 -> 2
    top = np.iinfo(np.uint32).max
    assert level_down(np.full((2, 2), top, np.uint32), None).tolist() == [[top]]
    lo = np.iinfo(np.int32).min
    assert level_down(np.array([[lo, lo], [lo, lo + 1]], np.int32), None).tolist() == [[lo]]   # lo + 1/4 -> lo
    assert level_down(np.array([[lo, lo + 1]], np.int32), None).tolist() == [[lo + 1]]         # lo + 1/2 -> lo + 1
    assert level_down(np.zeros((2, 2), np.uint16), 0).tolist() == [[0]]                        # no valid pixel: nodata


# -- the file format --------------------------------------------------------------------------------------------------------
def walk_ifds(path):
    """ [(tags of directory k as {code: (type, count, value-or-offset field)})] of a classic little-endian TIFF """
    buf = open(path, 'rb').read()
    assert buf[:4] == b'II*\0'
    (off,) = struct.unpack('<I', buf[4:8])
    dirs = []
    while off:
        (n,) = struct.unpack('<H', buf[off:off + 2])
        tags = {}
        for k in range(n):
            code, typ, count, val = struct.unpack('<HHII', buf[off + 2 + 12 * k: off + 14 + 12 * k])
            tags[code] = (typ, count, val if typ == 4 else val & 0xffff)
        dirs.append(tags)
        (off,) = struct.unpack('<I', buf[off + 2 + 12 * n: off + 6 + 12 * n])
    return dirs, len(buf)


TIFF_DTYPES = ['uint8', 'uint16', 'uint32', 'int8', 'int16', 'int32', 'float32', 'float64']


@pytest.mark.parametrize('dtype', TIFF_DTYPES)
def test_tiff_overviews_round_trip(tmp_path, dtype):
    rng = np.random.default_rng(TIFF_DTYPES.index(dtype))
    shape, nb = (301, 517), 2
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        a = rng.normal(0, 50, (nb, *shape)).astype(dt)
        a[rng.random(a.shape) < 0.2] = np.nan
        nodata = float('nan')
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, (nb, *shape), dtype=dt, endpoint=True)
        nodata = 3
        a[rng.random(a.shape) < 0.2] = nodata
    levels = overview_levels(a, nodata, 3)
    tf, crs, meta, names = Affine(10., 0., 500000., 0., -10., 6200000.), CRS('EPSG:32735'), {'FUSE_MODEL': 'gain'}, ['B1', 'B2']
    plain, with_ovw = tmp_path / 'plain.tif', tmp_path / 'ovw.tif'
    write_tiff(plain, a, tf, crs, nodata, meta, descriptions=names)
    write_tiff(with_ovw, a, tf, crs, nodata, meta, descriptions=names, overviews=levels)

    back = read_tiff_overviews(with_ovw)
    assert len(back) == 3
    for m, (x, y) in enumerate(zip(back, levels), 1):
        assert x.dtype == y.dtype == dt and x.shape == y.shape == (nb, math.ceil(shape[0] / 2 ** m), math.ceil(shape[1] / 2 ** m))
        assert x.tobytes() == y.tobytes(), f'level {m}'
    assert read_tiff_overviews(plain) == []

    r0, r1 = read_tiff(plain), read_tiff(with_ovw)
    assert r0.array.tobytes() == r1.array.tobytes() == a.tobytes() and r1.array.dtype == dt
    assert r0.transform == r1.transform == tf and r0.crs == r1.crs and r0.metadata == r1.metadata == meta
    assert r0.descriptions == r1.descriptions == tuple(names)
    assert (r0.nodata == r1.nodata) or (math.isnan(r0.nodata) and math.isnan(r1.nodata))

    (main0,), size0 = walk_ifds(plain)
    dirs, size1 = walk_ifds(with_ovw)
    assert len(dirs) == 4 and size1 > size0
    assert dirs[0] == main0                                  # the main image's directory is the same with and without
    assert 254 not in dirs[0] and 33550 in dirs[0] and 34735 in dirs[0]
    for m, d in enumerate(dirs[1:], 1):
        assert d[254][2] == 1                                # NewSubfileType: reduced resolution
        assert (d[257][2], d[256][2]) == (math.ceil(shape[0] / 2 ** m), math.ceil(shape[1] / 2 ** m))
        assert d[322][2] == d[323][2] == 128                 # GDAL's default overview block
        for code in (258, 259, 277, 284, 339):               # bits, compression, samples, planar configuration, format
            assert d[code][:2] == dirs[0][code][:2] and (d[code][1] > 2 or d[code][2] == dirs[0][code][2]), code
        assert 42113 in d                                    # GDAL_NODATA
        assert not {33550, 33922, 34264, 34735, 34736, 34737, 42112} & set(d)   # no geo tags, no metadata


def test_tiff_overviews_are_validated_and_optional(tmp_path):
    a = np.zeros((2, 40, 40), np.float32)
    tf = Affine.identity()
    with pytest.raises(ValueError):
        write_tiff(tmp_path / 'x.tif', a, tf, overviews=[np.zeros((1, 20, 20), np.float32)])      # band count
    with pytest.raises(ValueError):
        write_tiff(tmp_path / 'x.tif', a, tf, overviews=[np.zeros((2, 20, 20), np.float64)])      # dtype
    write_tiff(tmp_path / 'a.tif', a, tf)
    write_tiff(tmp_path / 'b.tif', a, tf, overviews=[])
    write_tiff(tmp_path / 'c.tif', a, tf, overviews=None)
    assert open(tmp_path / 'a.tif', 'rb').read() == open(tmp_path / 'b.tif', 'rb').read() == open(tmp_path / 'c.tif', 'rb').read()
    write_tiff(tmp_path / 'd.tif', a[0], tf, overviews=[np.ones((20, 20), np.float32)])           # 2-D in, 2-D levels
    (lv,) = read_tiff_overviews(tmp_path / 'd.tif')
    assert lv.shape == (1, 20, 20) and (lv == 1).all()
