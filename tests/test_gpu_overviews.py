""" GPU tests of the internal overviews (hk_overview.hip; hk_overviews / hk_overviews_dev; RasterFuse.process(build_ovw=True)).

float32 is held to the oracle itself -- ``oracle_np.reproject(level, nodata, (2, 0, 2, 0), ceil-shape, nodata, 'average')`` chained
level to level -- and, at size, to the library's own re-sampling kernel, an independent implementation the oracle pins.  The
integer types and float64 are held to the exact restatement of tests/test_overviews_cpu.py (which that file holds to the same
oracle for float32).  Every comparison is on the bits (a NaN equals a NaN); nothing here is a tolerance. """
import math

import numpy as np
import pytest

from conftest import assert_same_f32
from homonim_amd import ParamStats, RasterFuse, Resampling, _hk, overview_factors, read_tiff_overviews, utils
from homonim_amd.tiff import read_tiff
from test_overviews_cpu import NODATA, holed, levels_to_1x1, oracle_levels, overview_levels, walk_ifds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def assert_same_bits(got: np.ndarray, exp: np.ndarray, what: str):
    """ equal shape, dtype and bytes; floats: a NaN equals a NaN """
    assert got.shape == exp.shape and got.dtype == exp.dtype, f'{what}: {got.shape} {got.dtype} != {exp.shape} {exp.dtype}'
    same = (got == exp) | ((got != got) & (exp != exp)) if got.dtype.kind == 'f' else got == exp
    if got.dtype.kind == 'f':   # (+0 and -0 are different bits)
        same &= np.signbit(got) == np.signbit(exp)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f'{what}: {(~same).sum()} of {got.size} differ; first at {i}: {got[i]!r} != {exp[i]!r}')


SENTINEL = 0x5A


def overviews_dev(ctx, a: np.ndarray, nodata, n_levels: int, pad_cols=3, pad_rows=2, out_pad_cols=5, out_pad_rows=1):
    """ hk_overviews_dev on a (bands, h, w) raster laid out with a row pitch of w + pad_cols and pad_rows spare rows between the
    bands; the levels' planes have slack of their own, which must come back untouched. """
    nb, h, w = a.shape
    store = np.full((nb, h + pad_rows, w + pad_cols), 0, a.dtype)
    store.view(np.uint8)[...] = SENTINEL
    store[:, :h, :w] = a
    d_src = ctx.dev_alloc(store.nbytes)
    shapes = _hk.overview_shapes(h, w, n_levels)
    outs = [np.empty((nb, lh + out_pad_rows, lw + out_pad_cols), a.dtype) for lh, lw in shapes]
    d_outs = []
    try:
        ctx.h2d(d_src, store)
        for o in outs:
            o.view(np.uint8)[...] = SENTINEL
            d_outs.append(ctx.dev_alloc(o.nbytes))
            ctx.h2d(d_outs[-1], o)
        ctx.overviews_dev(d_src, a.dtype.name, nb, h, w, store.shape[2], store.shape[1] * store.shape[2], nodata, d_outs,
                          [o.shape[2] for o in outs], [o.shape[1] * o.shape[2] for o in outs])
        ctx.stream_sync(0)
        for o, d in zip(outs, d_outs):
            ctx.d2h(o, d)
    finally:
        for d in [d_src] + d_outs:
            ctx.dev_free(d)
    levels = []
    for o, (lh, lw) in zip(outs, shapes):
        slack = o.copy()
        slack[:, :lh, :lw].view(np.uint8)[...] = SENTINEL
        assert (slack.view(np.uint8) == SENTINEL).all(), 'a level was written outside its height x width'
        levels.append(np.ascontiguousarray(o[:, :lh, :lw]))
    return levels


# -- 1. float32 against the oracle ------------------------------------------------------------------------------------------------
def tiled_case(mode):
    """ larger than one 64 x 64 tile both ways, odd both ways; a tile without a valid pixel, and a lone 2 x 2 cell without one """
    a = holed((150, 203), mode, seed=77, hole_fraction=0.1)
    hole = np.float32('nan') if NODATA[mode] is None else np.float32(NODATA[mode])
    a[64:128, 64:128] = hole
    a[10:12, 20:22] = hole
    return a


ORACLE_SHAPES = [(1, 1), (3, 5), (64, 64), (65, 63), (257, 1025), (2, 3000), (3000, 2), 'tiled']


@pytest.mark.oracle
@pytest.mark.parametrize('mode', list(NODATA))
@pytest.mark.parametrize('shape', ORACLE_SHAPES, ids=str)
def test_float32_every_level_equals_the_chained_oracle(ctx, shape, mode):
    nodata = NODATA[mode]
    a = tiled_case(mode) if shape == 'tiled' else holed(shape, mode, seed=shape[0] * 4099 + shape[1])
    n = levels_to_1x1(a.shape)
    exp = oracle_levels(a, nodata, n)
    assert exp[-1].shape == (1, 1)
    host = ctx.overviews(a, nodata, n)
    second = np.ascontiguousarray(a[::-1, ::-1])   # a second band, so that the band strides are walked
    dev = overviews_dev(ctx, np.stack([a, second]), nodata, n)
    exp_second = oracle_levels(second, nodata, min(n, 2))
    for m in range(n):
        assert_same_f32(host[m], exp[m], f'hk_overviews {a.shape} {mode} level {m + 1}')
        assert_same_f32(dev[m][0], exp[m], f'hk_overviews_dev {a.shape} {mode} level {m + 1}')
    for m, e in enumerate(exp_second):
        assert_same_f32(dev[m][1], e, f'hk_overviews_dev band 2 {a.shape} {mode} level {m + 1}')


# -- 2. float32 at size against the re-sampling kernel ----------------------------------------------------------------------------
@pytest.mark.oracle
def test_float32_at_size_equals_chained_reproject_average(ctx):
    shape = (4097, 6145)
    rng = np.random.default_rng(11)
    a = rng.normal(1000.0, 300.0, shape).astype(np.float32)
    a[rng.random(shape) < 0.2] = np.nan
    a[1000:1300, 2000:2700] = np.nan
    n = levels_to_1x1(shape)
    got = ctx.overviews(a, float('nan'), n)
    cur = a
    for m in range(n):
        dst = ((cur.shape[0] + 1) // 2, (cur.shape[1] + 1) // 2)
        cur = ctx.reproject(cur, float('nan'), (2, 0, 2, 0), dst, int(Resampling.average), float('nan'))
        assert_same_f32(got[m], cur, f'level {m + 1}')
    assert got[-1].shape == (1, 1)


# -- 3. integer types and float64 against the exact restatement -------------------------------------------------------------------
def typed_case(dtype, nodata, seed):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    shape = (2, 131, 259)
    if dt.kind == 'f':
        a = rng.normal(0.0, 1e6, shape).astype(dt)
        a[rng.random(shape) < 0.25] = np.nan if (nodata is None or math.isnan(nodata)) else nodata
        a[0, 64:128, 64:128] = a[0, 0, 0] if nodata is None else nodata
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)      # both ends of the range occur
    if nodata is not None:
        a[rng.random(shape) < 0.25] = nodata
        a[0, 64:128, 64:128] = nodata
    a[0, 0:16, 0:32] = info.max                                                # sums at the top of the range must not wrap
    a[0, 16:32, 0:32] = info.min
    a[1, 0:8, 0:8] = [[info.max, info.max - 1] * 4, [info.max - 1, info.max - 1] * 4] * 4
    if info.min < 0:   # means that land on a negative half
        a[1, 20:22, 0:8] = [[-1, 0, -2, -1, -3, -4, info.min, info.min + 1], [0, 0, -1, -1, -4, -3, info.min + 1, info.min + 1]]
        if nodata is not None:
            a[1, 22:24, 0:8] = [[-1, 0, -2, -1, -3, -4, info.min, info.min + 1], [nodata] * 8]   # two valid pixels: -.5, -1.5, -3.5
    return a


TYPED = [(d, nd) for d in ('uint8', 'uint16', 'int16', 'uint32', 'int32') for nd in (None, 0, 'top')] + \
        [('float64', None), ('float64', float('nan')), ('float64', -9999.0)]


@pytest.mark.oracle
@pytest.mark.parametrize('dtype, nodata', TYPED, ids=str)
def test_integer_types_and_float64_equal_the_exact_restatement(ctx, dtype, nodata):
    if nodata == 'top':
        nodata = int(np.iinfo(dtype).max)
    a = typed_case(dtype, nodata, seed=len(dtype) * 100 + (0 if nodata is None else 1))
    n = levels_to_1x1(a.shape[1:])
    exp = overview_levels(a, nodata, n)
    host, dev = ctx.overviews(a, nodata, n), overviews_dev(ctx, a, nodata, n)
    for m in range(n):
        assert_same_bits(host[m], exp[m], f'hk_overviews {dtype} nodata {nodata} level {m + 1}')
        assert_same_bits(dev[m], exp[m], f'hk_overviews_dev {dtype} nodata {nodata} level {m + 1}')
    if np.dtype(dtype).kind != 'f':   # NaN nodata on an integer raster: every pixel is valid
        for x, y in zip(ctx.overviews(a, float('nan'), 2), overview_levels(a, None, 2)):
            assert_same_bits(x, y, f'{dtype} with NaN nodata')


@pytest.mark.oracle
def test_float32_value_nodata_is_compared_as_float32(ctx):
    """ nodata 0.1 marks the pixels that hold float32(0.1), as everywhere else in the library """
    a = np.full((4, 4), np.float32(0.1), np.float32)
    a[0, 0] = 3.0
    (lv,) = ctx.overviews(a, 0.1, 1)
    assert_same_f32(lv, np.array([[3.0, 0.1], [0.1, 0.1]], np.float32))


# -- 4. strips and layouts of the host call ---------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_small_strips_and_strided_views_give_the_same_bytes(ctx, dtype, monkeypatch):
    rng = np.random.default_rng(3)
    nb, h, w, n = 3, 1001, 301, 3
    if dtype == 'float32':
        big = rng.normal(0, 100, (nb, h + 5, w + 11)).astype(np.float32)
        big[rng.random(big.shape) < 0.2] = np.nan
        nodata = float('nan')
    else:
        big = rng.integers(0, 255, (nb, h + 5, w + 11), dtype=np.uint8, endpoint=True)
        nodata = 0
    view = big[:, 2:2 + h, 4:4 + w]                       # row stride > width, band stride with slack
    assert not view.flags['C_CONTIGUOUS']
    whole = np.ascontiguousarray(view)
    monkeypatch.delenv('HK_OVERVIEW_STRIP_KB', raising=False)
    one_piece = ctx.overviews(whole, nodata, n)
    strided = ctx.overviews(view, nodata, n)
    monkeypatch.setenv('HK_OVERVIEW_STRIP_KB', '64')      # 64 KiB / (3 x 301 x itemsize) rows, rounded down to a multiple of 8
    strips = ctx.overviews(whole, nodata, n)
    strips_strided = ctx.overviews(view, nodata, n)
    monkeypatch.setenv('HK_OVERVIEW_STRIP_KB', '1')       # below one unit: strips of 2^n rows
    tiny = ctx.overviews(whole, nodata, n)
    exp = overview_levels(whole, nodata, n)
    for m in range(n):
        for name, got in (('one piece', one_piece), ('strided view', strided), ('64 KiB strips', strips),
                          ('64 KiB strips of a strided view', strips_strided), ('8-row strips', tiny)):
            assert got[m].tobytes() == one_piece[m].tobytes(), f'{name}: level {m + 1} differs from the call in one piece'
        assert_same_bits(one_piece[m], exp[m], f'level {m + 1}')


@pytest.mark.oracle
def test_argument_errors_are_exceptions_with_a_message(ctx):
    a = np.ones((4, 8), np.uint8)
    with pytest.raises(ValueError, match='nodata'):
        ctx.overviews(a, 300, 1)                           # not a value of the type
    with pytest.raises(ValueError, match='nodata'):
        ctx.overviews(a, 0.5, 1)
    with pytest.raises(ValueError, match='n_levels'):
        ctx.overviews(a, None, 40)
    with pytest.raises(ValueError):
        ctx.overviews(np.ones((4, 8), np.complex64), None, 1)
    assert ctx.overviews(a, None, 0) == []
    (lv,) = ctx.overviews(a, None, 1)                      # (and the context still works)
    assert lv.tolist() == [[1] * 4] * 2


# -- 5. end to end ------------------------------------------------------------------------------------------------------------------
def seeded_pair(shape, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(20.0, 200.0, (3, *shape)).astype(np.float32)
    ref = (1.1 * src + 5.0 + rng.normal(0, 2.0, src.shape)).astype(np.float32)
    src[:, 100:180, 200:330] = np.nan
    return src, ref


@pytest.mark.oracle
@pytest.mark.parametrize('out_profile', [None, dict(dtype='uint8', nodata=0)], ids=['default', 'uint8'])
def test_process_writes_overviews(ctx, tmp_path, out_profile):
    shape = (1100, 1600)
    src, ref = seeded_pair(shape, 21)
    factors = overview_factors(shape)
    assert factors == [2, 4]
    corr_file, param_file = tmp_path / 'corr.tif', tmp_path / 'param.tif'
    corr, params = RasterFuse(src, ref).process(corr_file, 'gain-offset', (5, 5), param_filename=param_file, out_profile=out_profile)
    corr_nodata = float('nan') if out_profile is None else 0
    assert corr.dtype == (np.float32 if out_profile is None else np.uint8)
    for path, arr, nodata in ((corr_file, corr, corr_nodata), (param_file, params, float('nan'))):
        levels = read_tiff_overviews(path)
        assert len(levels) == len(factors)
        again = ctx.overviews(arr, nodata, len(factors))
        restated = overview_levels(arr, nodata, len(factors))
        for m, f in enumerate(factors):
            assert levels[m].shape == (arr.shape[0], math.ceil(shape[0] / f), math.ceil(shape[1] / f))
            assert_same_bits(levels[m], again[m], f'{path.name} level {m + 1} against Context.overviews')
            assert_same_bits(levels[m], restated[m], f'{path.name} level {m + 1} against the restatement')
        main = read_tiff(path)
        assert_same_bits(main.array, arr, f'{path.name} main image')
        dirs, _ = walk_ifds(path)
        assert len(dirs) == 1 + len(factors)
    assert (np.isnan(read_tiff_overviews(corr_file)[0]).any() if out_profile is None else (read_tiff_overviews(corr_file)[0] == 0).any())
    header = utils.validate_param_image(param_file)
    assert header.count == params.shape[0]
    with ParamStats(param_file, context=ctx) as ps:
        stats = ps.stats()
    assert len(stats) == params.shape[0] and stats[0]['n'] == int((~np.isnan(params[0])).sum())

    # build_ovw=False: a single directory, and the same main image
    corr2, params2 = RasterFuse(src, ref).process(tmp_path / 'corr2.tif', 'gain-offset', (5, 5), param_filename=tmp_path / 'param2.tif',
                                                  out_profile=out_profile, build_ovw=False)
    assert_same_bits(corr2, corr, 'corrected, build_ovw=False')
    assert_same_bits(params2, params, 'parameters, build_ovw=False')
    for name in ('corr2.tif', 'param2.tif'):
        assert len(walk_ifds(tmp_path / name)[0]) == 1 and read_tiff_overviews(tmp_path / name) == []
    assert_same_bits(read_tiff(tmp_path / 'corr2.tif').array, corr, 'corr2.tif')


@pytest.mark.oracle
@pytest.mark.parametrize('build_ovw', [True, False])
def test_a_small_raster_gets_a_single_directory_either_way(ctx, tmp_path, build_ovw):
    shape = (600, 400)
    assert overview_factors(shape) == []
    src, ref = seeded_pair(shape, 22)
    corr, params = RasterFuse(src, ref).process(tmp_path / 'c.tif', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.tif',
                                                build_ovw=build_ovw)
    for name, arr in (('c.tif', corr), ('p.tif', params)):
        assert len(walk_ifds(tmp_path / name)[0]) == 1 and read_tiff_overviews(tmp_path / name) == []
        assert_same_bits(read_tiff(tmp_path / name).array, arr, name)
    # (the ledger wants an oracle-checked launch in a test it counts: level 1 of the corrected raster against the restatement)
    assert_same_bits(ctx.overviews(corr, float('nan'), 1)[0], overview_levels(corr, float('nan'), 1)[0], 'level 1')
