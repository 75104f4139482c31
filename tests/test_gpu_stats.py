""" GPU tests of the parameter statistics (hk_param_stats.hip, homonim_amd/stats.py) against numpy / math.fsum in this file.

What is EQUAL and what is BOUNDED: min, max, N, N(x < thresh) and the bounding box do not depend on the order of a reduction,
so they equal numpy's.  The two sums are float64 sums of exactly representable float64 terms ((double)x, and (double)x squared:
24 x 24 bits fit in 53) in the GPU's own order; any order of adding n terms t_i in float64 ends within
(n - 1) * u * sum|t_i| / (1 - (n - 1) * u) of the exact sum, u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms,
eq. 4.4), which n * 2^-53 * sum|t_i| covers for every n <= 2^24 used here; math.fsum returns the exact sum rounded once, hence
one more ulp of it.  No pixel is excluded and nothing here is fitted to what the kernel returns. """
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import REPO
from homonim_amd import Model, ParamStats, RasterFuse, Window, _hk
from homonim_amd.errors import DeviceError

pytestmark = pytest.mark.gpu

TIFF_DIR = os.path.join(REPO, 'tests', 'golden', 'tiff')
PARAM_FILES = ['float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif', 'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM_tile_10x20.tif']
MIN, MAX, SUM, SUM2, N, N_BELOW, COL_MIN, ROW_MIN, COL_MAX, ROW_MAX = range(10)


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


# -- the reference ---------------------------------------------------------------------------------------------------------
def valid_mask(x, nodata):
    if nodata is None:
        return np.ones(x.shape, bool)
    return ~np.isnan(x) if math.isnan(nodata) else ~(x == np.float32(nodata))


def reference(x, nodata, thresh):
    """ -> (the equal part as a 10-vector with the sums left out, fsum of x, fsum of x^2, fsum of |x|, fsum of x^2) on float64 terms """
    valid = valid_mask(x, nodata)
    t = x.astype(np.float64)[valid]
    n = int(valid.sum())
    vec = np.array([np.inf, -np.inf, 0, 0, n, 0, x.shape[1], x.shape[0], -1, -1], np.float64)
    if n:
        vec[MIN], vec[MAX] = t.min(), t.max()
        vec[N_BELOW] = 0 if thresh is None else int((x.astype(np.float64) < thresh)[valid].sum())
        rows, cols = np.nonzero(valid.any(axis=1))[0], np.nonzero(valid.any(axis=0))[0]
        vec[COL_MIN], vec[ROW_MIN], vec[COL_MAX], vec[ROW_MAX] = cols[0], rows[0], cols[-1], rows[-1]
    if np.isfinite(t).all():
        s, s2 = math.fsum(t.tolist()), math.fsum((t * t).tolist())
        return vec, s, s2, math.fsum(np.abs(t).tolist()), s2
    with np.errstate(all='ignore'):   # an infinite pixel (fsum raises on inf - inf; none is made here)
        return vec, float(t.sum()), float((t * t).sum()), math.inf, math.inf


def check_vector(got, x, nodata, thresh, what):
    vec, s, s2, abs_sum, sq_sum = reference(x, nodata, thresh)
    n = vec[N]
    for k in (MIN, MAX, N, N_BELOW, COL_MIN, ROW_MIN, COL_MAX, ROW_MAX):
        assert got[k] == vec[k], f'{what}: value {k}: {got[k]!r} != {vec[k]!r}'
    for k, ref, mag in ((SUM, s, abs_sum), (SUM2, s2, sq_sum)):
        if not math.isfinite(ref):   # an infinite pixel: every order of adding finite terms and +inf gives +inf
            assert got[k] == ref, f'{what}: value {k}: {got[k]!r} != {ref!r}'
            continue
        bound = n * 2.0 ** -53 * mag + float(np.spacing(abs(ref)))
        err = abs(got[k] - ref)
        print(f'{what}: value {k}: |error| {err:.3e}, bound {bound:.3e}')
        assert err <= bound, f'{what}: value {k}: {got[k]!r} vs {ref!r}: error {err:.3e} > bound {bound:.3e}'


# -- the cases ----------------------------------------------------------------------------------------------------------------
# (height, width, row stride); the last two are taller than the 2048 workgroups a band gets, so that a workgroup walks a second and a
# third row: the per-row reset of the column maximum and the folds of the row range and of the 64-bit counts carried across rows
SHAPES = [(1, 1, None), (1, 7, None), (513, 3, None), (97, 1031, None), (2048, 2050, 2112), (4100, 9, None), (2049, 1031, 1088)]
ROWS_PER_PASS = 2048   # PSTATS_BLOCKS of hk_param_stats.hip: row y is walked by workgroup y % 2048, as its (y // 2048)-th row
VALUES = {'unit': (1.0, 0.3, 0.25), 'dn': (1000.0, 150.0, 900.0)}                            # mean, sigma, thresh
CASES = ['no_holes', 'nan_frame_holes', 'all_nan', 'nodata_0', 'inf_pixel', 'thresh_0p1', 'shrinking_box']


def make_case(shape, values, case):
    height, width, stride = shape
    mean, sigma, thresh = VALUES[values]
    rng = np.random.default_rng(height * 7919 + width * 104729 + list(VALUES).index(values) * 31 + CASES.index(case))
    store = rng.normal(mean, sigma, (height, stride or width)).astype(np.float32)
    x = store[:, :width]
    nodata = float('nan')

    def holes(value):
        for _ in range(4):   # clustered holes: rectangles of up to a quarter of each side
            h, w = rng.integers(1, max(2, height // 4 + 1)), rng.integers(1, max(2, width // 4 + 1))
            r, c = rng.integers(0, height - h + 1), rng.integers(0, width - w + 1)
            x[r:r + h, c:c + w] = value

    if case == 'no_holes':
        nodata = None
    elif case == 'nan_frame_holes':
        x[0, :] = x[-1, :] = np.nan
        x[:, 0] = x[:, -1] = np.nan
        holes(np.nan)
    elif case == 'all_nan':
        x[:] = np.nan
    elif case == 'nodata_0':
        nodata = 0.0
        holes(0.0)
    elif case == 'inf_pixel':
        x[rng.integers(0, height), rng.integers(0, width)] = np.inf
    elif case == 'thresh_0p1':
        thresh = 0.1   # not a float32 value: float32(0.1) = 0.100000001490116... is NOT below it, its predecessor is
        holes(np.nan)
        near = np.float32(0.1)
        for v in (near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(1))):
            x[rng.integers(0, height), rng.integers(0, width)] = v
    elif case == 'shrinking_box':
        x[~shrinking_box_valid(height, width)] = np.nan
    return x, nodata, thresh


def shrinking_box_valid(height, width):
    """ The valid pixels of 'shrinking_box'.  Row 0 alone is valid over its whole width, so both column bounds of the box come from
    the first row of workgroup 0; every other row y is valid in [inset, width - inset) with inset = 1 + y // 2048, so the second and
    third rows of every workgroup (y + 2048, y + 4096) are strictly narrower than its first, and empty where the width is used up.
    Rows with y % 5 == 3 hold no valid pixel, nor does the last row: the last valid row is followed, in the workgroups that walk
    the rows behind it, by an empty one, which a count or a column maximum left over from the row before would turn into data. """
    valid = np.zeros((height, width), bool)
    for y in range(height):
        inset = 1 + y // ROWS_PER_PASS if y else 0
        if y == 0 or not (y % 5 == 3 or y == height - 1):
            valid[y, inset:max(inset, width - inset)] = True
    return valid


def test_the_shrinking_box_is_what_it_says():
    """ (no device: the statement of the case, checked on the shapes that are taller than one pass) """
    for height, width, _ in SHAPES:
        valid = shrinking_box_valid(height, width)
        lo = np.where(valid.any(1), valid.argmax(1), width)
        hi = np.where(valid.any(1), width - 1 - valid[:, ::-1].argmax(1), -1)
        assert lo[0] == 0 and hi[0] == width - 1 and (lo[1:] > 0).all() and (hi[1:] < width - 1).all()
        for y in range(ROWS_PER_PASS, height):   # a workgroup's next row lies strictly inside the one before it, or is empty
            above = y - ROWS_PER_PASS
            assert not valid[y].any() or not valid[above].any() or (lo[y] > lo[above] and hi[y] < hi[above]), (height, width, y)
        if height > ROWS_PER_PASS:   # an empty row behind the last valid one, walked by a workgroup that has seen valid pixels
            last = int(np.nonzero(valid.any(1))[0][-1])
            assert any(valid[y - ROWS_PER_PASS].any() for y in range(max(last + 1, ROWS_PER_PASS), height)), (height, width)
        if height > ROWS_PER_PASS + 2:
            assert valid[ROWS_PER_PASS:].any() and last >= ROWS_PER_PASS


@pytest.mark.oracle
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('values', list(VALUES))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}' + (f's{s[2]}' if s[2] else ''))
def test_exact_values_and_the_sum_bound(ctx, shape, values, case):
    x, nodata, thresh = make_case(shape, values, case)
    got = ctx.param_stats(x, nodata, thresh)
    check_vector(got, x, nodata, thresh, f'{shape} {values} {case}')
    if case == 'all_nan':
        assert got.tolist() == [np.inf, -np.inf, 0, 0, 0, 0, shape[1], shape[0], -1, -1]
    assert np.array_equal(got, ctx.param_stats(x, nodata, thresh), equal_nan=True)   # run to run


@pytest.mark.oracle
@pytest.mark.parametrize('nodata', [None, 0.0])
def test_a_valid_nan_pixel_makes_min_max_and_sums_nan_as_in_numpy(ctx, nodata):
    rng = np.random.default_rng(5)
    x = rng.normal(1, 0.3, (40, 70)).astype(np.float32)
    x[3:6, 10:20] = 0.0
    x[17, 33] = np.nan
    got = ctx.param_stats(x, nodata, 0.9)
    valid = valid_mask(x, nodata)
    t = x.astype(np.float64)[valid]
    assert np.isnan([t.min(), t.max(), t.sum(), (t * t).sum()]).all()   # what numpy does
    assert np.isnan(got[[MIN, MAX, SUM, SUM2]]).all()
    assert got[N] == valid.sum() and got[N_BELOW] == (t < 0.9).sum()
    assert got[[COL_MIN, ROW_MIN, COL_MAX, ROW_MAX]].tolist() == [0, 0, 69, 39]
    assert ctx.param_stats(x, nodata, float('nan'))[N_BELOW] == 0   # a NaN thresh counts nothing


# -- 1. the real stack's numbers ---------------------------------------------------------------------------------------------
def _test_vals(param_stats):
    """ tests/test_stats.py:36-50 of the reference: gain = 1, offset = 0, r2 = 1 """
    assert len(param_stats) == 9
    for band_stats in param_stats:
        assert {'band', 'mean', 'std', 'min', 'max'} <= set(band_stats.keys())
    expected = (3 * [{'mean': 1, 'std': 0, 'min': 1, 'max': 1}] + 3 * [{'mean': 0, 'std': 0, 'min': 0, 'max': 0}] +
                3 * [{'mean': 1, 'std': 0, 'min': 1, 'max': 1, 'inpaint_p': 0}])
    for band_stats, exp in zip(param_stats, expected):
        for k, v in exp.items():
            assert band_stats[k] == pytest.approx(v, abs=1e-2)


@pytest.mark.oracle
@pytest.mark.parametrize('name', PARAM_FILES)
def test_real_stack_pin(ctx, name):
    """ The table homonim + GDAL printed for these files (tests/test_stats.py:136-144 of the reference, its test_cli criterion) """
    with ParamStats(os.path.join(TIFF_DIR, name), context=ctx) as ps:
        assert len(ps.metadata) > 0
        param_stats = ps.stats()
        window = ps._get_data_window()
    _test_vals(param_stats)
    assert [b['n'] for b in param_stats] == [144] * 9
    assert window == Window(1, 1, 8, 18)
    table = ''.join(ps.stats_table(param_stats).split())
    rows = ([f'B{i}_GAIN1.0000.0001.0001.000' for i in (1, 2, 3)] + [f'B{i}_OFFSET-0.0000.000-0.0010.000' for i in (1, 2, 3)] +
            [f'B{i}_R21.0000.0001.0001.0000.000' for i in (1, 2, 3)])
    for row in rows:
        assert row in table, (row, table)
    assert all('inpaint_p' not in b for b in param_stats[:6])


# -- 3. device-resident planes ----------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('n_bands, height, width, stride', [(3, 97, 1031, 1088), (12, 130, 260, 320), (3, 97, 1031, 1031)],
                         ids=['3-aligned', '12-aligned', '3-unaligned-rows'])
def test_device_resident_call_equals_the_host_call_bit_for_bit(ctx, n_bands, height, width, stride):
    """ All bands in one launch; the last layout (odd row stride: no 16-byte loads) takes the scalar path and still gives the
    host call's bits, because the threads walk the same pixels in the same order. """
    rng = np.random.default_rng(n_bands * 1000 + stride)
    band_stride = stride * height + (64 if stride % 4 == 0 else 3)
    store = np.full(n_bands * band_stride, np.nan, np.float32)
    planes = []
    for b in range(n_bands):
        plane = store[b * band_stride: b * band_stride + stride * height].reshape(height, stride)[:, :width]
        plane[:] = rng.normal(1 + b, 0.3, (height, width)).astype(np.float32)
        plane[:2 + b, :] = np.nan
        plane[:, -1 - b:] = np.nan
        plane[40:50, 100:130] = np.nan
        planes.append(plane)
    thresh = 1.05
    d_planes, d_stats = ctx.dev_alloc(store.nbytes), ctx.dev_alloc(n_bands * 80)
    try:
        ctx.h2d(d_planes, store)
        out = []
        for _ in range(2):
            ctx.memset(d_stats, 0, n_bands * 80)
            ctx.param_stats_dev(d_planes, n_bands, height, width, stride, band_stride, d_stats, float('nan'), thresh, stream=0)
            ctx.stream_sync(0)
            got = np.zeros((n_bands, 10))
            ctx.d2h(got, d_stats)
            out.append(got)
    finally:
        ctx.dev_free(d_planes)
        ctx.dev_free(d_stats)
    assert out[0].tobytes() == out[1].tobytes()   # a second run equals the first
    for b in range(n_bands):
        host = ctx.param_stats(planes[b], float('nan'), thresh)
        assert out[0][b].tobytes() == host.tobytes(), (b, out[0][b], host)
        check_vector(out[0][b], planes[b], float('nan'), thresh, f'device band {b}')


# -- 4. strips ------------------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_strip_accumulation_does_not_depend_on_threads(ctx):
    rng = np.random.default_rng(44)
    params = rng.normal(1, 0.3, (3, 301, 257)).astype(np.float32)
    params[:, :3, :] = params[:, -2:, :] = np.nan
    params[:, :, :5] = params[:, :, -1:] = np.nan
    params[1, 100:220, 30:90] = np.nan   # a hole that spans strips
    strip_bytes = 100 * 257 * 4           # 100 rows a strip: 4 strips a band
    runs = []
    for threads in (1, 4):
        ps = ParamStats.from_arrays(params, Model.gain_offset, r2_inpaint_thresh=0.9, context=ctx, strip_bytes=strip_bytes)
        assert len(ps._strips([0])) == 4
        runs.append((ps.stats(threads=threads), ps._reduce([0, 1, 2], threads), ps._get_data_window()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][2] == runs[1][2] == Window(5, 3, 251, 296)
    for stats_list, vectors, _ in runs:
        for b in range(3):
            check_vector(vectors[b], params[b], float('nan'), 0.9 if b == 2 else None, f'strips band {b}')
        assert [s['band'] for s in stats_list] == ['B1_GAIN', 'B1_OFFSET', 'B1_R2']
        assert 'inpaint_p' in stats_list[2] and 'inpaint_p' not in stats_list[0]


# -- 5. round trip with the product -------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_round_trip_with_raster_fuse(ctx, tmp_path):
    rng = np.random.default_rng(9)
    src = rng.uniform(0.1, 1.0, (2, 72, 90)).astype(np.float32)
    ref = (1.5 * src + 0.1 + rng.normal(0, 0.05, src.shape)).astype(np.float32)
    ref[:, 30:50, 40:70] = rng.uniform(0.1, 1.0, (2, 20, 30)).astype(np.float32)   # uncorrelated: low R2, in-painted
    src[:, :4, :] = np.nan
    param_file = tmp_path / 'p.tif'
    _, params = RasterFuse(src, ref).process(param_filename=param_file, model='gain-offset', kernel_shape=(5, 5))
    assert params.shape[0] == 6
    with ParamStats(param_file, context=ctx) as ps:
        stats_list = ps.stats()
    names = [s['band'] for s in stats_list]
    assert names == ['B1_GAIN', 'B2_GAIN', 'B1_OFFSET', 'B2_OFFSET', 'B1_R2', 'B2_R2']
    for bi, band_stats in enumerate(stats_list):
        valid = ~np.isnan(params[bi])
        t = params[bi].astype(np.float64)[valid]
        assert band_stats['n'] == valid.sum() and band_stats['min'] == t.min() and band_stats['max'] == t.max()
        if bi >= 4:
            assert band_stats['inpaint_p'] == 100 * (t < 0.25).sum() / valid.sum()
            assert band_stats['inpaint_p'] > 0
        else:
            assert 'inpaint_p' not in band_stats
    in_memory = ParamStats.from_arrays(params, Model.gain_offset, context=ctx).stats()
    assert [{k: v for k, v in s.items() if k != 'band'} for s in in_memory] == \
           [{k: v for k, v in s.items() if k != 'band'} for s in stats_list]


# -- 6. argument errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_argument_errors_are_exceptions_with_a_message(ctx):
    lib, h = ctx._lib, ctx.handle
    x = np.ones((4, 8), np.float32)
    out = np.zeros(10)
    xp, op = x.ctypes.data_as(_hk._f32p), out.ctypes.data_as(_hk._f64p)
    nan = float('nan')
    bad_host = [
        (None, 8, 1, nan, 0.5, 4, 8, op), (xp, 8, 1, nan, 0.5, 4, 8, None),   # NULL pointers
        (xp, 8, 1, nan, 0.5, 0, 8, op), (xp, 8, 1, nan, 0.5, 4, 0, op),       # empty raster
        (xp, 7, 1, nan, 0.5, 4, 8, op),                                       # stride < width
        (xp, 8, 7, nan, 0.5, 4, 8, op),                                       # bad nodata mode
    ]
    for args in bad_host:
        with pytest.raises(ValueError, match=r'\w+'):
            _hk._check(lib.hk_param_stats(h, *args))
    d = ctx.dev_alloc(4096)
    try:
        p, s = C.c_void_p(d), C.c_void_p(d + 2048)
        bad_dev = [
            (None, 1, 4, 8, 8, 32, 0, 1, nan, 0.5, s), (p, 1, 4, 8, 8, 32, 0, 1, nan, 0.5, None),
            (p, 0, 4, 8, 8, 32, 0, 1, nan, 0.5, s), (p, 1, 0, 8, 8, 32, 0, 1, nan, 0.5, s), (p, 1, 4, 0, 8, 32, 0, 1, nan, 0.5, s),
            (p, 1, 4, 8, 7, 32, 0, 1, nan, 0.5, s), (p, 1, 4, 8, 8, 32, 0, 3, nan, 0.5, s),
            (p, 1, 4, 8, 8, 32, 99, 1, nan, 0.5, s), (p, 1, 4, 8, 8, 32, -1, 1, nan, 0.5, s),   # bad stream
        ]
        for args in bad_dev:
            with pytest.raises(ValueError, match=r'\w+'):
                _hk._check(lib.hk_param_stats_dev(h, *args))
    finally:
        ctx.dev_free(d)
    with pytest.raises(ValueError):
        ctx.param_stats(np.ones((2, 3, 4), np.float32))
    with pytest.raises((ValueError, DeviceError)):
        _hk._check(lib.hk_param_stats(None, xp, 8, 1, nan, 0.5, 4, 8, op))   # NULL context
    assert ctx.param_stats(x, nan, 0.5)[N] == 32   # the context still works
