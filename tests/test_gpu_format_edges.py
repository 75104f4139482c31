"""
GPU test: the small element-wise kernels every corrected pixel passes on its way in and out -- cast_in_kernel / cast_out_kernel
(hk_convert.hip), mask_rows_kernel / mask_cols_kernel (hk_mask.hip), apply_kernel (hk_kernels.hip) -- held bit for bit to the exact
statements of tests/_format_edges.py (checked on the host by tests/test_format_edges_cpu.py), at the values where a conversion
rounds, ties, clips, overflows or underflows and at the shapes where the launches change behaviour: the 1024-column x block of the
casts, their 2048-row grid, the 256-lane block and the 1024-row grid of the mask, the scalar tail and the 4096-row grid of apply.

There is no tolerance anywhere: each of these has a closed-form answer.  float32 results compare by value with NaN == NaN
(any payload), everything else with assert_array_equal.
"""
import functools

import numpy as np
import pytest

import _format_edges as fe
from conftest import assert_same_f32
from homonim_amd import _hk
from homonim_amd.errors import DeviceError
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

F32 = np.float32
NAN = float('nan')
SENTINEL = 0xA5
OUT_CASES = [(d, nd) for d in fe.OUT_DTYPES for nd in fe.held_nodata(d)]


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, f'{what}: {got.dtype}{got.shape} != {exp.dtype}{exp.shape}'
    if got.dtype == F32:
        assert_same_f32(got, exp, what)
    else:
        np.testing.assert_array_equal(got, exp, err_msg=what)


@functools.lru_cache(maxsize=None)
def _out_plane(dtype):
    """ all families of `dtype` in one plane 1025 + 3 columns wide: a second x block of one lane """
    plane = fe.as_plane(np.concatenate(list(fe.cast_out_families(dtype).values())))
    plane.setflags(write=False)
    return plane


@functools.lru_cache(maxsize=None)
def _out_expected(dtype, nodata):
    exp = fe.cast_out_exact(_out_plane(dtype), dtype, None if nodata != nodata else nodata)
    exp.setflags(write=False)
    return exp


def _nd(nodata):
    return None if nodata is None else float(nodata)


# -- the casts alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype, nodata', OUT_CASES)
def test_cast_out_on_every_family(ctx, dtype, nodata):
    plane = _out_plane(dtype)
    assert plane.shape[1] == 1028 and plane.shape[0] >= 4
    got, exp = ctx.cast_out_plane(plane, dtype, nodata), _out_expected(dtype, _nd(nodata))
    _same(got, exp, f'cast_out {dtype}, nodata {nodata}')
    if np.dtype(dtype).kind == 'f':
        zero = plane == 0
        assert zero.any() and np.signbit(plane[zero]).any()
        np.testing.assert_array_equal(np.signbit(got[zero]), np.signbit(plane[zero]), err_msg='sign of zero')


@pytest.mark.parametrize('dtype', fe.IN_DTYPES)
def test_cast_in_on_every_family(ctx, dtype):
    """ float64: results in the float32 denormal range are kept, as numpy's astype keeps them on the reference's read
    (homonim/raster_array.py:178-188). """
    plane = fe.as_plane(fe.cast_in_family(dtype))
    exp = fe.cast_in_exact(plane, dtype)
    got = ctx.cast_in_plane(plane)
    _same(got, exp, f'cast_in {dtype}')
    np.testing.assert_array_equal(np.signbit(got), np.signbit(exp), err_msg=f'cast_in {dtype}: sign of zero')


SHAPES = [(1, 1), (1, 5), (3, 1023), (5, 1025), (2050, 5)]   # one lane; a tail; below / past the 1024-column block; past the 2048-row grid


def _fill(values, shape, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.asarray(values).ravel(), shape)


def _check_padding(full, w, what):
    """ What the row padding of a destination plane holds after a call.  Both kernels work on whole groups of four columns: the
    group that holds the last column is written to its end with the conversion of the source row's padding -- zero here, which
    converts to zero in every type -- and nothing behind that group is written: it still holds the sentinel.  Never another
    row's data. """
    w4 = (w + 3) // 4 * 4
    in_quad = full[:, w:w4]
    assert (in_quad.view(np.uint8) == 0).all(), f'{what}: the padding inside the last group of four is not zero'
    behind = np.ascontiguousarray(full[:, w4:])
    assert (behind.view(np.uint8) == SENTINEL).all(), f'{what}: columns behind the last group of four were written'


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('dtype', fe.OUT_DTYPES)
def test_cast_out_shapes_strides_and_padding(ctx, dtype, shape):
    fam = fe.cast_out_families(dtype)
    vals = _fill(np.concatenate(list(fam.values())), shape, 17)
    nodata = fe.held_nodata(dtype)[0]
    exp = fe.cast_out_exact(vals, dtype, nodata)
    w4 = (shape[1] + 3) // 4 * 4
    for stride, dst_stride in ((w4, w4), (w4 + 60, w4 + 60), (w4, w4 + 60), (w4 + 60, w4)):
        full = ctx.cast_out_plane(vals, dtype, nodata, stride=stride, dst_stride=dst_stride, sentinel=SENTINEL, full=True)
        assert full.shape == (shape[0], dst_stride)
        what = f'cast_out {dtype} {shape}, strides {stride} -> {dst_stride}'
        _same(np.ascontiguousarray(full[:, :shape[1]]), exp, what)
        _check_padding(full, shape[1], what)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('dtype', fe.IN_DTYPES)
def test_cast_in_shapes_strides_and_padding(ctx, dtype, shape):
    vals = _fill(fe.cast_in_family(dtype), shape, 19)
    exp = fe.cast_in_exact(vals, dtype)
    w4 = (shape[1] + 3) // 4 * 4
    for stride, dst_stride in ((w4, w4), (w4 + 60, w4 + 60), (w4, w4 + 60), (w4 + 60, w4)):
        full = ctx.cast_in_plane(vals, stride=stride, dst_stride=dst_stride, sentinel=SENTINEL, full=True)
        what = f'cast_in {dtype} {shape}, strides {stride} -> {dst_stride}'
        _same(np.ascontiguousarray(full[:, :shape[1]]), exp, what)
        _check_padding(full, shape[1], what)


def test_cast_plane_refusals_launch_nothing(ctx):
    h, w, stride = 6, 10, 12
    buf = ctx.dev_alloc(2 * h * stride * 8 + 64)
    try:
        ctx.memset(buf, 0, 2 * h * stride * 8 + 64)
        src, dst = buf, buf + h * stride * 8 + 32
        before = _hk.build_ledger()
        good = dict(to_typed=True, dtype='int16', src_dptr=src, src_stride=stride, dst_dptr=dst, dst_stride=stride, height=h, width=w,
                    has_nodata=True, nodata=-1.0, stream=0)
        bad = [
            dict(height=0), dict(width=0), dict(height=-1), dict(width=-2),                       # a shape below 1 x 1
            dict(src_stride=8), dict(dst_stride=8), dict(src_stride=0), dict(dst_stride=-12),     # a stride below the width
            dict(src_stride=13), dict(dst_stride=14), dict(src_stride=11, dst_stride=11),         # ... not a multiple of 4
            dict(src_dptr=src + 4), dict(src_dptr=src + 8),                                       # float32 side: 16-byte accesses
            dict(dst_dptr=dst + 1),                                                               # typed side: its own samples
            dict(to_typed=False, dtype='int16', dst_dptr=dst + 4), dict(to_typed=False, dtype='int32', src_dptr=src + 2),
            dict(to_typed=False, dtype='float64', src_dptr=src + 4),
            dict(dtype=7), dict(dtype=-1), dict(dtype=99),                                        # an unknown dtype
            dict(to_typed=False, dtype='float32'), dict(to_typed=False, dtype=0),                 # float32 has no input conversion
            dict(src_dptr=None), dict(dst_dptr=None), dict(stream=-1), dict(stream=10 ** 6),
            dict(nodata=0.5), dict(nodata=-32769.0), dict(nodata=NAN), dict(dtype='uint8', nodata=-1.0),   # as hk_fit_apply_io
        ]
        for change in bad:
            with pytest.raises(ValueError):
                ctx.cast_plane_dev(**dict(good, **change))
        assert _hk.build_ledger() == before, 'a refused call launched a kernel'
        ctx.cast_plane_dev(**good)
        ctx.cast_plane_dev(**dict(good, to_typed=False))
        assert _hk.build_ledger() != before
    finally:
        ctx.dev_free(buf)


# -- the launch sites ------------------------------------------------------------------------------------------------------
def _site_plane(dtype):
    """ The family as the reference of a gain fit with kernel 1 x 1 on a source of ones: the gain is ref / 1 and the corrected
    block ref * 1, the family itself -- +-inf, denormals and FLT_MAX included: a 1 x 1 window sum is the value, and the fit
    carries them (the test asserts the identity before it looks at the conversion). """
    return _out_plane(dtype)


@pytest.mark.parametrize('dtype, nodata', OUT_CASES)
def test_fit_apply_converts_as_the_cast_alone(ctx, dtype, nodata):
    ref = _site_plane(dtype)
    src = np.ones(ref.shape, F32)
    desc = _hk.make_desc('gain', (1, 1), False, None, None, NAN)
    _, ident, _, _ = ctx.fit_apply(desc, src, ref, 2, False, True)
    assert_same_f32(ident, ref, 'the corrected block of the identity correction')
    _, got, _, _ = ctx.fit_apply(desc, src, ref, 2, False, True, out_dtype=dtype, out_nodata=nodata)
    exp = fe.cast_out_exact(ref, dtype, _nd(nodata) if nodata == nodata else None)
    _same(got, exp, f'fit_apply out_dtype {dtype}, out_nodata {nodata}')
    _same(got, ctx.cast_out_plane(ref, dtype, nodata), f'fit_apply vs cast_out_plane, {dtype}, nodata {nodata}')


@pytest.mark.parametrize('dtype', fe.OUT_DTYPES)
def test_fit_apply_block_converts_into_a_window(ctx, dtype):
    ref = _site_plane(dtype)[:7]
    src = np.ones(ref.shape, F32)
    nodata = fe.held_nodata(dtype)[0]
    desc = _hk.make_desc('gain', (1, 1), False, None, None, NAN)
    row0, col0, rows, cols = 1, 5, ref.shape[0] - 2, 1021   # from inside a group of four, across the 1024-column block
    assert rows >= 2
    big = np.empty((rows + 4, cols + 9), dtype)
    big.view(np.uint8)[...] = SENTINEL
    before = big.copy()
    ctx.fit_apply_block(desc, src, ref, (row0, col0, rows, cols), big[2:2 + rows, 3:3 + cols], out_nodata=nodata)
    exp = fe.cast_out_exact(ref, dtype, nodata)[row0:row0 + rows, col0:col0 + cols]
    _same(np.ascontiguousarray(big[2:2 + rows, 3:3 + cols]), exp, f'fit_apply_block window, {dtype}')
    _same(np.ascontiguousarray(big[2:2 + rows, 3:3 + cols]),
          ctx.cast_out_plane(ref, dtype, nodata)[row0:row0 + rows, col0:col0 + cols], f'fit_apply_block vs cast_out_plane, {dtype}')
    outside = np.ones(big.shape, bool)
    outside[2:2 + rows, 3:3 + cols] = False
    assert (big.view(np.uint8).reshape(big.shape[0], big.shape[1], -1)[outside] ==
            before.view(np.uint8).reshape(big.shape[0], big.shape[1], -1)[outside]).all(), 'written outside the window'


# -- the refusal of an output nodata the output dtype cannot hold -----------------------------------------------------------
REFUSED = [('uint8', -9999), ('uint8', 256), ('uint8', 0.5), ('int16', 0.5), ('int16', -32769), ('uint16', 65536), ('uint32', -1),
           ('uint32', 4294967296), ('int32', 2147483648), ('float32', 1e39)]
REFUSED_AT_THE_C_BOUNDARY = REFUSED + [('uint8', NAN), ('int16', float('inf')), ('int32', float('-inf')), ('uint32', NAN)]
ACCEPTED = [('uint8', 255), ('int16', -32768), ('uint32', 4294967295), ('uint16', 0), ('int32', -2147483648), ('float32', float('inf')),
            ('float64', 1e300)]


def _entries(ctx):
    """ every entry that takes an hk_io_desc, on a tiny pair of constant rasters (across grids: average down, nearest up, exact on
    constants): name -> call(out_dtype, out_nodata) -> corrected block """
    src = np.full((16, 16), 2.0, F32)
    ref = np.full((16, 16), 6.0, F32)
    ref8 = np.full((8, 8), 6.0, F32)
    desc = _hk.make_desc('gain', (1, 1), False, None, None, None)

    def block(dt, nd):
        out = np.zeros((16, 16), dt)
        ctx.fit_apply_block(desc, src, ref, (0, 0, 16, 16), out, out_nodata=nd)
        return out

    return {
        'hk_fit_apply_io': lambda dt, nd: ctx.fit_apply(desc, src, ref, 2, False, True, out_dtype=dt, out_nodata=nd)[1],
        'hk_fit_apply_block': block,
        'hk_refspace_fit_apply': lambda dt, nd: ctx.refspace_fit_apply(desc, src, ref8, (2.0, 0.0, 2.0, 0.0), (0.5, 0.0, 0.5, 0.0), 5, 0,
                                                                      False, 2, False, out_dtype=dt, out_nodata=nd)[1],
        'hk_srcspace_fit_apply': lambda dt, nd: ctx.srcspace_fit_apply(desc, src, ref8, (0.5, 0.0, 0.5, 0.0), 0, False, 2, False,
                                                                      out_dtype=dt, out_nodata=nd)[1],
    }


def test_an_out_nodata_the_dtype_cannot_hold_is_refused(ctx, monkeypatch):
    entries = _entries(ctx)
    before = _hk.build_ledger()
    for name, call in entries.items():
        for dtype, nodata in REFUSED:       # Python: the reference's ValueError and message (homonim/raster_array.py:357-358)
            with pytest.raises(ValueError, match=rf"'nodata' value: .* cannot be safely cast to '{dtype}'"):
                call(dtype, nodata)
    # ... and the library itself, when the binding does not check first: HK_ERR_ARG before any launch
    monkeypatch.setattr(_hk, 'out_nodata_code', lambda dt, nd: (1, float(nd)))
    for name, call in entries.items():
        for dtype, nodata in REFUSED_AT_THE_C_BOUNDARY:
            with pytest.raises(ValueError, match=rf"'nodata' value: .* cannot be safely cast to '{dtype}'"):
                call(dtype, nodata)
    assert _hk.build_ledger() == before, 'a refused call launched a kernel'


def test_edge_values_of_out_nodata_are_accepted(ctx):
    """ gain 3 on a source of 2 with no nodata anywhere: the corrected block is 6 everywhere, whatever the nodata value. """
    for name, call in _entries(ctx).items():
        for dtype, nodata in ACCEPTED:
            got = call(dtype, nodata)
            assert got.dtype == np.dtype(dtype) and (got == 6).all(), (name, dtype, nodata)
    # the value itself arrives (4294967295 passes through a double): a masked pixel receives it
    ref = np.full((4, 8), 6.0, F32)
    ref[1, 2] = NAN
    desc = _hk.make_desc('gain', (1, 1), False, None, None, NAN)
    for dtype, nodata in ACCEPTED[:5]:
        _, got, _, _ = ctx.fit_apply(desc, np.ones((4, 8), F32), ref, 2, False, True, out_dtype=dtype, out_nodata=nodata)
        assert int(got[1, 2]) == nodata and int(got[0, 0]) == 6, (dtype, nodata)
    # NaN for an integer type stays what it was: 0
    _, got, _, _ = ctx.fit_apply(desc, np.ones((4, 8), F32), ref, 2, False, True, out_dtype='uint8', out_nodata=NAN)
    assert got[1, 2] == 0 and got[0, 0] == 6


def test_raster_fuse_refuses_the_nodata(ctx):
    from homonim_amd.fuse import RasterFuse
    src = np.ones((1, 32, 32), F32)
    with pytest.raises(ValueError, match=r"'nodata' value: -9999 cannot be safely cast to 'uint8'"):
        RasterFuse(src, src.copy()).process(out_profile=dict(dtype='uint8', nodata=-9999))


# -- mask_partial ------------------------------------------------------------------------------------------------------------
RASTERS = [(1, 1), (1, 300), (300, 1), (70, 257), (33, 513), (1030, 9)]   # ... wider than a 256-lane block, taller than the 1024-row grid
KERNELS = [(1, 1), (3, 3), (1, 9), (9, 1), (15, 15), (31, 5), (5, 31)]
# the structuring element (kh + 2) x (kw + 2) does not fit into the raster: nothing is covered, every output is NaN
DEGENERATE = ({((1, 1), k) for k in KERNELS} | {((1, 300), k) for k in KERNELS} | {((300, 1), k) for k in KERNELS} |
              {((1030, 9), (1, 9)), ((1030, 9), (15, 15)), ((1030, 9), (5, 31))} |
              {((5, 7), (7, 9)), ((40, 6), (3, 9)), ((6, 40), (9, 3))})
LARGER_THAN_THE_RASTER = [((5, 7), (7, 9)), ((40, 6), (3, 9)), ((6, 40), (9, 3))]   # in both directions, in one, in the other


def _planes(shape, n_bands, seed):
    g, s, o = fe.fma_values(shape, seed)
    bands = [g, o] + ([np.random.default_rng(seed + 1).uniform(0, 1, shape).astype(F32)] if n_bands == 3 else [])
    return np.stack(bands), s


def _expect(in_arr, mode, nodata, params, src, kernel):
    valid = fe.valid_exact(in_arr, mode, nodata, params)
    mask = fe.erode_exact(valid, kernel)
    nan = F32(np.nan)
    return mask, np.where(mask[None], params, nan), np.where(mask, fe.apply_two_roundings(params[0], src, params[1]), nan)


def _run_and_compare(ctx, in_arr, mode, nodata, params, src, kernel, exp, what):
    mask, p_exp, c_exp = exp
    in_nodata = {'none': None, 'nan': NAN, 'value': nodata, 'coverage': None}[mode]
    p, c, m = ctx.partial_mask(in_arr, in_nodata, params, kernel, src=src, want_params=True, want_corr=True, want_mask=True,
                               coverage=mode == 'coverage')
    np.testing.assert_array_equal(m, mask.astype(np.uint8), err_msg=f'{what}: mask')
    assert_same_f32(p, p_exp, f'{what}: params_out')
    assert_same_f32(c, c_exp, f'{what}: corr_out')
    # the two outputs agree bit for bit on the same case: covered exactly where the mask says, in every band
    np.testing.assert_array_equal(np.isnan(p).all(axis=0) | ~mask, ~mask | np.isnan(params).all(axis=0), err_msg=what)
    np.testing.assert_array_equal(np.isnan(c[~mask]), True, err_msg=what)


@pytest.mark.parametrize('kernel', KERNELS, ids=lambda k: f'k{k[0]}x{k[1]}')
@pytest.mark.parametrize('shape', RASTERS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_partial_mask_shapes_and_kernels(ctx, shape, kernel):
    h, w = shape
    n_bands = 2 + (h + kernel[0]) % 2
    params, src = _planes(shape, n_bands, seed=h * 7 + w + kernel[0])
    in_arr = src.copy()
    in_arr[h // 2, w // 3] = NAN                     # one hole in the input ...
    params[:, h // 3, (2 * w) // 3] = NAN            # ... and one in the parameters
    exp = _expect(in_arr, 'nan', None, params, src, kernel)
    if (shape, kernel) in DEGENERATE:
        assert not exp[0].any()
    else:
        assert exp[0].any() and not exp[0].all(), 'a case that tells nothing'
        two, one = fe.apply_two_roundings(params[0], src, params[1]), fe.apply_fused(params[0], src, params[1])
        assert (two != one).mean() >= 0.1            # an fmaf in place of the two roundings shows
        assert (two != one)[exp[0]].any()
    _run_and_compare(ctx, in_arr, 'nan', None, params, src, kernel, exp, f'{shape} {kernel} {n_bands} bands')


@pytest.mark.parametrize('shape, kernel', LARGER_THAN_THE_RASTER)
def test_partial_mask_kernel_larger_than_the_raster(ctx, shape, kernel):
    assert (shape, kernel) in DEGENERATE
    params, src = _planes(shape, 3, seed=23)
    exp = _expect(src, 'none', None, params, src, kernel)
    assert not exp[0].any() and np.isnan(exp[1]).all() and np.isnan(exp[2]).all()
    _run_and_compare(ctx, src, 'none', None, params, src, kernel, exp, f'{shape} {kernel}')


def test_partial_mask_at_the_largest_structuring_element(ctx):
    """ kernel (253, 255): (kh + 2) * (kw + 2) = 255 * 257 = 65535, the largest the 16-bit row counts are taken for.  The
    expectation is written out (tests/test_format_edges_cpu.py holds erode_exact to the same on the host). """
    shape, kernel = (260, 262), (253, 255)
    params, src = _planes(shape, 2, seed=29)
    nan = F32(np.nan)
    mask = np.zeros(shape, bool)
    mask[127:133, 128:134] = True                    # the central 6 x 6 pixels see no border
    exp = (mask, np.where(mask[None], params, nan), np.where(mask, fe.apply_two_roundings(params[0], src, params[1]), nan))
    _run_and_compare(ctx, src, 'none', None, params, src, kernel, exp, 'all valid')
    holed = src.copy()
    holed[130, 131] = NAN                            # one invalid pixel at the centre lies in every one of those windows
    none = np.zeros(shape, bool)
    exp = (none, np.full_like(params, nan), np.full(shape, nan, F32))
    _run_and_compare(ctx, holed, 'nan', None, params, src, kernel, exp, 'one hole at the centre')
    before = _hk.build_ledger()
    with pytest.raises(DeviceError, match='too large for mask_partial'):
        ctx.partial_mask(src, None, params, (255, 255), src=src, want_mask=True)
    assert _hk.build_ledger() == before


def _frame_and_holes(shape, seed, frame=2, share=0.004):
    rng = np.random.default_rng(seed)
    bad = rng.random(shape) < share
    if frame:
        bad[:frame], bad[-frame:], bad[:, :frame], bad[:, -frame:] = True, True, True, True
    return bad


VALIDITY = ['nan-frame-holes', 'value-0', 'value--9999', 'none', 'coverage', 'param-nans']


@pytest.mark.parametrize('n_bands', [2, 3])
@pytest.mark.parametrize('case', VALIDITY)
def test_partial_mask_validity_rules(ctx, case, n_bands):
    shape, kernel = (70, 257), (3, 5)
    params, src = _planes(shape, n_bands, seed=31)
    in_arr, mode, nodata = src.copy(), 'nan', None
    rng = np.random.default_rng(37)
    if case == 'nan-frame-holes':
        in_arr[_frame_and_holes(shape, 41)] = NAN
    elif case.startswith('value'):
        mode, nodata = 'value', float(case[6:])
        in_arr[_frame_and_holes(shape, 43, frame=0)] = nodata
        data_nan = rng.random(shape) < 0.05
        in_arr[data_nan] = NAN                       # NaN is data under a numeric nodata: valid
        assert fe.valid_exact(in_arr, mode, nodata, params)[data_nan].all()
        if nodata == 0:
            in_arr[5, 5] = F32(-0.0)                 # -0.0 equals the nodata 0
            assert not fe.valid_exact(in_arr, mode, nodata, params)[5, 5]
    elif case == 'none':
        mode = 'none'
        in_arr[rng.random(shape) < 0.3] = NAN        # no nodata: everything is valid, NaN too
        params[:, 30, 100] = NAN
    elif case == 'coverage':
        mode = 'coverage'
        one = F32(1)
        levels = np.array([one, one, one, one, one, one, np.nextafter(one, F32(2)), F32(np.inf)], F32)
        in_arr = rng.choice(levels, shape)
        rare = rng.random(shape) < 0.006
        in_arr[rare] = rng.choice(np.array([np.nextafter(one, F32(0)), 0, np.nan, 0.5], F32), int(rare.sum()))
        v = fe.valid_exact(in_arr, mode, None, params)
        assert not v[in_arr == np.nextafter(one, F32(0))].any() and v[in_arr == np.nextafter(one, F32(2))].all()
        assert v[np.isinf(in_arr)].all() and not v[np.isnan(in_arr)].any() and not v[in_arr == 0].any()
        assert all((in_arr == x).any() for x in (one, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), 0, np.inf)) and np.isnan(in_arr).any()
    else:
        # one band NaN alone leaves the parameter pixel valid (its own NaN comes through where covered), both NaN mask it
        params[0, 20, 50], params[1, 20, 120], params[:2, 20, 190] = NAN, NAN, NAN
        params[0, 45:48, 60:64] = NAN
        v = fe.valid_exact(in_arr, mode, None, params)
        assert v[20, 50] and v[20, 120] and not v[20, 190] and v[45:48, 60:64].all()
    exp = _expect(in_arr, mode, nodata, params, src, kernel)
    assert exp[0].any() and not exp[0].all()
    if case == 'param-nans':
        assert exp[0][20, 50] and exp[0][20, 120] and not exp[0][20, 190]
        assert np.isnan(exp[1][0, 20, 50]) and not np.isnan(exp[1][1, 20, 50]) and np.isnan(exp[2][20, 50])
    _run_and_compare(ctx, in_arr, mode, nodata, params, src, kernel, exp, f'{case}, {n_bands} bands')


@pytest.mark.parametrize('kernel', [(3, 5), (5, 3), (1, 1)], ids=lambda k: f'k{k[0]}x{k[1]}')
def test_partial_mask_reach_of_one_hole(ctx, kernel):
    """ A hole reaches exactly rhe = kh // 2 + 1 rows and rwe = kw // 2 + 1 columns: the pixel P is uncovered with the hole at that
    distance and covered with it one further, along either axis. """
    shape, (py, px) = (40, 60), (20, 30)
    rhe, rwe = kernel[0] // 2 + 1, kernel[1] // 2 + 1
    params, src = _planes(shape, 2, seed=47)
    for hole, covered in (((py, px + rwe), False), ((py, px + rwe + 1), True), ((py, px - rwe), False), ((py, px - rwe - 1), True),
                          ((py + rhe, px), False), ((py + rhe + 1, px), True), ((py - rhe, px), False), ((py - rhe - 1, px), True),
                          ((py + rhe, px + rwe), False), ((py + rhe + 1, px + rwe), True), ((py + rhe, px + rwe + 1), True)):
        in_arr = src.copy()
        in_arr[hole] = NAN
        exp = _expect(in_arr, 'nan', None, params, src, kernel)
        assert bool(exp[0][py, px]) is covered, (hole, kernel)
        _run_and_compare(ctx, in_arr, 'nan', None, params, src, kernel, exp, f'hole at {hole}, kernel {kernel}')


def test_partial_mask_row_strided_inputs(ctx):
    shape, kernel = (33, 300), (3, 3)
    params, src = _planes(shape, 2, seed=53)
    wide_in, wide_src = np.full((33, 340), F32(7)), np.full((33, 340), F32(-3))
    wide_src[:, 21:321] = src
    wide_in[:, 13:313] = src
    wide_in[:, 13:313][_frame_and_holes(shape, 59)] = NAN
    in_view, src_view = wide_in[:, 13:313], wide_src[:, 21:321]
    assert not in_view.flags['C_CONTIGUOUS'] and not src_view.flags['C_CONTIGUOUS']
    exp = _expect(in_view, 'nan', None, params, src_view, kernel)
    assert exp[0].any() and not exp[0].all()
    _run_and_compare(ctx, in_view, 'nan', None, params, src_view, kernel, exp, 'column slices of wider arrays')


# -- apply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (3, 1023), (5, 1025), (4100, 5), (7, 6)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_apply_two_roundings_bit_for_bit(ctx, shape):
    """ the scalar tail (width % 4 != 0), a second x block, the 4096-row grid stride; NaN, +-inf and -0.0 in each input """
    g, s, o = fe.fma_values(shape, seed=61 + shape[1])
    if shape != (1, 1):
        assert (fe.apply_two_roundings(g, s, o) != fe.apply_fused(g, s, o)).mean() >= 0.1
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32)
    rng = np.random.default_rng(67)
    if g.size > 30:
        for plane in (g, s, o):
            at = rng.choice(g.size, min(g.size // 6, 40), replace=False)
            plane.ravel()[at] = rng.choice(specials, at.size)
    exp = onp.apply(s, np.stack([g, o]))
    assert_same_f32(exp, fe.apply_two_roundings(g, s, o), 'the oracle and the statement')
    got = ctx.apply(s, np.stack([g, o]))
    assert_same_f32(got, exp, f'apply {shape}')
    zero = (exp == 0) & ~np.isnan(exp)
    np.testing.assert_array_equal(np.signbit(got[zero]), np.signbit(exp[zero]), err_msg='sign of zero')


def test_apply_specials_in_every_input(ctx):
    """ every combination of NaN, +-inf, +-0.0 and ordinary values over the three inputs, in a 49 x 7 raster: three columns of scalar tail """
    v = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.25], F32)
    g, s, o = (a.reshape(49, 7).copy() for a in np.meshgrid(v, v, v, indexing='ij'))
    exp = onp.apply(s, np.stack([g, o]))
    got = ctx.apply(s, np.stack([g, o]))
    assert_same_f32(got, exp, 'apply on special values')
    zero = exp == 0
    assert zero.any() and np.signbit(exp[zero]).any() and not np.signbit(exp[zero]).all()
    np.testing.assert_array_equal(np.signbit(got[zero]), np.signbit(exp[zero]), err_msg='sign of zero')
