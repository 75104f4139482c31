""" GPU tests of the written internal mask: validity beside the typed output of the block entries (cast_out_valid_kernel), average
overviews under a mask (overview_valid_kernel), and RasterFuse.process(out_profile=dict(nodata=None)) end to end.

Every comparison is exact.  Validity is held to ``~isnan`` of the float32 corrected block that TODAY's call returns, the typed samples
to today's entry, the masked overviews to the numpy statement of tests/_internal_mask.py (which tests/test_internal_mask_cpu.py holds
to a per-cell loop) and, independently, to the existing nodata build of the overview kernel. """
import ctypes as C
import warnings

import numpy as np
import pytest

from _internal_mask import holed_source, masked_overview_levels, overview_case, same_bits
from homonim_amd import (Affine, CRS, KernelModel, Model, RasterArray, RasterFuse, RefSpaceModel, SrcSpaceModel, _hk, overview_factors,
                         read_tiff_overviews)
from homonim_amd.fuse import dataset_masked
from homonim_amd.tiff import T_SUBFILE, _read_ifd, read_tiff, read_tiff_header, unpack_mask, write_tiff

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DTYPES = ['float32', 'uint8', 'uint16', 'int16', 'uint32', 'int32', 'float64']
NEW_BUILDS = [f'{k}<{t}>' for k in ('cast_out_valid_kernel', 'overview_valid_kernel')
              for t in ('float', 'unsigned char', 'unsigned short', 'short', 'unsigned int', 'int', 'double')]
CANARY = 0x5A


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def new_build_counts():
    ledger = _hk.build_ledger()
    return {k: ledger.get(k, 0) for k in NEW_BUILDS}


def test_the_library_holds_the_fourteen_new_builds(ctx):
    """ (the names the other tests watch are the ledger's own) """
    ctx.overviews(np.ones((4, 4), np.uint8), None, 1, valid=np.ones((4, 4), np.uint8))
    assert set(NEW_BUILDS) <= set(_hk.build_ledger())


# ---- 1. cast with validity, every dtype ------------------------------------------------------------------------------------------
def windows(h, w):
    """ (row0, col0, rows, cols): column offsets 0, 1, 3, 5 and widths that are no multiple of 4 """
    out = []
    for col0 in (0, 1, 3, 5):
        if col0 >= w - 1:
            continue
        cols = w - col0 if (w - col0) % 4 else w - col0 - 1
        row0 = 1 if h > 2 else 0
        out.append((row0, col0, h - row0 - (1 if h > 3 else 0), cols))
    return out


@pytest.fixture(scope='module')
def cast_blocks(ctx):
    """ per shape: the block pair, and the float32 corrected block of TODAY's float32 entry (computed once) """
    out = {}
    desc = _hk.make_desc('gain', (5, 5), False, None, np.nan, np.nan)
    for shape in ((3, 5), (37, 45), (64, 257)):
        rng = np.random.default_rng(shape[1])
        src = rng.uniform(-50.0, 400.0, shape).astype(np.float32)        # corrected values beyond both ends of uint8
        ref = (1.3 * src + rng.normal(0, 3.0, shape)).astype(np.float32)
        src[rng.random(shape) < 0.2] = np.nan
        src[0, 0] = src[-1, -1] = np.nan
        src[1, 2] = 100.0
        corr32 = np.empty(shape, np.float32)
        ctx.fit_apply_block(desc, src, ref, (0, 0, *shape), corr32)
        assert np.isnan(corr32).any() and (~np.isnan(corr32)).any()
        out[shape] = (src, ref, corr32)
    return desc, out


@pytest.mark.parametrize('shape', [(3, 5), (37, 45), (64, 257)], ids=str)
@pytest.mark.parametrize('dtype', DTYPES)
def test_cast_with_validity_every_dtype(ctx, cast_blocks, dtype, shape):
    desc, blocks = cast_blocks
    src, ref, corr32 = blocks[shape]
    dt = np.dtype(dtype)
    before = new_build_counts()
    for win in windows(*shape):
        row0, col0, rows, cols = win
        today_big = np.zeros((rows + 3, cols + 9), dt)
        today_big.view(np.uint8)[...] = CANARY
        got_big, valid_big = today_big.copy(), np.full(today_big.shape, CANARY, np.uint8)
        inner = (slice(1, 1 + rows), slice(4, 4 + cols))
        ctx.fit_apply_block(desc, src, ref, win, today_big[inner], out_nodata=None)                  # out_has_nodata = 0
        ctx.fit_apply_block(desc, src, ref, win, got_big[inner], out_nodata=None, valid_dst=valid_big[inner])
        assert got_big.tobytes() == today_big.tobytes(), f'{dtype} {shape} {win}: the typed window, or something beside it'
        exp_valid = (~np.isnan(corr32[row0:row0 + rows, col0:col0 + cols])).astype(np.uint8) * np.uint8(255)
        assert (valid_big[inner] == exp_valid).all(), f'{dtype} {shape} {win}: validity'
        outside = valid_big.copy()
        outside[inner] = CANARY
        assert (outside == CANARY).all(), f'{dtype} {shape} {win}: validity written outside the window'
        if dt.kind == 'f':   # a float output without nodata keeps its NaNs
            assert (np.isnan(got_big[inner]) == (exp_valid == 0)).all()
            assert same_bits(got_big[inner].astype(np.float32), corr32[row0:row0 + rows, col0:col0 + cols])
    name = NEW_BUILDS[DTYPES.index(dtype)]
    after = new_build_counts()
    assert after[name] > before[name] and sum(after.values()) - sum(before.values()) == after[name] - before[name]


def test_io_null_and_valid_null_keep_working(ctx, cast_blocks):
    desc, blocks = cast_blocks
    src, ref, corr32 = blocks[(37, 45)]
    lib, vp = _hk.load_library(), C.c_void_p
    corr, valid = np.empty((37, 45), np.float32), np.empty((37, 45), np.uint8)
    args = (ctx.handle, C.byref(desc), None, src.ctypes.data_as(vp), 45, ref.ctypes.data_as(vp), 45, 37, 45, None, None, 0,
            corr.ctypes.data_as(vp))
    _hk._check(lib.hk_fit_apply_block_valid(*args, valid.ctypes.data_as(vp), None, None, None))      # io NULL, no window
    assert same_bits(corr, corr32) and (valid == (~np.isnan(corr32)) * np.uint8(255)).all()
    corr[...] = 0
    before = new_build_counts()
    _hk._check(lib.hk_fit_apply_block_valid(*args, None, None, None, None))                          # valid_out NULL: today's entry
    assert same_bits(corr, corr32) and new_build_counts() == before


# ---- 2. the three families --------------------------------------------------------------------------------------------------------
def ra(array, transform):
    return RasterArray(array, CRS(), transform, nodata=float('nan'))


def family_pairs():
    """ name -> (model, src_ra, ref_ra): a shared grid; RefSpaceModel with the reference 2x and 3x coarser, mask_partial on and
    off; SrcSpaceModel with the reference 2x finer (`average`), mask_partial on and off """
    src, ref = holed_source((60, 72), seed=31)
    src, ref = src[0], ref[0]
    src_tf = Affine(10., 0., 1000., 0., -10., 5000.)
    out = {'shared': (KernelModel(Model.gain_blk_offset, (5, 5)), ra(src, src_tf), ra(ref, src_tf)),
           'shared-inpaint': (KernelModel(Model.gain_offset, (5, 5), r2_inpaint_thresh=0.999), ra(src, src_tf), ra(ref, src_tf))}
    for f in (2, 3):
        coarse = ref.reshape(60 // f, f, 72 // f, f).mean(axis=(1, 3)).astype(np.float32)
        for partial in (False, True):
            out[f'ref-{f}x-{"partial" if partial else "plain"}'] = (
                RefSpaceModel(Model.gain_blk_offset, (5, 5), mask_partial=partial), ra(src, src_tf),
                ra(coarse, Affine(10. * f, 0., 1000., 0., -10. * f, 5000.)))
    fine = np.repeat(np.repeat(ref, 2, axis=0), 2, axis=1)
    fine[7, 9] = np.nan
    for partial in (False, True):
        out[f'src-2x-finer-{"partial" if partial else "plain"}'] = (
            SrcSpaceModel(Model.gain_blk_offset, (5, 5), mask_partial=partial), ra(src, src_tf),
            ra(fine, Affine(5., 0., 1000., 0., -5., 5000.)))
    out['src-shared-partial'] = (SrcSpaceModel(Model.gain_blk_offset, (5, 5), mask_partial=True), ra(src, src_tf), ra(ref, src_tf))
    return out


FAMILIES = ['shared', 'shared-inpaint', 'ref-2x-plain', 'ref-2x-partial', 'ref-3x-plain', 'ref-3x-partial', 'src-2x-finer-plain',
            'src-2x-finer-partial', 'src-shared-partial']


@pytest.mark.parametrize('name', FAMILIES)
def test_the_three_families_return_the_validity_of_todays_block(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, src_ra, ref_ra = family_pairs()[name]
    today_ra, _ = model.fit_apply(src_ra, ref_ra)
    today = today_ra.array
    assert today.dtype == np.float32 and np.isnan(today).any() and (~np.isnan(today)).any()
    exp_valid = (~np.isnan(today)).astype(np.uint8) * np.uint8(255)
    corr_ra, param_ra, valid = model.fit_apply(src_ra, ref_ra, want_valid=True)
    assert param_ra is None and valid.dtype == np.uint8 and valid.shape == today.shape
    assert same_bits(corr_ra.array, today) and (valid == exp_valid).all()
    if 'partial' in name:   # the erosion shows: pixels the source has are invalid
        assert (exp_valid == 0)[~np.isnan(src_ra.array)].any()
    # a typed output without nodata: today's samples, the same validity
    today_u8, _ = model.fit_apply(src_ra, ref_ra, out_dtype='uint8', out_nodata=None)
    corr_u8, _, valid_u8 = model.fit_apply(src_ra, ref_ra, out_dtype='uint8', out_nodata=None, want_valid=True)
    assert corr_u8.array.dtype == np.uint8 and corr_u8.array.tobytes() == today_u8.array.tobytes() and (valid_u8 == exp_valid).all()
    assert (corr_u8.array[exp_valid == 0] == 0).all()
    if model.fuses_into(src_ra, ref_ra):
        h, w = today.shape
        win = (2, 3, h - 5, w - 7)
        corr, vraster = np.full((h, w), -1.0, np.float32), np.full((h, w), CANARY, np.uint8)
        region = (slice(1, 1 + win[2]), slice(2, 2 + win[3]))
        model.fit_apply_into(src_ra, ref_ra, win, corr[region], valid_dst=vraster[region])
        assert same_bits(corr[region], today[2:2 + win[2], 3:3 + win[3]])
        assert (vraster[region] == exp_valid[2:2 + win[2], 3:3 + win[3]]).all()
        vraster[region] = CANARY
        assert (vraster == CANARY).all()


# ---- 3. masked overviews, every dtype ---------------------------------------------------------------------------------------------
def strided(a, valid):
    """ the raster and its validity as views with row and band slack (not contiguous) """
    nb, h, w = a.shape
    big = np.zeros((nb, h + 5, w + 11), a.dtype)
    big.view(np.uint8)[...] = CANARY
    big[:, 2:2 + h, 4:4 + w] = a
    vbig = np.full((h + 3, w + 6), CANARY, np.uint8)
    vbig[1:1 + h, 5:5 + w] = valid
    return big[:, 2:2 + h, 4:4 + w], vbig[1:1 + h, 5:5 + w]


def check_levels(got, got_valid, exp, exp_valid, what):
    assert len(got) == len(got_valid) == len(exp)
    for m in range(len(exp)):
        assert got_valid[m].dtype == np.uint8 and (got_valid[m] == exp_valid[m]).all(), f'{what}: validity of level {m + 1}'
        assert same_bits(got[m], exp[m]), f'{what}: level {m + 1}'       # 0 / NaN at the invalid cells included
    assert (exp_valid[0] == 0).any() and (exp_valid[0] == 255).any()


@pytest.mark.parametrize('shape', [(5, 7), (33, 70), (129, 255)], ids=str)
@pytest.mark.parametrize('dtype', DTYPES)
def test_masked_overviews_every_dtype(ctx, monkeypatch, dtype, shape):
    a, valid = overview_case(dtype, shape, seed=shape[1] + len(dtype))
    exp, exp_valid = masked_overview_levels(a, valid, 3)
    monkeypatch.delenv('HK_OVERVIEW_STRIP_KB', raising=False)
    before = new_build_counts()
    got, got_valid = ctx.overviews(a, None, 3, valid=valid)
    check_levels(got, got_valid, exp, exp_valid, f'{dtype} {shape}')
    name = NEW_BUILDS[7 + DTYPES.index(dtype)]
    after = new_build_counts()
    assert after[name] > before[name] and sum(after.values()) - sum(before.values()) == after[name] - before[name]
    view, vview = strided(a, valid)
    assert not view.flags['C_CONTIGUOUS'] and not vview.flags['C_CONTIGUOUS']
    got, got_valid = ctx.overviews(view, None, 3, valid=vview)
    check_levels(got, got_valid, exp, exp_valid, f'{dtype} {shape} strided')
    got, got_valid = ctx.overviews(a, 12345 if dtype.startswith('float') else 1, 3, valid=valid != 0)   # bool; nodata is not read
    check_levels(got, got_valid, exp, exp_valid, f'{dtype} {shape} bool')
    plane, plane_valid = ctx.overviews(a[1], None, 3, valid=valid)                                       # a 2-D raster
    check_levels(plane, plane_valid, [e[1] for e in exp], exp_valid, f'{dtype} {shape} 2-D')
    if shape == (129, 255):
        monkeypatch.setenv('HK_OVERVIEW_STRIP_KB', '1')   # below one unit: strips of 2^3 rows
        got, got_valid = ctx.overviews(view, None, 3, valid=vview)
        check_levels(got, got_valid, exp, exp_valid, f'{dtype} {shape} 8-row strips')


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_masked_overviews_past_one_pass_and_on_the_device(ctx, dtype):
    """ 8 levels are two launches (6 + 2): the second cascades from level 6 and its validity as stored.  The device form on planes
    with slack of their own, which comes back untouched. """
    a, valid = overview_case(dtype, (300, 517), seed=3)
    valid[64:192, 128:384] = 0                                # whole tiles without a valid pixel
    n = 8
    exp, exp_valid = masked_overview_levels(a, valid, n)
    got, got_valid = ctx.overviews(a, None, n, valid=valid)
    for m in range(n):
        assert same_bits(got[m], exp[m]) and (got_valid[m] == exp_valid[m]).all(), f'level {m + 1}'
    nb, h, w = a.shape
    view, vview = strided(a, valid)
    store, vstore = view.base, vview.base
    shapes = _hk.overview_shapes(h, w, n)
    outs = [np.zeros((nb, lh + 1, lw + 5), a.dtype) for lh, lw in shapes]
    vouts = [np.full((lh + 2, lw + 3), CANARY, np.uint8) for lh, lw in shapes]
    for o in outs:
        o.view(np.uint8)[...] = CANARY
    dptrs = []
    try:
        for arr in [store, vstore] + outs + vouts:
            dptrs.append(ctx.dev_alloc(arr.nbytes))
            ctx.h2d(dptrs[-1], arr)
        d_src, d_valid, d_outs, d_vouts = dptrs[0], dptrs[1], dptrs[2:2 + n], dptrs[2 + n:]
        it = a.dtype.itemsize
        off = (2 * store.shape[2] + 4) * it                    # the view's first pixel inside its store
        ctx.overviews_valid_dev(d_src + off, dtype, nb, h, w, store.shape[2], store.shape[1] * store.shape[2],
                                d_valid + vstore.shape[1] + 5, vstore.shape[1], d_outs, [o.shape[2] for o in outs],
                                [o.shape[1] * o.shape[2] for o in outs], d_vouts, [o.shape[1] for o in vouts])
        ctx.stream_sync(0)
        for arr, d in zip(outs + vouts, dptrs[2:]):
            ctx.d2h(arr, d)
    finally:
        for d in dptrs:
            ctx.dev_free(d)
    for m, (lh, lw) in enumerate(shapes):
        assert same_bits(np.ascontiguousarray(outs[m][:, :lh, :lw]), exp[m]), f'device form, level {m + 1}'
        assert (vouts[m][:lh, :lw] == exp_valid[m]).all(), f'device form, validity of level {m + 1}'
        slack, vslack = outs[m].copy(), vouts[m].copy()
        slack[:, :lh, :lw].view(np.uint8)[...] = CANARY
        vslack[:lh, :lw] = CANARY
        assert (slack.view(np.uint8) == CANARY).all() and (vslack == CANARY).all(), f'level {m + 1} written outside its shape'


@pytest.mark.parametrize('shape', [(5, 7), (33, 70), (129, 255)], ids=str)
def test_masked_uint8_levels_equal_the_nodata_build_with_nodata_255(ctx, shape):
    """ The second, independent tie: valid values kept in 1..200 and invalid pixels set to 255 -- then no mean of valid values is
    255, a cell without a valid pixel gives 255 under the nodata build, and the two builds see the same valid sets level by level. """
    rng = np.random.default_rng(shape[0])
    a = rng.integers(1, 200, (2, *shape), dtype=np.uint8, endpoint=True)
    _, valid = overview_case('uint8', shape, seed=shape[0])
    a[:, valid == 0] = 255
    nodata_levels = ctx.overviews(a, 255, 3)
    levels, level_valids = ctx.overviews(a, None, 3, valid=valid)
    for m in range(3):
        ok = level_valids[m] != 0
        assert (level_valids[m] == (nodata_levels[m][0] != 255) * np.uint8(255)).all(), f'level {m + 1}'
        assert (level_valids[m] == (nodata_levels[m][1] != 255) * np.uint8(255)).all(), f'level {m + 1}'
        assert (levels[m][:, ok] == nodata_levels[m][:, ok]).all() and (levels[m][:, ~ok] == 0).all(), f'level {m + 1}'


# ---- 4. process, end to end ---------------------------------------------------------------------------------------------------------
TF = Affine(10., 0., 300000., 0., -10., 6200000.)
BLOCKS = {'one-block': None, 'four-blocks': dict(threads=2, max_block_mem=0.5)}


def process_pair(shape, seed):
    """ two bands; the holes of band 2 are NOT those of band 1, whose validity is the file's """
    src, ref = holed_source(shape, seed, bands=2)
    src[1, 40:60, 70:90] = np.nan
    src[1, shape[0] // 2, shape[1] // 2] = 100.0
    return src, ref


def run(tmp_path, name, src, ref, out_profile, block_config, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fuse = RasterFuse(src, ref, transform=TF)
        if block_config:
            blocks = list(fuse.block_pairs(overlap=(3, 3), max_block_mem=block_config['max_block_mem']))
            assert sum(bp.band_i == 0 for bp in blocks) >= 4
        out = fuse.process(tmp_path / f'{name}.tif', 'gain-offset', (5, 5), param_filename=tmp_path / f'{name}_param.tif',
                           out_profile=out_profile, block_config=block_config, **kw)
    return out


def subfile_types(path):
    buf = open(path, 'rb').read()
    out, nxt, first = [], None, True
    while first or nxt:
        _, t, nxt = _read_ifd(buf, None if first else nxt)
        out.append(t.get(T_SUBFILE, (0,))[0])
        first = False
    return out


@pytest.fixture(scope='module')
def baselines(tmp_path_factory):
    """ per block configuration: the default-profile run and the uint8 / nodata 0 run of the 520 x 600 pair (computed once) """
    tmp = tmp_path_factory.mktemp('baselines')
    src, ref = process_pair((520, 600), 41)
    out = {}
    for key, block_config in BLOCKS.items():
        corr32, _ = run(tmp, f'f32_{key}', src, ref, None, block_config)
        corr0, params0 = run(tmp, f'nd0_{key}', src, ref, dict(dtype='uint8', nodata=0), block_config)
        out[key] = (corr32, corr0, params0, (tmp / f'nd0_{key}_param.tif').read_bytes(), (tmp / f'nd0_{key}.tif').read_bytes())
    return src, ref, out


def check_masked_file(ctx, path, corr, valid, n_levels):
    tif, header = read_tiff(path), read_tiff_header(path)
    assert tif.nodata is None and header.nodata is None and header.has_mask
    assert (unpack_mask(tif.mask, corr.shape[2]) == (valid != 0)).all() and tif.array.tobytes() == corr.tobytes()
    masked, nodata, _ = dataset_masked(tif)
    assert np.isnan(nodata) and (np.isnan(masked) == ~np.broadcast_to(valid != 0, corr.shape)).all()
    assert (masked[:, valid != 0] == corr[:, valid != 0]).all()
    exp, exp_valid = masked_overview_levels(corr, valid, n_levels)
    levels, level_masks = read_tiff_overviews(path, masks=True)
    assert len(levels) == len(level_masks) == n_levels
    for m in range(n_levels):
        assert same_bits(levels[m], exp[m]) and (level_masks[m] == (exp_valid[m] != 0)).all(), f'level {m + 1}'
    assert subfile_types(path) == [0, 4] + [1] * n_levels + [5] * n_levels


@pytest.mark.parametrize('deflate', ['host', 'device'])
@pytest.mark.parametrize('blocks', list(BLOCKS))
def test_process_writes_the_mask_and_masked_overviews(ctx, tmp_path, baselines, blocks, deflate):
    src, ref, base = baselines
    corr32, corr0, params0, param_bytes, _ = base[blocks]
    exp_valid = (~np.isnan(corr32[0])).astype(np.uint8) * np.uint8(255)
    assert (exp_valid == 0).any() and (np.isnan(corr32[1]) != np.isnan(corr32[0])).any()
    before = new_build_counts()
    corr, params, valid = run(tmp_path, 'masked', src, ref, dict(dtype='uint8', nodata=None), BLOCKS[blocks],
                              device_config=dict(deflate=deflate), return_valid=True)
    after = new_build_counts()
    assert after['cast_out_valid_kernel<unsigned char>'] > before['cast_out_valid_kernel<unsigned char>']
    assert after['overview_valid_kernel<unsigned char>'] > before['overview_valid_kernel<unsigned char>']
    assert valid.dtype == np.uint8 and valid.shape == (520, 600) and (valid == exp_valid).all()
    assert corr.dtype == np.uint8 and (corr[:, valid != 0] == corr0[:, valid != 0]).all()
    assert (corr[0][valid == 0] == 0).all()
    check_masked_file(ctx, tmp_path / 'masked.tif', corr, valid, 1)
    # the parameter file is that of the nodata = 0 run: its rasters bit for bit, and (the baseline's tiles are zlib's) its bytes
    ptif = read_tiff(tmp_path / 'masked_param.tif')
    assert same_bits(params, params0) and ptif.mask is None and np.isnan(ptif.nodata) and same_bits(ptif.array, params0)
    assert subfile_types(tmp_path / 'masked_param.tif') == [0, 1]
    if deflate == 'host':
        assert (tmp_path / 'masked_param.tif').read_bytes() == param_bytes
    # without return_valid the call returns two values and writes the same file
    out = run(tmp_path, 'again', src, ref, dict(dtype='uint8', nodata=None), BLOCKS[blocks], device_config=dict(deflate=deflate))
    assert len(out) == 2 and (tmp_path / 'again.tif').read_bytes() == (tmp_path / 'masked.tif').read_bytes()


def test_process_two_levels(ctx, tmp_path):
    src, ref = process_pair((1100, 1030), 43)
    assert overview_factors((1100, 1030)) == [2, 4]
    corr32, _ = run(tmp_path, 'f32', src, ref, None, None)
    corr, params, valid = run(tmp_path, 'masked', src, ref, dict(dtype='uint8', nodata=None), None, return_valid=True)
    assert (valid == (~np.isnan(corr32[0])) * np.uint8(255)).all()
    check_masked_file(ctx, tmp_path / 'masked.tif', corr, valid, 2)


def test_npy_outputs_write_no_mask_and_return_valid_gives_it(tmp_path, baselines):
    src, ref, base = baselines
    corr32 = base['one-block'][0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        corr, params, valid = RasterFuse(src, ref, transform=TF).process(tmp_path / 'c.npy', 'gain-offset', (5, 5), return_valid=True,
                                                                         out_profile=dict(dtype='int16', nodata=None))
    assert (valid == (~np.isnan(corr32[0])) * np.uint8(255)).all() and np.load(tmp_path / 'c.npy').tobytes() == corr.tobytes()


# ---- 5. nothing new when not asked ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', list(BLOCKS))
def test_nothing_new_with_a_nodata_value(ctx, tmp_path, baselines, blocks):
    src, ref, base = baselines
    _, corr0, _, param_bytes, corr_bytes = base[blocks]
    before = new_build_counts()
    out = run(tmp_path, 'nd0', src, ref, dict(dtype='uint8', nodata=0), BLOCKS[blocks])
    assert new_build_counts() == before, 'a new build was launched by a call that asked for neither a mask nor validity'
    assert len(out) == 2 and out[0].tobytes() == corr0.tobytes()
    data = (tmp_path / 'nd0.tif').read_bytes()
    assert data == corr_bytes and (tmp_path / 'nd0_param.tif').read_bytes() == param_bytes
    assert subfile_types(tmp_path / 'nd0.tif') == [0, 1]
    # ... and the file is the one the writer gives these rasters without any mask keyword: same bytes, same length
    tif = read_tiff(tmp_path / 'nd0.tif')
    write_tiff(tmp_path / 'rewritten.tif', corr0, tif.transform, tif.crs, 0, tif.metadata, overviews=ctx.overviews(corr0, 0, 1))
    assert (tmp_path / 'rewritten.tif').read_bytes() == data


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_exceptions_with_a_message(ctx, cast_blocks):
    desc, blocks = cast_blocks
    src, ref, _ = blocks[(37, 45)]
    corr, valid = np.empty((37, 45), np.float32), np.empty((37, 45), np.uint8)
    lib, vp = _hk.load_library(), C.c_void_p
    win = _hk.OutWindow(20, 0, 0, 0, 37, 45, 0)              # a row stride of 20 for a window 45 wide
    rc = lib.hk_fit_apply_block_valid(ctx.handle, C.byref(desc), None, src.ctypes.data_as(vp), 45, ref.ctypes.data_as(vp), 45, 37, 45,
                                      None, None, 0, corr.ctypes.data_as(vp), valid.ctypes.data_as(vp), C.byref(win), None, None)
    assert rc != 0
    with pytest.raises(ValueError, match='stride'):
        _hk._check(rc)
    rc = lib.hk_fit_apply_block_valid(ctx.handle, C.byref(desc), None, src.ctypes.data_as(vp), 45, ref.ctypes.data_as(vp), 45, 37, 45,
                                      None, None, 0, None, valid.ctypes.data_as(vp), None, None, None)
    with pytest.raises(ValueError, match='corr_out'):
        _hk._check(rc)
    with pytest.raises(ValueError, match='valid_dst'):       # the binding: rows of the validity view 60 bytes apart, corr's 45
        ctx.fit_apply_block(desc, src, ref, (0, 0, 37, 45), corr, valid_dst=np.empty((37, 60), np.uint8)[:, :45])
    with pytest.raises(ValueError, match='valid_dst'):
        ctx.fit_apply_block(desc, src, ref, (0, 0, 37, 45), None, params_dst=np.empty((2, 37, 45), np.float32), valid_dst=valid)
    a = np.ones((2, 8, 12), np.uint8)
    for bad in (np.ones((8, 11), np.uint8), np.ones((2, 8, 12), np.uint8), np.ones((8, 12), np.float32)):
        with pytest.raises(ValueError, match='valid'):
            ctx.overviews(a, None, 1, valid=bad)
    for n in (0, -1, 32, 40):
        with pytest.raises(ValueError, match='n_levels'):
            ctx.overviews(a, None, n, valid=np.ones((8, 12), np.uint8))
    with pytest.raises(ValueError, match='validity'):
        ctx.overviews_valid_dev(0, 'uint8', 1, 8, 12, 12, 0, 0, 12, [0], [6], [0], [], [])
    levels, level_valids = ctx.overviews(a, None, 1, valid=np.ones((8, 12), np.uint8))           # (and the context still works)
    assert (levels[0] == 1).all() and (level_valids[0] == 255).all()
