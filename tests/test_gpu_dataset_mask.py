""" GPU tests of the per-dataset mask (hk_dataset_mask.hip; hk_dataset_mask / hk_dataset_mask_dev; the file branches of RasterFuse).

The reference is the numpy statement of tests/_masked_tiffs.py -- ``np.where(valid, a.astype(np.float32), nan)`` -- and every
comparison is on the BYTES: a valid float32 keeps its bits (-0.0, denormals, a NaN's payload), a masked pixel is 0x7FC00000.  The
shapes are the smallest at which the grouping of 8 pixels per lane can go wrong: below, at and above one group, one 16-byte store,
one wave (64 groups = 512 pixels: a whole wave of whole groups stores through an exchange of its halves); the device entry is run
on rows that allow the wide accesses and on rows that do not, inside planes filled with a canary.  End to end, a masked file gives exactly the bytes the same pipeline gives on the numpy-masked arrays. """
import os

import numpy as np
import pytest

import _masked_tiffs as mt
from conftest import GOLDEN_DIR
from homonim_amd import RasterCompare, RasterFuse, _hk
from homonim_amd.geo import Affine, CRS
from homonim_amd.tiff import read_tiff, write_tiff

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

MASK_DIR = os.path.join(GOLDEN_DIR, 'tiff', 'mask')
SHAPES = [(1, 1, 1), (3, 3, 7), (3, 2, 8), (1, 3, 9), (2, 3, 63), (2, 2, 64), (3, 2, 65), (1, 4, 130), (4, 5, 515),
          (2, 3, 1100),   # (two whole waves of 64 groups -- the path that exchanges a wave's halves -- and a part of one)
          (2, 2051, 9), (1, 4100, 515)]   # (taller than the 2048 grid rows of launch_dataset_mask: a workgroup walks 2 and 3 rows)
MASKS = ['all', 'none', 'random', 'last', 'alternating']
BUILDS = [(d, 'bits') for d in _hk.DTYPE_CODES] + [('uint8', 'alpha'), ('uint16', 'alpha')]
CANARY = 0xC3


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def pixels(dtype, shape, seed):
    """ (bands, h, w) of ``dtype``: the whole range of the integers; floats with -0.0, NaN, denormals and, float64, values that
    round to infinity and to zero in float32 """
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind in 'ui':
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    a = rng.normal(0., 1e3, shape).astype(dt)
    special = [-0.0, np.nan, 1e-45, -1e-40, 3.4e38] if dt == np.float32 else [-0.0, np.nan, 1e-310, 1e39, -1e39, 3.5e38, 1e-46, 16777217.0]
    flat = a.reshape(-1)
    for k, v in enumerate(special):
        flat[(k * 7) % flat.size if flat.size > len(special) else k % flat.size] = v
    return a


def validity(kind, h, w, seed):
    if kind == 'all':
        return np.ones((h, w), bool)
    if kind == 'none':
        return np.zeros((h, w), bool)
    if kind == 'random':
        return np.random.default_rng(seed).random((h, w)) < 0.5
    if kind == 'last':   # only the last pixel of each row invalid
        v = np.ones((h, w), bool)
        v[:, -1] = False
        return v
    bits = np.unpackbits(np.tile(np.array([0x80, 0x01], np.uint8), (h, (w + 15) // 16 + 1)), axis=1)   # bytes 0x80, 0x01, 0x80, ...
    return bits[:, :w].astype(bool)


def mask_source(how, valid, dtype, seed):
    """ -> (the keyword of Context.dataset_mask, the array): packed bits (pad bits SET: they must not be looked at) or an alpha plane """
    if how == 'bits':
        h, w = valid.shape
        padded = np.ones((h, (w + 7) // 8 * 8), bool)
        padded[:, :w] = valid
        return 'mask', np.packbits(padded, axis=1)
    top = np.iinfo(dtype).max
    alpha = np.random.default_rng(seed).integers(1, top, valid.shape, dtype=dtype, endpoint=True)   # valid: anything but 0
    return 'alpha', np.where(valid, alpha, 0).astype(dtype)


def on_device(ctx, a, how, m, pad):
    """ hk_dataset_mask_dev on planes, mask and output whose rows are ``pad`` elements (mask bits: bytes) longer than needed and
    which have a spare row per band, all filled with a canary: -> the output; every byte outside [0, w) of every row of it, and all
    of the inputs, must come back unchanged. """
    nb, h, w = a.shape
    src = np.empty((nb, h + 1, w + pad), a.dtype)
    src.view(np.uint8)[...] = CANARY
    src[:, :h, :w] = a
    msk = np.empty((h + 1, m.shape[1] + pad), m.dtype)
    msk.view(np.uint8)[...] = CANARY
    msk[:h, :m.shape[1]] = m
    out = np.empty((nb, h + 1, w + pad), np.float32)
    out.view(np.uint8)[...] = CANARY
    d = [ctx.dev_alloc(x.nbytes) for x in (src, msk, out)]
    try:
        for p, x in zip(d, (src, msk, out)):
            ctx.h2d(p, x)
        ctx.dataset_mask_dev(d[0], a.dtype.name, nb, h, w, src.shape[2], src.shape[1] * src.shape[2], d[1],
                             _hk.MASK_BITS if how == 'bits' else _hk.MASK_ALPHA, msk.shape[1], d[2], out.shape[2],
                             out.shape[1] * out.shape[2])
        ctx.stream_sync(0)
        back = [np.empty_like(x) for x in (src, msk, out)]
        for p, x in zip(d, back):
            ctx.d2h(x, p)
    finally:
        for p in d:
            ctx.dev_free(p)
    assert back[0].tobytes() == src.tobytes() and back[1].tobytes() == msk.tobytes(), 'an input was written'
    slack = back[2].copy()
    slack[:, :h, :w].view(np.uint8)[...] = CANARY
    assert (slack.view(np.uint8) == CANARY).all(), 'the output was written outside [0, width) of its rows'
    return np.ascontiguousarray(back[2][:, :h, :w])


@pytest.mark.parametrize('dtype, how', BUILDS, ids=[f'{d}-{k}' for d, k in BUILDS])
def test_every_build_both_entries_equal_the_numpy_statement_byte_for_byte(ctx, dtype, how):
    before = _hk.build_ledger()
    for si, shape in enumerate(SHAPES):
        a = pixels(dtype, shape, seed=100 + si)
        for mi, kind in enumerate(MASKS):
            valid = validity(kind, shape[1], shape[2], seed=7 * si + mi)
            key, m = mask_source(how, valid, dtype, seed=si + mi)
            exp = mt.masked_f32(a, valid)
            what = f'{dtype} {how} {shape} {kind}'
            assert mt.same_bytes(ctx.dataset_mask(a, **{key: m}), exp), f'hk_dataset_mask {what}'
            # rows that start where the wide accesses are allowed (a stride of a multiple of 16 elements), and rows that do not
            for pad in (-shape[2] % 16 + 16, 3):
                assert mt.same_bytes(on_device(ctx, a, how, m, pad), exp), f'hk_dataset_mask_dev {what} pad {pad}'
    after = _hk.build_ledger()
    launched = [b for b in after if after[b] > before.get(b, 0) and 'dataset_mask_kernel' in b]
    assert len(launched) == 1 and how.upper() in launched[0], launched   # one build per (dtype, kind): this one


def test_a_2d_raster_and_strided_views_give_the_same_bytes(ctx):
    a = pixels('uint16', (4, 9, 70), seed=5)
    valid = validity('random', 9, 70, seed=6)
    exp = mt.masked_f32(a[:3], valid)
    alpha = np.where(valid, a[3] | 1, 0).astype(np.uint16)
    held = a.copy()
    held[3] = alpha
    assert mt.same_bytes(ctx.dataset_mask(held[:3], alpha=held[3]), exp)            # the alpha band of the file's own array
    assert mt.same_bytes(ctx.dataset_mask(held[0], alpha=held[3]), exp[0])          # 2-D in, 2-D out
    wide = np.zeros((3, 9, 100), np.uint16)
    wide[:, :, 5:75] = a[:3]
    assert mt.same_bytes(ctx.dataset_mask(wide[:, :, 5:75], mask=mt.pack_bits(valid)), exp)   # strided rows
    with pytest.raises(ValueError, match='exactly one'):
        ctx.dataset_mask(a[:3])
    with pytest.raises(ValueError, match='`mask` must be uint8 of shape'):
        ctx.dataset_mask(a[:3], mask=mt.pack_bits(valid)[:, :-1])
    with pytest.raises(ValueError, match='alpha band masks uint8 and uint16'):
        ctx.dataset_mask(a[:3].astype(np.int16), alpha=alpha.astype(np.int16))


def test_the_host_entry_in_many_chunks_gives_the_bytes_of_one(ctx, monkeypatch):
    a = pixels('uint8', (3, 300, 130), seed=9)
    valid = validity('random', 300, 130, seed=10)
    bits = mt.pack_bits(valid)
    exp = mt.masked_f32(a, valid)
    one = ctx.dataset_mask(a, mask=bits)
    before = sum(n for b, n in _hk.build_ledger().items() if 'dataset_mask_kernel' in b)
    monkeypatch.setenv('HK_STAGE_CHUNK_KB', '16')   # a device row of all bands is 3 x 192 x 5 + 32 bytes: 5 rows per chunk
    many = ctx.dataset_mask(a, mask=bits)
    alpha = np.where(valid, 200, 0).astype(np.uint8)
    many_alpha = ctx.dataset_mask(a, alpha=alpha)
    launches = sum(n for b, n in _hk.build_ledger().items() if 'dataset_mask_kernel' in b) - before
    assert launches == 2 * 60, launches
    assert mt.same_bytes(one, exp) and mt.same_bytes(many, exp) and mt.same_bytes(many_alpha, exp)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
SRC_TF, REF_TF, EPSG = Affine(1., 0., 500000., 0., -1., 6200080.), Affine(2., 0., 500000., 0., -2., 6200080.), CRS('EPSG:32735')


@pytest.fixture(scope='module')
def references(tmp_path_factory):
    """ the reference rasters of the end-to-end tests, written once: on the 32 x 40 grid and on the sources' own grid, each with
    the geo-referencing of the internal-mask fixtures and with that of Pillow's files (none: the identity) """
    d = tmp_path_factory.mktemp('refs')
    coarse = mt.fixture_reference()
    fine = np.repeat(np.repeat(coarse, 2, axis=1), 2, axis=2) + np.float32(0.01)
    out = {}
    for geo, (tf_c, tf_f, crs) in {'utm': (REF_TF, SRC_TF, EPSG), 'plain': (Affine(2., 0., 0., 0., 2., 0.), Affine.identity(), None)}.items():
        for grid, arr, tf in (('coarse', coarse, tf_c), ('same', fine, tf_f)):
            path = d / f'ref_{geo}_{grid}.tif'
            write_tiff(path, arr, tf, crs, nodata=float('nan'), tile=16)
            out[geo, grid] = (str(path), arr, tf, crs)
    return out


@pytest.mark.parametrize('inflate', ['host', 'device'])
@pytest.mark.parametrize('grid', ['coarse', 'same'])
@pytest.mark.parametrize('name, geo', [('rgb_mask_tiles_deflate.tif', 'utm'), ('rgb_mask_strips_lzw.tif', 'utm'), ('rgba_u8.tif', 'plain')])
def test_a_masked_file_gives_the_bytes_of_the_numpy_masked_arrays_end_to_end(references, name, geo, grid, inflate):
    src_path = os.path.join(MASK_DIR, name)
    ref_path, ref, ref_tf, crs = references[geo, grid]
    tif = read_tiff(src_path)
    masked = mt.masked_f32(tif.array[:3], mt.fixture_valid())
    assert np.isnan(masked).any() and not np.isnan(masked).all()
    kw = dict(model='gain-offset', kernel_shape=(5, 5), param_filename=True, build_ovw=False)
    corr, params = RasterFuse(src_path, ref_path, inflate=inflate).process(None, **kw)
    exp_corr, exp_params = RasterFuse(masked, ref, src_nodata=float('nan'), ref_nodata=float('nan'), transform=tif.transform,
                                      ref_transform=ref_tf, crs=crs, ref_crs=crs).process(None, **kw)
    assert corr.shape == (3, 80, 64) and params is not None and np.isfinite(corr).any()
    assert mt.same_bytes(corr, exp_corr) and mt.same_bytes(params, exp_params)
    table = RasterCompare(src_path, ref_path, inflate=inflate).process(threads=1)
    exp_table = RasterCompare(masked, ref, src_nodata=float('nan'), ref_nodata=float('nan'), transform=tif.transform, ref_transform=ref_tf,
                              crs=crs, ref_crs=crs).process(threads=1)
    assert table == exp_table and len(table) == 4 and table['Mean']['n'] > 0


def test_the_nine_builds_are_on_the_ledger():
    names = sorted(b for b in _hk.build_ledger() if 'dataset_mask_kernel' in b)
    assert len(names) == 9 and sum('ALPHA' in b for b in names) == 2 and sum('BITS' in b for b in names) == 7, names
