""" Masked GeoTIFFs without a GPU: the 1-bit mask directory and the alpha bands in ``tiff.read_tiff`` / ``read_tiff_header`` /
``read_tiff_overviews``, the rule that decides what masks an image, its way through ``RasterFuse`` with a stubbed
context, the two new entry points of the C ABI, and the group arithmetic of hk_dataset_mask.hip as a host program
(tests/c/maskbits_core_host.cpp, built with the address and undefined-behaviour sanitizers; it runs as its own process).

The references are this suite's own: the files are made by tests/_masked_tiffs.py with ``struct`` (and by Pillow), the bits are
numpy's ``packbits``, the masked pixels ``np.where(valid, a.astype(np.float32), nan)`` compared as bytes.  The kernel itself:
tests/test_gpu_dataset_mask.py. """
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _masked_tiffs as mt
from conftest import GOLDEN_DIR, REPO
from homonim_amd import RasterFuse, _hk, tiff
from homonim_amd.errors import IoError
from homonim_amd.fuse import dataset_masked
from homonim_amd.geo import Affine, CRS
from homonim_amd.tiff import read_tiff, read_tiff_header, read_tiff_overviews, write_tiff

MASK_DIR = os.path.join(GOLDEN_DIR, 'tiff', 'mask')
TF = Affine(1., 0., 500000., 0., -1., 6200080.)


def fixture(name):
    return os.path.join(MASK_DIR, name)


def _plain(tmp_path, shape, name='plain.tif', **kw):
    """ a file write_tiff wrote: (bands, h, w) uint8 counting pixels; -> its bytes """
    a = (np.arange(int(np.prod(shape))) % 251).astype(np.uint8).reshape(shape)
    path = tmp_path / name
    write_tiff(path, a, TF, CRS('EPSG:32735'), tile=16, **kw)
    return a, path.read_bytes()


def _valid(h, w, seed=3):
    v = np.random.default_rng(seed + 31 * w + h).random((h, w)) < 0.5
    v[0, 0], v[-1, -1] = True, False
    return v


# ---- 1. the bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compression', sorted(mt.COMPRESSIONS))
@pytest.mark.parametrize('width', [1, 7, 8, 9, 17, 33])
def test_bit_rows_in_strips_decode_to_the_bits_they_were_packed_from(tmp_path, width, compression):
    h = 11   # two strips of 8 rows, the last one short
    _, data = _plain(tmp_path, (1, h, width))
    valid = _valid(h, width)
    path = tmp_path / 'masked.tif'
    path.write_bytes(mt.append_mask(data, valid, compression=mt.COMPRESSIONS[compression]))
    for hooks in ({}, dict(lzw=_hk.lzw_image_host)):
        tif = read_tiff(path, **hooks)
        assert tif.mask.dtype == np.uint8 and tif.mask.shape == (h, (width + 7) // 8)
        assert mt.same_bytes(tif.mask, mt.pack_bits(valid))   # (as stored: the pad bits of these files are 0)
    assert read_tiff_header(path).has_mask


@pytest.mark.parametrize('compression', sorted(mt.COMPRESSIONS))
def test_a_tiled_mask_decodes_to_the_bits_it_was_packed_from(tmp_path, compression):
    h, w = 35, 40   # 3 x 3 tiles of 16 x 16, the last ones partial
    a, data = _plain(tmp_path, (2, h, w))
    valid = _valid(h, w)
    path = tmp_path / 'masked.tif'
    path.write_bytes(mt.append_mask(data, valid, tile=16, compression=mt.COMPRESSIONS[compression]))
    for hooks in ({}, dict(lzw=_hk.lzw_image_host)):
        tif = read_tiff(path, **hooks)
        assert mt.same_bytes(tif.mask, mt.pack_bits(valid))
        assert mt.same_bytes(tif.array, a) and tif.alpha_bands == () and tif.mask_band is None
    # a width that is no multiple of 8 inside tiles: the bits past the width are padding of the tile, whatever they hold
    h, w = 20, 37
    _, data = _plain(tmp_path, (1, h, w), 'p2.tif')
    valid = _valid(h, w)
    path.write_bytes(mt.append_mask(data, valid, tile=16, compression=mt.COMPRESSIONS[compression]))
    got = read_tiff(path).mask
    assert got.shape == (h, 5) and (mt.unpack_bits(got, w) == valid).all()


# ---- 2. the rule --------------------------------------------------------------------------------------------------------------
class _StubContext:
    """ Context.dataset_mask as the numpy statement; keeps what it was handed """

    def __init__(self):
        self.calls = []

    def dataset_mask(self, array, mask=None, alpha=None):
        self.calls.append((array, mask, alpha))
        h, w = array.shape[-2:]
        valid = mt.unpack_bits(mask, w) if mask is not None else alpha != 0
        return mt.masked_f32(array, valid)


@pytest.fixture
def stub(monkeypatch):
    ctx = _StubContext()
    monkeypatch.setattr(_hk, 'default_context', lambda: ctx)
    return ctx


def _nan_nodata(nodata):
    return isinstance(nodata, float) and np.isnan(nodata)


@pytest.mark.parametrize('name', ['rgb_mask_tiles_deflate.tif', 'rgb_mask_strips_lzw.tif'])
def test_an_internal_mask_beats_the_nodata_tag(stub, name):
    tif = read_tiff(fixture(name))
    assert tif.nodata == 0 and tif.alpha_bands == () and tif.mask_band is None
    assert (mt.unpack_bits(tif.mask, 64) == mt.fixture_valid()).all()
    array, nodata, _ = dataset_masked(tif)
    assert _nan_nodata(nodata) and mt.same_bytes(array, mt.masked_f32(tif.array, mt.fixture_valid()))
    (planes, mask, alpha), = stub.calls
    assert planes is tif.array and mask is tif.mask and alpha is None
    hd = read_tiff_header(fixture(name))
    assert hd.has_mask and hd.alpha_bands == () and hd.nodata == 0


def test_the_nodata_tag_beats_an_alpha_band(stub):
    tif = read_tiff(fixture('rgba_u8_nodata.tif'))
    assert tif.nodata == 0 and tif.alpha_bands == (3,) and tif.mask_band is None and tif.mask is None
    array, nodata, _ = dataset_masked(tif)
    assert nodata == 0 and array.dtype == np.uint8 and mt.same_bytes(array, tif.array[:3]) and not stub.calls


@pytest.mark.parametrize('name, bands, dtype', [('rgba_u8.tif', 4, 'uint8'), ('la_u8.tif', 2, 'uint8'), ('rgba_u16.tif', 4, 'uint16')])
def test_a_trailing_alpha_band_masks_the_image(stub, name, bands, dtype):
    tif = read_tiff(fixture(name))
    assert tif.array.shape == (bands, 80, 64) and tif.array.dtype == dtype and tif.nodata is None and tif.mask is None
    assert tif.alpha_bands == (bands - 1,) and tif.mask_band == bands - 1
    alpha = tif.array[bands - 1]
    assert ((alpha != 0) == mt.fixture_valid()).all() and len(np.unique(alpha)) > 2   # (valid is `!= 0`, not `== max`)
    array, nodata, _ = dataset_masked(tif)
    assert _nan_nodata(nodata) and array.shape == (bands - 1, 80, 64)
    assert mt.same_bytes(array, mt.masked_f32(tif.array[:bands - 1], mt.fixture_valid()))
    (planes, mask, got_alpha), = stub.calls
    assert mask is None and mt.same_bytes(planes, tif.array[:bands - 1]) and mt.same_bytes(got_alpha, alpha)
    hd = read_tiff_header(fixture(name))
    assert hd.alpha_bands == (bands - 1,) and not hd.has_mask and hd.count == bands


def test_pillow_reads_the_same_pixels_from_its_own_files():
    Image = pytest.importorskip('PIL.Image')
    for name, bands in (('rgba_u8.tif', 4), ('la_u8.tif', 2)):
        with Image.open(fixture(name)) as im:
            theirs = np.moveaxis(np.asarray(im), 2, 0)
        assert mt.same_bytes(read_tiff(fixture(name)).array, theirs)


@pytest.mark.parametrize('name, alpha, keep', [('five_band_alpha.tif', 4, [0, 1, 2, 3]), ('alpha_not_last.tif', 1, [0, 2, 3]),
                                               ('rgba_f32.tif', 3, [0, 1, 2])])
def test_an_alpha_band_that_does_not_qualify_is_dropped_and_not_applied(stub, name, alpha, keep):
    tif = read_tiff(fixture(name))
    assert tif.alpha_bands == (alpha,) and tif.mask_band is None and tif.mask is None and tif.nodata is None
    array, nodata, descriptions = dataset_masked(tif)
    assert nodata is None and array.dtype == tif.array.dtype and mt.same_bytes(array, tif.array[keep]) and not stub.calls
    assert len(descriptions) == len(keep)


# ---- 3. refusals and skips ----------------------------------------------------------------------------------------------------
def test_a_mask_of_another_size_a_predictor_and_fill_order_2_are_refused_by_name(tmp_path):
    _, data = _plain(tmp_path, (1, 20, 24))
    path = tmp_path / 'bad.tif'
    path.write_bytes(mt.append_mask(data, _valid(20, 16)))
    with pytest.raises(IoError, match=r'internal mask is 20 x 16, the image 20 x 24'):
        read_tiff(path)
    with pytest.raises(IoError, match=r'20 x 16'):
        read_tiff_header(path)
    path.write_bytes(mt.append_mask(data, _valid(20, 24), compression=mt.DEFLATE, predictor=2))
    with pytest.raises(IoError, match=r'predictor 2 for a 1-bit mask'):
        read_tiff(path)
    path.write_bytes(mt.append_mask(data, _valid(20, 24), fill_order=2))
    with pytest.raises(IoError, match=r'FillOrder 2'):
        read_tiff(path)
    path.write_bytes(mt.append_mask(data, _valid(20, 24), predictor=1, fill_order=1))   # (the tags at their defaults are fine)
    assert (mt.unpack_bits(read_tiff(path).mask, 24) == _valid(20, 24)).all()


def test_a_mask_of_an_overview_is_no_overview_and_no_mask_of_the_image(tmp_path):
    a = (np.arange(64 * 48) % 199).astype(np.uint8).reshape(1, 64, 48)
    ovr = a[:, ::2, ::2].copy()
    path = tmp_path / 'ovr.tif'
    write_tiff(path, a, TF, CRS('EPSG:32735'), tile=16, overviews=[ovr])
    data = path.read_bytes()
    path.write_bytes(mt.append_mask(data, _valid(32, 24), subfile=5))
    levels = read_tiff_overviews(path)
    assert len(levels) == 1 and mt.same_bytes(levels[0], ovr)
    tif = read_tiff(path)
    assert tif.mask is None and not read_tiff_header(path).has_mask
    # the image's own mask behind the overview and its mask: found, the others still skipped
    valid = _valid(64, 48)
    path.write_bytes(mt.append_mask(path.read_bytes(), valid, tile=16, compression=mt.LZW))
    assert (mt.unpack_bits(read_tiff(path).mask, 48) == valid).all() and len(read_tiff_overviews(path)) == 1


# ---- 4. files without a mask ---------------------------------------------------------------------------------------------------
def test_every_other_committed_file_reads_as_ever(stub):
    tiff_dir = os.path.join(GOLDEN_DIR, 'tiff')
    decoded = dict(np.load(os.path.join(tiff_dir, 'decoded.npz')))
    decoded.update(np.load(os.path.join(tiff_dir, 'lzw', 'lzw_decoded.npz')))
    paths = sorted(glob.glob(os.path.join(tiff_dir, '*.tif')) + glob.glob(os.path.join(tiff_dir, 'lzw', '*.tif')) +
                   glob.glob(os.path.join(GOLDEN_DIR, 'rasters', '*.tif')) + glob.glob(os.path.join(GOLDEN_DIR, 'rotated', '*.tif')))
    assert len(paths) >= 15
    held = 0
    for p in paths:
        tif, hd = read_tiff(p, lzw=_hk.lzw_image_host), read_tiff_header(p)
        assert tif.mask is None and tif.alpha_bands == () and tif.mask_band is None, p
        assert hd.alpha_bands == () and not hd.has_mask, p
        array, nodata, descriptions = dataset_masked(tif)
        assert array is tif.array and descriptions is tif.descriptions, p
        assert nodata is tif.nodata or nodata == tif.nodata or _nan_nodata(nodata) and _nan_nodata(tif.nodata), p
        key = os.path.splitext(os.path.basename(p))[0]
        if key in decoded:
            assert mt.same_bytes(tif.array, decoded[key].astype(tif.array.dtype).reshape(tif.array.shape)), p
            held += 1
    assert held >= 10 and not stub.calls


# ---- 5. RasterFuse ------------------------------------------------------------------------------------------------------------
def _reference_file(tmp_path, descriptions=('red', 'green', 'blue')):
    path = tmp_path / 'ref.tif'
    write_tiff(path, mt.fixture_reference(), Affine(2., 0., 0., 0., 2., 0.), None, nodata=float('nan'), tile=16, descriptions=descriptions)
    return path


def test_raster_fuse_pairs_the_three_bands_of_an_rgba_file_with_a_three_band_reference(stub, tmp_path):
    """ on the parent commit: ValueError('`ref` has fewer bands than `src`') """
    tif = read_tiff(fixture('rgba_u8.tif'))
    fuse = RasterFuse(fixture('rgba_u8.tif'), _reference_file(tmp_path))
    (planes, mask, alpha), = stub.calls
    assert mask is None and mt.same_bytes(planes, tif.array[:3]) and mt.same_bytes(alpha, tif.array[3])
    assert fuse._src.shape == (3, 80, 64) and fuse._src.dtype == np.float32 and _nan_nodata(fuse._src_nodata)
    assert fuse._ref.shape == (3, 40, 32) and fuse._ref_descriptions == ('red', 'green', 'blue')
    # (a file without geo tags has the identity transform, which is south-up: RasterFuse brings it north-up by flipping the rows)
    assert mt.same_bytes(fuse._src[:, ::-1], mt.masked_f32(tif.array[:3], mt.fixture_valid()))


def test_raster_fuse_hands_an_internal_mask_to_the_context_and_ignores_the_nodata_tag(stub, tmp_path):
    name = fixture('rgb_mask_tiles_deflate.tif')
    tif = read_tiff(name)
    ref = tmp_path / 'ref.tif'
    write_tiff(ref, mt.fixture_reference(), Affine(2., 0., 500000., 0., -2., 6200080.), CRS('EPSG:32735'), nodata=float('nan'), tile=16)
    fuse = RasterFuse(name, ref)
    (planes, mask, alpha), = stub.calls
    assert alpha is None and mt.same_bytes(planes, tif.array) and mt.same_bytes(mask, tif.mask)
    assert _nan_nodata(fuse._src_nodata) and mt.same_bytes(fuse._src, mt.masked_f32(tif.array, mt.fixture_valid()))


def test_a_masked_reference_file_loses_its_alpha_band_and_keeps_the_names_of_the_others(stub, tmp_path):
    src = np.ones((3, 80, 64), np.float32)
    fuse = RasterFuse(src, fixture('rgba_u16.tif'), transform=TF, crs=CRS('EPSG:32735'))
    assert fuse._ref.shape == (3, 80, 64) and fuse._ref.dtype == np.float32 and _nan_nodata(fuse._ref_nodata)
    assert len(fuse._ref_descriptions) == 3 and len(stub.calls) == 1
    assert fuse._param_descriptions(9)[:3] == ['B1_GAIN', 'B2_GAIN', 'B3_GAIN']


def test_arrays_and_files_without_a_mask_never_reach_the_context(stub, tmp_path):
    a = np.ones((2, 20, 24), np.float32)
    RasterFuse(a, a.copy())
    _, data = _plain(tmp_path, (2, 20, 24), 'src.tif')
    RasterFuse(tmp_path / 'src.tif', a, ref_transform=TF, ref_crs=CRS('EPSG:32735'))
    assert not stub.calls


# ---- 6. the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def test_the_library_exports_the_entry_points_and_the_binding_knows_them(lib):
    for name in ('hk_dataset_mask', 'hk_dataset_mask_dev'):
        assert hasattr(lib, name) and name in _hk.SIGNATURES
    assert (_hk.MASK_BITS, _hk.MASK_ALPHA) == (0, 1)
    assert lib.hk_abi_version() == _hk.ABI_VERSION
    header = open(os.path.join(REPO, 'include', 'homonim_hk.h')).read()
    assert 'HK_MASK_BITS = 0, HK_MASK_ALPHA = 1' in header and 'hk_dataset_mask and hk_dataset_mask_dev' in header
    assert hasattr(_hk.Context, 'dataset_mask') and hasattr(_hk.Context, 'dataset_mask_dev')


def test_the_nine_builds_are_on_the_ledger(lib):
    names = [b for b in _hk.build_ledger() if 'dataset_mask_kernel' in b]
    assert len(names) == 9 and sum('ALPHA' in b for b in names) == 2 and sum('BITS' in b for b in names) == 7, names


def test_every_bad_argument_is_refused_by_name_without_a_device(lib):
    ctx = C.create_string_buffer(4096)          # (never looked at: every call below is refused before the context is)
    buf = C.create_string_buffer(4096)
    p, out = C.cast(buf, C.c_void_p), C.cast(buf, C.POINTER(C.c_float))
    HK_ERR_ARG = -1
    good = dict(ctx=C.cast(ctx, C.c_void_p), planes=p, dtype=1, n_bands=2, height=3, width=20, stride=20, mask=p, mask_kind=0,
                mask_stride=3, out=out, out_stride=20)

    def refused(text, **change):
        a = dict(good, **change)
        rc = lib.hk_dataset_mask(*a.values())
        assert rc == HK_ERR_ARG and text in lib.hk_last_error().decode(), (change, rc, lib.hk_last_error())
        dev = list(a.values())
        dev.insert(7, 0), dev.extend([0, 0])   # band_stride; out_band_stride, stream
        dev[11] = C.cast(a['out'], C.c_void_p)
        rc = lib.hk_dataset_mask_dev(*dev)
        assert rc == HK_ERR_ARG and text in lib.hk_last_error().decode(), (change, rc, lib.hk_last_error())

    assert list(good) == ['ctx', 'planes', 'dtype', 'n_bands', 'height', 'width', 'stride', 'mask', 'mask_kind', 'mask_stride', 'out', 'out_stride']
    refused('ctx is NULL', ctx=None)
    refused('planes is NULL', planes=None)
    refused('mask is NULL', mask=None)
    refused('out is NULL', out=None)
    for dtype in (-1, 7):
        refused('dtype', dtype=dtype)
    for kind in (-1, 2):
        refused('mask_kind', mask_kind=kind)
    for dtype in (0, 3, 4, 5, 6):   # an alpha band of anything but uint8 / uint16
        refused('alpha takes dtype uint8 or uint16', dtype=dtype, mask_kind=1, mask_stride=20)
    refused('n_bands', n_bands=0)
    refused('height', height=0)
    refused('width', width=-1)
    refused('stride 19', stride=19)
    refused('out_stride 19', out_stride=19)
    refused('mask_stride 2', mask_stride=2)                             # ceil(20 / 8) = 3 bytes
    refused('mask_stride 19', mask_kind=1, mask_stride=19)              # an alpha row: 20 samples


# ---- 7. the group arithmetic as a host program ---------------------------------------------------------------------------------
def test_the_group_functions_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / 'maskbits_core_host_san'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(REPO, 'homonim_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'maskbits_core_host.cpp'),
                    '-o', str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, res.stderr[-3000:]
    # widths 1 .. 130 x two addresses x three patterns, seven sample types under bits and two under alpha
    assert res.stdout.split('\n')[:-1] == [f'bits: {130 * 2 * 3 * 7} rows', f'alpha: {130 * 2 * 3 * 2} rows']
