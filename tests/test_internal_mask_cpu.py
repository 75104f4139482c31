""" CPU tests of the written internal mask (homonim_amd/tiff.py write_tiff(mask=, overview_masks=), read_tiff_overviews(masks=True))
and of the numpy statement of the masked overviews that the GPU tests hold the kernels to (tests/_internal_mask.py).

The reader of masked files (read_tiff / read_tiff_header / fuse.dataset_masked) is the one tests/test_dataset_mask_cpu.py holds to
files it assembles itself; Pillow's libtiff is a second, independent reader of the directories written here. """
import struct

import numpy as np
import pytest

from _internal_mask import masked_overview_levels, masked_overview_levels_loop, same_bits
from homonim_amd import _hk
from homonim_amd.fuse import dataset_masked
from homonim_amd.geo import Affine
from homonim_amd.tiff import (T_BITS, T_COMPRESSION, T_FILL_ORDER, T_HEIGHT, T_PHOTOMETRIC, T_PREDICTOR, T_SPP, T_SUBFILE, T_TILE_H,
                              T_TILE_W, T_WIDTH, _read_ifd, read_tiff, read_tiff_header, read_tiff_overviews, unpack_mask, write_tiff)

TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 6500000.0)

# (dtype, (bands, h, w), tile): 3 x 4 tiles of 64 with partial ones and a width that is no multiple of 8; 3 x 3 tiles of 16
CASES = [('uint8', (3, 150, 201), 64), ('float32', (1, 37, 45), 16)]


def raster(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 200.0, shape).astype(dtype)
    mask = rng.random(shape[1:]) >= 0.3
    mask[:3, :] = False                     # a frame, a hole, and whole bytes of either kind
    mask[:, -2:] = False
    mask[10:14, 8:24] = False
    mask[20:23, 16:32] = True
    return a, mask


def directories(path):
    """ the tags of every directory of the file, in chain order """
    buf = open(path, 'rb').read()
    out, nxt, first = [], None, True
    while first or nxt:
        _, t, nxt = _read_ifd(buf, None if first else nxt)
        out.append(t)
        first = False
    return out


class _StubContext:
    """ Context.dataset_mask as its numpy statement (float32 of the samples, NaN where the packed mask bit is 0) """

    def dataset_mask(self, array, mask=None, alpha=None):
        out = array.astype(np.float32)
        out[:, ~unpack_mask(mask, array.shape[-1])] = np.nan
        return out


# ---- 1. the main image's mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bigtiff', ['no', 'yes'])
@pytest.mark.parametrize('compress', [True, False], ids=['deflate', 'raw'])
@pytest.mark.parametrize('dtype, shape, tile', CASES, ids=['u8x3', 'f32x1'])
def test_a_written_mask_reads_back(tmp_path, monkeypatch, dtype, shape, tile, compress, bigtiff):
    a, mask = raster(dtype, shape, seed=5)
    path = tmp_path / 'm.tif'
    write_tiff(path, a, TF, None, None, tile=tile, compress=compress, bigtiff=bigtiff, mask=mask)
    assert open(path, 'rb').read(4) == (b'II\x2b\x00' if bigtiff == 'yes' else b'II\x2a\x00')
    tif = read_tiff(path)
    assert tif.nodata is None and tif.mask is not None and tif.mask.shape == (shape[1], -(-shape[2] // 8))
    assert (unpack_mask(tif.mask, shape[2]) == mask).all()
    assert tif.array.dtype == a.dtype and tif.array.tobytes() == a.tobytes()
    assert read_tiff_header(path).has_mask and read_tiff_header(path).nodata is None
    monkeypatch.setattr(_hk, 'default_context', lambda: _StubContext())
    masked, nodata, _ = dataset_masked(tif)
    assert np.isnan(nodata) and masked.dtype == np.float32
    assert (np.isnan(masked) == ~np.broadcast_to(mask, a.shape)).all()          # NaN exactly outside the mask
    assert (masked[:, mask] == a[:, mask].astype(np.float32)).all()
    # the directory is the one the writer's contract names
    main, md = directories(path)
    assert md[T_SUBFILE] == (4,) and (md[T_HEIGHT][0], md[T_WIDTH][0]) == shape[1:] and md[T_BITS] == (1,) and md[T_SPP] == (1,)
    assert md[T_PHOTOMETRIC] == (4,) and T_FILL_ORDER not in md and T_PREDICTOR not in md
    assert md[T_TILE_W] == md[T_TILE_H] == main[T_TILE_W] == (tile,) and md[T_COMPRESSION] == ((8,) if compress else (1,))
    assert T_SUBFILE not in main


def test_an_array_mask_is_valid_where_it_is_not_zero(tmp_path):
    a, mask = raster('uint8', (1, 37, 45), seed=6)
    as_bytes = np.where(mask, np.uint8(7), np.uint8(0))
    as_bytes[mask & (np.arange(45) % 2 == 0)] = 255
    write_tiff(tmp_path / 'b.tif', a, TF, None, None, tile=16, mask=as_bytes)
    write_tiff(tmp_path / 'c.tif', a, TF, None, None, tile=16, mask=mask)
    assert (tmp_path / 'b.tif').read_bytes() == (tmp_path / 'c.tif').read_bytes()


# ---- 2. Pillow's libtiff as an independent reader -------------------------------------------------------------------------------
# (Pillow opens no band-separate uncompressed file of several bands, with or without a mask: that case stays with section 1)
@pytest.mark.parametrize('dtype, shape, tile, compress, bigtiff', [
    ('uint8', (3, 150, 201), 64, True, 'no'), ('uint8', (3, 150, 201), 64, True, 'yes'), ('float32', (1, 37, 45), 16, True, 'no'),
    ('float32', (1, 37, 45), 16, True, 'yes'), ('float32', (1, 37, 45), 16, False, 'no'), ('float32', (1, 37, 45), 16, False, 'yes')])
def test_pillow_reads_the_samples_and_the_mask(tmp_path, monkeypatch, dtype, shape, tile, compress, bigtiff):
    """ Frame 0 gives the samples of the first plane, and a frame of mode '1' of the image's size gives the mask.  Pillow's table of
    pixel modes has no row for PhotometricInterpretation 4 (transparency mask), which the mask directory carries as TIFF 6.0
    asks: the row is added here -- it names the mode the 1-bit frame is handed back in -- and libtiff decodes the tiles. """
    Image = pytest.importorskip('PIL.Image')
    features = pytest.importorskip('PIL.features')
    if not features.check('libtiff'):
        pytest.skip('Pillow without libtiff')
    from PIL import TiffImagePlugin
    monkeypatch.setitem(TiffImagePlugin.OPEN_INFO, (b'II', 4, (1,), 1, (1,), ()), ('1', '1'))
    a, mask = raster(dtype, shape, seed=7)
    path = tmp_path / 'p.tif'
    write_tiff(path, a, TF, None, None, tile=tile, compress=compress, bigtiff=bigtiff, mask=mask)
    with Image.open(path) as im:
        assert im.n_frames == 2
        im.seek(0)
        first = np.asarray(im)
        assert first.shape == shape[1:] and first.tobytes() == a[0].tobytes()
        im.seek(1)
        assert im.mode == '1' and im.size == (shape[2], shape[1])
        assert (np.asarray(im) == mask).all()


# ---- 3. masks of overview levels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compress', [True, False], ids=['deflate', 'raw'])
def test_overview_masks_read_back_and_leave_the_other_readers_alone(tmp_path, compress):
    a, mask = raster('uint8', (3, 150, 201), seed=8)
    levels, level_masks = masked_overview_levels(a, mask, 2)
    assert [lv.shape for lv in levels] == [(3, 75, 101), (3, 38, 51)]
    path = tmp_path / 'o.tif'
    write_tiff(path, a, TF, None, None, tile=64, compress=compress, overviews=levels, mask=mask, overview_masks=level_masks)
    got, got_masks = read_tiff_overviews(path, masks=True)
    assert len(got) == len(got_masks) == 2
    for m in range(2):
        assert got[m].tobytes() == levels[m].tobytes()
        assert got_masks[m].dtype == bool and (got_masks[m] == (level_masks[m] != 0)).all()
    plain = read_tiff_overviews(path)                      # the default: exactly the levels
    assert isinstance(plain, list) and [p.tobytes() for p in plain] == [lv.tobytes() for lv in levels]
    tif = read_tiff(path)                                  # the main mask, not a level's
    assert (unpack_mask(tif.mask, 201) == mask).all() and tif.array.tobytes() == a.tobytes()
    # order: main image, its mask, the levels, their masks; a level's mask is reduced + mask at the overview tile size
    subs = [d.get(T_SUBFILE, (0,))[0] for d in directories(path)]
    assert subs == [0, 4, 1, 1, 5, 5]
    for d, lv in zip(directories(path)[4:], levels):
        assert (d[T_HEIGHT][0], d[T_WIDTH][0]) == lv.shape[1:] and d[T_TILE_W] == d[T_TILE_H] == (128,) and d[T_PHOTOMETRIC] == (4,)
    # levels without masks: None per level
    write_tiff(path, a, TF, None, None, tile=64, compress=compress, overviews=levels, mask=mask)
    assert read_tiff_overviews(path, masks=True)[1] == [None, None]


def test_the_main_image_lies_where_it_lies_without_a_mask(tmp_path):
    a, mask = raster('uint8', (3, 150, 201), seed=9)
    write_tiff(tmp_path / 'plain.tif', a, TF, None, None, tile=64)
    write_tiff(tmp_path / 'masked.tif', a, TF, None, None, tile=64, mask=mask)
    plain, masked = (tmp_path / 'plain.tif').read_bytes(), (tmp_path / 'masked.tif').read_bytes()
    assert masked[:len(plain)] != plain and len(masked) > len(plain)
    n = struct.unpack('<H', plain[8:10])[0]
    nxt = 10 + 12 * n                                       # the next-directory pointer of the first directory
    assert plain[nxt:nxt + 4] == b'\0\0\0\0' and struct.unpack('<I', masked[nxt:nxt + 4])[0] == len(plain)
    assert masked[:nxt] == plain[:nxt] and masked[nxt + 4:len(plain)] == plain[nxt + 4:]


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------
def test_argument_errors(tmp_path):
    a, mask = raster('uint8', (3, 150, 201), seed=10)
    levels, level_masks = masked_overview_levels(a, mask, 2)
    path = tmp_path / 'x.tif'
    with pytest.raises(ValueError, match='nodata'):
        write_tiff(path, a, TF, None, 0, mask=mask)
    with pytest.raises(ValueError, match='nodata'):
        write_tiff(path, a, TF, None, 0, overviews=levels, overview_masks=level_masks)
    with pytest.raises(ValueError, match='mask of shape'):
        write_tiff(path, a, TF, None, None, mask=mask[:, :-1])
    with pytest.raises(ValueError, match='mask of shape'):
        write_tiff(path, a, TF, None, None, mask=np.broadcast_to(mask, a.shape))
    with pytest.raises(ValueError, match='1 overview masks for 2'):
        write_tiff(path, a, TF, None, None, overviews=levels, mask=mask, overview_masks=level_masks[:1])
    with pytest.raises(ValueError, match='overview mask of shape'):
        write_tiff(path, a, TF, None, None, overviews=levels, mask=mask, overview_masks=[level_masks[0], level_masks[1][:-1]])
    assert not path.exists()


def test_without_a_mask_the_bytes_are_those_of_the_defaults(tmp_path):
    for k, (dtype, shape, tile) in enumerate(CASES):
        a, _ = raster(dtype, shape, seed=11)
        nodata = 0 if dtype == 'uint8' else float('nan')
        lv = masked_overview_levels(a, np.ones(shape[1:], bool), 1)[0]
        write_tiff(tmp_path / 'a.tif', a, TF, None, nodata, tile=tile, overviews=lv)
        write_tiff(tmp_path / 'b.tif', a, TF, None, nodata, tile=tile, overviews=lv, mask=None, overview_masks=None)
        assert (tmp_path / 'a.tif').read_bytes() == (tmp_path / 'b.tif').read_bytes()
        assert [d.get(T_SUBFILE, (0,))[0] for d in directories(tmp_path / 'a.tif')] == [0, 1]


# ---- 5. the numpy statement of the masked overviews against a per-cell loop ----------------------------------------------------------
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_the_numpy_statement_equals_a_per_cell_loop(dtype):
    rng = np.random.default_rng(12)
    h, w = 7, 9
    a = rng.integers(0, 255, (h, w), dtype=np.uint8, endpoint=True) if dtype == 'uint8' else rng.normal(0, 1e4, (h, w)).astype(np.float32)
    valid = (rng.random((h, w)) >= 0.4).astype(np.uint8) * np.uint8(255)
    valid[0:2, 0:2] = 0            # a cell without a valid pixel
    valid[2:4, 2:4] = 0
    valid[2, 3] = 1                # one valid pixel, and "valid" is "not 0"
    valid[-1, :] = 0               # the odd last row is invalid
    valid[4:6, 4:6] = 255
    if dtype == 'float32':
        a[4, 5] = np.nan           # a NaN under a valid bit is data
    levels, valids = masked_overview_levels(a, valid, 3)
    loop_levels, loop_valids = masked_overview_levels_loop(a, valid, 3)
    assert [lv.shape for lv in levels] == [(4, 5), (2, 3), (1, 2)]
    for m in range(3):
        assert same_bits(levels[m], loop_levels[m]), f'level {m + 1}'
        assert (valids[m] == loop_valids[m]).all() and set(np.unique(valids[m])) <= {0, 255}
    assert valids[0][0, 0] == 0 and (levels[0][0, 0] == 0 or np.isnan(levels[0][0, 0]))
    assert valids[0][1, 1] == 255 and levels[0][1, 1] == a[2, 3]
    if dtype == 'float32':
        assert valids[0][2, 2] == 255 and np.isnan(levels[0][2, 2])
    # all valid: the statement of the unmasked average, integer rounding half up
    u = np.array([[1, 2], [2, 2]], np.uint8)
    assert masked_overview_levels(u, np.ones((2, 2), bool), 1)[0][0].tolist() == [[2]]          # 7 / 4 -> 2
    assert masked_overview_levels(u, np.array([[1, 1], [0, 0]]), 1)[0][0].tolist() == [[2]]     # 3 / 2 -> 2 (half up)
