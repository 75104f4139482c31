""" The host side of the device DEFLATE path (no GPU needed): the ``compressor`` hook of ``tiff.write_tiff``, the three entry
points of the C ABI with ``hk_deflate_bound``'s arithmetic and argument checks, and the ``deflate`` switch of the device
configuration.  The streams themselves are tested on the GPU (tests/test_gpu_deflate.py). """
import zlib

import numpy as np
import pytest

from homonim_amd import _hk
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.tiff import OVERVIEW_TILE, _tile_chunks, read_tiff, read_tiff_overviews, write_tiff

TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)


def _levels(a, n):
    """ some overviews of the right shapes and dtype (their values are not the point) """
    out = []
    for m in range(1, n + 1):
        out.append(np.ascontiguousarray(a[:, ::1 << m, ::1 << m]))
    return out


def _rasters():
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 255, (3, 37, 53), dtype=np.uint8, endpoint=True)
    f32 = rng.normal(0, 10, (2, 300, 200)).astype(np.float32)
    f32[:, :40] = np.nan
    return [('uint8', u8, []), ('float32', f32, _levels(f32, 2))]


class Level1:
    """ a host compressor: zlib level 1 on the writer's own tiles; remembers what it was asked for """
    def __init__(self):
        self.calls = []

    def __call__(self, array, tile):
        assert array.ndim == 3
        self.calls.append((array.shape, array.dtype, tile))
        return [zlib.compress(raw, 1) for raw in _tile_chunks(array, tile, False)]


@pytest.mark.parametrize('name, a, levels', _rasters(), ids=lambda v: v if isinstance(v, str) else '')
def test_write_tiff_takes_its_streams_from_the_compressor(tmp_path, name, a, levels):
    f = Level1()
    path = tmp_path / 'c.tif'
    write_tiff(path, a, TF, CRS('EPSG:32735'), nodata=None, overviews=levels, compressor=f)
    assert f.calls == [(a.shape, a.dtype, 512)] + [(lv.shape, lv.dtype, OVERVIEW_TILE) for lv in levels]
    back = read_tiff(path)
    assert back.array.dtype == a.dtype and back.array.tobytes() == a.tobytes()
    got = read_tiff_overviews(path)
    assert len(got) == len(levels)
    for g, lv in zip(got, levels):
        assert g.dtype == lv.dtype and g.tobytes() == lv.tobytes()
    # the file differs from the default's only in its tile data: level 6 there
    ref = tmp_path / 'ref.tif'
    write_tiff(ref, a, TF, CRS('EPSG:32735'), nodata=None, overviews=levels)
    assert read_tiff(ref).array.tobytes() == a.tobytes()
    assert ref.read_bytes() != path.read_bytes()


def test_without_a_compressor_the_file_is_what_it_was(tmp_path):
    _, a, levels = _rasters()[1]
    write_tiff(tmp_path / 'a.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), overviews=levels)
    write_tiff(tmp_path / 'b.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), overviews=levels, compressor=None)
    one = (tmp_path / 'a.tif').read_bytes()
    assert one == (tmp_path / 'b.tif').read_bytes()
    # and its tiles are zlib level 6 of the writer's own tile bytes
    for raw in _tile_chunks(a, 512, False):
        assert zlib.compress(raw, 6) in one


def test_a_wrong_number_of_streams_and_an_uncompressed_file_are_refused(tmp_path):
    _, a, _ = _rasters()[0]
    with pytest.raises(ValueError, match='streams'):
        write_tiff(tmp_path / 'x.tif', a, TF, compressor=lambda arr, tile: Level1()(arr, tile)[:-1])
    with pytest.raises(ValueError, match='streams'):
        write_tiff(tmp_path / 'x.tif', a, TF, tile=16, compressor=lambda arr, tile: Level1()(arr, tile) + [b''])
    with pytest.raises(ValueError, match='compress=False'):
        write_tiff(tmp_path / 'x.tif', a, TF, compress=False, compressor=Level1())


def test_tiff_module_imports_no_gpu_module():
    """ the hook is a callable handed in: the module's own imports stay what they were (the package's __init__ is another matter) """
    import ast
    import homonim_amd.tiff as t
    names = set()
    for node in ast.walk(ast.parse(open(t.__file__).read())):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module)
    assert names == {'mmap', 're', 'struct', 'zlib', 'typing', 'xml.sax.saxutils', 'numpy', 'homonim_amd.errors', 'homonim_amd.geo'}


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def test_the_library_exports_the_three_entry_points(lib):
    for name in ('hk_deflate_bound', 'hk_deflate_tiles', 'hk_deflate_tiles_dev'):
        assert hasattr(lib, name) and name in _hk.SIGNATURES
    assert lib.hk_abi_version() == 12 == _hk.ABI_VERSION
    assert _hk.DEFLATE_CHUNK == 16384


def _bound(itemsize, nb, h, w, tile):
    raw = tile * tile * itemsize
    chunks = [min(_hk.DEFLATE_CHUNK, raw - o) for o in range(0, raw, _hk.DEFLATE_CHUNK)]
    per_tile = 2 + sum(c + 5 for c in chunks) + 6
    n = nb * (-(-h // tile)) * (-(-w // tile))
    return n, n * (per_tile + per_tile % 2)


@pytest.mark.parametrize('shape', [(1, 1), (16, 16), (37, 53), (600, 520)])
@pytest.mark.parametrize('tile', [16, 128, 512])
@pytest.mark.parametrize('dtype', ['uint8', 'float64'])
def test_deflate_bound_is_the_stored_form_of_every_chunk(lib, shape, tile, dtype):
    for nb in (1, 3):
        assert _hk.deflate_bound(dtype, nb, *shape, tile) == _bound(np.dtype(dtype).itemsize, nb, *shape, tile)


def test_deflate_bound_refuses_bad_arguments(lib):
    for tile in (0, 24, 1024, -16, 8):
        with pytest.raises(ValueError, match='tile'):
            _hk.deflate_bound('uint8', 1, 100, 100, tile)
    import ctypes as C
    n, b = C.c_int64(), C.c_int64()
    assert lib.hk_deflate_bound(7, 1, 10, 10, 16, C.byref(n), C.byref(b)) != 0 and b'dtype' in lib.hk_last_error()
    assert lib.hk_deflate_bound(1, 1, 0, 10, 16, C.byref(n), C.byref(b)) != 0
    assert lib.hk_deflate_bound(1, 1, 10, 10, 16, None, C.byref(b)) != 0


def test_device_config_has_a_deflate_switch():
    assert RasterFuse.create_device_config()['deflate'] == 'host'
    assert RasterFuse.create_device_config(deflate='device')['deflate'] == 'device'
    for bad in ('x', '', None, 'gpu'):
        with pytest.raises(ValueError, match='deflate'):
            RasterFuse.create_device_config(deflate=bad)
