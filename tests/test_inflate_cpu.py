""" The device INFLATE path without a GPU: the decoder core of hk_inflate.hip compiled for the host and held to zlib on every
stream of tests/_inflate_streams.py; the ``inflater`` hook of ``tiff.read_tiff`` with a host inflater built on zlib; the three
entry points of the C ABI with ``hk_inflate_bound``'s arithmetic and the argument refusals; the ``inflate`` switches.  The kernels
themselves are tested on the GPU (tests/test_gpu_inflate.py), on the same streams. """
import ctypes as C
import glob
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import _inflate_streams as st
from conftest import GOLDEN_DIR, REPO
from homonim_amd import _hk
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.stats import ParamStats
from homonim_amd.tiff import BlockLayout, read_tiff, read_tiff_overviews, write_tiff

GOLDEN_TIFS = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'rasters', '*.tif')) + glob.glob(os.path.join(GOLDEN_DIR, 'tiff', '*.tif')))


# ---- 1. the decoder core on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def core(tmp_path_factory):
    """ tests/c/inflate_core_host.cpp built with the host compiler (no sanitizer); -> a function streams -> [(status, bytes)] """
    d = tmp_path_factory.mktemp('inflate_core')
    exe = d / 'inflate_core_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(REPO, 'homonim_amd', 'csrc'),
                    os.path.join(REPO, 'tests', 'c', 'inflate_core_host.cpp'), '-o', str(exe)], check=True)

    def run(streams):
        with open(d / 'in.bin', 'wb') as f:
            f.write(struct.pack('<I', len(streams)))
            for s in streams:
                f.write(struct.pack('<II', len(s.data), len(s.raw)) + s.data)
        subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], check=True, timeout=300)
        out, pos, res = (d / 'out.bin').read_bytes(), 0, []
        for s in streams:
            (status,) = struct.unpack_from('<I', out, pos)
            res.append((status, out[pos + 4:pos + 4 + len(s.raw)]))
            pos += 4 + len(s.raw)
        assert pos == len(out)
        return res

    return run


def test_the_stream_set_is_what_it_claims():
    """ (checked on the CPU, so that the GPU test can rely on it) """
    a = {s.name: s for s in st.set_a()}
    assert len(a) == 17 * 8
    for s in a.values():
        assert zlib.decompress(s.data) == s.raw
    # Z_HUFFMAN_ONLY on the strict Fibonacci chunk needs 15-bit codes; the levels stay well below
    assert st.max_code_length(a['huffman:strict-fibonacci'].data) == 15
    assert all(st.max_code_length(a[f'level{k}:strict-fibonacci'].data) <= 12 for k in (1, 6, 9))
    # random bytes at level 6 come out stored; Z_FIXED gives type-1 blocks; float32 at level 0 is two stored blocks
    assert st.block_types(a['level6:random-uint8'].data) == 0 and st.block_types(a['fixed:runs-uint8'].data) == 1
    two = a['level0:random-float32'].data
    first = two[3] | two[4] << 8   # (zlib's stored blocks are a few bytes short of 65535)
    assert len(a['level0:random-float32'].raw) == 65536 and len(two) == 2 + 2 * 5 + 65536 + 4
    assert two[2] == 0 and first < 65536 and two[2 + 5 + first] == 1
    for s in st.set_b():
        assert zlib.decompress(s.data) == s.raw
    c = {s.name: s for s in st.set_c()}
    assert len(c) == 15 and set(st.ZLIB_SAYS) == set(c) - {'more', 'fewer'}
    for name, says in st.ZLIB_SAYS.items():
        got = st.zlib_refusal(c[name].data)
        assert (says in got and says != '') or got == says, (name, got)
    # the two zlib cannot refuse, because it does not know the block's size: they inflate to one byte more, and to seven fewer
    assert len(zlib.decompress(c['more'].data)) == len(c['more'].raw) + 1
    assert len(zlib.decompress(c['fewer'].data)) == len(c['fewer'].raw) - 7
    assert zlib.decompressobj().decompress(c['trailing-garbage'].data) == c['trailing-garbage'].raw
    d = st.set_d()
    assert len(d) == 4096 and all(len(s.raw) == 256 for s in d) and {st.block_types(s.data) for s in d} == {0, 1, 2}


@pytest.mark.parametrize('which', ['a', 'b', 'c', 'd'])
def test_the_core_gives_zlibs_bytes_and_names_every_refusal(core, which):
    streams = getattr(st, 'set_' + which)()
    for s, (status, raw) in zip(streams, core(streams)):
        assert status == s.status, f'{s.name}: status {status}, expected {s.status}'
        if s.status == st.OK:
            assert raw == s.raw, f'{s.name}: the bytes differ from zlib\'s'


def test_the_status_codes_are_the_headers():
    header = open(os.path.join(REPO, 'include', 'homonim_hk.h')).read()
    for name in ('OK', 'TRUNCATED', 'BAD_HEADER', 'BAD_BLOCK', 'BAD_STORED', 'BAD_CODE', 'BAD_SYMBOL', 'FAR', 'OVERRUN', 'SHORT', 'ADLER'):
        assert f'HK_INFLATE_{name} = {getattr(st, name)}' in header
        assert getattr(_hk, 'INFLATE_' + name) == getattr(st, name)
    core_h = open(os.path.join(REPO, 'homonim_amd', 'csrc', 'hk_inflate_core.h')).read()
    assert 'OK = 0, TRUNCATED = 1, BAD_HEADER = 2, BAD_BLOCK = 3, BAD_STORED = 4, BAD_CODE = 5, BAD_SYMBOL = 6, FAR = 7, OVERRUN = 8,' in core_h
    assert 'SHORT = 9, ADLER = 10' in core_h


# ---- 2. the hook ---------------------------------------------------------------------------------------------------------
def zlib_inflater(streams, lay):
    """ what an inflater has to do, on zlib and numpy: written from the BlockLayout's own description """
    cspp = 1 if lay.separate else lay.spp
    across, down = -(-lay.width // lay.block_w), -(-lay.height // lay.block_h)
    dt = np.dtype(f'<u{lay.sample_bytes}')
    out = np.empty((lay.spp, lay.height, lay.width), dt)
    assert len(streams) == (lay.spp if lay.separate else 1) * across * down
    for idx, s in enumerate(streams):
        plane, rem = divmod(idx, across * down) if lay.separate else (0, idx)
        by, bx = divmod(rem, across)
        rows = lay.block_h if lay.tiled else min(lay.block_h, lay.height - by * lay.block_h)
        raw = zlib.decompress(s)
        assert len(raw) == rows * lay.block_w * cspp * lay.sample_bytes
        blk = np.frombuffer(raw, dt).reshape(rows, lay.block_w, cspp)
        if lay.predictor == 2:
            blk = np.cumsum(blk, axis=1, dtype=dt)
        y0, x0 = by * lay.block_h, bx * lay.block_w
        hh, ww = min(rows, lay.height - y0), min(lay.block_w, lay.width - x0)
        if lay.separate:
            out[plane, y0:y0 + hh, x0:x0 + ww] = blk[:hh, :ww, 0]
        else:
            out[:, y0:y0 + hh, x0:x0 + ww] = np.moveaxis(blk[:hh, :ww], 2, 0)
    return out


class Counting:
    def __init__(self, f=zlib_inflater):
        self.f, self.calls = f, []

    def __call__(self, streams, layout):
        assert isinstance(streams, list) and all(isinstance(s, bytes) for s in streams) and isinstance(layout, BlockLayout)
        self.calls.append((len(streams), layout))
        return self.f(streams, layout)


def same_raster(a, b):
    assert a.array.dtype == b.array.dtype and a.array.shape == b.array.shape and a.array.tobytes() == b.array.tobytes()
    assert a.transform == b.transform and a.crs == b.crs and a.metadata == b.metadata and a.descriptions == b.descriptions
    assert a.nodata == b.nodata or (np.isnan(a.nodata) and np.isnan(b.nodata))


# (number of streams, layout) of the DEFLATE files, as the files are known to be laid out
LAYOUTS = {
    'landsat8_byte': (454, BlockLayout(1, 24, 454, 267, 267, 1, 0, 0, 1)),            # 24 bands, pixel-interleaved strips of one row
    'ngi_rgb_byte_1': (72, BlockLayout(1, 3, 1421, 805, 256, 256, 1, 1, 1)),          # 256-pixel separate tiles
    'ngi_rgb_byte_2': (72, BlockLayout(1, 3, 1421, 806, 256, 256, 1, 1, 1)),
    'ngi_rgb_byte_3': (72, BlockLayout(1, 3, 1406, 792, 256, 256, 1, 1, 1)),
    'ngi_rgb_byte_4': (72, BlockLayout(1, 3, 1411, 795, 256, 256, 1, 1, 1)),
    'sentinel2_b432_byte': (454, BlockLayout(1, 3, 1361, 797, 797, 3, 0, 0, 1)),      # strips of 3 rows, the last one of 2
    'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM': (18, BlockLayout(4, 9, 20, 10, 16, 16, 1, 1, 1)),
    'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM_tile_10x20': (9, BlockLayout(4, 9, 20, 10, 10, 20, 0, 1, 1)),
    'modis_nbar': (15, BlockLayout(2, 15, 31, 18, 256, 256, 1, 1, 1)),
    'synth_bigtiff_f64_tiles': (12, BlockLayout(8, 2, 70, 90, 48, 32, 1, 1, 1)),      # 64-bit samples
    'synth_contig_strips_u8': (21, BlockLayout(1, 3, 61, 47, 47, 3, 0, 0, 1)),
    'synth_pred2_contig_i16': (6, BlockLayout(2, 4, 35, 50, 32, 16, 1, 0, 2)),        # predictor 2, pixel-interleaved tiles
    'synth_pred2_u16_strips': (6, BlockLayout(2, 2, 40, 33, 33, 16, 0, 1, 2)),        # predictor 2, separate strips, the last one short
    'synth_separate_tiles_u8': (12, BlockLayout(1, 3, 300, 270, 256, 256, 1, 1, 1)),
}


def test_the_golden_set_is_the_one_the_layouts_are_for():
    names = {os.path.splitext(os.path.basename(p))[0] for p in GOLDEN_TIFS}
    assert names == set(LAYOUTS) | {'synth_bigendian_f32'}


@pytest.mark.parametrize('path', GOLDEN_TIFS, ids=lambda p: os.path.splitext(os.path.basename(p))[0])
def test_read_tiff_with_a_host_inflater_is_read_tiff(path):
    name = os.path.splitext(os.path.basename(path))[0]
    f = Counting()
    same_raster(read_tiff(path, inflater=f), read_tiff(path))
    same_raster(read_tiff(path, inflater=None), read_tiff(path))
    if name == 'synth_bigendian_f32':
        assert f.calls == []   # a big-endian file goes the host way
    else:
        assert f.calls == [LAYOUTS[name]]


def test_an_uncompressed_file_does_not_reach_the_hook(tmp_path):
    a = np.arange(3 * 40 * 50, dtype=np.uint16).reshape(3, 40, 50)
    write_tiff(tmp_path / 'u.tif', a, Affine(1.0, 0.0, 0.0, 0.0, -1.0, 0.0), compress=False)
    f = Counting()
    assert read_tiff(tmp_path / 'u.tif', inflater=f).array.tobytes() == a.tobytes() and f.calls == []


def test_overviews_go_through_the_hook_level_by_level(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.normal(0, 10, (2, 300, 200)).astype(np.float32)
    levels = [np.ascontiguousarray(a[:, ::2, ::2]), np.ascontiguousarray(a[:, ::4, ::4])]
    write_tiff(tmp_path / 'o.tif', a, Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0), CRS('EPSG:32735'), overviews=levels)
    f = Counting()
    got, exp = read_tiff_overviews(tmp_path / 'o.tif', inflater=f), read_tiff_overviews(tmp_path / 'o.tif')
    assert len(got) == len(exp) == 2
    for g, e, lv in zip(got, exp, levels):
        assert g.dtype == e.dtype and g.tobytes() == e.tobytes() == lv.tobytes()
    assert f.calls == [(2 * 2 * 1, BlockLayout(4, 2, 150, 100, 128, 128, 1, 1, 1)), (2, BlockLayout(4, 2, 75, 50, 128, 128, 1, 1, 1))]
    g = Counting()
    same_raster(read_tiff(tmp_path / 'o.tif', inflater=g), read_tiff(tmp_path / 'o.tif'))
    assert g.calls == [(2, BlockLayout(4, 2, 300, 200, 512, 512, 1, 1, 1))]


def test_a_wrong_answer_of_the_hook_is_refused():
    path = os.path.join(GOLDEN_DIR, 'tiff', 'synth_separate_tiles_u8.tif')
    with pytest.raises(Exception, match='inflater returned'):
        read_tiff(path, inflater=lambda s, lay: np.zeros((3, 300, 271), np.uint8))
    with pytest.raises(Exception, match='inflater returned'):
        read_tiff(path, inflater=lambda s, lay: np.zeros((3, 300, 270), np.uint16))


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def test_the_library_exports_the_three_entry_points(lib):
    for name in ('hk_inflate_bound', 'hk_inflate_image', 'hk_inflate_image_dev'):
        assert hasattr(lib, name) and name in _hk.SIGNATURES
    assert lib.hk_abi_version() == 12 == _hk.ABI_VERSION


def test_the_layout_struct_is_the_headers(tmp_path):
    assert [n for n, _ in _hk.InflateLayout._fields_] == list(BlockLayout._fields)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "homonim_hk.h"', 'int main(void) {',
             '    printf("%zu\\n", sizeof(hk_inflate_layout));']
    lines += [f'    printf("%zu\\n", offsetof(hk_inflate_layout, {n}));' for n in BlockLayout._fields]
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines + ['    return 0;', '}']) + '\n')
    subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), str(src), '-o',
                    str(tmp_path / 'layout')], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(_hk.InflateLayout) == 36
    assert got[1:] == [getattr(_hk.InflateLayout, n).offset for n in BlockLayout._fields]


@pytest.mark.parametrize('lay, n_blocks, raw', [
    (BlockLayout(1, 3, 1421, 805, 256, 256, 1, 1, 1), 3 * 6 * 4, 256 * 256),          # separate tiles: one plane per block
    (BlockLayout(2, 4, 35, 50, 32, 16, 1, 0, 2), 3 * 2, 32 * 16 * 4 * 2),            # pixel-interleaved tiles: spp samples per pixel
    (BlockLayout(1, 3, 1361, 797, 797, 3, 0, 0, 1), 454, 797 * 3 * 3),               # strips, the last one short: a full strip's size
    (BlockLayout(2, 2, 40, 33, 33, 16, 0, 1, 2), 2 * 3, 33 * 16 * 2),                # separate strips
    (BlockLayout(8, 1, 1, 1, 1, 1, 0, 0, 1), 1, 8),
    (BlockLayout(4, 1, 100, 3, 3, 7, 0, 1, 1), 15, 3 * 7 * 4),                       # a slot is 84 bytes rounded up to 96
])
def test_inflate_bound_arithmetic(lib, lay, n_blocks, raw):
    assert _hk.inflate_bound(lay) == (n_blocks, raw, n_blocks * (-(-raw // 16) * 16))


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    good = BlockLayout(1, 3, 300, 270, 256, 256, 1, 1, 1)
    for field, value, word in [('sample_bytes', 3, 'sample_bytes'), ('sample_bytes', 0, 'sample_bytes'), ('sample_bytes', 16, 'sample_bytes'),
                               ('spp', 0, 'empty raster'), ('height', 0, 'empty raster'), ('width', -1, 'empty raster'),
                               ('block_w', 0, 'empty block'), ('block_h', -5, 'empty block'), ('predictor', 3, 'predictor'),
                               ('predictor', 0, 'predictor'), ('tiled', 2, '0 or 1'), ('separate', -1, '0 or 1')]:
        with pytest.raises(ValueError, match=word):
            _hk.inflate_bound(good._replace(**{field: value}))
    with pytest.raises(ValueError, match='strip'):
        _hk.inflate_bound(good._replace(tiled=0))           # a strip narrower than the image
    with pytest.raises(ValueError, match='more than'):
        _hk.inflate_bound(BlockLayout(8, 1, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1, 1, 1))
    n, r, w = C.c_int64(), C.c_int64(), C.c_int64()
    lay = _hk._inflate_layout(good)
    assert lib.hk_inflate_bound(None, C.byref(n), C.byref(r), C.byref(w)) == _hk.HK_ERR_ARG and b'NULL' in lib.hk_last_error()
    assert lib.hk_inflate_bound(C.byref(lay), None, C.byref(r), C.byref(w)) == _hk.HK_ERR_ARG
    assert lib.hk_inflate_bound(C.byref(lay), C.byref(n), C.byref(r), None) == _hk.HK_ERR_ARG
    # the two calls that need a context refuse a missing one, and null pointers, before they touch a device
    buf = (C.c_ubyte * 16)()
    off, siz, status = (C.c_int64 * 12)(), (C.c_int64 * 12)(), (C.c_int32 * 12)()
    assert lib.hk_inflate_image(None, C.byref(lay), buf, off, siz, buf, 270, 300 * 270, status) == _hk.HK_ERR_ARG
    assert b'ctx' in lib.hk_last_error()
    assert lib.hk_inflate_image_dev(None, C.byref(lay), buf, buf, buf, buf, buf, 270, 300 * 270, buf, 0) == _hk.HK_ERR_ARG


def test_the_inflate_switches_refuse_other_values(tmp_path):
    a = np.zeros((1, 8, 8), np.float32)
    for bad in ('x', '', None, 'gpu'):
        with pytest.raises(ValueError, match='inflate'):
            RasterFuse(a, a, inflate=bad)
        with pytest.raises(ValueError, match='inflate'):
            ParamStats(os.path.join(GOLDEN_DIR, 'tiff', 'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif'), inflate=bad)
    RasterFuse(a, a, inflate='host')
    RasterFuse(a, a, inflate='device')   # (arrays: nothing to inflate, no device needed)
    from homonim_amd.compare import RasterCompare
    with pytest.raises(ValueError, match='inflate'):
        RasterCompare(a, a, inflate='x')
    from homonim_amd import stats
    with pytest.raises(SystemExit):
        stats.main(['--inflate', 'x', 'nothing.tif'])
