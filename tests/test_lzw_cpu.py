""" The LZW reader without a GPU: ``tiff.lzw_decode`` and the decoder core of hk_lzw.hip compiled for the host (the stand-alone
program tests/c/lzw_core_host.cpp, plain and under AddressSanitizer + UBSan, and ``hk_lzw_image_host`` of the library) held to
Pillow's libtiff -- six files it wrote (tests/golden/tiff/lzw, tools/make_lzw_fixtures.py) -- and to the streams of
tests/_lzw_streams.py, good and malformed, which Pillow reads back where it can open the layout.  The kernel is tested on the GPU
(tests/test_gpu_lzw.py), on the same streams. """
import ctypes as C
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _lzw_streams as st
from conftest import GOLDEN_DIR, REPO
from homonim_amd import _hk
from homonim_amd.errors import IoError
from homonim_amd.tiff import LZW_REASONS, BlockLayout, lzw_decode, read_tiff

LZW_DIR = os.path.join(GOLDEN_DIR, 'tiff', 'lzw')
FIXTURES = ('lzw_u8_noise_strips', 'lzw_u8_smooth_strips', 'lzw_u8_flat_strips', 'lzw_rgb_pred2_strips', 'lzw_u16_pred2_strips',
            'lzw_f32_strips')


@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


@pytest.fixture(scope='module')
def all_streams():
    raw, data, rec = st.chain_walk_tile()
    return st.good_set() + st.malformed_set() + st.sweep_set(256) + [st.Stream('chain-walk', data, raw, st.OK)]


def _build_core(d, flags):
    exe = d / ('lzw_core_host' + ('_san' if flags else ''))
    subprocess.run(['g++', '-O1' if flags else '-O2', '-g', '-std=c++17', '-Wall', '-Werror', *flags, '-I', os.path.join(REPO, 'homonim_amd', 'csrc'),
                    os.path.join(REPO, 'tests', 'c', 'lzw_core_host.cpp'), '-o', str(exe)], check=True)
    return exe


def _run_core(exe, d, streams):
    """ -> [(status, bytes)] of the stand-alone program over ``streams`` """
    with open(d / 'in.bin', 'wb') as f:
        f.write(struct.pack('<I', len(streams)))
        for s in streams:
            f.write(struct.pack('<II', len(s.data), len(s.raw)) + s.data)
    res = subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, res.stderr[-3000:]
    out, pos, got = (d / 'out.bin').read_bytes(), 0, []
    for s in streams:
        (status,) = struct.unpack_from('<I', out, pos)
        got.append((status, out[pos + 4:pos + 4 + len(s.raw)]))
        pos += 4 + len(s.raw)
    assert pos == len(out)
    return got


def _python_status(s):
    """ -> (status, bytes or None) of ``tiff.lzw_decode``, the status from the reason it names """
    try:
        return st.OK, lzw_decode(s.data, len(s.raw))
    except IoError as ex:
        (status,) = [k for k, reason in enumerate(LZW_REASONS) if k and reason in str(ex)]
        return status, None


# ---- 1. the fixtures Pillow wrote --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_a_pillow_file_reads_as_pillow_reads_it(lib, name):
    exp = np.load(os.path.join(LZW_DIR, 'lzw_decoded.npz'))[name]
    calls = []

    def hook(streams, layout):
        calls.append(layout)
        return _hk.lzw_image_host(streams, layout)

    for got in (read_tiff(os.path.join(LZW_DIR, name + '.tif')).array, read_tiff(os.path.join(LZW_DIR, name + '.tif'), lzw=hook).array):
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    assert len(calls) == 1 and calls[0].predictor == (2 if 'pred2' in name else 1) and calls[0].tiled == 0
    # (a DEFLATE hook is not asked about an LZW file)
    assert read_tiff(os.path.join(LZW_DIR, name + '.tif'), inflater=lambda s, lay: 1 / 0).array.tobytes() == exp.tobytes()


def test_the_fixtures_show_what_they_are_there_for():
    """ counted from the files with the helper's tracer (tools/make_lzw_fixtures.py prints the same) """
    def records(name):
        raster = read_tiff(os.path.join(LZW_DIR, name + '.tif'))
        seen = []
        read_tiff(os.path.join(LZW_DIR, name + '.tif'), lzw=lambda s, lay: (seen.append((s, lay)), raster.array)[1])
        (streams, lay), = seen
        row = lay.width * lay.spp * lay.sample_bytes
        return [st.trace(s, min(lay.block_h, lay.height - k * lay.block_h) * row) for k, s in enumerate(streams)]

    noise, smooth, flat = records('lzw_u8_noise_strips'), records('lzw_u8_smooth_strips'), records('lzw_u8_flat_strips')
    assert max(r['max_width'] for r in noise) == 12 and all(r['clears'] >= 2 for r in noise[:-1])
    assert sum(r['kwkwk'] for r in smooth) >= 20 and sum(r['codes'] for r in smooth) > 20 * sum(r['kwkwk'] for r in smooth)
    assert max(r['max_len'] for r in flat) > 64 and all(r['kwkwk'] * 10 >= (r['codes'] - 3) * 9 for r in flat)


# ---- 2. the encoder's streams, 3. the malformed set --------------------------------------------------------------------------
def test_the_stream_set_is_what_it_claims():
    good = {s.name: s for s in st.good_set()}
    assert len(good) == 11 * len(st.SWITCHES)
    t = st.trace(good['noise-96x96:0'].data, 96 * 96)
    assert t['max_width'] == 12 and t['clears'] >= 2                      # widths 9 -> 12 and a Clear inside one block
    t = st.trace(good['noise-96x96:1'].data, 96 * 96)
    assert t['clears'] == 1 and t['codes'] > 2 * 4096                     # never cleared: the table is full for most of the block
    t = st.trace(good['flat-128x128:0'].data, 128 * 128)
    assert t['max_len'] > 64 and t['kwkwk'] * 10 >= t['codes'] * 9        # strings far longer than a wave, KwKwK throughout
    assert st.trace(good['noise-96x96:5'].data, 96 * 96)['clears'] == 0   # starts without a Clear, never emits one
    assert all(st.trace(good[f'flat-cut-9875:{i}'].data, 9875)['cut'] == 136 for i in range(len(st.SWITCHES)))   # a long last string, cut
    assert sum(st.trace(good[f'smooth-cut-9001:{i}'].data, 9001)['cut'] >= 1 for i in range(len(st.SWITCHES))) >= 3   # short ones
    assert 9875 % 16 and 9001 % 16
    assert st.trace(good['flat-odd-10007:0'].data, 10007)['cut'] == 0 and 10007 % 16
    assert good['noise-96x96:0'].data.startswith(good['noise-96x96:2'].data[:-1])   # the same stream without its end code
    raw, data, rec = st.chain_walk_tile()
    assert len(raw) == 512 * 512 >= 4 * 65536 and rec['far'] >= 1 and rec['clears'] == 1
    assert [s.status for s in st.malformed_set()] == [0, 1, 0, 1, 2, 0, 3, 4, 5, 0]


def test_lzw_decode_reads_every_stream_and_names_every_refusal(all_streams):
    for s in all_streams:
        status, raw = _python_status(s)
        assert status == s.status, f'{s.name}: {st.STATUS_NAMES[status]}, expected {st.STATUS_NAMES[s.status]}'
        assert raw is None or raw == s.raw, s.name


def test_the_host_core_reads_every_stream_and_names_every_refusal(all_streams, tmp_path):
    for s, (status, raw) in zip(all_streams, _run_core(_build_core(tmp_path, []), tmp_path, all_streams)):
        assert status == s.status, f'{s.name}: status {status}, expected {s.status}'
        assert s.status != st.OK or raw == s.raw, f'{s.name}: the bytes differ'


def test_the_host_core_is_clean_under_the_sanitizers(all_streams, tmp_path):
    """ the stand-alone program built with AddressSanitizer and UBSan over the whole set, good and malformed: every stream in an
    allocation that ends with it, every slot exactly its size """
    exe = _build_core(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    for s, (status, raw) in zip(all_streams, _run_core(exe, tmp_path, all_streams)):
        assert status == s.status and (s.status != st.OK or raw == s.raw), s.name


def test_pillow_reads_the_encoders_streams():
    Image = pytest.importorskip('PIL.Image')
    features = pytest.importorskip('PIL.features')
    if not features.check('libtiff'):
        pytest.skip("Pillow's libtiff is absent")
    opened = 0
    safe = [k for k, kw in enumerate(st.SWITCHES) if kw in st.LIBTIFF_SWITCHES]
    assert len(safe) == 4
    for s in st.good_set():   # every stream libtiff's rules allow (st.LIBTIFF_SWITCHES) as a file of one strip of one row
        if int(s.name.rsplit(':', 1)[1]) not in safe:
            continue
        lay = st.Layout(s.name, 'u1', 1, 1, len(s.raw), 0, 1, 0, 1)
        a = np.frombuffer(s.raw, np.uint8).reshape(1, 1, -1)
        got = np.array(Image.open(io.BytesIO(st.build_tiff(a, lay, streams=[s.data]))))
        assert got.tobytes() == s.raw, s.name
    for lay in st.LAYOUTS:    # ... and the layouts Pillow can open
        a, streams = st.layout_streams(lay, st.LIBTIFF_SWITCHES)
        try:
            im = Image.open(io.BytesIO(st.build_tiff(a, lay, streams=streams)))
        except Exception:     # (3 x 16 bits, 64-bit samples: no mode of Pillow's)
            assert lay.name in ('tiles16-contig3-u16', 'strips-separate-u64'), lay.name
            continue
        got = np.array(im)
        opened += 1
        exp = a[0] if got.ndim == 2 else np.moveaxis(a, 0, 2)   # (of separate planes Pillow shows the first)
        assert got.shape == exp.shape and got.astype(exp.dtype).tobytes() == exp.tobytes(), lay.name
    assert opened == len(st.LAYOUTS) - 2


def test_a_refused_block_is_named_and_its_neighbours_are_untouched(lib):
    ms = st.malformed_set()
    lay = BlockLayout(1, 1, 10, 300 * len(ms), 300, 10, 1, 0, 1)   # one tile of 10 x 300 per stream, side by side
    packed = _hk._pack_streams([s.data for s in ms])
    out, status = _hk.lzw_image_host_packed(*packed, lay, strict=False)
    assert status.tolist() == [s.status for s in ms]
    for k, s in enumerate(ms):
        if s.status == st.OK:
            assert out[0, :, 300 * k:300 * (k + 1)].tobytes() == s.raw, s.name
    with pytest.raises(IoError, match=re.escape(f'block 1 is refused: {LZW_REASONS[st.TRUNCATED]}')):
        _hk.lzw_image_host([s.data for s in ms], lay)
    for k, s in enumerate(ms):   # every reason by name, from the library and from lzw_decode
        if s.status != st.OK:
            with pytest.raises(IoError, match=re.escape(f'block 0 is refused: {LZW_REASONS[s.status]}')):
                _hk.lzw_image_host([s.data], BlockLayout(1, 1, 10, 300, 300, 10, 1, 0, 1))
            with pytest.raises(IoError, match=re.escape(LZW_REASONS[s.status])):
                lzw_decode(s.data, len(s.raw))


@pytest.mark.parametrize('lay', st.LAYOUTS, ids=lambda lay: lay.name)
def test_every_layout_through_the_host_decoder_and_through_read_tiff(lib, lay, tmp_path):
    a, streams = st.layout_streams(lay)
    got = _hk.lzw_image_host(streams, BlockLayout(*st.block_layout(lay)))
    assert got.dtype == a.dtype and got.tobytes() == a.tobytes()
    if lay.name != 'tiles512-u8':   # (a megabyte through the Python decoder: the chain-walk tile has been there)
        (tmp_path / 'f.tif').write_bytes(st.build_tiff(a, lay, streams=streams))
        assert read_tiff(tmp_path / 'f.tif').array.tobytes() == a.tobytes()
        assert read_tiff(tmp_path / 'f.tif', lzw=_hk.lzw_image_host).array.tobytes() == a.tobytes()


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------
def test_the_status_codes_are_the_headers():
    header = open(os.path.join(REPO, 'include', 'homonim_hk.h')).read()
    for name in st.STATUS_NAMES:
        assert f'HK_LZW_{name} = {getattr(st, name)}' in header
        assert getattr(_hk, 'LZW_' + name) == getattr(st, name)
    assert 'enum Status { OK = 0, TRUNCATED = 1, OLD_STYLE = 2, BAD_FIRST = 3, BAD_CODE = 4, SHORT = 5 };' in \
        open(os.path.join(REPO, 'homonim_amd', 'csrc', 'hk_lzw_core.h')).read()
    assert len(LZW_REASONS) == 6


def test_the_library_exports_the_three_entry_points(lib):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'homonim_hk.h')).read(), flags=re.S)
    args = {name: re.search(name + r'\s*\(([^)]*)\)\s*;', header).group(1).split(',')
            for name in ('hk_lzw_image', 'hk_lzw_image_host', 'hk_lzw_image_dev', 'hk_inflate_image', 'hk_inflate_image_dev')}
    for name in ('hk_lzw_image', 'hk_lzw_image_host', 'hk_lzw_image_dev'):
        assert hasattr(lib, name) and name in _hk.SIGNATURES and len(_hk.SIGNATURES[name][1]) == len(args[name])
    norm = lambda decls: [' '.join(d.split()) for d in decls]   # noqa: E731
    assert norm(args['hk_lzw_image']) == norm(args['hk_inflate_image'])
    assert norm(args['hk_lzw_image_dev']) == norm(args['hk_inflate_image_dev'])
    assert norm(args['hk_lzw_image_host']) == norm(args['hk_inflate_image'])[1:]   # the same without the context
    assert _hk.SIGNATURES['hk_lzw_image'] == _hk.SIGNATURES['hk_inflate_image']
    assert _hk.SIGNATURES['hk_lzw_image_dev'] == _hk.SIGNATURES['hk_inflate_image_dev']
    assert lib.hk_abi_version() == 12 == _hk.ABI_VERSION


def test_bad_arguments_are_refused_before_anything_else_is_looked_at(lib):
    good = BlockLayout(1, 3, 300, 270, 256, 256, 1, 1, 1)
    buf = (C.c_ubyte * 16)()
    off, siz, status = (C.c_int64 * 12)(), (C.c_int64 * 12)(), (C.c_int32 * 12)()
    for bad, word in ((good._replace(predictor=3), b'predictor'), (good._replace(predictor=0), b'predictor'),
                      (good._replace(tiled=0), b'strip'), (good._replace(sample_bytes=3), b'sample_bytes')):
        lay = _hk._inflate_layout(bad)
        # (null streams and no context behind the bad layout: the layout is what is named)
        assert lib.hk_lzw_image_host(C.byref(lay), None, off, siz, buf, 270, 300 * 270, status) == _hk.HK_ERR_ARG
        assert word in lib.hk_last_error()
        assert lib.hk_lzw_image(None, C.byref(lay), None, off, siz, buf, 270, 300 * 270, status) == _hk.HK_ERR_ARG
        assert lib.hk_lzw_image_dev(None, C.byref(lay), None, buf, buf, buf, buf, 270, 300 * 270, buf, 0) == _hk.HK_ERR_ARG
    lay = _hk._inflate_layout(good)
    assert lib.hk_lzw_image(None, C.byref(lay), buf, off, siz, buf, 270, 300 * 270, status) == _hk.HK_ERR_ARG and b'ctx' in lib.hk_last_error()
    assert lib.hk_lzw_image_host(C.byref(lay), None, off, siz, buf, 270, 300 * 270, status) == _hk.HK_ERR_ARG and b'NULL' in lib.hk_last_error()
    assert lib.hk_lzw_image_host(C.byref(lay), buf, off, siz, buf, 269, 300 * 270, status) == _hk.HK_ERR_ARG and b'stride' in lib.hk_last_error()

    # The host decoder has no context in front of its checks: every refusal of a layout, a pointer, a stride or a band stride, one
    # wrong thing at a time, with the status and the whole text (the checks it shares with hk_lzw_image / hk_inflate_image)
    def refused(layout, streams=buf, offsets=off, sizes=siz, out=buf, stride=270, band_stride=300 * 270):
        lay = None if layout is None else C.byref(_hk._inflate_layout(layout))
        assert lib.hk_lzw_image_host(lay, streams, offsets, sizes, out, stride, band_stride, status) == _hk.HK_ERR_ARG
        return lib.hk_last_error().decode()

    assert refused(None) == 'layout is NULL'
    assert refused(good._replace(sample_bytes=3)) == 'sample_bytes 3 is not 1, 2, 4 or 8'
    assert refused(good._replace(spp=0)) == 'empty raster 0 x 300 x 270'
    assert refused(good._replace(height=0)) == 'empty raster 3 x 0 x 270'
    assert refused(good._replace(block_w=0)) == 'empty block 256 x 0'
    assert refused(good._replace(predictor=3)) == 'predictor 3 is not 1 or 2'
    assert refused(good._replace(tiled=2)) == 'tiled and separate are 0 or 1'
    assert refused(good._replace(separate=-1)) == 'tiled and separate are 0 or 1'
    assert refused(good._replace(tiled=0)) == 'a strip is as wide as the image: block_w 256, width 270'
    assert refused(good._replace(block_w=65536, block_h=32768)) == \
        'a block of 32768 x 65536 x 1 samples of 1 bytes is more than 1073741824 bytes'
    assert refused(good._replace(height=2**31 - 1, width=2**31 - 1, block_w=1, block_h=1)) == \
        'too many blocks: 3 x 2147483647 x 2147483647 of 16 bytes'
    for null in ('streams', 'offsets', 'sizes', 'out'):
        assert refused(good, **{null: None}) == 'NULL pointer argument'
    assert refused(good, stride=269) == 'row stride smaller than width'
    assert refused(good, band_stride=-1) == 'band_stride -1 is smaller than a plane'
    assert refused(good, band_stride=300 * 270 - 1) == 'band_stride 80999 is smaller than a plane'
    assert refused(good, stride=280, band_stride=299 * 280 + 269) == 'band_stride 83989 is smaller than a plane'
    wide = np.zeros(3 * 300 * 270 + 1, np.uint16)
    assert refused(good._replace(sample_bytes=2), out=C.c_void_p(wide.ctypes.data + 1)) == 'out is not aligned to its samples'
    off[5] = -1
    assert refused(good) == 'block 5: offset -1, size 0'
    off[5], siz[7] = 0, -2
    assert refused(good) == 'block 7: offset 0, size -2'
    siz[7] = 0
    # ... and with nothing wrong the same arguments decode: twelve empty streams are twelve refused blocks, not refused arguments
    out = np.zeros(3 * 300 * 270, np.uint8)
    assert lib.hk_lzw_image_host(C.byref(lay), buf, off, siz, out.ctypes.data_as(C.c_void_p), 270, 300 * 270, status) == _hk.HK_ERR_ARG
    assert lib.hk_last_error().startswith(b'lzw: block 0 is refused') and all(status)


# ---- 5. files outside the hook's contract, and the product's switch ----------------------------------------------------------
def test_big_endian_and_predictor_3_files_are_read_here_hook_or_not(tmp_path):
    def never(streams, layout):
        raise AssertionError('the hook was asked')

    rng = np.random.default_rng(5)
    be = st.Layout('be', 'u2', 2, 30, 41, 16, 0, 1, 2)
    a = rng.integers(0, 65536, (2, 30, 41)).astype('<u2')
    (tmp_path / 'be.tif').write_bytes(st.build_tiff(a, be, byteorder='>'))
    p3 = st.Layout('p3', 'f4', 3, 25, 19, 0, 6, 0, 3)
    f = (rng.normal(0, 100, (3, 25, 19)) // 1 / 8).astype('<f4')
    (tmp_path / 'p3.tif').write_bytes(st.build_tiff(f, p3))
    for hook in (None, never):
        got = read_tiff(tmp_path / 'be.tif', lzw=hook).array
        assert got.dtype == np.uint16 and got.tobytes() == a.tobytes()
        got = read_tiff(tmp_path / 'p3.tif', lzw=hook).array
        assert got.dtype == np.float32 and got.tobytes() == f.tobytes()


def test_a_refused_block_of_a_file_is_an_io_error(tmp_path):
    lay = st.Layout('bad', 'u1', 1, 20, 30, 0, 10, 0, 1)
    a = np.zeros((1, 20, 30), np.uint8)
    (tmp_path / 'bad.tif').write_bytes(st.build_tiff(a, lay, streams=[st.encode(bytes(300)), st.pack([256, 65, 66, 257])]))
    with pytest.raises(IoError, match=re.escape(f'block 1 is refused: LZW: {LZW_REASONS[st.SHORT]}')):
        read_tiff(tmp_path / 'bad.tif')


def test_the_host_switch_reads_lzw_through_the_library(lib, tmp_path, monkeypatch):
    """ ``inflate='host'``, the default: ParamStats and RasterFuse hand LZW files to ``_hk.lzw_image_host``, never to the Python
    decoder """
    from homonim_amd import tiff
    from homonim_amd.fuse import RasterFuse
    from homonim_amd.stats import ParamStats
    calls = []
    real = _hk.lzw_image_host
    monkeypatch.setattr(_hk, 'lzw_image_host', lambda s, lay: (calls.append(lay), real(s, lay))[1])
    monkeypatch.setattr(tiff, 'lzw_decode', lambda *a: 1 / 0)
    rng = np.random.default_rng(8)
    a = rng.uniform(1, 200, (1, 40, 50)).astype('<f4')
    lay = st.Layout('src', 'f4', 1, 40, 50, 16, 0, 1, 1)
    (tmp_path / 'src.tif').write_bytes(st.build_tiff(a, lay))
    fuse = RasterFuse(str(tmp_path / 'src.tif'), a)
    assert len(calls) == 1 and fuse is not None
    src = tiff.read_tiff(os.path.join(GOLDEN_DIR, 'tiff', 'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif'))
    assert ParamStats(os.path.join(GOLDEN_DIR, 'tiff', 'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif')) is not None
    assert src.array.shape[0] == 9 and len(calls) == 1   # (a DEFLATE file does not come here)
