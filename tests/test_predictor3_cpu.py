""" TIFF predictor 3 (the floating-point predictor) behind the block decoders, without a GPU: ``hk_lzw_image_host`` of the library,
the row function it shares with the kernel (homonim_amd/csrc/hk_fpred_core.h) as a stand-alone program under AddressSanitizer +
UBSan, ``hk_inflate_bound``, and the hook contract of ``tiff.read_tiff`` up to ``RasterFuse`` and ``ParamStats``.

The reference is exact: the array a file was made from (random bit patterns, tests/_predictor3_cases.py), the bytes
``tiff._unpredict_float`` gives for the same raw blocks, and what the Python reader reads from the same file.  The kernels are
tested on the GPU (tests/test_gpu_predictor3.py), on the same images. """
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _lzw_streams as st
import _predictor3_cases as p3
from conftest import GOLDEN_DIR, REPO
from homonim_amd import _hk, tiff
from homonim_amd.errors import IoError
from homonim_amd.geo import Affine
from homonim_amd.tiff import BlockLayout, read_tiff, write_tiff

NAMES = [lay.name for lay in p3.LAYOUTS]
PARAM = os.path.join(GOLDEN_DIR, 'tiff', 'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif')


@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def same_bits(got, exp):
    return got.shape == exp.shape and got.dtype.itemsize == exp.dtype.itemsize and got.tobytes() == exp.tobytes()


# ---- 1. the host decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_the_host_decoder_gives_the_array_back(lib, name):
    lay, a, blocks = p3.case(name)
    bl = BlockLayout(*st.block_layout(lay))
    assert bl.predictor == 3
    got = _hk.lzw_image_host(list(p3.lzw_streams(name)), bl)
    assert got.dtype == np.dtype(f'u{bl.sample_bytes}') and same_bits(got, a)


def test_the_layouts_hold_what_they_are_there_for():
    """ the oracle on the same raw blocks: ``tiff._unpredict_float`` gives every block's pixels; and the images do have edge tiles,
    more than one wave step, a short strip, and the bit patterns no arithmetic on floats would keep """
    for name in NAMES:
        lay, a, blocks = p3.case(name)
        es, bw, bh, cspp = st.block_layout(lay)[0], *st.block_layout(lay)[4:6], 1 if lay.separate else lay.spp
        geo = p3.block_geometry(lay)
        assert len(geo) == len(blocks)
        across, down = -(-lay.width // bw), -(-lay.height // bh)
        for k, (raw, (rows, cols)) in enumerate(zip(blocks, geo)):
            assert len(raw) == rows * bw * cspp * es
            plane, rem = divmod(k, across * down)
            by, bx = divmod(rem, across)
            blk = tiff._unpredict_float(raw, rows, bw, cspp, es)
            hh = min(rows, lay.height - by * bh)
            exp = a[plane:plane + 1] if lay.separate else a
            exp = np.moveaxis(exp[:, by * bh:by * bh + hh, bx * bw:bx * bw + cols], 0, 2)
            assert blk[:hh, :cols].astype(f'<f{es}').tobytes() == np.ascontiguousarray(exp).tobytes(), (name, k)
    geo = p3.block_geometry(p3.BY_NAME['t16-f4'])
    assert {c for _, c in geo} == {16, 13} and p3.BY_NAME['t16-f4'].height % 16
    assert {c for _, c in p3.block_geometry(p3.BY_NAME['t80-f4'])} == {80, 40}        # two steps, the second ragged; a cropped tile
    assert {r for r, _ in p3.block_geometry(p3.BY_NAME['strips-short-f4'])} == {16, 2}
    a = p3.case('strip-wide-f4')[1]
    u = a.view('<u4')
    nan = (u & 0x7F800000 == 0x7F800000) & (u & 0x007FFFFF != 0)
    denormal = (u & 0x7F800000 == 0) & (u & 0x007FFFFF != 0)
    assert nan.sum() > 10 and denormal.sum() > 10 and len(set(u[nan].tolist())) > 10   # NaNs of many payloads


# ---- 2. the row function under the sanitizers ------------------------------------------------------------------------------------
def test_the_row_function_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / 'fpred_core_host_san'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(REPO, 'homonim_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'fpred_core_host.cpp'),
                    '-o', str(exe)], check=True)
    exp, n = [], 0
    with open(tmp_path / 'in.bin', 'wb') as f:
        f.write(struct.pack('<I', sum(len(p3.case(name)[2]) for name in NAMES)))
        for name in NAMES:
            lay, a, blocks = p3.case(name)
            es, bw, cspp = st.block_layout(lay)[0], st.block_layout(lay)[4], 1 if lay.separate else lay.spp
            for raw, (rows, cols) in zip(blocks, p3.block_geometry(lay)):
                f.write(struct.pack('<5I', es, bw, cspp, rows, cols) + raw)
                # the program's output bytes: row after row, sample c of a pixel after sample c - 1, cols little-endian samples
                blk = tiff._unpredict_float(raw, rows, bw, cspp, es)[:, :cols, :].astype(f'<f{es}')
                b = np.ascontiguousarray(blk.transpose(0, 2, 1)).view(np.uint8).ravel().astype(np.uint64)
                exp.append(f'{int(b.sum(dtype=np.uint64))} {int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))}')
                n += 1
    res = subprocess.run([str(exe), str(tmp_path / 'in.bin')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, res.stderr[-3000:]
    got = res.stdout.split('\n')[:-1]
    assert len(got) == n and got == exp, [k for k, (g, e) in enumerate(zip(got, exp)) if g != e]


# ---- 3. the layout check ---------------------------------------------------------------------------------------------------------
def test_inflate_bound_takes_predictor_3_for_4_and_8_byte_samples_only(lib):
    for lay in (BlockLayout(4, 3, 300, 270, 256, 256, 1, 1, 3), BlockLayout(8, 2, 41, 29, 29, 7, 0, 0, 3),
                BlockLayout(4, 1, 100, 3, 3, 7, 0, 1, 3)):
        assert _hk.inflate_bound(lay) == _hk.inflate_bound(lay._replace(predictor=1))
    for es in (1, 2):
        with pytest.raises(ValueError, match=r'predictor 3 is not 1 or 2$'):
            _hk.inflate_bound(BlockLayout(es, 3, 300, 270, 256, 256, 1, 1, 3))
    for es in (4, 8):
        for bad in (0, 4, -1):
            with pytest.raises(ValueError, match='predictor'):
                _hk.inflate_bound(BlockLayout(es, 3, 300, 270, 256, 256, 1, 1, bad))
    assert lib.hk_abi_version() == 12 and C.sizeof(_hk.InflateLayout) == 36


# ---- 4. the hook contract --------------------------------------------------------------------------------------------------------
def test_the_declared_predictors():
    for fn in (_hk.lzw_image_host, _hk.lzw_image_host_packed, _hk.Context.inflate_image, _hk.Context.inflate_image_packed,
               _hk.Context.lzw_image, _hk.Context.lzw_image_packed, _hk.Context.inflate_image_dev, _hk.Context.lzw_image_dev):
        assert fn.predictors == (1, 2, 3), fn
    assert _hk.block_decoders('host')[1].predictors == (1, 2, 3)


@pytest.mark.parametrize('name', ['t16-contig3-f4', 'strips-contig3-f8'])
def test_read_tiff_hands_an_lzw_predictor_3_file_to_the_host_decoder(lib, tmp_path, monkeypatch, name):
    lay, a, _ = p3.case(name)
    (tmp_path / 'p3.tif').write_bytes(p3.tiff_bytes(name, 5))
    exp = read_tiff(tmp_path / 'p3.tif').array      # the Python reader
    assert exp.dtype == a.dtype and same_bits(exp, a)
    monkeypatch.setattr(tiff, 'lzw_decode', lambda *args: 1 / 0)
    got = read_tiff(tmp_path / 'p3.tif', lzw=_hk.lzw_image_host).array
    assert got.dtype == a.dtype and same_bits(got, a)


@pytest.mark.parametrize('compression', [5, 8])
def test_a_hook_is_asked_for_predictor_3_only_if_it_says_so(tmp_path, compression):
    lay, a, _ = p3.case('t16-f4')
    (tmp_path / 'p3.tif').write_bytes(p3.tiff_bytes('t16-f4', compression))
    calls = []

    def silent(streams, layout):
        raise AssertionError('the hook was asked')

    def speaking(streams, layout):
        calls.append((len(streams), layout))
        return a.view('<u4')

    def two_only(streams, layout):
        raise AssertionError('the hook was asked')

    speaking.predictors = (1, 2, 3)
    two_only.predictors = (1, 2)
    kw = 'lzw' if compression == 5 else 'inflater'
    for hook in (silent, two_only):
        assert same_bits(read_tiff(tmp_path / 'p3.tif', **{kw: hook}).array, a)
    got = read_tiff(tmp_path / 'p3.tif', **{kw: speaking}).array
    assert got.dtype == np.float32 and same_bits(got, a)
    assert calls == [(9, BlockLayout(4, 1, 37, 45, 16, 16, 1, 0, 3))]
    # (the other kind of hook is not asked about this file)
    assert same_bits(read_tiff(tmp_path / 'p3.tif', **{'inflater' if compression == 5 else 'lzw': speaking}).array, a) and len(calls) == 1


def test_overviews_follow_the_same_rule(lib, tmp_path, monkeypatch):
    a = p3.random_bits((2, 70, 90), 'f4', 77)
    ovw = np.ascontiguousarray(a[:, ::2, ::2])
    write_tiff(tmp_path / 'w3.tif', a, Affine(10.0, 0.0, 0.0, 0.0, -10.0, 0.0), tile=32, predictor=3, overviews=[ovw])
    (tmp_path / 'w3_lzw.tif').write_bytes(st.lzw_copy((tmp_path / 'w3.tif').read_bytes()))
    calls = []

    def hook(streams, layout):
        calls.append(layout.predictor)
        return _hk.lzw_image_host(streams, layout)

    monkeypatch.setattr(tiff, 'lzw_decode', lambda *args: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        tiff.read_tiff_overviews(tmp_path / 'w3_lzw.tif', lzw=hook)     # no ``predictors``: the Python reader
    hook.predictors = (1, 2, 3)
    (got,) = tiff.read_tiff_overviews(tmp_path / 'w3_lzw.tif', lzw=hook)
    assert same_bits(got, ovw) and calls == [3]
    assert same_bits(read_tiff(tmp_path / 'w3_lzw.tif', lzw=hook).array, a) and calls == [3, 3]


def test_the_host_switch_reads_lzw_predictor_3_through_the_library(lib, tmp_path, monkeypatch):
    """ ``inflate='host'``, the default: ParamStats and RasterFuse hand an LZW + predictor 3 file to ``_hk.lzw_image_host`` """
    from homonim_amd.fuse import RasterFuse
    from homonim_amd.stats import ParamStats
    calls, real = [], _hk.lzw_image_host

    def recorder(streams, layout):
        calls.append(layout.predictor)
        return real(streams, layout)

    recorder.predictors = real.predictors
    monkeypatch.setattr(_hk, 'lzw_image_host', recorder)
    monkeypatch.setattr(tiff, 'lzw_decode', lambda *args: 1 / 0)
    lay, a, _ = p3.case('t16-contig3-f4')
    (tmp_path / 'src.tif').write_bytes(p3.tiff_bytes('t16-contig3-f4', 5))
    fuse = RasterFuse(str(tmp_path / 'src.tif'), str(tmp_path / 'src.tif'))
    assert calls == [3, 3] and fuse is not None
    par = read_tiff(PARAM)
    write_tiff(tmp_path / 'param.tif', par.array, par.transform, par.crs, nodata=par.nodata, metadata=par.metadata, tile=16,
               descriptions=par.descriptions, predictor=3)
    (tmp_path / 'param_lzw.tif').write_bytes(st.lzw_copy((tmp_path / 'param.tif').read_bytes()))
    with ParamStats(tmp_path / 'param_lzw.tif') as ps:
        assert calls == [3, 3, 3] and ps is not None
    with pytest.raises(ZeroDivisionError):
        read_tiff(tmp_path / 'param_lzw.tif', lzw=lambda s, lay: 1 / 0)      # (the file is what it is said to be)
    assert same_bits(read_tiff(tmp_path / 'param_lzw.tif', lzw=recorder).array, par.array)


# ---- 5. a refused block ----------------------------------------------------------------------------------------------------------
def test_a_refused_block_of_a_predictor_3_image_is_named_and_leaves_the_others_alone(lib, tmp_path):
    name = 't16-f4'
    lay, a, _ = p3.case(name)
    bl = BlockLayout(*st.block_layout(lay))
    streams = list(p3.lzw_streams(name))
    streams[4] = streams[4][:len(streams[4]) // 2]
    with pytest.raises(IoError, match=re.escape(f'block 4 is refused: {tiff.LZW_REASONS[st.TRUNCATED]}')):
        _hk.lzw_image_host(streams, bl)
    (tmp_path / 'bad.tif').write_bytes(st.build_tiff(a, lay, streams=streams))
    with pytest.raises(IoError, match='block 4 is refused'):
        read_tiff(tmp_path / 'bad.tif', lzw=_hk.lzw_image_host)
    # strict=False, into a raster that was filled before: the middle tile (rows 16..31, columns 16..31) keeps the filling
    buf, offsets, sizes = _hk._pack_streams(streams)
    out = np.full((1, 37, 45), 0xABABABAB, np.uint32)
    status = np.full(9, -1, np.int32)
    cl = _hk._inflate_layout(bl)
    rc = lib.hk_lzw_image_host(C.byref(cl), buf.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                               sizes.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.c_void_p), 45, 37 * 45,
                               status.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == _hk.HK_ERR_ARG and status.tolist() == [0, 0, 0, 0, st.TRUNCATED, 0, 0, 0, 0]
    exp = a.view('<u4').copy()
    exp[0, 16:32, 16:32] = 0xABABABAB
    assert out.tobytes() == exp.tobytes()
    got, status = _hk.lzw_image_host_packed(buf, offsets, sizes, bl, strict=False)
    keep = np.ones((37, 45), bool)
    keep[16:32, 16:32] = False
    assert status.tolist() == [0, 0, 0, 0, st.TRUNCATED, 0, 0, 0, 0] and (got[0][keep] == a.view('<u4')[0][keep]).all()
