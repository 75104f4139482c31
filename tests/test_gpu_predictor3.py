""" GPU tests of TIFF predictor 3 (the floating-point predictor) undone behind the device block decoders: untile_fp_kernel<4> and <8>
of hk_inflate.hip behind inflate_block_kernel and lzw_block_kernel (hk_inflate_image / hk_lzw_image and their _dev forms;
Context.inflate_image / lzw_image; read_tiff(inflater=..., lzw=...); RasterFuse / ParamStats(..., inflate='device')).

The reference is exact: the array an image was made from -- random bit patterns viewed as floats, in the layouts of
tests/_predictor3_cases.py, whose raw blocks ``tiff._unpredict_float``, the Python reader and the library's host decoder give back
on the CPU (tests/test_predictor3_cpu.py) -- and, for the product, the bytes it gives on the same rasters stored without a
predictor. """
import numpy as np
import pytest

import _lzw_streams as st
import _predictor3_cases as p3
from homonim_amd import _hk
from homonim_amd.errors import IoError
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.stats import ParamStats
from homonim_amd.tiff import BlockLayout, read_tiff, write_tiff

pytestmark = pytest.mark.gpu

NAMES = [lay.name for lay in p3.LAYOUTS]
TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)
FILL = 0xAB


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def packed(streams):
    """ the streams one behind the other, a byte apart: they start at every place of a 16-byte group """
    sizes = np.array([len(s) for s in streams], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]]).astype(np.int64)
    buf = np.full(int((sizes + 1).sum()), 0xEE, np.uint8)
    for o, s in zip(offsets.tolist(), streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return buf, offsets, sizes


def into_a_strided_raster(ctx, kind, bl, streams):
    """ the ``_dev`` entry of ``kind`` ('inflate' or 'lzw') into a device raster filled with FILL whose rows and planes have room
    between them -> (planes (spp, band_stride) of the sample's unsigned type, status, stride) """
    es, (n_blocks, _, work_bytes) = bl.sample_bytes, _hk.inflate_bound(bl)
    assert n_blocks == len(streams)
    stride, band_stride = bl.width + 7, (bl.width + 7) * (bl.height + 3) + 5
    buf, offsets, sizes = packed(streams)
    out_bytes = bl.spp * band_stride * es
    ptrs = [ctx.dev_alloc(n) for n in (buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, out_bytes, 4 * n_blocks)]
    d_buf, d_off, d_siz, d_work, d_out, d_st = ptrs
    try:
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)
        ctx.h2d(d_out, np.full(out_bytes, FILL, np.uint8))
        entry = ctx.inflate_image_dev if kind == 'inflate' else ctx.lzw_image_dev
        entry(bl, d_buf, d_off, d_siz, d_work, d_out, stride, band_stride, d_st, stream=0)
        ctx.stream_sync(0)
        got, status = np.empty(out_bytes, np.uint8), np.empty(n_blocks, np.int32)
        ctx.d2h(got, d_out), ctx.d2h(status, d_st)
    finally:
        for p in ptrs:
            ctx.dev_free(p)
    return got.view(f'<u{es}').reshape(bl.spp, band_stride), status, stride


def assert_raster(planes, stride, bl, exp, untouched=()):
    """ the image inside the strided raster is ``exp`` and everything else still FILL; ``untouched``: (plane, rows, columns) slices
    of the image that have to be FILL too """
    exp = exp.view(planes.dtype).copy()
    fill = np.frombuffer(bytes([FILL]) * planes.dtype.itemsize, planes.dtype)[0]
    for sl in untouched:
        exp[sl] = fill
    inside = np.zeros(planes.shape, bool)
    for c in range(bl.spp):
        rows = planes[c, :stride * bl.height].reshape(bl.height, stride)
        assert rows[:, :bl.width].tobytes() == exp[c].tobytes(), f'plane {c}'
        inside[c, :stride * bl.height].reshape(bl.height, stride)[:, :bl.width] = True
    assert (planes[~inside] == fill).all(), 'something was written outside the image'


def streams_of(kind, name):
    return list(p3.deflate_streams(name) if kind == 'inflate' else p3.lzw_streams(name))


# ---- 1. every layout, behind both first stages, through both entry points -------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('name', NAMES)
def test_every_layout_through_the_host_pointer_calls(ctx, name):
    lay, a, _ = p3.case(name)
    bl = BlockLayout(*st.block_layout(lay))
    for kind, call in (('inflate', ctx.inflate_image), ('lzw', ctx.lzw_image)):
        got = call(streams_of(kind, name), bl)
        assert got.dtype == np.dtype(f'u{bl.sample_bytes}') and got.shape == a.shape and got.tobytes() == a.tobytes(), kind


@pytest.mark.oracle
@pytest.mark.parametrize('name', NAMES)
def test_every_layout_into_a_strided_device_raster(ctx, name):
    lay, a, _ = p3.case(name)
    bl = BlockLayout(*st.block_layout(lay))
    for kind in ('inflate', 'lzw'):
        planes, status, stride = into_a_strided_raster(ctx, kind, bl, streams_of(kind, name))
        assert not status.any(), kind
        assert_raster(planes, stride, bl, a)


@pytest.mark.oracle
def test_small_groups_give_the_same_bytes(ctx, monkeypatch):
    for name in ('t80-f4', 't48-sep-f8'):
        lay, a, _ = p3.case(name)
        bl = BlockLayout(*st.block_layout(lay))
        for kind, call in (('inflate', ctx.inflate_image), ('lzw', ctx.lzw_image)):
            monkeypatch.setenv('HK_INFLATE_GROUP_KB', '1')   # one block row per group
            got = call(streams_of(kind, name), bl)
            monkeypatch.delenv('HK_INFLATE_GROUP_KB')
            assert got.tobytes() == a.tobytes(), (name, kind)


# ---- 2. a refused block ----------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('kind', ['inflate', 'lzw'])
def test_a_truncated_stream_among_good_ones_keeps_its_pixels_and_its_status(ctx, kind):
    name = 't16-f4'
    lay, a, _ = p3.case(name)
    bl = BlockLayout(*st.block_layout(lay))
    streams = streams_of(kind, name)
    streams[4] = streams[4][:len(streams[4]) // 2]      # the middle tile: rows 16..31, columns 16..31
    planes, status, stride = into_a_strided_raster(ctx, kind, bl, streams)
    assert status[4] != 0 and not np.delete(status, 4).any()
    assert_raster(planes, stride, bl, a, untouched=[(0, slice(16, 32), slice(16, 32))])
    call = ctx.inflate_image_packed if kind == 'inflate' else ctx.lzw_image_packed
    got, status2 = call(*packed(streams), bl, strict=False)
    assert status2.tolist() == status.tolist()
    keep = np.ones((37, 45), bool)
    keep[16:32, 16:32] = False
    assert (got[0][keep] == a.view('<u4')[0][keep]).all()
    with pytest.raises(IoError, match='block 4 is refused'):
        call(*packed(streams), bl, strict=True)


# ---- 3. the package's own writer, and back --------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('dtype, shape', [('f4', (2, 300, 270)), ('f8', (1, 130, 140))])
def test_what_the_device_writer_wrote_with_predictor_3_comes_back_through_the_device_reader(ctx, tmp_path, dtype, shape):
    rng = np.random.default_rng(31)
    a = np.round(rng.uniform(20.0, 200.0, shape), 2).astype(f'<{dtype}')
    a[:, :7] = a[:, -9:] = np.nan
    a[:, :, :5] = a[:, :, -11:] = np.nan      # a NaN frame
    write_tiff(tmp_path / 'w3.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=128, compressor=ctx.deflate_tiles, predictor=3)
    calls = []

    def hook(streams, layout):
        calls.append(layout)
        return ctx.inflate_image(streams, layout)

    hook.predictors = ctx.inflate_image.predictors
    got = read_tiff(tmp_path / 'w3.tif', inflater=hook).array
    assert got.dtype == a.dtype and got.tobytes() == a.tobytes()
    assert len(calls) == 1 and calls[0][:7] == (a.dtype.itemsize, shape[0], shape[1], shape[2], 128, 128, 1) and calls[0].predictor == 3
    assert read_tiff(tmp_path / 'w3.tif').array.tobytes() == a.tobytes()      # (zlib and numpy read the same)


# ---- 4. the product ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def product(ctx, tmp_path_factory):
    """ a source and a reference of 3 x 300 x 270 float32, stored plain and with predictor 3 (DEFLATE), and what the product makes
    of the plain pair -> (directory, (corrected file, parameter file) of the plain pair) """
    d = tmp_path_factory.mktemp('p3_product')
    rng = np.random.default_rng(23)
    src = np.round(rng.uniform(20.0, 200.0, (3, 300, 270))).astype(np.float32)
    ref = np.round(1.1 * src + 5.0 + rng.normal(0, 2.0, src.shape), 1).astype(np.float32)
    src[:, 50:80, 100:150] = np.nan
    for name, a in (('src', src), ('ref', ref)):
        write_tiff(d / f'{name}.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=64)
        write_tiff(d / f'{name}_p3.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=64, predictor=3)
    (d / 'plain').mkdir()
    plain = (d / 'plain' / 'corr.tif', d / 'plain' / 'param.tif')
    with RasterFuse(d / 'src.tif', d / 'ref.tif') as rf:
        rf.process(plain[0], 'gain-offset', (5, 5), param_filename=plain[1])
    return d, plain


def process_on_the_device(d, suffix):
    out = d / f'device{suffix}'
    out.mkdir()
    files = (out / 'corr.tif', out / 'param.tif')
    with RasterFuse(d / f'src{suffix}.tif', d / f'ref{suffix}.tif', inflate='device') as rf:
        rf.process(files[0], 'gain-offset', (5, 5), param_filename=files[1])
    return files


@pytest.mark.oracle
def test_process_on_deflate_predictor_3_copies_is_what_it_is_on_the_plain_files(ctx, product):
    d, plain = product
    for name in ('src', 'ref'):
        assert read_tiff(d / f'{name}_p3.tif', inflater=ctx.inflate_image).array.tobytes() == read_tiff(d / f'{name}.tif').array.tobytes()
    for exp, got in zip(plain, process_on_the_device(d, '_p3')):
        assert read_tiff(exp).array.tobytes() == read_tiff(got).array.tobytes()


@pytest.mark.oracle
def test_process_on_lzw_predictor_3_copies_is_what_it_is_on_the_plain_files(ctx, product):
    d, plain = product
    for name in ('src', 'ref'):
        (d / f'{name}_p3_lzw.tif').write_bytes(st.lzw_copy((d / f'{name}_p3.tif').read_bytes()))
        assert read_tiff(d / f'{name}_p3_lzw.tif', lzw=ctx.lzw_image).array.tobytes() == read_tiff(d / f'{name}.tif').array.tobytes()
    for exp, got in zip(plain, process_on_the_device(d, '_p3_lzw')):
        assert read_tiff(exp).array.tobytes() == read_tiff(got).array.tobytes()


@pytest.mark.oracle
def test_stats_of_a_predictor_3_parameter_file_are_those_of_its_plain_twin(ctx, product):
    d, plain = product
    par = read_tiff(plain[1])
    write_tiff(d / 'param_p3.tif', par.array, par.transform, par.crs, nodata=par.nodata, metadata=par.metadata, tile=64,
               descriptions=par.descriptions, predictor=3)
    with ParamStats(plain[1]) as ps:
        exp = ps.stats()
    with ParamStats(d / 'param_p3.tif', inflate='device') as ps:
        assert repr(ps.stats()) == repr(exp)   # (repr: a NaN equals itself)
