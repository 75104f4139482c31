""" GPU tests of the device INFLATE path (hk_inflate.hip; hk_inflate_image / hk_inflate_image_dev; Context.inflate_image;
read_tiff(inflater=...); RasterFuse(..., inflate='device'); ParamStats(..., inflate='device')).

The reference is exact: for a well-formed stream ``zlib.decompress``, for a file ``read_tiff`` without the hook, for a malformed
stream zlib's refusal and the status the decoder core gives on the host (tests/test_inflate_cpu.py, on the same streams:
tests/_inflate_streams.py). """
import glob
import os

import numpy as np
import pytest

import _inflate_streams as st
from conftest import GOLDEN_DIR
from homonim_amd import _hk
from homonim_amd.errors import IoError
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.stats import ParamStats
from homonim_amd.tiff import BlockLayout, read_tiff, read_tiff_overviews, write_tiff

pytestmark = pytest.mark.gpu

GOLDEN_TIFS = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'rasters', '*.tif')) + glob.glob(os.path.join(GOLDEN_DIR, 'tiff', '*.tif')))
TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def row_layout(n, raw):
    """ ``n`` blocks of ``raw`` bytes each as an image: one strip of one row of ``raw`` uint8 samples per block """
    return BlockLayout(1, 1, n, raw, raw, 1, 0, 0, 1)


def packed(streams):
    """ the streams one behind the other, a byte apart: they start at every place of a 16-byte group """
    sizes = np.array([len(s.data) for s in streams], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]]).astype(np.int64)
    buf = np.full(int((sizes + 1).sum()), 0xEE, np.uint8)
    for o, s in zip(offsets.tolist(), streams):
        buf[o:o + len(s.data)] = np.frombuffer(s.data, np.uint8)
    return buf, offsets, sizes


def inflate_rows(ctx, streams, strict=True):
    """ streams of one raw size, one call -> (array (n, raw), status) """
    raw = len(streams[0].raw)
    assert all(len(s.raw) == raw for s in streams)
    out, status = ctx.inflate_image_packed(*packed(streams), row_layout(len(streams), raw), strict=strict)
    assert out.shape == (1, len(streams), raw) and out.dtype == np.uint8 and status.shape == (len(streams),)
    return out[0], status


def assert_rows(streams, out, status):
    for k, s in enumerate(streams):
        assert status[k] == s.status, f'{s.name}: status {status[k]}, expected {s.status}'
        if s.status == st.OK:
            assert out[k].tobytes() == s.raw, f'{s.name}: the bytes differ from zlib\'s'


# ---- 1. well-formed streams -------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('raw', [16384, 65536])
def test_what_zlib_writes_in_its_modes(ctx, raw):
    streams = [s for s in st.set_a() if len(s.raw) == raw]
    assert len(streams) == (9 if raw == 16384 else 8) * 8
    assert_rows(streams, *inflate_rows(ctx, streams))


@pytest.mark.oracle
@pytest.mark.parametrize('k', range(len(st.PREFIXES)), ids=lambda k: str(st.PREFIXES[k]))
def test_hand_built_blocks_with_the_longest_distance(ctx, k):
    streams = [st.set_b()[k]]
    assert_rows(streams, *inflate_rows(ctx, streams))


@pytest.mark.oracle
def test_seeded_sweep_of_4096_small_blocks_in_one_call(ctx):
    streams = st.set_d()
    out, status = inflate_rows(ctx, streams)
    assert not status.any()
    assert out.tobytes() == b''.join(s.raw for s in streams)


# ---- 2. malformed streams among good ones ------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_every_refusal_has_its_status_and_leaves_the_other_blocks_alone(ctx):
    good = st.set_b()[0]
    bad = st.set_c()
    assert len(good.raw) == len(bad[0].raw)
    streams = []
    for s in bad:
        streams += [s, good]
    out, status = inflate_rows(ctx, streams, strict=False)
    assert_rows(streams, out, status)
    assert sorted(set(status.tolist())) == list(range(11))   # every status occurs
    with pytest.raises(IoError, match=r'block 0 .*ends too soon'):
        inflate_rows(ctx, streams, strict=True)
    with pytest.raises(IoError, match=r'block 1 .*Adler'):
        inflate_rows(ctx, [good, bad[1], bad[2]], strict=True)
    with pytest.raises(IoError, match=r'block 2 '):
        ctx.inflate_image([good.data, good.data, bad[3].data], row_layout(3, len(good.raw)))
    # a call of refused blocks only, and the one that is accepted with two bytes behind its trailer
    out, status = inflate_rows(ctx, bad, strict=False)
    assert_rows(bad, out, status)
    assert status[-1] == 0 and bad[-1].name == 'trailing-garbage'


# ---- 3. files ------------------------------------------------------------------------------------------------------------
def same_raster(a, b):
    assert a.array.dtype == b.array.dtype and a.array.shape == b.array.shape and a.array.tobytes() == b.array.tobytes()
    assert a.transform == b.transform and a.crs == b.crs and a.metadata == b.metadata and a.descriptions == b.descriptions
    assert a.nodata == b.nodata or (np.isnan(a.nodata) and np.isnan(b.nodata))


@pytest.mark.oracle
@pytest.mark.parametrize('path', GOLDEN_TIFS, ids=lambda p: os.path.splitext(os.path.basename(p))[0])
def test_every_golden_file_reads_the_same(ctx, path):
    calls = []

    def inflater(streams, layout):
        calls.append(layout)
        return ctx.inflate_image(streams, layout)

    same_raster(read_tiff(path, inflater=inflater), read_tiff(path))
    assert len(calls) == (0 if 'bigendian' in path else 1)


# ---- 4. round trips ------------------------------------------------------------------------------------------------------
def _mixed(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    a = np.round(rng.normal(100, 30, shape)).astype(dtype)
    a[:, : shape[1] // 3] = 0
    return a


@pytest.mark.oracle
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32', 'float64'])
def test_the_device_compressors_streams_inflate_to_the_raster(ctx, dtype):
    a = _mixed(dtype, (2, 300, 200), 51)
    streams = ctx.deflate_tiles(a, 128)
    got = ctx.inflate_image(streams, BlockLayout(a.dtype.itemsize, 2, 300, 200, 128, 128, 1, 1, 1))
    assert got.shape == a.shape and got.dtype.kind == 'u' and got.view(a.dtype).tobytes() == a.tobytes()


@pytest.mark.oracle
def test_a_file_written_with_the_device_compressor_reads_back_through_the_device(ctx, tmp_path):
    rng = np.random.default_rng(52)
    a = np.round(rng.normal(100, 20, (2, 700, 900)), 1).astype(np.float32)
    a[:, :60] = np.nan
    levels = ctx.overviews(a, float('nan'), 2)
    write_tiff(tmp_path / 'd.tif', a, TF, CRS('EPSG:32735'), nodata=float('nan'), overviews=levels, compressor=ctx.deflate_tiles)
    d = read_tiff(tmp_path / 'd.tif', inflater=ctx.inflate_image)
    same_raster(d, read_tiff(tmp_path / 'd.tif'))
    assert d.array.tobytes() == a.tobytes()
    got = read_tiff_overviews(tmp_path / 'd.tif', inflater=ctx.inflate_image)
    assert len(got) == 2 and all(g.dtype == lv.dtype and g.tobytes() == lv.tobytes() for g, lv in zip(got, levels))


# ---- 5. entry points -----------------------------------------------------------------------------------------------------
def _file_blocks(path):
    """ (streams, layout) of a file, as read_tiff hands them to its hook """
    seen = []

    def grab(streams, layout):
        seen.append((streams, layout))
        raise StopIteration

    with pytest.raises(StopIteration):
        read_tiff(path, inflater=grab)
    return seen[0]


@pytest.mark.oracle
@pytest.mark.parametrize('name', ['rasters/ngi_rgb_byte_1', 'tiff/synth_pred2_contig_i16', 'tiff/synth_pred2_u16_strips',
                                  'tiff/synth_bigtiff_f64_tiles'])
def test_device_entry_point_gives_the_host_entry_points_bytes_inside_a_strided_raster(ctx, name):
    path = os.path.join(GOLDEN_DIR, name + '.tif')
    streams, lay = _file_blocks(path)
    exp = ctx.inflate_image(streams, lay)
    assert exp.view(read_tiff(path).array.dtype).tobytes() == read_tiff(path).array.tobytes()
    es, (n_blocks, _, work_bytes) = lay.sample_bytes, _hk.inflate_bound(lay)
    assert n_blocks == len(streams)
    stride, band_stride = lay.width + 7, (lay.width + 7) * (lay.height + 3) + 5   # rows and planes with room between them
    buf, offsets, sizes = packed([st.Stream('', s, b'', 0) for s in streams])
    out_bytes = lay.spp * band_stride * es
    ptrs = [ctx.dev_alloc(n) for n in (buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, out_bytes, 4 * n_blocks)]
    d_buf, d_off, d_siz, d_work, d_out, d_st = ptrs
    try:
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)
        ctx.h2d(d_out, np.full(out_bytes, 0xAB, np.uint8))
        ctx.inflate_image_dev(lay, d_buf, d_off, d_siz, d_work, d_out, stride, band_stride, d_st, stream=0)
        ctx.stream_sync(0)
        got, status = np.empty(out_bytes, np.uint8), np.empty(n_blocks, np.int32)
        ctx.d2h(got, d_out), ctx.d2h(status, d_st)
    finally:
        for p in ptrs:
            ctx.dev_free(p)
    assert not status.any()
    planes = got.view(exp.dtype).reshape(lay.spp, band_stride)
    inside = np.zeros((lay.spp, band_stride), bool)
    for c in range(lay.spp):
        rows = planes[c, :stride * lay.height].reshape(lay.height, stride)
        assert rows[:, :lay.width].tobytes() == exp[c].tobytes()
        inside[c, :stride * lay.height].reshape(lay.height, stride)[:, :lay.width] = True
    assert (planes[~inside].view(np.uint8) == 0xAB).all(), 'something was written outside the image'


@pytest.mark.oracle
def test_small_groups_give_the_same_bytes(ctx, monkeypatch):
    for name in ('rasters/ngi_rgb_byte_1', 'rasters/sentinel2_b432_byte', 'tiff/synth_pred2_u16_strips'):
        path = os.path.join(GOLDEN_DIR, name + '.tif')
        exp = read_tiff(path)
        monkeypatch.setenv('HK_INFLATE_GROUP_KB', '1')   # one block row per group
        same_raster(read_tiff(path, inflater=ctx.inflate_image), exp)
        monkeypatch.delenv('HK_INFLATE_GROUP_KB')


def test_argument_errors_are_exceptions_with_a_message(ctx):
    lay = row_layout(2, 100)
    good = np.zeros(64, np.uint8)
    with pytest.raises(ValueError, match='offsets'):
        ctx.inflate_image_packed(good, [0], [10], lay)
    with pytest.raises(ValueError, match='outside'):
        ctx.inflate_image_packed(good, [0, 60], [10, 10], lay)
    with pytest.raises(ValueError, match='outside'):
        ctx.inflate_image_packed(good, [0, -1], [10, 10], lay)
    with pytest.raises(ValueError, match='sample_bytes'):
        ctx.inflate_image_packed(good, [0, 10], [10, 10], lay._replace(sample_bytes=3))
    with pytest.raises(ValueError, match='aligned'):
        ctx.inflate_image_dev(lay, 4096, 4096, 4096, 4097, 4096, 100, 200, 4096)


# ---- 6. integration ------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_process_and_stats_are_the_same_with_device_inflate(ctx, tmp_path):
    from test_gpu_overviews import seeded_pair
    src, ref = seeded_pair((300, 400), 23)
    write_tiff(tmp_path / 'src.tif', src, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=128)
    write_tiff(tmp_path / 'ref.tif', ref, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=128)
    files = {}
    for mode in ('host', 'device'):
        d = tmp_path / mode
        d.mkdir()
        files[mode] = (d / 'corr.tif', d / 'param.tif')
        with RasterFuse(tmp_path / 'src.tif', tmp_path / 'ref.tif', inflate=mode) as rf:
            rf.process(files[mode][0], 'gain-offset', (5, 5), param_filename=files[mode][1])
    for h, d in zip(files['host'], files['device']):
        assert h.read_bytes() == d.read_bytes()
    with ParamStats(files['host'][1]) as ps:
        exp = ps.stats()
    with ParamStats(files['host'][1], inflate='device') as ps:
        got = ps.stats()
    assert repr(got) == repr(exp) and len(got) == 9   # (repr: a NaN equals itself)
