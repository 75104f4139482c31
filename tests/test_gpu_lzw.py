""" GPU tests of the device LZW path (hk_lzw.hip; hk_lzw_image / hk_lzw_image_dev; Context.lzw_image; read_tiff(lzw=...);
RasterFuse(..., inflate='device'); ParamStats(..., inflate='device')).

The reference is exact: for the files Pillow's libtiff wrote, the pixels Pillow reads back (tests/golden/tiff/lzw); for the streams
of tests/_lzw_streams.py the bytes they were encoded from, which ``tiff.lzw_decode``, the host build of the same decoder and,
where it can, Pillow give back on the CPU (tests/test_lzw_cpu.py, on the same streams); for a malformed stream the status named
there. """
import os

import numpy as np
import pytest

import _lzw_streams as st
from conftest import GOLDEN_DIR
from homonim_amd import _hk
from homonim_amd.errors import IoError
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.stats import ParamStats
from homonim_amd.tiff import LZW_REASONS, BlockLayout, lzw_decode, read_tiff, write_tiff

pytestmark = pytest.mark.gpu

LZW_DIR = os.path.join(GOLDEN_DIR, 'tiff', 'lzw')
FIXTURES = ('lzw_u8_noise_strips', 'lzw_u8_smooth_strips', 'lzw_u8_flat_strips', 'lzw_rgb_pred2_strips', 'lzw_u16_pred2_strips',
            'lzw_f32_strips')
TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)
CHUNKS = sorted({s.name.rsplit(':', 1)[0] for s in st.good_set()})


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def row_layout(n, raw):
    """ ``n`` blocks of ``raw`` bytes each as an image: one strip of one row of ``raw`` uint8 samples per block """
    return BlockLayout(1, 1, n, raw, raw, 1, 0, 0, 1)


def packed(streams):
    """ the streams one behind the other, a byte apart: they start at every place of a 16-byte group """
    sizes = np.array([len(s) for s in streams], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]]).astype(np.int64)
    buf = np.full(int((sizes + 1).sum()), 0xEE, np.uint8)
    for o, s in zip(offsets.tolist(), streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return buf, offsets, sizes


def lzw_rows(ctx, streams, strict=True):
    """ streams of one raw size, one call -> (array (n, raw), status) """
    raw = len(streams[0].raw)
    assert all(len(s.raw) == raw for s in streams)
    out, status = ctx.lzw_image_packed(*packed([s.data for s in streams]), row_layout(len(streams), raw), strict=strict)
    assert out.shape == (1, len(streams), raw) and out.dtype == np.uint8 and status.shape == (len(streams),)
    return out[0], status


def assert_rows(streams, out, status):
    for k, s in enumerate(streams):
        assert status[k] == s.status, f'{s.name}: status {status[k]}, expected {s.status}'
        if s.status == st.OK:
            assert out[k].tobytes() == s.raw, f'{s.name}: the bytes differ'


# ---- 1. what Pillow's libtiff wrote -------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('name', FIXTURES)
def test_a_pillow_file_reads_as_pillow_reads_it(ctx, name):
    exp = np.load(os.path.join(LZW_DIR, 'lzw_decoded.npz'))[name]
    got = read_tiff(os.path.join(LZW_DIR, name + '.tif'), lzw=ctx.lzw_image).array
    assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


# ---- 2. the encoder's streams: width steps and Clears, the full table, long strings, a cut last string, no end code ----------------
@pytest.mark.oracle
@pytest.mark.parametrize('chunk', CHUNKS)
def test_every_chunk_under_every_encoder_switch(ctx, chunk):
    """ (what the streams hold -- 12-bit codes and Clears in the noise tile, a full table under the never-Clear switch, strings far
    longer than a wave in the constant ones, a raw size that is no multiple of 16 -- is asserted in tests/test_lzw_cpu.py) """
    streams = [s for s in st.good_set() if s.name.rsplit(':', 1)[0] == chunk]
    assert len(streams) == len(st.SWITCHES)
    out, status = lzw_rows(ctx, streams)
    assert_rows(streams, out, status)


@pytest.mark.oracle
def test_strings_whose_last_appearance_has_left_the_ring_are_used_again(ctx):
    raw, data, rec = st.chain_walk_tile(_hk_history())
    assert len(raw) == 512 * 512 >= 4 * 65536 and rec['far'] >= 1, rec
    out, status = ctx.lzw_image_packed(*packed([data]), BlockLayout(1, 1, 512, 512, 512, 512, 1, 0, 1))
    assert status.tolist() == [0] and out.tobytes() == lzw_decode(data, len(raw)) == raw


def _hk_history():
    """ the decoder's HISTORY (hk_lzw_core.h): how far back a string's last appearance may lie to be copied """
    import re
    text = open(os.path.join(os.path.dirname(_hk.__file__), 'csrc', 'hk_lzw_core.h')).read()
    ring = int(re.search(r'constexpr unsigned RING = (\d+),', text).group(1))
    assert re.search(r'constexpr unsigned HISTORY = RING - 4096;', text)
    return ring - 4096


@pytest.mark.oracle
def test_seeded_sweep_of_2048_small_blocks_in_one_call(ctx):
    streams = st.sweep_set(2048, pad_to=600)
    out, status = lzw_rows(ctx, streams)
    assert not status.any()
    for k, s in enumerate(streams):
        assert out[k].tobytes() == s.raw, s.name


# ---- 3. layouts, through both entry points ------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('lay', st.LAYOUTS, ids=lambda lay: lay.name)
def test_every_layout_through_the_host_pointer_call_and_into_a_strided_device_raster(ctx, lay):
    a, streams = st.layout_streams(lay)
    bl = BlockLayout(*st.block_layout(lay))
    exp = ctx.lzw_image(streams, bl)
    assert exp.dtype == a.dtype and exp.tobytes() == a.tobytes()
    es, (n_blocks, _, work_bytes) = bl.sample_bytes, _hk.inflate_bound(bl)
    assert n_blocks == len(streams)
    stride, band_stride = bl.width + 7, (bl.width + 7) * (bl.height + 3) + 5   # rows and planes with room between them
    buf, offsets, sizes = packed(streams)
    out_bytes = bl.spp * band_stride * es
    ptrs = [ctx.dev_alloc(n) for n in (buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, out_bytes, 4 * n_blocks)]
    d_buf, d_off, d_siz, d_work, d_out, d_st = ptrs
    try:
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)
        ctx.h2d(d_out, np.full(out_bytes, 0xAB, np.uint8))
        ctx.lzw_image_dev(bl, d_buf, d_off, d_siz, d_work, d_out, stride, band_stride, d_st, stream=0)
        ctx.stream_sync(0)
        got, status = np.empty(out_bytes, np.uint8), np.empty(n_blocks, np.int32)
        ctx.d2h(got, d_out), ctx.d2h(status, d_st)
    finally:
        for p in ptrs:
            ctx.dev_free(p)
    assert not status.any()
    planes = got.view(exp.dtype).reshape(bl.spp, band_stride)
    inside = np.zeros((bl.spp, band_stride), bool)
    for c in range(bl.spp):
        rows = planes[c, :stride * bl.height].reshape(bl.height, stride)
        assert rows[:, :bl.width].tobytes() == exp[c].tobytes()
        inside[c, :stride * bl.height].reshape(bl.height, stride)[:, :bl.width] = True
    assert (planes[~inside].view(np.uint8) == 0xAB).all(), 'something was written outside the image'


@pytest.mark.oracle
def test_small_groups_give_the_same_bytes(ctx, monkeypatch):
    for lay in st.LAYOUTS:
        if lay.name in ('tiles48-separate-u16-pred2', 'tiles16-contig3-u16', 'strips-short-u32-pred2', 'strips-separate-u64'):
            a, streams = st.layout_streams(lay)
            monkeypatch.setenv('HK_INFLATE_GROUP_KB', '1')   # one block row per group
            got = ctx.lzw_image(streams, BlockLayout(*st.block_layout(lay)))
            monkeypatch.delenv('HK_INFLATE_GROUP_KB')
            assert got.tobytes() == a.tobytes(), lay.name


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_every_refusal_has_its_status_and_leaves_the_other_blocks_alone(ctx):
    ms = st.malformed_set()
    out, status = lzw_rows(ctx, ms, strict=False)
    assert_rows(ms, out, status)
    assert sorted(set(status.tolist())) == list(range(6))   # every status occurs
    with pytest.raises(IoError, match=r'block 1 is refused: the stream ends too soon'):
        lzw_rows(ctx, ms, strict=True)
    for s in ms:
        if s.status != st.OK:
            with pytest.raises(IoError) as ex:
                ctx.lzw_image([ms[0].data, s.data, ms[2].data], row_layout(3, len(s.raw)))
            assert f'block 1 is refused: {LZW_REASONS[s.status]}' in str(ex.value), s.name
    with pytest.raises(ValueError, match='predictor'):
        ctx.lzw_image_packed(np.zeros(64, np.uint8), [0, 10], [10, 10], row_layout(2, 100)._replace(predictor=3))
    with pytest.raises(ValueError, match='aligned'):
        ctx.lzw_image_dev(row_layout(2, 100), 4096, 4096, 4096, 4097, 4096, 100, 200, 4096)


# ---- 5. the product ---------------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_process_and_stats_on_lzw_copies_are_what_they_are_on_the_deflate_originals(ctx, tmp_path):
    rng = np.random.default_rng(23)
    src = np.round(rng.uniform(20.0, 200.0, (2, 140, 180))).astype(np.float32)
    ref = np.round(1.1 * src + 5.0 + rng.normal(0, 2.0, src.shape), 1).astype(np.float32)
    src[:, 50:80, 100:150] = np.nan
    write_tiff(tmp_path / 'src.tif', src, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=64)
    write_tiff(tmp_path / 'ref.tif', ref, TF, CRS('EPSG:32735'), nodata=float('nan'), tile=64)
    for name in ('src', 'ref'):
        (tmp_path / f'{name}_lzw.tif').write_bytes(st.lzw_copy((tmp_path / f'{name}.tif').read_bytes()))
        assert read_tiff(tmp_path / f'{name}_lzw.tif', lzw=ctx.lzw_image).array.tobytes() == read_tiff(tmp_path / f'{name}.tif').array.tobytes()
    files = {}
    for mode, suffix in (('host', ''), ('host', '_lzw'), ('device', '_lzw')):
        d = tmp_path / (mode + suffix)
        d.mkdir()
        files[mode + suffix] = (d / 'corr.tif', d / 'param.tif')
        with RasterFuse(tmp_path / f'src{suffix}.tif', tmp_path / f'ref{suffix}.tif', inflate=mode) as rf:
            rf.process(files[mode + suffix][0], 'gain-offset', (5, 5), param_filename=files[mode + suffix][1])
    for key in ('host_lzw', 'device_lzw'):
        for exp, got in zip(files['host'], files[key]):
            assert read_tiff(exp).array.tobytes() == read_tiff(got).array.tobytes(), key
    param = files['host'][1]
    (tmp_path / 'param_lzw.tif').write_bytes(st.lzw_copy(param.read_bytes()))
    with ParamStats(param) as ps:
        exp = ps.stats()
    for mode in ('host', 'device'):
        with ParamStats(tmp_path / 'param_lzw.tif', inflate=mode) as ps:
            assert repr(ps.stats()) == repr(exp), mode   # (repr: a NaN equals itself)
