""" GPU tests of the device DEFLATE path (hk_deflate.hip; hk_deflate_tiles / hk_deflate_tiles_dev; Context.deflate_tiles;
write_tiff(compressor=...); RasterFuse.process(device_config={'deflate': 'device'})).

The reference is exact: a zlib stream is right if and only if ``zlib.decompress`` gives back the tile's raw bytes, which are what
``tiff._tile_chunks`` compresses on the host path.  Every stream of every test is also held to the size the format guarantees --
2 + sum over the chunks of (chunk + 5) + 6 -- and every offset to being even and increasing. """
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from homonim_amd import _hk
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd.tiff import _tile_chunks, read_tiff, read_tiff_header, read_tiff_overviews, write_tiff

pytestmark = pytest.mark.gpu

CHUNK = _hk.DEFLATE_CHUNK


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


def raw_tiles(a, tile):
    a = a if a.ndim == 3 else a[None]
    return _tile_chunks(a.astype(a.dtype.newbyteorder('<'), copy=False), tile, False)


def tile_bound(raw_len):
    return 2 + sum(min(CHUNK, raw_len - o) + 5 for o in range(0, raw_len, CHUNK)) + 6


def checked(ctx, a, tile):
    """ the streams of ``a``, each inflated against its tile's bytes and held to the bound; the packed form's offsets """
    out, offsets, sizes = ctx.deflate_tiles_packed(a, tile)
    raws = raw_tiles(a, tile)
    assert len(sizes) == len(raws) and len(offsets) == len(raws) + 1
    assert (offsets % 2 == 0).all() and offsets[0] == 0 and (np.diff(offsets) > 0).all()
    assert (np.diff(offsets) == sizes + sizes % 2).all() and offsets[-1] <= out.size
    streams = [out[o:o + n].tobytes() for o, n in zip(offsets[:-1].tolist(), sizes.tolist())]
    for t, (s, raw) in enumerate(zip(streams, raws)):
        assert len(s) <= tile_bound(len(raw)), f'tile {t}: {len(s)} bytes exceed the bound {tile_bound(len(raw))}'
        d = zlib.decompressobj()
        assert d.decompress(s) == raw, f'tile {t} does not inflate to its bytes'
        assert d.eof and d.unused_data == b'', f'tile {t}: the stream does not end where its size says'
    assert streams == ctx.deflate_tiles(a, tile)
    return streams


def all_stored(stream, raw):
    """ is the stream 78 9C, one stored block per chunk, 03 00, Adler-32? """
    if len(stream) != tile_bound(len(raw)) or stream[:2] != b'\x78\x9c':
        return False
    pos = 2
    for o in range(0, len(raw), CHUNK):
        n = min(CHUNK, len(raw) - o)
        head = bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255])
        if stream[pos:pos + 5] != head or stream[pos + 5:pos + 5 + n] != raw[o:o + n]:
            return False
        pos += 5 + n
    return stream[pos:pos + 2] == b'\x03\x00'


# ---- shapes and types ------------------------------------------------------------------------------------------------
@pytest.mark.oracle
@pytest.mark.parametrize('dtype', ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64'])
def test_every_dtype_with_edge_tiles(ctx, dtype):
    rng = np.random.default_rng(11)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        a = np.round(rng.normal(100, 20, (3, 37, 53)), 1).astype(dt)
        a[:, :5, :] = np.nan
    else:
        a = (rng.integers(0, 40, (3, 37, 53)) + np.arange(53) // 8).astype(dt)
    checked(ctx, a, 16)


@pytest.mark.oracle
def test_float64_at_tile_512_has_128_chunks_and_row_distance_4096(ctx):
    rng = np.random.default_rng(12)
    a = np.repeat(rng.normal(0, 1, (1, 150, 520)), 4, axis=1)   # every row four times: the row above is a candidate that pays
    a[:, 400:, 300:] = np.nan
    streams = checked(ctx, a, 512)
    assert len(streams) == 4 and sum(map(len, streams)) < 0.6 * 4 * 512 * 512 * 8


@pytest.mark.oracle
def test_float32_at_tile_128(ctx):
    rng = np.random.default_rng(13)
    a = rng.uniform(0.05, 1, (2, 300, 200)).astype(np.float32)
    a[:, :, 150:] = np.nan
    checked(ctx, a, 128)


@pytest.mark.oracle
def test_a_single_pixel(ctx):
    for tile in (16, 512):
        (s,) = checked(ctx, np.array([[[7]]], np.uint8), tile)
        assert len(s) < 60 * -(-tile * tile // CHUNK) + 40   # (per chunk as in test_chosen_content)


# ---- content: one 128 x 128 tile; uint8 is one chunk, uint16 two, float32 four (history crosses chunk boundaries) -----------
def _fibonacci_bytes(rng):
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    body = np.repeat(np.arange(19, dtype=np.uint8) + 40, fib)
    assert body.size == 10945
    rng.shuffle(body)
    return body


def _content(kind, n):
    """ ``n`` bytes of tile content """
    rng = np.random.default_rng(sum(map(ord, kind)))
    if kind == 'zeros':
        return np.zeros(n, np.uint8)
    if kind == 'nan':
        return np.full(n // 4, np.nan, np.float32).view(np.uint8)
    if kind == 'random':
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 'runs':
        parts = []
        for k, length in enumerate((1, 2, 3, 4, 257, 258, 259, 260, 516, 600) * 3):
            parts += [np.full(length, 10 + k % 7, np.uint8), np.array([200 + k, 100 + k], np.uint8)]
        b = np.concatenate(parts)
        return np.concatenate([b, (np.arange(n - b.size) * 7 % 251).astype(np.uint8)])
    if kind == 'straddle':
        b = rng.integers(0, 256, n, dtype=np.uint8)
        b[CHUNK - 300:CHUNK + 500] = 77
        return b
    if kind == 'rows':
        return np.tile(rng.integers(0, 256, n // 128, dtype=np.uint8), 128)
    if kind == 'one-but-one':
        b = np.full(n, 9, np.uint8)
        b[n // 3] = 10
        return b
    if kind == 'fibonacci':   # byte counts F(1) .. F(19), shuffled (see test_the_15_bit_limit_has_to_act for what these do not force)
        body = _fibonacci_bytes(rng)
        reps = -(-n // (body.size + 5439))
        return np.concatenate([np.concatenate([body, np.full(5439, 58, np.uint8)]) for _ in range(reps)])[:n]
    raise KeyError(kind)


CONTENTS = ['zeros', 'nan', 'random', 'runs', 'straddle', 'rows', 'one-but-one', 'fibonacci']


@pytest.mark.oracle
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32'])
@pytest.mark.parametrize('kind', CONTENTS)
def test_chosen_content(ctx, kind, dtype):
    dt = np.dtype(dtype)
    a = _content(kind, 128 * 128 * dt.itemsize).view(dt).reshape(1, 128, 128)
    (s,), (raw,) = checked(ctx, a, 128), raw_tiles(a, 128)
    assert len(raw) == CHUNK * dt.itemsize
    if kind == 'random':
        assert all_stored(s, raw), 'uniform random bytes: every chunk is stored, chunk + 5 bytes long'
    elif kind in ('zeros', 'one-but-one') or (kind == 'nan' and dtype == 'float32'):
        # per chunk: about 64 matches of 258 at one or two bits each, a header of a few symbols, the 5-byte marker
        assert len(s) < 60 * dt.itemsize + 40
    elif kind == 'rows':
        assert len(s) < 700 * dt.itemsize   # one row of literals, then matches at the row distance
    else:
        assert not all_stored(s, raw)


def _strict_fibonacci_chunk(seed):
    """ 16384 bytes whose literal/length counts are 1 (the end of block), 1, 2, 3, 5, ... 2584 and 9621: every partial sum is
    below the next count but one, strictly, so EVERY Huffman code of them is a chain 18 deep whatever the tie-breaking.  The bytes are
    placed so that no three consecutive positions repeat the byte 1 or 128 back: no match exists and the counts are exactly these.
    (The shuffled F(1) .. F(19) of 'fibonacci' do not force the limit: the end-of-block symbol is a third count of 1, which
    turns the chain into a tree 12 to 14 deep, and the runs a shuffle leaves become matches.) """
    fib = [1, 2]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    counts = fib[:-1] + [CHUNK - sum(fib[:-1])]
    top = 40 + 17
    others = np.repeat(np.arange(17, dtype=np.uint8) + 40, counts[:-1])
    np.random.default_rng(seed).shuffle(others)
    b = np.full(CHUNK, top, np.uint8)   # top top x top top x ..., the rest of the others on every twelfth place
    thirds = np.arange(2, CHUNK, 3)
    b[np.sort(np.concatenate([thirds, np.arange(0, CHUNK, 12)[:others.size - thirds.size]]))] = others
    b = b.tolist()

    def bad(p):
        return any(p - 2 - d >= 0 and b[p] == b[p - d] and b[p - 1] == b[p - 1 - d] and b[p - 2] == b[p - 2 - d] for d in (1, 128))

    for p in range(CHUNK):
        if bad(p):
            for q in range(p + 1, CHUNK):
                if b[q] == top or b[p] == top:
                    continue
                b[p], b[q] = b[q], b[p]
                if not bad(p):
                    break
                b[p], b[q] = b[q], b[p]
            else:
                raise AssertionError(f'no swap repairs position {p}')
    b = np.array(b, np.uint8)
    assert not any(bad(p) for p in range(CHUNK)) and sorted(np.bincount(b)[40:58].tolist()) == sorted(counts)
    return b


@pytest.mark.oracle
def test_the_15_bit_limit_has_to_act(ctx):
    a = _strict_fibonacci_chunk(3).reshape(1, 128, 128)
    (s,) = checked(ctx, a, 128)
    assert not all_stored(s, a.tobytes())
    # all literals: no prefix code beats the entropy of the counts, and a Huffman code stays within p_max + 0.086 bits per symbol
    # of it (Gallager); 150 bytes for the header, the marker and what the limit costs on counts that sum to 33 of 16384
    counts = np.bincount(a.ravel())[40:58].astype(float)
    entropy_bytes = -(counts * np.log2(counts / counts.sum())).sum() / 8
    assert entropy_bytes < len(s) < entropy_bytes + (counts.max() / counts.sum() + 0.086) * CHUNK / 8 + 150


# ---- seeded sweep: 4096 tiles of 16 x 16 bytes in one call ---------------------------------------------------------------
def _sweep_tile(i):
    rng = np.random.default_rng(1000 + i)
    kind = i % 4
    if kind == 0 or kind == 1:   # a geometric distribution of random ratio over a random alphabet
        n_sym = int(rng.integers(1, 257))
        alphabet = rng.permutation(256)[:n_sym]
        ratio = rng.uniform(0.3, 0.99) if kind == 0 else rng.uniform(0.5, 0.7)
        p = ratio ** np.arange(n_sym)
        return alphabet[rng.choice(n_sym, 256, p=p / p.sum())].astype(np.uint8)
    if kind == 2:                # runs and literals mixed
        out = []
        while sum(map(len, out)) < 256:
            if rng.random() < 0.5:
                out.append(np.full(int(rng.integers(1, 40)), rng.integers(0, 256), np.uint8))
            else:
                out.append(rng.integers(0, int(rng.integers(1, 257)), int(rng.integers(1, 20))).astype(np.uint8))
        return np.concatenate(out)[:256]
    b = np.full(256, rng.integers(0, 256), np.uint8)   # sparse spikes
    b[rng.choice(256, int(rng.integers(0, 12)), replace=False)] = rng.integers(0, 256)
    return b


@pytest.mark.oracle
def test_seeded_sweep_of_4096_small_tiles(ctx):
    tiles = np.stack([_sweep_tile(i) for i in range(4096)]).reshape(16, 16, 16, 16, 16)   # band, tile row, tile column, 16 x 16
    a = np.ascontiguousarray(tiles.transpose(0, 1, 3, 2, 4)).reshape(16, 256, 256)
    assert raw_tiles(a, 16)[4095] == _sweep_tile(4095).tobytes()
    streams = checked(ctx, a, 16)
    assert len(streams) == 4096
    raws = raw_tiles(a, 16)
    n_stored = sum(all_stored(s, r) for s, r in zip(streams, raws))
    assert 0 < n_stored < 4096   # both forms occur


# ---- determinism and entry points ---------------------------------------------------------------------------------------
def _mixed(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    a = np.round(rng.normal(100, 30, shape)).astype(dtype)
    a[:, : shape[1] // 3] = 0
    return a


@pytest.mark.oracle
def test_two_calls_give_the_same_bytes(ctx):
    a = _mixed(np.float32, (2, 300, 200), 31)
    first = checked(ctx, a, 128)
    for _ in range(2):
        assert ctx.deflate_tiles(a, 128) == first


@pytest.mark.oracle
@pytest.mark.parametrize('dtype, tile', [('uint8', 16), ('uint16', 128), ('float64', 512)])
def test_device_entry_point_gives_the_bytes_of_the_host_entry_point(ctx, dtype, tile):
    a = _mixed(dtype, (2, 150, 333), 32)
    out, offsets, sizes = ctx.deflate_tiles_packed(a, tile)
    checked(ctx, a, tile)
    nb, h, w = a.shape
    n_tiles, cap = _hk.deflate_bound(dtype, nb, h, w, tile)
    d_src, d_out = ctx.dev_alloc(a.nbytes), ctx.dev_alloc(cap)
    d_off, d_siz = ctx.dev_alloc(8 * (n_tiles + 1)), ctx.dev_alloc(8 * n_tiles)
    try:
        ctx.h2d(d_src, a)
        ctx.deflate_tiles_dev(d_src, dtype, nb, h, w, w, h * w, tile, d_out, cap, d_off, d_siz, stream=0)
        ctx.stream_sync(0)
        got_off, got_siz, got = np.empty(n_tiles + 1, np.int64), np.empty(n_tiles, np.int64), np.empty(cap, np.uint8)
        ctx.d2h(got_off, d_off), ctx.d2h(got_siz, d_siz), ctx.d2h(got, d_out)
    finally:
        for p in (d_src, d_out, d_off, d_siz):
            ctx.dev_free(p)
    assert (got_off == offsets).all() and (got_siz == sizes).all()
    assert got[:got_off[-1]].tobytes() == out[:offsets[-1]].tobytes()


@pytest.mark.oracle
def test_strided_views_and_small_groups_give_the_same_bytes(ctx, monkeypatch):
    big = _mixed(np.uint16, (3, 310, 420), 33)
    view = big[:, 5:305, 11:411]
    assert not view.flags['C_CONTIGUOUS']
    exp = checked(ctx, np.ascontiguousarray(view), 128)
    assert ctx.deflate_tiles(view, 128) == exp
    assert ctx.deflate_tiles(view[::2], 128) == exp[:12] + exp[24:]       # a band stride of two planes
    assert ctx.deflate_tiles(view[0, ::2], 128) == checked(ctx, np.ascontiguousarray(view[:1, ::2]), 128)   # 2-D, a row stride of two
    monkeypatch.setenv('HK_DEFLATE_GROUP_KB', '1')                         # one tile row per group
    assert ctx.deflate_tiles(view, 128) == exp


def test_argument_errors_are_exceptions_with_a_message(ctx):
    a = np.zeros((1, 20, 20), np.uint8)
    for tile in (0, 24, 1024):
        with pytest.raises(ValueError, match='tile'):
            ctx.deflate_tiles(a, tile)
    with pytest.raises(ValueError):
        ctx.deflate_tiles(a.astype(np.complex64), 16)
    with pytest.raises(ValueError):
        ctx.deflate_tiles(np.zeros((0, 4), np.uint8), 16)


# ---- size ---------------------------------------------------------------------------------------------------------------
def host_rle_size(raw):
    """ zlib with the Z_RLE strategy at level 6, flushed every DEFLATE_CHUNK bytes: the host coder nearest to the device's scheme """
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    n = 0
    for o in range(0, len(raw), CHUNK):
        n += len(c.compress(raw[o:o + CHUNK])) + len(c.flush(zlib.Z_SYNC_FLUSH))
    return n + len(c.flush())


def _size_rasters():
    for name in ('sentinel2_b432_byte', 'ngi_rgb_byte_1', 'landsat8_byte'):
        yield name, read_tiff(os.path.join(GOLDEN_DIR, 'rasters', name + '.tif')).array
    f = np.random.default_rng(0).uniform(0.05, 1, (1, 1024, 1024)).astype(np.float32)
    f[:, :100] = np.nan
    f[:, :, 900:] = np.nan
    yield 'float32-nan-borders', f


@pytest.mark.oracle
@pytest.mark.parametrize('name, a', list(_size_rasters()), ids=lambda v: v if isinstance(v, str) else '')
def test_size_is_within_two_percent_of_host_rle(ctx, name, a):
    """ (the scheme's size model against the same reference: 0.992 / 0.999 / 0.975 / 0.894) """
    streams = checked(ctx, a, 512)
    raws = raw_tiles(a, 512)
    dev, host = sum(map(len, streams)), sum(host_rle_size(r) + 6 for r in raws)
    level6 = sum(len(zlib.compress(r, 6)) for r in raws)
    print(f'[deflate size] {name}: device {dev}, Z_RLE reference {host}, ratio {dev / host:.4f}; level 6 {level6}, ratio {dev / level6:.4f}')
    assert dev <= 1.02 * host


# ---- integration --------------------------------------------------------------------------------------------------------
@pytest.mark.oracle
def test_write_tiff_with_the_device_compressor(ctx, tmp_path):
    rng = np.random.default_rng(41)
    a = np.round(rng.normal(100, 20, (2, 700, 900)), 1).astype(np.float32)
    a[:, :60] = np.nan
    levels = ctx.overviews(a, float('nan'), 2)
    tf = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)
    write_tiff(tmp_path / 'd.tif', a, tf, CRS('EPSG:32735'), nodata=float('nan'), overviews=levels, compressor=ctx.deflate_tiles)
    write_tiff(tmp_path / 'h.tif', a, tf, CRS('EPSG:32735'), nodata=float('nan'), overviews=levels)
    d, h = read_tiff(tmp_path / 'd.tif'), read_tiff(tmp_path / 'h.tif')
    assert d.array.tobytes() == a.tobytes() == h.array.tobytes()
    assert d.transform == h.transform and d.crs == h.crs and d.metadata == h.metadata and np.isnan(d.nodata)
    got = read_tiff_overviews(tmp_path / 'd.tif')
    assert len(got) == 2 and all(g.tobytes() == lv.tobytes() for g, lv in zip(got, levels))
    checked(ctx, a, 512)


@pytest.mark.oracle
def test_process_writes_the_same_rasters_with_device_deflate(ctx, tmp_path):
    from test_gpu_overviews import seeded_pair
    src, ref = seeded_pair((1100, 1600), 21)
    files = {}
    for mode in ('host', 'device'):
        files[mode] = (tmp_path / f'corr_{mode}.tif', tmp_path / f'param_{mode}.tif')
        corr, params = RasterFuse(src, ref).process(files[mode][0], 'gain-offset', (5, 5), param_filename=files[mode][1],
                                                    device_config=dict(deflate=mode))
    for host_file, dev_file, arr in zip(files['host'], files['device'], (corr, params)):
        h, d = read_tiff(host_file), read_tiff(dev_file)
        assert d.array.dtype == h.array.dtype and d.array.tobytes() == h.array.tobytes() == arr.tobytes()
        assert d.transform == h.transform and d.crs == h.crs and d.metadata == h.metadata and d.descriptions == h.descriptions
        assert (d.nodata == h.nodata) or (np.isnan(d.nodata) and np.isnan(h.nodata))
        assert read_tiff_header(dev_file)[:4] == read_tiff_header(host_file)[:4]
        lh, ld = read_tiff_overviews(host_file), read_tiff_overviews(dev_file)
        assert len(lh) == len(ld) == 2 and all(x.tobytes() == y.tobytes() for x, y in zip(lh, ld))
        assert host_file.read_bytes() != dev_file.read_bytes()
    checked(ctx, corr, 512)
