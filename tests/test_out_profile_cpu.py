""" The output profile's creation options without a GPU: TIFF predictors 2 and 3 and BigTIFF in ``tiff.write_tiff``, predictor 3 in
``tiff.read_tiff``, ``tiff.bigtiff_wanted``, the options' way through ``RasterFuse.process``, the two new entry points of the C ABI,
and the chunk coder of hk_deflate.hip over predicted bytes as a host program (tests/c/deflate_pred_host.cpp, built with the address
and undefined-behaviour sanitizers).

The references are this file's own: a numpy statement of both predictors (forward and inverse) written from their definition, a
hand-rolled TIFF / BigTIFF writer for the inputs of the reading tests, a directory parser for the layout of the files written,
zlib for every stream, and -- where it is installed with libtiff -- Pillow as an independent reader.  The streams themselves on
the device: tests/test_gpu_out_profile.py. """
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import REPO
from homonim_amd import _hk
from homonim_amd.errors import IoError
from homonim_amd.fuse import RasterFuse
from homonim_amd.geo import Affine, CRS
from homonim_amd import tiff
from homonim_amd.tiff import bigtiff_wanted, read_tiff, read_tiff_overviews, write_tiff

TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)
CHUNK = 16384


# ---- the predictors, stated here -------------------------------------------------------------------------------------------
def predict(rows: np.ndarray, predictor: int, spp: int = 1) -> np.ndarray:
    """ (n_rows, samples) of a sample dtype -> (n_rows, bytes) uint8: the bytes a little-endian file holds under the predictor.
    ``spp`` interleaved samples per pixel: the differencing distance is ``spp`` samples (2) or ``spp`` bytes (3). """
    es = rows.dtype.itemsize
    le = rows.astype(rows.dtype.newbyteorder('<')).view(np.uint8).reshape(rows.shape[0], rows.shape[1], es)
    if predictor == 1:
        return le.reshape(rows.shape[0], -1).copy()
    if predictor == 2:
        wide = np.zeros(rows.shape, object)
        for b in range(es):
            wide = wide + le[:, :, b].astype(object) * (1 << (8 * b))
        diff = wide.copy()
        diff[:, spp:] = (wide[:, spp:] - wide[:, :-spp]) % (1 << (8 * es))
        out = np.zeros(le.shape, np.uint8)
        for b in range(es):
            out[:, :, b] = ((diff >> (8 * b)) % 256).astype(np.uint8)
        return out.reshape(rows.shape[0], -1)
    q = np.concatenate([le[:, :, es - 1 - p] for p in range(es)], axis=1).astype(np.int64)
    d = q.copy()
    d[:, spp:] = (q[:, spp:] - q[:, :-spp]) % 256
    return d.astype(np.uint8)


def unpredict(data: np.ndarray, dtype, predictor: int, spp: int = 1) -> np.ndarray:
    """ the inverse: (n_rows, bytes) uint8 -> (n_rows, samples) of ``dtype`` """
    dtype = np.dtype(dtype)
    es, n_rows = dtype.itemsize, data.shape[0]
    n = data.shape[1] // es
    if predictor == 3:
        q = data.astype(np.int64)
        for k in range(spp, q.shape[1]):
            q[:, k] = (q[:, k] + q[:, k - spp]) % 256
        le = np.stack([q[:, (es - 1 - b) * n:(es - b) * n] for b in range(es)], axis=2).astype(np.uint8)
        return np.ascontiguousarray(le).view(dtype.newbyteorder('<')).reshape(n_rows, n).astype(dtype)
    le = data.reshape(n_rows, n, es)
    if predictor == 1:
        return np.ascontiguousarray(le).view(dtype.newbyteorder('<')).reshape(n_rows, n).astype(dtype)
    wide = np.zeros((n_rows, n), object)
    for b in range(es):
        wide = wide + le[:, :, b].astype(object) * (1 << (8 * b))
    for k in range(spp, n):
        wide[:, k] = (wide[:, k] + wide[:, k - spp]) % (1 << (8 * es))
    out = np.zeros(le.shape, np.uint8)
    for b in range(es):
        out[:, :, b] = ((wide >> (8 * b)) % 256).astype(np.uint8)
    return out.view(dtype.newbyteorder('<')).reshape(n_rows, n).astype(dtype)


def predicted_tiles(a: np.ndarray, tile: int, predictor: int):
    """ the predicted bytes of every zero-padded tile of (bands, h, w), in the writer's order """
    out = []
    for b in range(a.shape[0]):
        for y in range(0, a.shape[1], tile):
            for x in range(0, a.shape[2], tile):
                blk = np.zeros((tile, tile), a.dtype)
                part = a[b, y:y + tile, x:x + tile]
                blk[:part.shape[0], :part.shape[1]] = part
                out.append(predict(blk, predictor).tobytes())
    return out


def special(dtype, shape, seed=0):
    """ content with the values a predictor can trip over: NaN (payloads kept), +-inf, -0.0, denormals; the integer extremes and
    steps that wrap around (255 -> 0) """
    dt, rng = np.dtype(dtype), np.random.default_rng(seed)
    if dt.kind == 'f':
        a = rng.normal(0, 1000, shape).astype(dt)
        flat = a.reshape(-1)
        tiny = np.finfo(dt).tiny
        picks = [np.nan, np.inf, -np.inf, -0.0, 0.0, tiny / 4, -tiny / 8, np.finfo(dt).max, np.finfo(dt).min]
        flat[np.linspace(5, flat.size - 1, len(picks)).astype(int)] = picks
        flat[1:4] = np.nan
        flat.view(f'u{dt.itemsize}')[2] |= 0x1234    # a NaN with a payload
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    flat = a.reshape(-1)
    flat[:6] = [info.max, info.min, info.min, info.max, 0, info.max]
    return a


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- a hand-rolled TIFF / BigTIFF writer for inputs --------------------------------------------------------------------------
_FMT = {1: 'B', 2: 's', 3: 'H', 4: 'I', 16: 'Q'}


def make_tiff(path, a, *, bo='<', big=False, tile=None, rows_per_strip=None, contig=False, predictor=1, lie=None):
    """ (spp, h, w) -> a DEFLATE TIFF: tiles of ``tile`` or strips of ``rows_per_strip`` rows, planar separate or ``contig``,
    classic or BigTIFF, either byte order.  ``lie``: the Predictor tag's value where it is not the predictor applied. """
    spp, h, w = a.shape
    dt = a.dtype
    es = dt.itemsize
    planes = [a[k:k + 1] for k in range(spp)] if not contig else [a]
    blocks = []
    for pl in planes:
        px = np.moveaxis(pl, 0, 2)                                  # (h, w, cspp)
        cspp = px.shape[2]
        if tile:
            for y in range(0, h, tile):
                for x in range(0, w, tile):
                    blk = np.zeros((tile, tile, cspp), dt)
                    part = px[y:y + tile, x:x + tile]
                    blk[:part.shape[0], :part.shape[1]] = part
                    blocks.append(blk.reshape(tile, tile * cspp))
        else:
            for y in range(0, h, rows_per_strip):
                blocks.append(np.ascontiguousarray(px[y:y + rows_per_strip]).reshape(-1, w * cspp))
    cspp = spp if contig else 1
    streams = []
    for blk in blocks:
        data = predict(blk, predictor, cspp)
        if bo == '>' and predictor != 3:    # (predictor 3 orders the bytes itself; the others leave the file's byte order)
            data = np.ascontiguousarray(data.reshape(data.shape[0], -1, es)[:, :, ::-1]).reshape(data.shape[0], -1)
        streams.append(zlib.compress(data.tobytes(), 6))
    kind = {'u': 1, 'i': 2, 'f': 3}[dt.kind]
    word = 16 if big else 4
    entries = [(256, 4, [w]), (257, 4, [h]), (258, 3, [8 * es] * spp), (259, 3, [8]), (262, 3, [1]), (277, 3, [spp]),
               (284, 3, [1 if contig else 2]), (317, 3, [lie or predictor]), (339, 3, [kind] * spp)]
    if tile:
        entries += [(322, 4, [tile]), (323, 4, [tile]), (324, word, None), (325, word, [len(s) for s in streams])]
    else:
        entries += [(278, 4, [rows_per_strip]), (273, word, None), (279, word, [len(s) for s in streams])]
    entries.sort()
    head = 16 if big else 8
    inline, esz = (8, 20) if big else (4, 12)
    ifd_size = (8 + esz * len(entries) + 8) if big else (2 + esz * len(entries) + 4)
    size_of = lambda typ, vals: struct.calcsize('=' + _FMT[typ]) * len(vals)      # noqa: E731
    n_blocks = len(streams)
    pos = head + ifd_size
    where = {}
    for code, typ, vals in entries:
        size = size_of(typ, vals if vals is not None else [0] * n_blocks)
        if size > inline:
            where[code] = pos
            pos += size
    offsets = []
    for s in streams:
        offsets.append(pos)
        pos += len(s)
    off_fmt = 'Q' if big else 'I'
    out = [(b'II' if bo == '<' else b'MM') + (struct.pack(bo + 'HHHQ', 43, 8, 0, head) if big else struct.pack(bo + 'HI', 42, head))]
    out.append(struct.pack(bo + ('Q' if big else 'H'), len(entries)))
    tails = []
    for code, typ, vals in entries:
        vals = offsets if vals is None else vals
        payload = struct.pack(bo + _FMT[typ] * len(vals), *vals)
        out.append(struct.pack(bo + 'HH' + off_fmt, code, typ, len(vals)))
        if len(payload) <= inline:
            out.append(payload.ljust(inline, b'\0'))
        else:
            out.append(struct.pack(bo + off_fmt, where[code]))
            tails.append(payload)
    out.append(struct.pack(bo + off_fmt, 0))
    with open(path, 'wb') as f:
        f.write(b''.join(out + tails + streams))


def parse_ifds(buf: bytes):
    """ the directories of a little-endian TIFF / BigTIFF: -> (is BigTIFF, [ {tag: (type, values)} ]) """
    assert buf[:2] == b'II'
    magic = struct.unpack_from('<H', buf, 2)[0]
    big = magic == 43
    assert magic in (42, 43)
    off = struct.unpack_from('<Q', buf, 8)[0] if big else struct.unpack_from('<I', buf, 4)[0]
    fmts = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 12: 'd', 16: 'Q'}
    dirs = []
    while off:
        n = struct.unpack_from('<Q' if big else '<H', buf, off)[0]
        pos = off + (8 if big else 2)
        tags = {}
        for _ in range(n):
            code, typ = struct.unpack_from('<HH', buf, pos)
            count = struct.unpack_from('<Q' if big else '<I', buf, pos + 4)[0]
            vpos = pos + (12 if big else 8)
            size = struct.calcsize('=' + fmts[typ]) * count
            if size > (8 if big else 4):
                vpos = struct.unpack_from('<Q' if big else '<I', buf, vpos)[0]
            tags[code] = (typ, struct.unpack_from('<' + fmts[typ] * count, buf, vpos))
            pos += 20 if big else 12
        dirs.append(tags)
        off = struct.unpack_from('<Q' if big else '<I', buf, pos)[0]
    return big, dirs


# ---- 1. reading predictor 3 -----------------------------------------------------------------------------------------------
READ_CASES = [
    dict(dtype='float32', shape=(1, 37, 21), rows_per_strip=8),                              # strips, the last one short
    dict(dtype='float64', shape=(2, 37, 21), rows_per_strip=8),
    dict(dtype='float32', shape=(2, 40, 50), tile=16),                                       # tiles with edge tiles
    dict(dtype='float64', shape=(1, 100, 130), tile=48),
    dict(dtype='float32', shape=(3, 40, 50), tile=16, contig=True),                          # 3 samples per pixel interleaved
    dict(dtype='float64', shape=(3, 37, 21), rows_per_strip=5, contig=True),
    dict(dtype='float32', shape=(2, 40, 50), tile=16, bo='>'),                               # big-endian
    dict(dtype='float64', shape=(3, 37, 21), rows_per_strip=8, contig=True, bo='>'),
    dict(dtype='float32', shape=(2, 40, 50), tile=16, big=True),                             # BigTIFF
    dict(dtype='float64', shape=(1, 37, 21), rows_per_strip=8, big=True, bo='>'),
]


@pytest.mark.parametrize('case', READ_CASES, ids=lambda c: '-'.join(f'{k}={v}' for k, v in c.items() if k != 'shape'))
def test_hand_made_predictor_3_files_decode_to_their_input(tmp_path, case):
    kw = dict(case)
    a = special(kw.pop('dtype'), kw.pop('shape'), seed=3)
    make_tiff(tmp_path / 'p3.tif', a, predictor=3, **kw)
    got = read_tiff(tmp_path / 'p3.tif').array
    assert same_bits(got, a)
    # (the helper is held to its own inverse and, for predictor 1, to the existing reader)
    make_tiff(tmp_path / 'p1.tif', a, predictor=1, **kw)
    assert same_bits(read_tiff(tmp_path / 'p1.tif').array, a)


def test_the_numpy_statement_inverts_itself():
    for dtype in ('uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'uint64', 'float32', 'float64'):
        for spp in (1, 3):
            rows = special(dtype, (5, 48 * spp), seed=7)
            pred = 3 if rows.dtype.kind == 'f' else 2
            assert same_bits(unpredict(predict(rows, pred, spp), dtype, pred, spp), rows)
    # the definition on a row one can check by hand: 255 -> 0 wraps to 1, 0 -> 255 to 255
    assert predict(np.array([[255, 0, 255, 255]], np.uint8), 2).tolist() == [[255, 1, 255, 0]]
    assert predict(np.array([[0x0100, 0x00FF]], np.uint16), 2).tolist() == [[0x00, 0x01, 0xFF, 0xFF]]
    # float32 1.0 = 3F 80 00 00, 2.0 = 40 00 00 00: planes 3F 40 | 80 00 | 00 00 | 00 00, then differenced across the planes
    assert predict(np.array([[1.0, 2.0]], np.float32), 3).tolist() == [[0x3F, 0x01, 0x40, 0x80, 0, 0, 0, 0]]


def test_predictors_on_the_wrong_sample_kind_stay_refused(tmp_path):
    make_tiff(tmp_path / 'f2.tif', special('float32', (1, 20, 20)), tile=16, predictor=1, lie=2)
    make_tiff(tmp_path / 'i3.tif', special('int32', (1, 20, 20)), tile=16, predictor=1, lie=3)
    make_tiff(tmp_path / 'i4.tif', special('int32', (1, 20, 20)), tile=16, predictor=1, lie=4)
    for name in ('f2.tif', 'i3.tif', 'i4.tif'):
        with pytest.raises(IoError, match='predictor'):
            read_tiff(tmp_path / name)


def test_a_predictor_3_file_is_not_handed_to_the_inflater(tmp_path):
    calls = []

    def inflater(streams, layout):
        calls.append(layout)
        out = np.empty((layout.spp, layout.height, layout.width), f'u{layout.sample_bytes}')
        raw = [zlib.decompress(s) for s in streams]
        per = -(-layout.width // layout.block_w) * -(-layout.height // layout.block_h)
        for i, r in enumerate(raw):
            p, rem = divmod(i, per)
            by, bx = divmod(rem, -(-layout.width // layout.block_w))
            blk = np.frombuffer(r, out.dtype).reshape(layout.block_h, layout.block_w)
            y, x = by * layout.block_h, bx * layout.block_w
            out[p, y:y + layout.block_h, x:x + layout.block_w] = blk[:layout.height - y, :layout.width - x]
        return out

    a = special('float32', (2, 40, 50), seed=5)
    make_tiff(tmp_path / 'p3.tif', a, tile=16, predictor=3)
    make_tiff(tmp_path / 'p1.tif', a, tile=16, predictor=1)
    assert same_bits(read_tiff(tmp_path / 'p3.tif', inflater=inflater).array, a) and calls == []
    assert same_bits(read_tiff(tmp_path / 'p1.tif', inflater=inflater).array, a) and len(calls) == 1   # (the recorder does record)
    write_tiff(tmp_path / 'w3.tif', a, TF, tile=16, predictor=3, overviews=[a[:, ::2, ::2].copy()])
    assert same_bits(read_tiff_overviews(tmp_path / 'w3.tif', inflater=inflater)[0], a[:, ::2, ::2]) and len(calls) == 1


# ---- 2. writing ----------------------------------------------------------------------------------------------------------
WRITER_DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64']
SHAPES = [((3, 100, 130), 64), ((1, 17, 5), 512), ((2, 50, 170), 80)]


def _levels(a):
    return [np.ascontiguousarray(a[:, ::2, ::2]), np.ascontiguousarray(a[:, ::4, ::4])]


@pytest.mark.parametrize('shape, tile', SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f't{v}')
@pytest.mark.parametrize('dtype', WRITER_DTYPES)
def test_round_trip_of_every_predictor_layout_and_dtype(tmp_path, dtype, shape, tile):
    a = special(dtype, shape, seed=11)
    path = tmp_path / 'w.tif'
    for predictor in (1, 3 if a.dtype.kind == 'f' else 2):
        for big in ('yes', 'no'):
            for levels in ([], _levels(a)):
                write_tiff(path, a, TF, CRS('EPSG:32735'), nodata=0, tile=tile, overviews=levels, predictor=predictor, bigtiff=big,
                           metadata={'K': 'v'}, descriptions=[f'b{i}' for i in range(a.shape[0])])
                back = read_tiff(path)
                assert same_bits(back.array, a), (predictor, big, len(levels))
                assert back.transform == TF and back.metadata == {'K': 'v'} and back.nodata == 0
                assert back.descriptions == tuple(f'b{i}' for i in range(a.shape[0]))
                got = read_tiff_overviews(path)
                assert len(got) == len(levels) and all(same_bits(g, lv) for g, lv in zip(got, levels))
                buf = path.read_bytes()
                is_big, dirs = parse_ifds(buf)
                assert is_big == (big == 'yes') and len(dirs) == 1 + len(levels)
                if is_big:
                    assert buf[:16] == b'II' + struct.pack('<HHHQ', 43, 8, 0, 16)
                for k, (d, img, t) in enumerate(zip(dirs, [a] + levels, [tile] + [128] * len(levels))):
                    assert (317 in d) == (predictor != 1) and (predictor == 1 or d[317] == (3, (predictor,)))
                    assert d[322][1] == (t,) == d[323][1] and (254 in d) == (k > 0)
                    assert d[324][0] == d[325][0] == (16 if is_big else 4)
                    # the tiles the offsets point to are the predicted tiles of the image, in order
                    want = predicted_tiles(img, t, predictor)
                    assert len(d[324][1]) == len(want)
                    for off, cnt, raw in zip(d[324][1], d[325][1], want):
                        assert zlib.decompress(buf[off:off + cnt]) == raw


def test_default_arguments_write_the_classic_file_as_ever(tmp_path):
    a = special('float32', (3, 100, 130), seed=12)
    kw = dict(nodata=float('nan'), tile=64, overviews=_levels(a), metadata={'K': 'v'})
    write_tiff(tmp_path / 'd.tif', a, TF, CRS('EPSG:32735'), **kw)
    write_tiff(tmp_path / 'e.tif', a, TF, CRS('EPSG:32735'), predictor=1, bigtiff='no', **kw)
    buf = (tmp_path / 'd.tif').read_bytes()
    assert buf == (tmp_path / 'e.tif').read_bytes()
    assert buf[:8] == b'II' + struct.pack('<HI', 42, 8)
    is_big, dirs = parse_ifds(buf)
    assert not is_big and all(317 not in d and d[324][0] == 4 for d in dirs)
    # level 6 of the raw tiles, the first tile right behind the directory's values: the layout this writer always had
    raws = predicted_tiles(a, 64, 1)
    assert [zlib.decompress(buf[o:o + n]) for o, n in zip(dirs[0][324][1], dirs[0][325][1])] == raws
    assert buf[dirs[0][324][1][0]:][:dirs[0][325][1][0]] == zlib.compress(raws[0], 6)


def test_writer_refusals(tmp_path):
    f, i = special('float32', (1, 20, 20)), special('uint16', (1, 20, 20))
    with pytest.raises(ValueError, match='predictor'):
        write_tiff(tmp_path / 'x.tif', f, TF, predictor=2)
    with pytest.raises(ValueError, match='predictor'):
        write_tiff(tmp_path / 'x.tif', i, TF, predictor=3)
    with pytest.raises(ValueError, match='predictor'):
        write_tiff(tmp_path / 'x.tif', i, TF, predictor=4)
    with pytest.raises(ValueError, match='predictor'):
        write_tiff(tmp_path / 'x.tif', i, TF, predictor=2, compress=False)
    with pytest.raises(ValueError, match='bigtiff'):
        write_tiff(tmp_path / 'x.tif', i, TF, bigtiff='maybe')
    assert not (tmp_path / 'x.tif').exists()
    write_tiff(tmp_path / 'u.tif', i, TF, compress=False, bigtiff='YES')
    assert parse_ifds((tmp_path / 'u.tif').read_bytes())[0] and same_bits(read_tiff(tmp_path / 'u.tif').array, i)


def test_the_compressor_is_told_the_predictor_only_when_there_is_one(tmp_path):
    calls = []

    def compressor(array, tile, **kw):
        calls.append((array.shape, tile, kw))
        return [zlib.compress(raw, 1) for raw in predicted_tiles(array, tile, kw.get('predictor', 1))]

    a = special('int16', (2, 300, 200), seed=13)
    levels = _levels(a)[:1]
    write_tiff(tmp_path / 'p1.tif', a, TF, overviews=levels, compressor=compressor)
    assert calls == [(a.shape, 512, {}), (levels[0].shape, 128, {})]
    del calls[:]
    write_tiff(tmp_path / 'p2.tif', a, TF, overviews=levels, compressor=compressor, predictor=2, bigtiff=True)
    assert calls == [(a.shape, 512, dict(predictor=2)), (levels[0].shape, 128, dict(predictor=2))]
    for name in ('p1.tif', 'p2.tif'):
        assert same_bits(read_tiff(tmp_path / name).array, a) and same_bits(read_tiff_overviews(tmp_path / name)[0], levels[0])


# ---- Pillow with libtiff as an independent reader ------------------------------------------------------------------------
@pytest.mark.parametrize('big', ['no', 'yes'])
@pytest.mark.parametrize('dtype, predictor', [('uint8', 1), ('uint8', 2), ('uint16', 2), ('int32', 2), ('float32', 1), ('float32', 3)])
def test_pillow_reads_what_write_tiff_writes(tmp_path, dtype, predictor, big):
    Image = pytest.importorskip('PIL.Image')
    features = pytest.importorskip('PIL.features')
    if not features.check('libtiff'):
        pytest.skip('Pillow without libtiff')
    a = special(dtype, (1, 100, 130), seed=14)
    write_tiff(tmp_path / 'w.tif', a, TF, tile=64, predictor=predictor, bigtiff=big)
    with Image.open(tmp_path / 'w.tif') as im:
        got = np.asarray(im)
    assert got.shape == a.shape[1:] and got.dtype.itemsize == a.dtype.itemsize
    assert got.tobytes() == a[0].tobytes()   # bit for bit: NaN payloads, -0.0 and denormals included


# ---- 3. bigtiff_wanted -----------------------------------------------------------------------------------------------------
def test_bigtiff_wanted():
    small, end = 1000, 5000
    for mode in ('yes', 'YES', True, 'Yes'):
        assert bigtiff_wanted(mode, small, True, end) is True
    for mode in ('no', 'NO', False):
        assert bigtiff_wanted(mode, small, True, end) is False
        assert bigtiff_wanted(mode, 3 * 10 ** 9, True, 2 ** 32 - 1) is False
        with pytest.raises(IoError, match='classic'):
            bigtiff_wanted(mode, small, True, 2 ** 32)
    for mode in ('if_safer', 'IF_SAFER'):
        assert bigtiff_wanted(mode, 2_000_000_000, True, end) is False
        assert bigtiff_wanted(mode, 2_000_000_001, True, end) is True
        assert bigtiff_wanted(mode, 2_000_000_001, False, end) is True
        assert bigtiff_wanted(mode, small, True, 2 ** 32 - 1) is False
        assert bigtiff_wanted(mode, small, True, 2 ** 32) is True         # the departure: the classic layout would not fit
    for mode in ('if_needed', 'If_Needed'):
        assert bigtiff_wanted(mode, 4_200_000_000, False, end) is False
        assert bigtiff_wanted(mode, 4_200_000_001, False, end) is True
        assert bigtiff_wanted(mode, 4_200_000_001, True, end) is False     # compressed: not by the raw size
        assert bigtiff_wanted(mode, 2_000_000_001, False, end) is False
        assert bigtiff_wanted(mode, small, True, 2 ** 32 - 1) is False
        assert bigtiff_wanted(mode, 4_200_000_001, True, 2 ** 32) is True  # the departure
    for bad in ('maybe', '', None, 1.5):
        with pytest.raises(ValueError, match='bigtiff'):
            bigtiff_wanted(bad, small, True, end)


# ---- 4. the host build of the coder over predicted bytes ------------------------------------------------------------------
@pytest.fixture(scope='module')
def coder(tmp_path_factory):
    """ tests/c/deflate_pred_host.cpp built with the sanitizers; -> a function [(tile array, predictor)] -> [stream] """
    d = tmp_path_factory.mktemp('deflate_pred')
    exe = d / 'deflate_pred_host'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(REPO, 'homonim_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'deflate_pred_host.cpp'),
                    '-o', str(exe)], check=True)

    def run(cases):
        with open(d / 'in.bin', 'wb') as f:
            f.write(struct.pack('<I', len(cases)))
            for t, predictor in cases:
                assert t.ndim == 2 and t.shape[0] == t.shape[1]
                f.write(struct.pack('<III', t.dtype.itemsize, t.shape[0], predictor) + t.astype(t.dtype.newbyteorder('<')).tobytes())
        subprocess.run([str(exe), str(d / 'in.bin'), str(d / 'out.bin')], check=True, timeout=300)
        out, pos, res = (d / 'out.bin').read_bytes(), 0, []
        for _ in cases:
            (n,) = struct.unpack_from('<I', out, pos)
            res.append(out[pos + 4:pos + 4 + n])
            pos += 4 + n
        assert pos == len(out)
        return res

    return run


def _tile(dtype, tile, kind, seed=0):
    dt, rng = np.dtype(dtype), np.random.default_rng(seed)
    if kind == 'special':
        t = special(dtype, (tile, tile), seed)
    elif kind == 'smooth':
        y, x = np.mgrid[:tile, :tile]
        t = (1000 + 3 * x + 5 * y + rng.integers(0, 3, (tile, tile))).astype(dt)
    elif kind == 'constant':
        t = np.full((tile, tile), 7, dt)
    else:   # 'nan' / extremes: long matches that cross chunk boundaries
        t = np.full((tile, tile), np.nan if dt.kind == 'f' else np.iinfo(dt).max, dt)
    if kind != 'constant':
        t[:, -tile // 5:] = 0     # as an edge tile: the step into the zero padding is part of the row
        t[-3:] = 0
    return t


HOST_CASES = [(dtype, tile, kind)
              for dtype, tiles in [('uint8', (16, 80, 128)), ('int16', (80,)), ('uint32', (80,)), ('int32', (16, 128)), ('uint64', (48,)),
                                   ('float32', (16, 80, 128)), ('float64', (16, 80))]
              for tile in tiles for kind in ('special', 'smooth', 'constant', 'extreme')]


def inflate_tokens(stream: bytes):
    """ a plain inflater that records every match: -> (bytes, [(distance, length)]) of a zlib stream """
    pos, out, matches = 16, bytearray(), []     # bit position behind the two header bytes
    data = int.from_bytes(stream, 'little')

    def bits(n):
        nonlocal pos
        v = (data >> pos) & ((1 << n) - 1)
        pos += n
        return v

    def table(lengths):
        code, tab = 0, {}
        for ln in range(1, 16):
            for s, sl in enumerate(lengths):
                if sl == ln:
                    tab[(ln, code)] = s
                    code += 1
            code <<= 1
        return tab

    def symbol(tab):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | bits(1)
            if (ln, code) in tab:
                return tab[(ln, code)]
        raise AssertionError('no code')

    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
    dext = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
    while True:
        final, btype = bits(1), bits(2)
        if btype == 0:
            pos = (pos + 7) // 8 * 8
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            out += stream[pos // 8:pos // 8 + n]
            pos += 8 * n
        else:
            if btype == 1:
                ll, dd = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = bits(3)
                cl_tab, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = symbol(cl_tab)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                ll, dd = table(lens[:hlit]), table(lens[hlit:])
            while True:
                s = symbol(ll)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = lbase[s - 257] + bits(lext[s - 257])
                    ds = symbol(dd)
                    dist = dbase[ds] + bits(dext[ds])
                    matches.append((dist, length))
                    for _ in range(length):
                        out.append(out[-dist])
        if final:
            return bytes(out), matches


def test_the_host_coder_inflates_to_the_predicted_bytes(coder):
    cases = []
    for dtype, tile, kind in HOST_CASES:
        t = _tile(dtype, tile, kind, seed=len(cases))
        for predictor in (1, 3 if t.dtype.kind == 'f' else 2):
            cases.append((t, predictor))
    streams = coder(cases)
    for (t, predictor), s in zip(cases, streams):
        want = predict(t, predictor).tobytes()
        d = zlib.decompressobj()
        assert d.decompress(s) == want, (t.dtype, t.shape, predictor)
        assert d.eof and d.unused_data == b''
        n = len(want)
        assert len(s) <= 2 + sum(min(CHUNK, n - o) + 5 for o in range(0, n, CHUNK)) + 6
        if t.dtype.itemsize * t.shape[0] <= 128:   # (the recording inflater is slow: the small tiles)
            got, matches = inflate_tokens(s)
            assert got == want
            first = 1 if predictor == 3 else t.dtype.itemsize
            assert {dist for dist, _ in matches} <= {first, t.shape[0] * t.dtype.itemsize}, (t.dtype, t.shape, predictor)


def test_a_predictor_3_stream_matches_at_distance_1_and_the_row_length_only(coder):
    y, x = np.mgrid[:128, :128]
    smooth = (100 + 0.25 * x + 0.5 * (y // 4)).astype(np.float32)     # every row four times: both distances pay
    (s,) = coder([(smooth, 3)])
    got, matches = inflate_tokens(s)
    assert got == predict(smooth, 3).tobytes()
    dists = {d for d, _ in matches}
    assert dists == {1, 512}, dists
    assert len(s) < 0.25 * smooth.nbytes
    # the same tile without a predictor: sample size and row length
    (s1,) = coder([(smooth, 1)])
    assert {d for d, _ in inflate_tokens(s1)[1]} <= {4, 512}


# The streams of predictor 1, pinned: SHA-256 over the streams of arithmetic tiles (no random numbers), made with the coder as it
# stood before the predictors were added.
PINNED_PREDICTOR_1 = '8e9756965ef6ccae28ad42541915d97d6fa6a712d294a6c752cebc8f6812fb61'


def _pinned_tiles():
    y, x = np.mgrid[:128, :128]
    yield ((x * 7 + y * 13) % 251).astype(np.uint8)
    yield ((x // 3) * 257 + (y // 5)).astype(np.uint16)
    yield (np.sin(x / 9.0) * 100 + (y // 2)).astype(np.float32)
    y, x = np.mgrid[:48, :48]
    yield (x * y + 0.5).astype(np.float64)
    yield np.zeros((16, 16), np.int32)


def test_predictor_1_gives_the_bytes_it_gave(coder):
    streams = coder([(t, 1) for t in _pinned_tiles()])
    for t, s in zip(_pinned_tiles(), streams):
        assert zlib.decompress(s) == t.tobytes()
    assert hashlib.sha256(b''.join(streams)).hexdigest() == PINNED_PREDICTOR_1


# ---- 5. process ----------------------------------------------------------------------------------------------------------------
def _pair():
    rng = np.random.default_rng(2)
    src = rng.uniform(20, 200, (2, 60, 70)).astype(np.float32)
    return src, (1.1 * src + 5).astype(np.float32)


REFUSED = [
    ('compress', dict(compress='lzw')), ('compress', dict(compress='zstd')), ('interleave', dict(interleave='pixel')),
    ('tiled', dict(tiled=False)), ('blockysize', dict(blockxsize=256, blockysize=128)), ('blockxsize', dict(blockxsize=100, blockysize=100)),
    ('blockxsize', dict(blockxsize=1024, blockysize=1024)), ('blockxsize', dict(blockxsize=0, blockysize=0)),
    ('predictor', dict(predictor=2)), ('predictor', dict(predictor=4)), ('predictor', dict(predictor='x')),
    ('predictor', dict(predictor=3, compress=None)), ('bigtiff', dict(bigtiff='perhaps')),
]


@pytest.mark.parametrize('key, options', REFUSED, ids=lambda v: ','.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else '')
def test_process_refuses_what_it_cannot_write_before_any_block(monkeypatch, tmp_path, key, options):
    def reached(*a, **k):
        raise AssertionError('a refused option reached the device')

    monkeypatch.setattr(_hk, 'get_context', reached)
    monkeypatch.setattr(_hk, 'Context', reached)
    monkeypatch.setattr(RasterFuse, '_run_blocks', staticmethod(reached))
    with pytest.raises(ValueError, match=f'`{key}`'):
        RasterFuse(*_pair()).process(tmp_path / 'c.tif', 'gain-offset', (5, 5), out_profile=dict(creation_options=options))
    assert not (tmp_path / 'c.tif').exists()


def test_process_refuses_a_predictor_the_output_dtype_does_not_take(monkeypatch, tmp_path):
    def reached(*a, **k):
        raise AssertionError('a refused option reached the device')

    monkeypatch.setattr(_hk, 'get_context', reached)
    monkeypatch.setattr(RasterFuse, '_run_blocks', staticmethod(reached))
    with pytest.raises(ValueError, match='`predictor`'):     # an integer output with the floating-point predictor
        RasterFuse(*_pair()).process(tmp_path / 'c.tif', 'gain-offset', (5, 5),
                                     out_profile=dict(dtype='uint8', nodata=0, creation_options=dict(predictor=3)))
    with pytest.raises(ValueError, match='`predictor`'):     # the parameter file is float32 whatever the output is
        RasterFuse(*_pair()).process(tmp_path / 'c.tif', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.tif',
                                     out_profile=dict(dtype='uint8', nodata=0, creation_options=dict(predictor=2)))


def test_the_options_are_checked_against_the_tif_files_that_are_written_only(monkeypatch, tmp_path):
    """ with no .tif to write the options stay ignored, as they always were; the predictor is held to the files that exist """
    calls, saved = [], []
    monkeypatch.setattr(_hk, 'get_context', lambda dev, streams: _StubContext())
    monkeypatch.setattr(RasterFuse, '_run_blocks', staticmethod(lambda *a, **k: None))
    monkeypatch.setattr(RasterFuse, '_pin', staticmethod(lambda c, arrays: []))
    monkeypatch.setattr(tiff, 'write_tiff', lambda path, array, *a, **kw: calls.append((os.path.basename(path), kw['predictor'])))
    monkeypatch.setattr(np, 'save', lambda path, array: saved.append(os.path.basename(path)))
    bad = dict(compress='lzw', predictor=7, interleave='pixel', tiled=False, blockxsize=100, blockysize=7, bigtiff='perhaps')
    fuse = lambda: RasterFuse(*_pair())   # noqa: E731
    fuse().process(None, 'gain-offset', (5, 5), out_profile=dict(creation_options=bad))
    fuse().process(tmp_path / 'c.npy', 'gain-offset', (5, 5), param_filename=True, out_profile=dict(creation_options=bad))
    assert calls == [] and saved == ['c.npy']
    # uint8 output to .npy, the float32 parameters to .tif: predictor 3 suits the only .tif there is
    fuse().process(tmp_path / 'c.npy', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.tif', build_ovw=False,
                   out_profile=dict(dtype='uint8', nodata=0, creation_options=dict(predictor=3)))
    assert calls == [('p.tif', 3)]
    # and the other way round: predictor 2 for a uint8 .tif while the parameters are not written as .tif
    del calls[:]
    fuse().process(tmp_path / 'c.tif', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.npy', build_ovw=False,
                   out_profile=dict(dtype='uint8', nodata=0, creation_options=dict(predictor=2)))
    assert calls == [('c.tif', 2)]
    with pytest.raises(ValueError, match='`compress`'):      # one .tif is enough for the options to count
        fuse().process(tmp_path / 'c.npy', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.tif', out_profile=dict(creation_options=bad))


class _StubContext:
    device = 0

    def deflate_tiles(self, array, tile, predictor=1):
        raise AssertionError('the stubbed writer compresses nothing')


@pytest.mark.parametrize('deflate', ['host', 'device'])
def test_the_creation_options_reach_the_writer(monkeypatch, tmp_path, deflate):
    ctx, calls = _StubContext(), []
    monkeypatch.setattr(_hk, 'get_context', lambda dev, streams: ctx)
    monkeypatch.setattr(RasterFuse, '_run_blocks', staticmethod(lambda *a, **k: None))
    monkeypatch.setattr(RasterFuse, '_pin', staticmethod(lambda c, arrays: []))
    monkeypatch.setattr(tiff, 'write_tiff', lambda path, array, *a, **kw: calls.append((os.path.basename(path), array.dtype.name, kw)))

    def run(options, **profile):
        del calls[:]
        RasterFuse(*_pair()).process(tmp_path / 'c.tif', 'gain-offset', (5, 5), param_filename=tmp_path / 'p.tif',
                                     out_profile=dict(creation_options=options, **profile) if options is not None else None,
                                     device_config=dict(deflate=deflate), build_ovw=False)
        assert [c[:2] for c in calls] == [('c.tif', profile.get('dtype', 'float32')), ('p.tif', 'float32')]
        return [{k: kw[k] for k in ('tile', 'compress', 'predictor', 'bigtiff', 'compressor')} for _, _, kw in calls]

    comp = ctx.deflate_tiles if deflate == 'device' else None
    default = dict(tile=512, compress=True, predictor=1, bigtiff='if_safer', compressor=comp)
    assert run(None) == [default] * 2
    assert run(dict(driver='GTiff', photometric='rgb', num_threads=4)) == [default] * 2            # other keys stay ignored
    assert run(dict(predictor='3', blockxsize=128, blockysize=128, bigtiff='YES')) == \
        [dict(tile=128, compress=True, predictor=3, bigtiff='YES', compressor=comp)] * 2         # the rest from the default profile
    assert run(dict(compress='DEFLATE', predictor=1, BLOCKXSIZE=16, blockysize='16', bigtiff=False, tiled='yes', interleave='BAND')) == \
        [dict(tile=16, compress=True, predictor=1, bigtiff=False, compressor=comp)] * 2
    for none in (None, 'none', 'NONE'):
        assert run(dict(compress=none, bigtiff='if_needed')) == \
            [dict(tile=512, compress=False, predictor=1, bigtiff='if_needed', compressor=None)] * 2


# ---- 6. the library ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def test_the_library_exports_the_predictor_entry_points(lib):
    for name in ('hk_deflate_tiles_pred', 'hk_deflate_tiles_pred_dev'):
        assert hasattr(lib, name) and name in _hk.SIGNATURES
    assert lib.hk_abi_version() == 12 == _hk.ABI_VERSION


def test_bad_predictor_and_dtype_pairs_are_refused_without_a_context(lib):
    codes = _hk.DTYPE_CODES
    bad = [(codes['float32'], 2), (codes['float64'], 2)] + [(codes[n], 3) for n in ('uint8', 'uint16', 'int16', 'uint32', 'int32')]
    bad += [(codes['uint8'], 0), (codes['uint8'], 4), (codes['float32'], -1), (99, 2)]
    for dtype, predictor in bad:
        # (no context, no buffers: the pair is refused before anything else is looked at)
        rc = lib.hk_deflate_tiles_pred(None, None, dtype, 1, 10, 10, 10, 0, 16, None, 0, None, None, predictor)
        assert rc == _hk.HK_ERR_ARG and (b'predictor' in lib.hk_last_error() or b'dtype' in lib.hk_last_error())
        rc = lib.hk_deflate_tiles_pred_dev(None, None, dtype, 1, 10, 10, 10, 0, 16, None, 0, None, None, 0, predictor)
        assert rc == _hk.HK_ERR_ARG and (b'predictor' in lib.hk_last_error() or b'dtype' in lib.hk_last_error())
    # a good pair gets as far as the missing context
    for dtype, predictor in [(codes['float32'], 3), (codes['uint16'], 2), (codes['float64'], 1)]:
        rc = lib.hk_deflate_tiles_pred(None, None, dtype, 1, 10, 10, 10, 0, 16, None, 0, None, None, predictor)
        assert rc == _hk.HK_ERR_ARG and b'ctx' in lib.hk_last_error()
    # the existing entry points check what they checked, in their order: the context first, whatever the dtype
    assert lib.hk_deflate_tiles(None, None, 99, 1, 10, 10, 10, 0, 16, None, 0, None, None) == _hk.HK_ERR_ARG
    assert b'ctx' in lib.hk_last_error()
    assert lib.hk_deflate_tiles_dev(None, None, 99, 1, 10, 10, 10, 0, 16, None, 0, None, None, 0) == _hk.HK_ERR_ARG
    assert b'ctx' in lib.hk_last_error()
