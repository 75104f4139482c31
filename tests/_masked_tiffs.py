""" Masked GeoTIFFs for the tests of the per-dataset mask (tests/test_dataset_mask_cpu.py, tests/test_gpu_dataset_mask.py,
tools/make_mask_fixtures.py): a classic little-endian file that ``tiff.write_tiff`` wrote gets a 1-bit mask directory appended,
or its ExtraSamples tag (338) patched, with ``struct`` -- none of the package's reading code is involved -- and the numpy statement
of what a masked read returns.

The mask directory is what GDAL writes with GDAL_TIFF_INTERNAL_MASK: NewSubfileType 4, 1 bit per sample, 1 sample per pixel,
photometric 4 (transparency mask), FillOrder 1 (the most significant bit is the first pixel), strips or tiles, uncompressed,
DEFLATE or LZW. """
import struct
import zlib

import numpy as np

import _lzw_streams

NONE, LZW, DEFLATE = 1, 5, 8
COMPRESSIONS = {'none': NONE, 'deflate': DEFLATE, 'lzw': LZW}


def pack_bits(valid: np.ndarray) -> np.ndarray:
    """ (h, w) bool -> (h, ceil(w / 8)) uint8, the most significant bit first, pad bits 0 """
    return np.packbits(np.asarray(valid, bool), axis=1)


def unpack_bits(packed: np.ndarray, width: int) -> np.ndarray:
    return np.unpackbits(packed, axis=1)[:, :width].astype(bool)


def masked_f32(array: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """ THE STATEMENT: what a masked read of (bands, h, w) ``array`` under the (h, w) validity gives; compare as bytes """
    with np.errstate(over='ignore'):   # (a float64 past float32's range rounds to infinity: that is the conversion)
        return np.where(valid, array.astype(np.float32), np.float32('nan'))


def same_bytes(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _code(raw: bytes, compression: int) -> bytes:
    if compression == NONE:
        return raw
    if compression == DEFLATE:
        return zlib.compress(raw, 6)
    if compression == LZW:
        return _lzw_streams.encode(raw)
    raise ValueError(compression)


def mask_blocks(valid: np.ndarray, tile=None, rows_per_strip=None):
    """ the raw bytes of every block of the 1-bit image of ``valid``: tiles of ``tile`` x ``tile`` pixels (a multiple of 16), padded
    with zero bits, or strips of ``rows_per_strip`` rows (default: 8), the last one short """
    h, w = valid.shape
    if tile:
        across, down = -(-w // tile), -(-h // tile)
        padded = np.zeros((down * tile, across * tile), bool)
        padded[:h, :w] = valid
        return [pack_bits(padded[by * tile:(by + 1) * tile, bx * tile:(bx + 1) * tile]).tobytes() for by in range(down) for bx in range(across)]
    rps = rows_per_strip or 8
    return [pack_bits(valid[r0:r0 + rps]).tobytes() for r0 in range(0, h, rps)]


def _ifd_chain(buf):
    """ offsets of the directories of a classic little-endian TIFF, and where the last one's next pointer lies """
    assert bytes(buf[:4]) == b'II*\0', 'a classic little-endian TIFF'
    (off,) = struct.unpack_from('<I', buf, 4)
    chain, at = [], 4
    while off:
        (n,) = struct.unpack_from('<H', buf, off)
        chain.append(off)
        at = off + 2 + 12 * n
        (off,) = struct.unpack_from('<I', buf, at)
    return chain, at


def append_mask(data: bytes, valid: np.ndarray, tile=None, compression=NONE, rows_per_strip=None, subfile=4, predictor=None,
                fill_order=None) -> bytes:
    """ ``data`` (a classic little-endian TIFF) with a mask directory of ``valid`` (h, w) chained behind its last directory.
    ``subfile``: NewSubfileType (4: the mask of the main image; 5: a mask of an overview).  ``predictor`` / ``fill_order``: the tags
    317 / 266 where given (the blocks are written as with 1 / 1 whatever they say: the reader refuses such files by the tag). """
    buf = bytearray(data)
    _, next_at = _ifd_chain(buf)
    if len(buf) % 2:
        buf += b'\0'
    h, w = valid.shape
    streams = [_code(raw, compression) for raw in mask_blocks(valid, tile, rows_per_strip)]
    entries = [(254, 4, [subfile]), (256, 4, [w]), (257, 4, [h]), (258, 3, [1]), (259, 3, [compression]), (262, 3, [4])]
    if fill_order is not None:
        entries.append((266, 3, [fill_order]))
    entries.append((277, 3, [1]))
    if predictor is not None:
        entries.append((317, 3, [predictor]))
    if tile:
        entries += [(322, 4, [tile]), (323, 4, [tile]), (324, 4, None), (325, 4, [len(s) for s in streams])]
    else:
        entries += [(273, 4, None), (278, 4, [rows_per_strip or 8]), (279, 4, [len(s) for s in streams])]
    entries.sort(key=lambda e: e[0])
    ifd_off = len(buf)
    pos = ifd_off + 2 + 12 * len(entries) + 4
    fmt = {3: 'H', 4: 'I'}
    placed = {}
    for code, typ, values in entries:   # the values that do not fit an entry
        count = len(streams) if values is None else len(values)
        if count * struct.calcsize(fmt[typ]) > 4:
            placed[code] = pos
            pos += count * struct.calcsize(fmt[typ])
            pos += pos % 2
    offsets = []
    for s in streams:
        offsets.append(pos)
        pos += len(s) + len(s) % 2
    out = bytearray(struct.pack('<H', len(entries)))
    tail = bytearray()
    for code, typ, values in entries:
        values = offsets if values is None else values
        payload = struct.pack('<' + fmt[typ] * len(values), *values)
        out += struct.pack('<HHI', code, typ, len(values))
        if code in placed:
            out += struct.pack('<I', placed[code])
            assert ifd_off + 2 + 12 * len(entries) + 4 + len(tail) == placed[code]
            tail += payload + b'\0' * (len(payload) % 2)
        else:
            out += payload.ljust(4, b'\0')
    out += struct.pack('<I', 0) + tail
    for s in streams:
        out += s + b'\0' * (len(s) % 2)
    struct.pack_into('<I', buf, next_at, ifd_off)
    return bytes(buf + out)


def set_extra_samples(data: bytes, values: dict) -> bytes:
    """ ``data`` with entries of the first directory's ExtraSamples (338) replaced: {band: value}; the tag of a file of n bands that
    ``write_tiff`` wrote has n - 1 entries, for the bands 1 .. n - 1 """
    buf = bytearray(data)
    chain, _ = _ifd_chain(buf)
    off = chain[0]
    (n,) = struct.unpack_from('<H', buf, off)
    tags = {struct.unpack_from('<H', buf, off + 2 + 12 * k)[0]: off + 2 + 12 * k for k in range(n)}
    (spp,) = struct.unpack_from('<H', buf, tags[277] + 8)
    e = tags[338]
    typ, count = struct.unpack_from('<HI', buf, e + 2)
    assert typ == 3
    at = e + 8 if count * 2 <= 4 else struct.unpack_from('<I', buf, e + 8)[0]
    for band, value in values.items():
        idx = band - (spp - count)
        assert 0 <= idx < count, (band, spp, count)
        struct.pack_into('<H', buf, at + 2 * idx, value)
    return bytes(buf)


# ---- the committed fixtures (tools/make_mask_fixtures.py writes them; tests/golden/tiff/mask/) -------------------------------
FIXTURE_SHAPE = (80, 64)   # height, width of the source files; the reference is 40 x 32 on the same extent


def fixture_pixels(bands=3, dtype='uint8', seed=5):
    """ (bands, 80, 64) smooth pixels with noise, never 0 """
    h, w = FIXTURE_SHAPE
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    scale = 1 if np.dtype(dtype).itemsize == 1 else 200
    a = [(60 + 50 * np.sin(x / 9.0 + b) + 40 * np.cos(y / 7.0 - b) + rng.integers(0, 2, (h, w))) * scale for b in range(bands)]
    return np.clip(np.stack(a), 1, 255 * scale).astype(dtype)


def fixture_valid():
    """ the footprint of the fixtures: a tilted quadrilateral with a hole, so rows start and end off the byte boundaries """
    h, w = FIXTURE_SHAPE
    y, x = np.mgrid[0:h, 0:w]
    inside = (x + 0.3 * y > 9) & (x - 0.2 * y < 57) & (y + 0.15 * x > 5) & (y - 0.1 * x < 70)
    hole = (x - 37) ** 2 + (y - 41) ** 2 < 30
    return inside & ~hole


def fixture_reference():
    """ (3, 40, 32) float32: the 2 x 2 means of a smooth relative of the source, with an offset and a gain per band """
    a = fixture_pixels(3, 'uint8', seed=6).astype(np.float32)
    ref = a.reshape(3, 40, 2, 32, 2).mean(axis=(2, 4))
    return (ref * np.array([0.004, 0.003, 0.0035], np.float32)[:, None, None] + np.array([0.02, 0.05, 0.01], np.float32)[:, None, None]).astype(np.float32)
