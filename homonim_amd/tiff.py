"""
Minimal GeoTIFF reader / writer for the rasters either side of the hot path (no GDAL, no rasterio in this image).

Covers what the reference reads and writes (all of homonim's test rasters and its own output
profile, homonim/fuse.py:124-149): classic or BigTIFF, little / big endian, strips or tiles, planar ``separate`` or
``contig``, uncompressed, DEFLATE (zlib) or LZW with predictor none / horizontal differencing / floating point (3), 8 / 16 /
32 / 64-bit integer and IEEE float samples; geo-referencing from ModelPixelScale + ModelTiepoint or ModelTransformation; nodata
from GDAL_NODATA; EPSG code / citation from the GeoKey directory; the ``<GDALMetadata>`` items (where the reference keeps
its FUSE_* provenance, fuse.py:193-207) and the per-band ``DESCRIPTION`` items among them (the band names of a parameter
file, fuse.py:241-248).  The writer produces tiled, DEFLATE, band-separate files like the reference's
default output profile -- classic or BigTIFF, with predictor 2 or 3 on request -- with internal overviews (reduced-resolution
images chained behind the first) on request;
``read_tiff_overviews`` reads those back.  A rotated or sheared grid is read from, and on request written as, a
ModelTransformation matrix.  Alpha bands (ExtraSamples 1 / 2) are named and an internal 1-bit mask directory (NewSubfileType 4) is
decoded to its packed bits (``TiffRaster.alpha_bands``, ``mask_band``, ``mask``; applying them is ``fuse.dataset_masked``'s).  The writer
chains such a mask behind an image without a nodata value on request, and one (NewSubfileType 5) behind every overview level;
``read_tiff_overviews(masks=True)`` reads those back.  LZW is read only (``lzw_decode``, or a hook of ``read_tiff``).  Everything else (other
compressions, palettes) raises.
"""
import mmap
import re
import struct
import zlib
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple
from xml.sax.saxutils import escape, unescape

import numpy as np

from homonim_amd.errors import IoError
from homonim_amd.geo import Affine, CRS

_TYPES = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 5: 'II', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 10: 'ii', 11: 'f', 12: 'd', 16: 'Q',
          17: 'q', 18: 'Q'}
_SAMPLE_DTYPES = {(1, 8): 'u1', (1, 16): 'u2', (1, 32): 'u4', (1, 64): 'u8', (2, 8): 'i1', (2, 16): 'i2', (2, 32): 'i4',
                  (2, 64): 'i8', (3, 32): 'f4', (3, 64): 'f8'}

T_SUBFILE = 254   # NewSubfileType: bit 0 = reduced-resolution version of another image of the file, bit 2 = transparency mask of one
T_FILL_ORDER = 266
T_WIDTH, T_HEIGHT, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_STRIP_OFFSETS, T_SPP, T_ROWS_PER_STRIP = 256, 257, 258, 259, 262, 273, 277, 278
T_STRIP_COUNTS, T_PLANAR, T_PREDICTOR, T_TILE_W, T_TILE_H, T_TILE_OFFSETS, T_TILE_COUNTS, T_EXTRA, T_FORMAT = 279, 284, 317, 322, 323, 324, 325, 338, 339
T_PIXEL_SCALE, T_TIEPOINT, T_TRANSFORMATION, T_GEOKEYS, T_GEODOUBLES, T_GEOASCII, T_GDAL_METADATA, T_GDAL_NODATA = 33550, 33922, 34264, 34735, 34736, 34737, 42112, 42113


class TiffRaster(NamedTuple):
    array: np.ndarray            # (bands, height, width), the file's sample dtype
    transform: Affine
    crs: CRS
    nodata: Optional[float]
    metadata: Dict[str, str]     # dataset-level <GDALMetadata> items
    descriptions: Tuple[Optional[str], ...] = ()   # per band: GDAL's band description, None where the file has none
    mask: Optional[np.ndarray] = None              # the internal mask as stored: packed bits (height, ceil(width / 8)) uint8, most significant bit first, 1 = valid
    alpha_bands: Tuple[int, ...] = ()              # 0-based: the bands whose ExtraSamples entry is 1 or 2
    mask_band: Optional[int] = None                # the alpha band that acts as the mask (no internal mask, no nodata tag)


class TiffHeader(NamedTuple):
    """ What ``read_tiff_header`` finds without decoding a pixel. """
    count: int
    height: int
    width: int
    dtype: str                   # numpy name of the sample type, or '' outside the reader's subset
    transform: Affine
    crs: CRS
    nodata: Optional[float]
    metadata: Dict[str, str]
    descriptions: Tuple[Optional[str], ...]
    alpha_bands: Tuple[int, ...] = ()   # as in TiffRaster
    has_mask: bool = False              # an internal mask directory is chained behind the first image


class BlockLayout(NamedTuple):
    """ How the blocks (tiles or strips) of one image lie in its raster: what an ``inflater`` of ``read_tiff`` is told (the
    fields of hk_inflate_layout, include/homonim_hk.h, in its order).  An ``lzw`` hook is told the same. """
    sample_bytes: int            # 1, 2, 4, 8; the samples are little-endian
    spp: int
    height: int
    width: int
    block_w: int                 # tile size; strips: the image's width and the rows per strip
    block_h: int
    tiled: int                   # 1: every block holds block_h rows; 0: the last strip is short
    separate: int                # 1: one plane per block, blocks ordered plane, block row, block column; 0: pixel-interleaved
    predictor: int               # 1 none, 2 horizontal differencing, 3 floating point (only for a hook whose ``predictors`` has 3)


def _read_ifd(buf: bytes, offset: Optional[int] = None):
    """ -> (byte order, tags, offset of the next directory or 0) of the directory at ``offset`` (None: the file's first) """
    if buf[:2] == b'II':
        bo = '<'
    elif buf[:2] == b'MM':
        bo = '>'
    else:
        raise IoError('not a TIFF file')
    magic = struct.unpack(bo + 'H', buf[2:4])[0]
    if magic == 42:
        big, (off,) = False, struct.unpack(bo + 'I', buf[4:8])
        off = off if offset is None else offset
        n, pos, esz, cfmt, vsz = struct.unpack(bo + 'H', buf[off:off + 2])[0], off + 2, 12, 'I', 4
    elif magic == 43:
        big, (off,) = True, struct.unpack(bo + 'Q', buf[8:16])
        off = off if offset is None else offset
        n, pos, esz, cfmt, vsz = struct.unpack(bo + 'Q', buf[off:off + 8])[0], off + 8, 20, 'Q', 8
    else:
        raise IoError('not a TIFF file')
    tags = {}
    for i in range(n):
        e = buf[pos + i * esz: pos + (i + 1) * esz]
        code, typ = struct.unpack(bo + 'HH', e[:4])
        count = struct.unpack(bo + cfmt, e[4:4 + vsz])[0]
        if typ not in _TYPES:
            continue
        item = _TYPES[typ]
        size = struct.calcsize('=' + item) * count
        if size <= vsz:
            raw = e[4 + vsz:4 + vsz + size]
        else:
            (voff,) = struct.unpack(bo + cfmt, e[4 + vsz:4 + 2 * vsz])
            raw = buf[voff:voff + size]
        if typ == 2:
            tags[code] = raw.split(b'\0')[0].decode('latin-1') if code != T_GEOASCII else raw.decode('latin-1').rstrip('\0')
        elif typ in (5, 10):
            v = struct.unpack(bo + item[0] * (2 * count), raw)
            tags[code] = tuple(v[2 * k] / v[2 * k + 1] if v[2 * k + 1] else 0. for k in range(count))
        else:
            tags[code] = struct.unpack(bo + item * count, raw)
    (next_off,) = struct.unpack(bo + cfmt, buf[pos + n * esz: pos + n * esz + vsz])
    return bo, tags, next_off


def _geo(tags, height):
    if T_TRANSFORMATION in tags:
        m = tags[T_TRANSFORMATION]   # the 4 x 4 matrix, row-major: rotation and shear terms included
        tf = Affine(m[0], m[1], m[3], m[4], m[5], m[7])
    elif T_PIXEL_SCALE in tags and T_TIEPOINT in tags:
        sx, sy = tags[T_PIXEL_SCALE][:2]
        i, j, _, x, y, _ = tags[T_TIEPOINT][:6]
        tf = Affine(sx, 0., x - i * sx, 0., -sy, y + j * sy)
    else:
        tf = Affine.identity()
    name = None
    if T_GEOKEYS in tags:
        keys = tags[T_GEOKEYS]
        ascii_params, doubles = tags.get(T_GEOASCII, ''), tags.get(T_GEODOUBLES, ())
        entries = {keys[4 + 4 * k]: keys[5 + 4 * k: 8 + 4 * k] for k in range(keys[3])}

        def value(key):
            loc, cnt, off = entries[key]
            if loc == 0:
                return off
            if loc == T_GEODOUBLES:
                return doubles[off] if cnt == 1 else tuple(doubles[off:off + cnt])
            if loc == T_GEOASCII:
                return ascii_params[off:off + cnt].rstrip('|')
            return None

        model_type = value(1024) if 1024 in entries else None
        code_key = 2048 if model_type == 2 else 3072  # geographic / projected CS type
        if code_key in entries and entries[code_key][0] == 0 and value(code_key) not in (0, 32767):
            name = f'EPSG:{value(code_key)}'
        else:
            # user-defined CRS (all of the reference's test rasters): the label is the full key list, citations aside,
            # so two rasters compare equal exactly when their definitions do
            body = '; '.join(f'{k}={value(k)}' for k in sorted(entries) if k not in (1026, 2049, 3073))
            cite = next((value(k) for k in (1026, 3073, 2049) if k in entries and entries[k][0] == T_GEOASCII), '')
            # (a citation that already carries a key list is a label this module wrote: keep it, so it round-trips)
            name = cite if ('[' in cite and cite.endswith(']')) else (f'{cite} [{body}]' if cite else f'[{body}]')
    return tf, CRS(name) if name else CRS()


def _metadata(tags) -> Dict[str, str]:
    xml = tags.get(T_GDAL_METADATA)
    if not xml:
        return {}
    out = {}
    for m in re.finditer(r'<Item name="([^"]*)"([^>]*)>(.*?)</Item>', xml, flags=re.S):
        if 'sample=' not in m.group(2):  # dataset-level items only
            out[unescape(m.group(1), {'&quot;': '"'})] = unescape(m.group(3), {'&quot;': '"'})
    return out


def _descriptions(tags, count: int) -> Tuple[Optional[str], ...]:
    """ GDAL's band descriptions: ``<Item name="DESCRIPTION" sample="N" role="description">`` with N counted from 0 """
    out = [None] * count
    for m in re.finditer(r'<Item name="DESCRIPTION"([^>]*)>(.*?)</Item>', tags.get(T_GDAL_METADATA) or '', flags=re.S):
        sample = re.search(r'sample="(\d+)"', m.group(1))
        if sample and 'role="description"' in m.group(1) and int(sample.group(1)) < count:
            out[int(sample.group(1))] = unescape(m.group(2), {'&quot;': '"'})
    return tuple(out)


def _nodata_tag(t) -> Optional[float]:
    try:
        return float(t[T_GDAL_NODATA].strip()) if T_GDAL_NODATA in t else None
    except ValueError:
        return None


def _alpha_bands(t) -> Tuple[int, ...]:
    """ The bands ExtraSamples (338) calls alpha, associated (1) or not (2): its entries describe the LAST len(extra) samples """
    spp, extra = t.get(T_SPP, (1,))[0], t.get(T_EXTRA, ())
    first = spp - len(extra)
    return tuple(first + i for i, e in enumerate(extra) if e in (1, 2) and 0 <= first + i < spp)


def _is_mask(t) -> bool:
    """ Is this directory a transparency mask (NewSubfileType bit 2), of the main image or of an overview? """
    return bool(t.get(T_SUBFILE, (0,))[0] & 4)


def _mask_directory(buf, t0, nxt):
    """ The tags of the internal mask of the first image (tags ``t0``; ``nxt``: the offset of the directory behind it), or None: the
    first directory of the chain with NewSubfileType bit 2 set and bit 0 clear, 1 bit per sample and 1 sample per pixel.  It has
    the first image's size, or the file is refused. """
    seen = set()
    while nxt and nxt not in seen:
        seen.add(nxt)
        _, t, following = _read_ifd(buf, nxt)
        sub = t.get(T_SUBFILE, (0,))[0]
        if sub & 4 and not sub & 1 and tuple(t.get(T_BITS, (1,))) == (1,) and t.get(T_SPP, (1,))[0] == 1 and T_WIDTH in t and T_HEIGHT in t:
            shape, main = (t[T_HEIGHT][0], t[T_WIDTH][0]), (t0[T_HEIGHT][0], t0[T_WIDTH][0])
            if shape != main:
                raise IoError(f'the internal mask is {shape[0]} x {shape[1]}, the image {main[0]} x {main[1]}')
            return t
        nxt = following
    return None


def _decode_mask(buf, bo, t, inflater=None, lzw=None) -> np.ndarray:
    """ The packed bits of a 1-bit mask directory, (height, ceil(width / 8)) uint8 as stored: the directory is decoded as the BYTE
    image it is -- a block row of ``bw`` pixels is ``bw / 8`` bytes (tile widths are multiples of 16), a strip row ceil(width / 8) --
    so the block decoders and the hooks of ``read_tiff`` take it as they are. """
    predictor, order = t.get(T_PREDICTOR, (1,))[0], t.get(T_FILL_ORDER, (1,))[0]
    if predictor != 1:
        raise IoError(f'unsupported TIFF predictor {predictor} for a 1-bit mask (none is)')
    if order != 1:
        raise IoError(f'unsupported FillOrder {order} for a 1-bit mask (1, most significant bit first, is)')
    w = t[T_WIDTH][0]
    as_bytes = dict(t)
    as_bytes[T_WIDTH], as_bytes[T_BITS], as_bytes[T_SPP], as_bytes[T_FORMAT] = (-(-w // 8),), (8,), (1,), (1,)
    as_bytes.pop(T_EXTRA, None)
    if T_TILE_OFFSETS in t:
        if t[T_TILE_W][0] % 8:
            raise IoError(f'unsupported tile width {t[T_TILE_W][0]} for a 1-bit mask (a multiple of 8 is)')
        as_bytes[T_TILE_W] = (t[T_TILE_W][0] // 8,)
    return _decode_image(buf, bo, as_bytes, inflater, lzw)[0]


def _mask_band(t, dtype, nodata, has_mask: bool, alpha: Tuple[int, ...]) -> Optional[int]:
    """ The alpha band that masks the image: no internal mask, no nodata tag, exactly 2 or 4 bands, the last one alpha, uint8 or
    uint16 samples (GDAL's GetMaskBand order as its documentation gives it) """
    spp = t.get(T_SPP, (1,))[0]
    if has_mask or nodata is not None or spp not in (2, 4) or (spp - 1) not in alpha or str(dtype) not in ('uint8', 'uint16'):
        return None
    return spp - 1


def read_tiff_header(path) -> TiffHeader:
    """ Shape, geo-referencing, nodata, ``<GDALMetadata>`` items and band descriptions of the first image of a GeoTIFF.  Only
    the directory and the values it points to are read (the file is mapped, not loaded): validating a parameter file does not
    cost its pixels. """
    with open(path, 'rb') as f:
        try:
            buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:   # an empty file cannot be mapped
            raise IoError('not a TIFF file')
        with buf:
            bo, t, nxt = _read_ifd(buf)
            if T_WIDTH not in t or T_HEIGHT not in t:
                raise IoError('not a TIFF file')
            has_mask = _mask_directory(buf, t, nxt) is not None
    w, h = t[T_WIDTH][0], t[T_HEIGHT][0]
    spp = t.get(T_SPP, (1,))[0]
    bits, fmt = t.get(T_BITS, (1,)), t.get(T_FORMAT, (1,) * spp)
    uniform = len(set(bits)) == 1 and len(set(fmt)) == 1 and (fmt[0], bits[0]) in _SAMPLE_DTYPES
    dtype = np.dtype(_SAMPLE_DTYPES[(fmt[0], bits[0])]).name if uniform else ''
    tf, crs = _geo(t, h)
    return TiffHeader(spp, h, w, dtype, tf, crs, _nodata_tag(t), _metadata(t), _descriptions(t, spp), _alpha_bands(t), has_mask)


def read_tiff(path, inflater=None, lzw=None) -> TiffRaster:
    """ Read the first image of a GeoTIFF into a (bands, height, width) array.  ``inflater``: a callable ``(streams, layout) ->
    array`` that takes the zlib streams of ALL blocks of a DEFLATE image (a list of ``bytes`` in the file's block order) and
    their ``BlockLayout`` and returns the image as a (spp, height, width) array of unsigned integers of the sample size, the
    predictor undone, in place of ``zlib.decompress`` block after block on this thread (e.g. ``Context.inflate_image``: this
    module itself imports no GPU code).  It is handed little-endian DEFLATE images only; anything else, and everything with
    None, is decoded here as ever.  ``lzw``: the same hook for LZW images (compression 5), under the same contract: the LZW
    streams of all blocks of a little-endian image with predictor 1 or 2 (e.g. ``Context.lzw_image`` or ``_hk.lzw_image_host``).
    With None, and for big-endian images, the blocks go through ``lzw_decode``, which is slow.  Predictor 3 (floating point): a
    hook of either kind is handed such an image only if it has an attribute ``predictors`` that holds 3, as those of
    ``homonim_amd._hk`` have -- it then undoes the predictor as ``_unpredict_float`` states it and returns the samples' bit
    patterns; for a hook without the attribute the image is decoded here as with None. """
    with open(path, 'rb') as f:
        buf = f.read()
    bo, t, nxt = _read_ifd(buf)
    out = _decode_image(buf, bo, t, inflater, lzw)
    tf, crs = _geo(t, out.shape[1])
    mt = _mask_directory(buf, t, nxt)
    mask = None if mt is None else _decode_mask(buf, bo, mt, inflater, lzw)
    nodata, alpha = _nodata_tag(t), _alpha_bands(t)
    return TiffRaster(out, tf, crs, nodata, _metadata(t), _descriptions(t, out.shape[0]), mask, alpha,
                      _mask_band(t, out.dtype, nodata, mask is not None, alpha))


def read_tiff_overviews(path, inflater=None, lzw=None, masks: bool = False):
    """ The internal overviews of a GeoTIFF: the reduced-resolution images (NewSubfileType bit 0) chained behind the first, in
    file order, each as a (bands, height, width) array.  ``[]`` for a file without any.  ``inflater``, ``lzw``: as in ``read_tiff``,
    called once per level.  ``masks``: return ``(levels, level_masks)`` -- a level's mask is the first directory with NewSubfileType
    5 (reduced + mask), 1 bit per sample and one sample per pixel that has the level's shape, as an (h, w) bool array, True = valid;
    None for a level without one. """
    with open(path, 'rb') as f:
        buf = f.read()
    bo, t, nxt = _read_ifd(buf)
    out, mask_dirs, seen = [], [], set()
    while nxt and nxt not in seen:
        seen.add(nxt)
        bo, t, following = _read_ifd(buf, nxt)
        if t.get(T_SUBFILE, (0,))[0] & 1 and not _is_mask(t):   # (a mask of an overview is no overview)
            out.append(_decode_image(buf, bo, t, inflater, lzw))
        elif t.get(T_SUBFILE, (0,))[0] & 5 == 5 and tuple(t.get(T_BITS, (1,))) == (1,) and t.get(T_SPP, (1,))[0] == 1:
            mask_dirs.append(t)
        nxt = following
    if not masks:
        return out
    level_masks = []
    for lv in out:
        mt = next((t for t in mask_dirs if (t[T_HEIGHT][0], t[T_WIDTH][0]) == lv.shape[1:]), None)
        level_masks.append(None if mt is None else unpack_mask(_decode_mask(buf, bo, mt, inflater, lzw), lv.shape[2]))
    return out, level_masks


def unpack_mask(packed: np.ndarray, width: int) -> np.ndarray:
    """ The packed bits of an internal mask (``TiffRaster.mask``: (height, ceil(width / 8)) uint8, most significant bit first) as
    an (height, width) bool array, True = valid """
    return np.unpackbits(packed, axis=1, count=width).astype(bool)


# why ``lzw_decode`` refuses a stream: the texts of HK_LZW_* (include/homonim_hk.h), by status
LZW_REASONS = ('ok', 'the stream ends too soon', 'old-style (pre-6.0) LZW bit order', 'the first code after a Clear is no byte',
               'a code beyond the table', "end of information before the block's bytes are there")


def lzw_decode(stream, raw_size: int) -> bytes:
    """ The ``raw_size`` bytes of one TIFF LZW stream (compression 5), in plain Python: SLOW (well below 1 MB/s) -- the product
    reads whole rasters through the library (``_hk.lzw_image_host``, ``Context.lzw_image``); this one reads a file where there
    is no library, and is what the tests hold those two to.  Codes of 9..12 bits, most significant bit first; 256 Clear, 257 end
    of information, entries from 258; the width grows once the next free entry is 2^width - 1 (libtiff's early change); a full
    table adds nothing more; the stream starts as if behind a Clear; decoding ends with the raw size, a last string is cut.
    ``IoError`` with one of ``LZW_REASONS`` otherwise. """
    data = bytes(stream)
    if not data:
        raise IoError(f'LZW: {LZW_REASONS[1]}')
    if len(data) >= 2 and data[0] == 0 and data[1] & 1:
        raise IoError(f'LZW: {LZW_REASONS[2]}')
    table = [bytes([i]) for i in range(256)] + [b'', b'']
    out = bytearray()
    acc = nacc = pos = used = 0
    width, prev, limit = 9, None, 8 * len(data)
    while len(out) < raw_size:
        while nacc < width:   # (bits past the end are zero bits, and taking one is refused below)
            acc = (acc << 8) | (data[pos] if pos < len(data) else 0)
            pos, nacc = pos + 1, nacc + 8
        nacc, used = nacc - width, used + width
        if used > limit:
            raise IoError(f'LZW: {LZW_REASONS[1]}')
        c = acc >> nacc
        acc &= (1 << nacc) - 1
        if c == 256:
            del table[258:]
            width, prev = 9, None
            continue
        if c == 257:
            raise IoError(f'LZW: {LZW_REASONS[5]}')
        if prev is None:
            if c > 255:
                raise IoError(f'LZW: {LZW_REASONS[3]}')
            s = table[c]
        else:
            n = len(table)
            if c > n:
                raise IoError(f'LZW: {LZW_REASONS[4]}')
            s = table[c] if c < n else prev + prev[:1]
            if n < 4096:
                table.append(prev + s[:1])
                if n + 1 == (1 << width) - 1 and width < 12:
                    width += 1
        out += s
        prev = s
    return bytes(out[:raw_size])


def _decode_image(buf, bo, t, inflater=None, lzw=None) -> np.ndarray:
    """ The pixels of the image a directory describes, (bands, height, width) in native byte order """
    w, h = t[T_WIDTH][0], t[T_HEIGHT][0]
    spp = t.get(T_SPP, (1,))[0]
    bits = t.get(T_BITS, (1,))
    fmt = t.get(T_FORMAT, (1,) * spp)
    if len(set(bits)) != 1 or len(set(fmt)) != 1 or (fmt[0], bits[0]) not in _SAMPLE_DTYPES:
        raise IoError(f'unsupported sample layout: bits {bits}, format {fmt}')
    dtype = np.dtype(bo + _SAMPLE_DTYPES[(fmt[0], bits[0])])
    compression = t.get(T_COMPRESSION, (1,))[0]
    if compression not in (1, 5, 8, 32946):
        raise IoError(f'unsupported TIFF compression {compression} (none, LZW and DEFLATE are)')
    predictor = t.get(T_PREDICTOR, (1,))[0]
    if predictor not in (1, 2, 3) or (predictor == 2 and dtype.kind == 'f') or (predictor == 3 and dtype.kind != 'f'):
        raise IoError(f'unsupported TIFF predictor {predictor} for samples of {dtype}')
    planar = t.get(T_PLANAR, (1,))[0]
    if T_TILE_OFFSETS in t:
        bw, bh, offs, cnts = t[T_TILE_W][0], t[T_TILE_H][0], t[T_TILE_OFFSETS], t[T_TILE_COUNTS]
    else:
        bw, bh = w, min(t.get(T_ROWS_PER_STRIP, (h,))[0], h)
        offs, cnts = t[T_STRIP_OFFSETS], t[T_STRIP_COUNTS]
    across, down = -(-w // bw), -(-h // bh)
    chunk_spp = 1 if planar == 2 else spp
    tiled = T_TILE_OFFSETS in t
    # (a hook's contract knows predictors 1 and 2; the floating-point predictor goes to a hook that names 3 in its ``predictors``
    # and is undone here for every other)
    if compression == 5:
        inflater = lzw
    if inflater is not None and compression != 1 and bo == '<' and (predictor != 3 or 3 in getattr(inflater, 'predictors', (1, 2))):
        if len(offs) != len(cnts) or len(offs) != (spp if planar == 2 else 1) * across * down:
            raise IoError(f'{len(offs)} block offsets and {len(cnts)} byte counts for {(spp if planar == 2 else 1) * across * down} blocks')
        layout = BlockLayout(dtype.itemsize, spp, h, w, bw, bh, int(tiled), int(planar == 2), predictor)
        got = np.asarray(inflater([bytes(buf[off:off + cnt]) for off, cnt in zip(offs, cnts)], layout))
        if got.shape != (spp, h, w) or got.dtype.itemsize != dtype.itemsize:
            raise IoError(f'the inflater returned {got.shape} of {got.dtype} for an image of {(spp, h, w)} of {dtype}')
        return np.ascontiguousarray(got).view(dtype.newbyteorder('='))
    out = np.empty((spp, h, w), dtype.newbyteorder('='))
    for idx, (off, cnt) in enumerate(zip(offs, cnts)):
        plane, rem = divmod(idx, across * down) if planar == 2 else (0, idx)
        by, bx = divmod(rem, across)
        rows = bh if tiled else min(bh, h - by * bh)
        raw = buf[off:off + cnt]
        if compression == 5:
            try:
                raw = lzw_decode(raw, rows * bw * chunk_spp * dtype.itemsize)
            except IoError as ex:
                raise IoError(f'block {idx} is refused: {ex}') from None
        elif compression != 1:
            raw = zlib.decompress(raw)
        if predictor == 3:
            block = _unpredict_float(raw, rows, bw, chunk_spp, dtype.itemsize)
        else:
            block = np.frombuffer(raw, dtype, count=rows * bw * chunk_spp).reshape(rows, bw, chunk_spp)
        if predictor == 2:
            block = np.cumsum(block, axis=1, dtype=dtype.newbyteorder('='))
        y0, x0 = by * bh, bx * bw
        hh, ww = min(rows, h - y0), min(bw, w - x0)
        if planar == 2:
            out[plane, y0:y0 + hh, x0:x0 + ww] = block[:hh, :ww, 0]
        else:
            out[:, y0:y0 + hh, x0:x0 + ww] = np.moveaxis(block[:hh, :ww, :], 2, 0)
    return out


def _unpredict_float(raw, rows: int, bw: int, cspp: int, es: int) -> np.ndarray:
    """ libtiff's floating-point predictor (3) undone on a block of ``rows`` rows of ``bw`` pixels of ``cspp`` samples of ``es``
    bytes: every row is differenced byte by byte at a distance of ``cspp`` bytes, and holds ``es`` planes of ``bw * cspp`` bytes,
    the most significant byte of every sample first -- whatever the file's byte order.  -> (rows, bw, cspp), native floats """
    n = bw * cspp
    d = np.frombuffer(raw, np.uint8, count=rows * n * es).reshape(rows, n * es // cspp, cspp)
    q = np.cumsum(d, axis=1, dtype=np.uint8).reshape(rows, es, n)
    be = np.ascontiguousarray(q.transpose(0, 2, 1))   # per sample its bytes, most significant first
    return be.view(f'>f{es}').reshape(rows, bw, cspp).astype(f'=f{es}')


def _predict_rows(blk: np.ndarray, predictor: int) -> bytes:
    """ The bytes of a block of little-endian samples (rows, samples) under TIFF predictor 2 (integers: every sample minus the one
    before it in its row, modulo 2^bits) or 3 (floats: the row's bytes as planes, most significant byte first, then differenced
    byte by byte over the whole row) -- what a DEFLATE tile of a file with tag 317 holds; 1: the bytes themselves """
    if predictor == 1:
        return blk.tobytes()
    es = blk.dtype.itemsize
    if predictor == 2:
        u = blk.view(f'<u{es}')
        out = u.copy()
        out[:, 1:] = u[:, 1:] - u[:, :-1]
        return out.tobytes()
    q = np.ascontiguousarray(blk).view(np.uint8).reshape(blk.shape[0], blk.shape[1], es)[:, :, ::-1]
    q = np.ascontiguousarray(q.transpose(0, 2, 1)).reshape(blk.shape[0], es * blk.shape[1])
    out = q.copy()
    out[:, 1:] = q[:, 1:] - q[:, :-1]
    return out.tobytes()


# ----------------------------------------------------------------------------------------------------------------------
OVERVIEW_TILE = 128   # GDAL's default block size of overviews (GDAL_TIFF_OVR_BLOCKSIZE)


def _tile_chunks(a: np.ndarray, tile: int, compress: bool, predictor: int = 1) -> List[bytes]:
    nb, h, w = a.shape
    across, down = -(-w // tile), -(-h // tile)
    chunks = []
    for b in range(nb):
        for by in range(down):
            for bx in range(across):
                blk = np.zeros((tile, tile), a.dtype)
                part = a[b, by * tile:(by + 1) * tile, bx * tile:(bx + 1) * tile]
                blk[:part.shape[0], :part.shape[1]] = part
                raw = _predict_rows(blk, predictor)
                chunks.append(zlib.compress(raw, 6) if compress else raw)
    return chunks


BIGTIFF_SAFER_BYTES = 2_000_000_000    # 'if_safer': BigTIFF for a main image of more raw bytes than this
BIGTIFF_NEEDED_BYTES = 4_200_000_000   # 'if_needed': ... for an uncompressed one of more raw bytes than this


def bigtiff_wanted(mode, raw_bytes: int, compressed: bool, classic_end: int) -> bool:
    """ Is the file written as BigTIFF?  ``mode``: the ``bigtiff`` creation option -- 'yes' / True, 'no' / False, 'if_needed',
    'if_safer' in any case; ``raw_bytes``: bands x height x width x itemsize of the main image; ``classic_end``: where the
    file would end in the classic layout (every size is known before the first byte is written).  'yes': BigTIFF.  'no':
    classic, an ``IoError`` where that does not fit.  'if_needed': BigTIFF for an uncompressed file of more than 4 200 000 000
    raw bytes.  'if_safer': BigTIFF for more than 2 000 000 000 raw bytes.  In both ``if_`` modes a file whose classic layout would
    not fit is BigTIFF whatever its raw size (the thresholds restate GDAL's rule, the last clause is this
    package's own). """
    if isinstance(mode, bool):
        mode = 'yes' if mode else 'no'
    mode = str(mode).lower()
    fits = classic_end < 2 ** 32
    if mode == 'yes':
        return True
    if mode == 'no':
        if not fits:
            raise IoError("raster too large for a classic TIFF (bigtiff='no')")
        return False
    if mode == 'if_needed':
        return (not compressed and raw_bytes > BIGTIFF_NEEDED_BYTES) or not fits
    if mode == 'if_safer':
        return raw_bytes > BIGTIFF_SAFER_BYTES or not fits
    raise ValueError(f"`bigtiff` must be 'yes', 'no', 'if_needed' or 'if_safer', not {mode!r}")


def _layout(entries, chunks, ifd_off: int, big: bool):
    """ Where one image placed at ``ifd_off`` puts what.  ``entries``: its directory without the tile offsets and byte counts; they
    are added here as LONG, or LONG8 in a BigTIFF.  -> (all entries in tag order, offsets of the values that do not fit an entry by
    tag, tile offsets, offset just behind the image: where the next directory goes) """
    inline, typ = (8, 16) if big else (4, 4)
    counts = struct.pack('<' + _TYPES[typ] * len(chunks), *[len(c) for c in chunks])
    entries = sorted(list(entries) + [(T_TILE_OFFSETS, typ, len(chunks), b'\0' * len(counts)), (T_TILE_COUNTS, typ, len(chunks), counts)],
                     key=lambda e: e[0])
    extra_off = ifd_off + ((8 + 20 * len(entries) + 8) if big else (2 + 12 * len(entries) + 4))
    placed = {}
    for code, _, _, payload in entries:
        if len(payload) > inline:
            placed[code] = extra_off
            extra_off += len(payload) + len(payload) % 2
    offsets, pos = [], extra_off
    for c in chunks:
        offsets.append(pos)
        pos += len(c) + (len(c) % 2)
    return entries, placed, offsets, pos


def _directory(entries, chunks, ifd_off: int, has_next: bool, big: bool = False) -> Tuple[bytes, int]:
    """ One image of a classic TIFF (``big``: of a BigTIFF -- 64-bit entry count, 20-byte entries with up to 8 bytes inline,
    64-bit next offset) placed at ``ifd_off``: directory, the values that do not fit an entry, tile data.  ``entries``: as in
    ``_layout``.  -> (bytes, offset just behind them: where the next directory goes) """
    entries, placed, offsets, pos = _layout(entries, chunks, ifd_off, big)
    if not big and pos >= 2 ** 32:
        raise IoError('raster too large for a classic TIFF')
    inline, word = (8, 'Q') if big else (4, 'I')
    off_payload = struct.pack('<' + word * len(offsets), *offsets)
    entries = [(code, typ, count, off_payload if code == T_TILE_OFFSETS else payload) for code, typ, count, payload in entries]
    parts = [struct.pack('<' + ('Q' if big else 'H'), len(entries))]
    for code, typ, count, payload in entries:
        parts.append(struct.pack('<HH' + word, code, typ, count))
        parts.append(payload.ljust(inline, b'\0') if len(payload) <= inline else struct.pack('<' + word, placed[code]))
    parts.append(struct.pack('<' + word, pos if has_next else 0))
    for code, typ, count, payload in entries:
        if len(payload) > inline:
            parts.append(payload + b'\0' * (len(payload) % 2))
    for c in chunks:
        parts.append(c + b'\0' * (len(c) % 2))
    return b''.join(parts), pos


def write_tiff(path, array: np.ndarray, transform: Affine, crs: Optional[CRS] = None, nodata: Optional[float] = None,
               metadata: Optional[Dict[str, str]] = None, tile: int = 512, compress: bool = True,
               descriptions: Optional[Sequence[Optional[str]]] = None, overviews: Optional[Sequence[np.ndarray]] = None,
               rotated: bool = False, compressor=None, predictor: int = 1, bigtiff='if_safer', mask: Optional[np.ndarray] = None,
               overview_masks: Optional[Sequence[np.ndarray]] = None):
    """ Write (bands, height, width) as a little-endian GeoTIFF: tiled, DEFLATE, band-separate -- the reference's
    default output profile (homonim/fuse.py:124-149: tiled 512 x 512, compress=deflate, interleave=band).  ``descriptions``:
    one band description per band (None: none for that band), written as GDAL writes them.  ``overviews``: the internal
    overviews (homonim/fuse.py:152-165), finest first, each (bands, h_m, w_m) of the raster's dtype: one directory per level
    chained behind the main image's, NewSubfileType = 1, 128-pixel tiles, the main image's sample format, planar
    configuration and compression, GDAL_NODATA and no geo tags.  The main image is written the same with and without them.
    ``rotated``: accept a rotated / sheared ``transform`` and write it as a ModelTransformation matrix instead of pixel scale +
    tie point; without it such a transform is refused -- everything this package produces is north-up, so a rotated grid on
    the way out is a mistake unless it is asked for.  ``compressor``: a callable ``(array3d, tile) -> list of bytes`` that returns
    one zlib stream per tile of a (bands, h, w) array in this writer's tile order -- band, tile row, tile column; a tile is
    ``tile`` rows of ``tile`` little-endian samples, edge tiles zero-padded -- used for the main image (at ``tile``) and for every
    overview level (at 128) in place of ``zlib.compress`` (e.g. ``Context.deflate_tiles``: this module itself imports no GPU
    code).  None: zlib level 6 on this thread, the same bytes as ever.  ``predictor``: TIFF tag 317 of the main image and of every
    overview level -- 1 none (no tag), 2 horizontal differencing (integer dtypes), 3 the floating-point predictor (float dtypes):
    every padded tile row is predicted before it is compressed (``_predict_rows``); a compressor is then called as
    ``compressor(array3d, tile, predictor=predictor)`` and returns the streams of the predicted tiles; it needs ``compress``.
    ``bigtiff``: 'yes', 'no', 'if_needed' or 'if_safer' (``bigtiff_wanted``): classic TIFF or BigTIFF (magic 43, 64-bit offsets,
    tile offsets and byte counts as LONG8).  A main image of at most 2 000 000 000 raw bytes is, with the defaults, the classic
    file this function always wrote.
    ``mask``: an (height, width) array, a pixel valid where it is not 0 -- the per-dataset internal mask of an image WITHOUT a nodata
    value (rasterio's ``write_mask`` under GDAL_TIFF_INTERNAL_MASK=True); ``overview_masks``: one such mask per overview level, of
    the level's shape.  Either beside a nodata value is a ``ValueError``: the reader lets a mask overrule the tag, and this writer
    does not produce such files.  Every mask is a directory of its own: NewSubfileType 4 (the main image's) or 5 (a level's:
    reduced + mask), the image's width and length, 1 bit per sample, 1 sample per pixel, PhotometricInterpretation 4
    (transparency mask), no FillOrder (most significant bit first), no predictor, tiled at its image's tile size (a tile row is
    ``tile / 8`` bytes, edge tiles zero-padded), Compression 8 with one zlib stream per tile where the file is compressed, else
    1.  The bits are packed with ``numpy.packbits`` and compressed with zlib on this thread: ``compressor`` is for sample tiles.
    Directory order: the main image, its mask, the overview levels, their masks in level order; the main image's directory and
    data lie where they lie without a mask, only its next-directory pointer differs. """
    if compressor is not None and not compress:
        raise ValueError('a compressor was given for an uncompressed file (compress=False)')
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[None]
    predictor = int(predictor)
    if predictor not in (1, 2, 3):
        raise ValueError(f'`predictor` must be 1, 2 or 3, not {predictor}')
    if predictor != 1 and not compress:
        raise ValueError(f'predictor {predictor} was given for an uncompressed file (compress=False)')
    if (predictor == 2 and a.dtype.kind == 'f') or (predictor == 3 and a.dtype.kind != 'f'):
        raise ValueError(f"predictor {predictor} does not apply to dtype '{a.dtype}' (2: integers, 3: floats)")
    bigtiff_wanted(bigtiff, 0, compress, 0)   # (an unknown mode is refused before anything is compressed)
    key = {('u', 1): (1, 8), ('u', 2): (1, 16), ('u', 4): (1, 32), ('i', 1): (2, 8), ('i', 2): (2, 16), ('i', 4): (2, 32),
           ('f', 4): (3, 32), ('f', 8): (3, 64)}.get((a.dtype.kind, a.dtype.itemsize))
    if key is None:
        raise IoError(f"unsupported dtype '{a.dtype}'")
    if (transform.b != 0 or transform.d != 0) and not rotated:
        raise IoError('rotated / sheared grids are not written unless asked for (rotated=True)')
    fmt, bits = key
    nb, h, w = a.shape
    levels = []
    for lv in (overviews or ()):
        lv = np.asarray(lv)
        lv = lv[None] if lv.ndim == 2 else lv
        if lv.ndim != 3 or lv.shape[0] != nb or lv.dtype != a.dtype or lv.size == 0:
            raise ValueError(f'an overview of shape {lv.shape}, dtype {lv.dtype} for a raster of {nb} band(s), dtype {a.dtype}')
        levels.append(lv.astype(lv.dtype.newbyteorder('<'), copy=False))
    if (mask is not None or overview_masks is not None) and nodata is not None:
        raise ValueError(f'an internal mask beside a nodata value ({nodata}): a masked file carries no nodata tag')
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (h, w):
            raise ValueError(f'a mask of shape {mask.shape} for a raster of {h} x {w}')
    level_masks = [np.asarray(m) for m in overview_masks] if overview_masks is not None else []
    if overview_masks is not None:
        if len(level_masks) != len(levels):
            raise ValueError(f'{len(level_masks)} overview masks for {len(levels)} overview levels')
        for m, lv in zip(level_masks, levels):
            if m.shape != lv.shape[1:]:
                raise ValueError(f'an overview mask of shape {m.shape} for a level of {lv.shape[1]} x {lv.shape[2]}')
    a = a.astype(a.dtype.newbyteorder('<'), copy=False)
    tile = max(16, (int(tile) + 15) // 16 * 16)

    def ascii_(s):
        return s.encode('latin-1', 'replace') + b'\0'

    def image_entries(img, img_tile, reduced):
        """ the directory of one image without its tile offsets and byte counts (``_directory`` adds those, in the layout's width) """
        entries = []  # (code, type, count, payload bytes)

        def add(code, typ, values):
            if typ == 2:
                payload = ascii_(values)
                entries.append((code, 2, len(payload), payload))
            else:
                payload = struct.pack('<' + _TYPES[typ] * len(values), *values)
                entries.append((code, typ, len(values), payload))

        if reduced:
            add(T_SUBFILE, 4, [1])
        add(T_WIDTH, 4, [img.shape[2]]), add(T_HEIGHT, 4, [img.shape[1]]), add(T_BITS, 3, [bits] * nb)
        add(T_COMPRESSION, 3, [8 if compress else 1]), add(T_PHOTOMETRIC, 3, [1]), add(T_SPP, 3, [nb]), add(T_PLANAR, 3, [2])
        if predictor != 1:
            add(T_PREDICTOR, 3, [predictor])
        add(T_TILE_W, 4, [img_tile]), add(T_TILE_H, 4, [img_tile])
        if nb > 1:
            add(T_EXTRA, 3, [0] * (nb - 1))
        add(T_FORMAT, 3, [fmt] * nb)
        if nodata is not None:
            add(T_GDAL_NODATA, 2, 'nan' if (isinstance(nodata, float) and np.isnan(nodata)) else repr(float(nodata)) if a.dtype.kind == 'f' else str(int(nodata)))
        if not reduced:
            geo_entries(add)
        return entries

    def mask_image(m, img_tile, reduced):
        """ (directory entries, tile chunks) of the 1-bit mask directory of an image tiled at ``img_tile`` """
        mh, mw = m.shape
        bits_ = np.zeros((-(-mh // img_tile) * img_tile, -(-mw // img_tile) * img_tile), np.uint8)
        bits_[:mh, :mw] = m != 0
        packed = np.packbits(bits_, axis=1)   # most significant bit first; a tile row is img_tile / 8 bytes
        tb = img_tile // 8
        chunks = []
        for by in range(bits_.shape[0] // img_tile):
            for bx in range(bits_.shape[1] // img_tile):
                raw = packed[by * img_tile:(by + 1) * img_tile, bx * tb:(bx + 1) * tb].tobytes()
                chunks.append(zlib.compress(raw, 6) if compress else raw)
        entries = [(code, typ, len(values), struct.pack('<' + _TYPES[typ] * len(values), *values)) for code, typ, values in (
            (T_SUBFILE, 4, [5 if reduced else 4]), (T_WIDTH, 4, [mw]), (T_HEIGHT, 4, [mh]), (T_BITS, 3, [1]),
            (T_COMPRESSION, 3, [8 if compress else 1]), (T_PHOTOMETRIC, 3, [4]), (T_SPP, 3, [1]), (T_PLANAR, 3, [1]),
            (T_TILE_W, 4, [img_tile]), (T_TILE_H, 4, [img_tile]))]
        return entries, chunks

    def tile_streams(img, img_tile):
        if compressor is None:
            return _tile_chunks(img, img_tile, compress, predictor)
        streams = [bytes(c) for c in (compressor(img, img_tile) if predictor == 1 else compressor(img, img_tile, predictor=predictor))]
        expected = img.shape[0] * (-(-img.shape[1] // img_tile)) * (-(-img.shape[2] // img_tile))
        if len(streams) != expected:
            raise ValueError(f'the compressor returned {len(streams)} streams for {expected} tiles')
        return streams

    if descriptions is not None and len(descriptions) != nb:
        raise ValueError(f'{len(descriptions)} band descriptions for {nb} bands')

    def geo_entries(add):
        if transform.b != 0 or transform.d != 0:   # a rotated / sheared grid: the full matrix instead of pixel scale + tie point
            add(T_TRANSFORMATION, 12, [float(transform.a), float(transform.b), 0., float(transform.c),
                                       float(transform.d), float(transform.e), 0., float(transform.f),
                                       0., 0., 0., 0., 0., 0., 0., 1.])
        else:
            add(T_PIXEL_SCALE, 12, [float(transform.a), float(-transform.e), 0.])
            add(T_TIEPOINT, 12, [0., 0., 0., float(transform.c), float(transform.f), 0.])
        name = crs.to_string() if crs is not None else ''
        m = re.fullmatch(r'EPSG:(\d+)', name or '')
        if m:
            geographic = int(m.group(1)) in (4326, 4269, 4258)
            add(T_GEOKEYS, 3, [1, 1, 0, 3, 1024, 0, 1, 2 if geographic else 1, 1025, 0, 1, 1,
                               2048 if geographic else 3072, 0, 1, int(m.group(1))])
        elif name:
            add(T_GEOKEYS, 3, [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 1026, T_GEOASCII, len(name) + 1, 0])
            add(T_GEOASCII, 2, name + '|')
        if metadata or (descriptions and any(d is not None for d in descriptions)):
            items = ''.join(f'  <Item name="{escape(str(k), {chr(34): "&quot;"})}">{escape(str(v))}</Item>\n' for k, v in (metadata or {}).items())
            items += ''.join(f'  <Item name="DESCRIPTION" sample="{i}" role="description">{escape(str(d))}</Item>\n'
                             for i, d in enumerate(descriptions or ()) if d is not None)
            add(T_GDAL_METADATA, 2, f'<GDALMetadata>\n{items}</GDALMetadata>\n')

    # every tile of every image is compressed first: then all sizes are known, the layout (classic or BigTIFF) is decided before a
    # byte is written, and a raster past 4 GiB is never lost after the work is done.  The images lie one behind the other, each
    # directory in front of its own data: the main image lies where it does without overviews.
    images = [(image_entries(a, tile, False), tile_streams(a, tile))]
    if mask is not None:
        images.append(mask_image(mask, tile, False))
    images += [(image_entries(lv, OVERVIEW_TILE, True), tile_streams(lv, OVERVIEW_TILE)) for lv in levels]
    images += [mask_image(m, OVERVIEW_TILE, True) for m in level_masks]
    classic_end = 8
    for entries, chunks in images:
        classic_end = _layout(entries, chunks, classic_end, False)[3]
    big = bigtiff_wanted(bigtiff, a.size * a.dtype.itemsize, compress, classic_end)
    with open(path, 'wb') as f:
        f.write(b'II' + (struct.pack('<HHHQ', 43, 8, 0, 16) if big else struct.pack('<HI', 42, 8)))
        pos = 16 if big else 8
        for k, (entries, chunks) in enumerate(images):
            blob, pos = _directory(entries, chunks, pos, k + 1 < len(images), big)
            f.write(blob)
