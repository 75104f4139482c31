""" The LZW fixtures of tests/golden/tiff/lzw: six small files written by Pillow's libtiff -- an LZW writer this project has no part in --
and ``lzw_decoded.npz``, the pixels as Pillow itself reads each file back (which must be what was written), as (bands, height,
width) arrays under the files' stems.

    python tools/make_lzw_fixtures.py            # needs Pillow built with libtiff; run by hand, never imported by a test

Per file it prints the strips, the bytes and what the streams hold -- Clears, KwKwK codes, the widest code, the longest string --
counted by the tracer of tests/_lzw_streams.py, and it stops if a rebuilt file no longer shows what its row in the table below
says: change the sizes then.  The seeds are fixed; the bytes may still differ between libtiff versions, the pixels may not. """
import os
import struct
import sys

import numpy as np
from PIL import Image, TiffImagePlugin, features

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'tiff', 'lzw')   # (a folder of their own: other tests take every *.tif of tests/golden/tiff)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from _lzw_streams import trace   # noqa: E402


def arrays():
    rng = np.random.default_rng(20261019)
    y, x = np.mgrid[0:130, 0:259]
    smooth = ((np.sin(x / 23.0) + np.cos(y / 17.0)) * 20 + 128).astype(np.uint8)
    y, x = np.mgrid[0:90, 0:131]
    rgb = np.stack([(x + y) // 2 + rng.integers(0, 3, x.shape), 255 - x + rng.integers(0, 3, x.shape), y * 2 + rng.integers(0, 3, x.shape)],
                   axis=2).astype(np.uint8)
    y, x = np.mgrid[0:77, 0:140]
    u16 = (1000 + 37 * x + 11 * y + rng.integers(0, 4, x.shape)).astype(np.uint16)
    y, x = np.mgrid[0:60, 0:90]
    f32 = (np.hypot(x - 40.0, y - 30.0) // 4 * 0.25).astype(np.float32)
    # name -> (pixels, predicted, what the file has to show: a test on its trace records)
    return {
        'lzw_u8_noise_strips': (rng.integers(0, 256, (67, 301), dtype=np.uint8), False,
                                lambda r: max(t['max_width'] for t in r) == 12 and min(t['clears'] for t in r[:-1]) >= 2),
        'lzw_u8_smooth_strips': (smooth, False, lambda r: sum(t['kwkwk'] for t in r) >= 20 and sum(t['codes'] for t in r) > 20 * sum(t['kwkwk'] for t in r)),
        'lzw_u8_flat_strips': (np.full((200, 300), 77, np.uint8), False,
                               lambda r: max(t['max_len'] for t in r) > 64 and all(t['kwkwk'] * 10 >= (t['codes'] - 3) * 9 for t in r)),
        'lzw_rgb_pred2_strips': (rgb, True, lambda r: True),
        'lzw_u16_pred2_strips': (u16, True, lambda r: True),
        'lzw_f32_strips': (f32, False, lambda r: True),
    }


def strips(path):
    """ [(stream, raw size)] of a classic little-endian strip file, read with struct alone """
    buf = open(path, 'rb').read()
    assert buf[:4] == b'II*\0'
    (ifd,) = struct.unpack_from('<I', buf, 4)
    (n,) = struct.unpack_from('<H', buf, ifd)
    tags = {}
    for i in range(n):
        tag, typ, cnt = struct.unpack_from('<HHI', buf, ifd + 2 + 12 * i)
        size = {1: 1, 3: 2, 4: 4}.get(typ)
        if size is None:
            continue
        at = ifd + 2 + 12 * i + 8
        if size * cnt > 4:
            (at,) = struct.unpack_from('<I', buf, at)
        tags[tag] = struct.unpack_from('<' + {1: 'B', 3: 'H', 4: 'I'}[typ] * cnt, buf, at)
    assert tags[259] == (5,)
    h, w, rps, spp = tags[257][0], tags[256][0], tags[278][0], tags.get(277, (1,))[0]
    row = w * spp * tags[258][0] // 8
    return [(buf[o:o + c], min(rps, h - k * rps) * row) for k, (o, c) in enumerate(zip(tags[273], tags[279]))], tags.get(317, (1,))[0]


def main():
    if not features.check('libtiff'):
        sys.exit('Pillow has no libtiff: the fixtures cannot be written')
    TiffImagePlugin.STRIP_SIZE = 8192
    os.makedirs(OUT, exist_ok=True)
    decoded = {}
    for name, (a, predicted, shows) in arrays().items():
        path = os.path.join(OUT, name + '.tif')
        Image.fromarray(a).save(path, compression='tiff_lzw', **({'tiffinfo': {317: 2}} if predicted else {}))
        back = np.array(Image.open(path))
        assert back.dtype == a.dtype and np.array_equal(back, a), f'{name}: Pillow does not read back what it wrote'
        decoded[name] = np.ascontiguousarray(back[None] if back.ndim == 2 else np.moveaxis(back, 2, 0))
        blocks, predictor = strips(path)
        assert predictor == (2 if predicted else 1), name
        recs = [trace(s, raw) for s, raw in blocks]
        size = os.path.getsize(path)
        print(f'{name}: {a.shape} {a.dtype}, predictor {predictor}, {len(blocks)} strips, {size} bytes; clears {sum(r["clears"] for r in recs)}, '
              f'KwKwK {sum(r["kwkwk"] for r in recs)} of {sum(r["codes"] for r in recs)} codes, widest code {max(r["max_width"] for r in recs)} bits, '
              f'longest string {max(r["max_len"] for r in recs)} bytes')
        assert size < 45 * 1024, f'{name}: {size} bytes'
        assert shows(recs), f'{name} no longer shows what it is there for: adjust its size'
    np.savez_compressed(os.path.join(OUT, 'lzw_decoded.npz'), **decoded)


if __name__ == '__main__':
    main()
