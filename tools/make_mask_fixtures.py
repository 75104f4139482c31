#!/usr/bin/env python
""" Writes the masked GeoTIFFs of tests/golden/tiff/mask/ (tests/test_dataset_mask_cpu.py, tests/test_gpu_dataset_mask.py):

    python tools/make_mask_fixtures.py

  rgba_u8.tif, la_u8.tif         Pillow's own RGBA / LA files (ExtraSamples = 2, no nodata tag, no geo tags): the alpha band masks
  rgba_u16.tif                   write_tiff + tag 338 patched: a uint16 alpha band masks
  rgb_mask_tiles_deflate.tif     3 bands + an internal 1-bit mask in 16 x 16 DEFLATE tiles, AND a nodata tag the mask overrules
  rgb_mask_strips_lzw.tif        the same pixels, the mask in LZW strips of 8 rows
  rgba_u8_nodata.tif             an alpha band AND a nodata tag: the tag stands, the alpha band only leaves the band list
  five_band_alpha.tif            five bands, the last one alpha: dropped, not applied
  alpha_not_last.tif             four bands, band 1 alpha: dropped, not applied
  rgba_f32.tif                   a float32 alpha band: dropped, not applied

All are 64 x 80 (tests/_masked_tiffs.py: FIXTURE_SHAPE, fixture_pixels, fixture_valid).  The files are a function of this script,
numpy's generator and zlib; the tests read what the files hold, not what this script meant to write. """
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import _masked_tiffs as mt   # noqa: E402
from homonim_amd.geo import Affine, CRS   # noqa: E402
from homonim_amd.tiff import write_tiff   # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'tiff', 'mask')
TRANSFORM, EPSG = Affine(1., 0., 500000., 0., -1., 6200080.), CRS('EPSG:32735')


def alpha_of(valid, dtype):
    """ an alpha band of the footprint: opaque, but for a stripe of valid pixels at 1 and at half (valid is `!= 0`, not `== max`) """
    top = np.iinfo(dtype).max
    a = np.where(valid, top, 0).astype(dtype)
    a[20:24][valid[20:24]] = 1
    a[50:52][valid[50:52]] = top // 2
    return a


def written(name, array, **kw):
    path = os.path.join(OUT, name)
    write_tiff(path, array, TRANSFORM, EPSG, tile=16, **kw)
    with open(path, 'rb') as f:
        return path, f.read()


def main():
    from PIL import Image, features
    os.makedirs(OUT, exist_ok=True)
    valid = mt.fixture_valid()
    rgb = mt.fixture_pixels(3, 'uint8')
    compression = 'tiff_adobe_deflate' if features.check('libtiff') else None
    rgba = np.concatenate([rgb, alpha_of(valid, np.uint8)[None]])
    Image.fromarray(np.ascontiguousarray(np.moveaxis(rgba, 0, 2)), 'RGBA').save(os.path.join(OUT, 'rgba_u8.tif'), compression=compression)
    Image.fromarray(np.ascontiguousarray(np.moveaxis(rgba[[0, 3]], 0, 2)), 'LA').save(os.path.join(OUT, 'la_u8.tif'), compression=compression)

    def patched(name, array, extra, **kw):
        path, data = written(name, array, **kw)
        with open(path, 'wb') as f:
            f.write(mt.set_extra_samples(data, extra))

    rgb16 = mt.fixture_pixels(3, 'uint16')
    patched('rgba_u16.tif', np.concatenate([rgb16, alpha_of(valid, np.uint16)[None]]), {3: 2})
    patched('rgba_u8_nodata.tif', rgba, {3: 2}, nodata=0)
    patched('five_band_alpha.tif', np.concatenate([mt.fixture_pixels(4, 'uint8'), alpha_of(valid, np.uint8)[None]]), {4: 2})
    patched('alpha_not_last.tif', rgba[[0, 3, 1, 2]], {1: 1})
    patched('rgba_f32.tif', rgba.astype(np.float32), {3: 2})
    for name, kw in (('rgb_mask_tiles_deflate.tif', dict(tile=16, compression=mt.DEFLATE)),
                     ('rgb_mask_strips_lzw.tif', dict(rows_per_strip=8, compression=mt.LZW))):
        path, data = written(name, rgb, nodata=0)
        with open(path, 'wb') as f:
            f.write(mt.append_mask(data, valid, **kw))
    for name in sorted(os.listdir(OUT)):
        print(f'{os.path.getsize(os.path.join(OUT, name)):7d}  {name}')


if __name__ == '__main__':
    main()
