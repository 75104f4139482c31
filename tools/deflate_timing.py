#!/usr/bin/env python3
""" Timing and sizes of the device DEFLATE path (hk_deflate.hip) beside zlib level 6 on the host, the default of ``tiff.write_tiff``.

Two rasters: ``--size``^2 float32 in 4 bands (uniform values inside a NaN frame, like the benchmark's tiles) and ``--size``^2
uint8 in 3 bands (a real-imagery fixture of tests/golden/rasters tiled up).  Per raster:
  * wall time of ``write_tiff`` on the host path (``compressor=None``, once: it takes tens of seconds) and on the device path
    (``compressor=Context.deflate_tiles``; one warm-up, then the median of ``--reps``), both ending in a closed file;
  * the kernels alone on device-resident planes (``hk_deflate_tiles_dev`` between two events; warm-up, median of >= 10);
  * the bytes that cross PCIe each way on the device path;
  * the file sizes, and the device's streams as a fraction of level 6's.
``--predictor 2`` / ``3``: both paths write with that TIFF predictor (the host path predicts with numpy, the device path in
deflate_pred_chunk_kernel); a raster the predictor does not apply to (2: the floats, 3: the integers) is left out, and the kernels
are timed at predictor 1 as well, in the same process, for the cost of the predicted launch.
The report goes to stdout and to ``--out``. """
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homonim_amd import _hk  # noqa: E402
from homonim_amd.geo import Affine, CRS  # noqa: E402
from homonim_amd.tiff import read_tiff, write_tiff  # noqa: E402

TF = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 7000000.0)


def rasters(size):
    rng = np.random.default_rng(0)
    f = rng.uniform(0.05, 1.0, (4, size, size)).astype(np.float32)
    frame = max(1, size // 32)
    f[:, :frame] = f[:, -frame:] = np.nan
    f[:, :, :frame] = f[:, :, -frame:] = np.nan
    yield 'float32 4 bands, NaN frame', f, float('nan')
    fixture = read_tiff(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'rasters',
                                     'sentinel2_b432_byte.tif')).array
    reps = (1, -(-size // fixture.shape[1]), -(-size // fixture.shape[2]))
    yield 'uint8 3 bands, sentinel2 fixture tiled up', np.ascontiguousarray(np.tile(fixture, reps)[:, :size, :size]), 0


def kernels_ms(ctx, a, tile, reps, predictor=1):
    nb, h, w = a.shape
    n_tiles, cap = _hk.deflate_bound(a.dtype.name, nb, h, w, tile)
    d_src, d_out = ctx.dev_alloc(a.nbytes), ctx.dev_alloc(cap)
    d_off, d_siz = ctx.dev_alloc(8 * (n_tiles + 1)), ctx.dev_alloc(8 * n_tiles)
    try:
        ctx.h2d(d_src, a)

        def launch():
            ctx.deflate_tiles_dev(d_src, a.dtype.name, nb, h, w, w, h * w, tile, d_out, cap, d_off, d_siz, stream=0, predictor=predictor)

        for _ in range(2):
            launch()
        ctx.stream_sync(0)
        ev = [(ctx.event(), ctx.event()) for _ in range(reps)]
        for e0, e1 in ev:
            ctx.event_record(e0, 0)
            launch()
            ctx.event_record(e1, 0)
        ctx.stream_sync(0)
        ms = [ctx.event_elapsed_ms(e0, e1) for e0, e1 in ev]
        for e0, e1 in ev:
            ctx.event_destroy(e0), ctx.event_destroy(e1)
        offsets = np.empty(n_tiles + 1, np.int64)
        ctx.d2h(offsets, d_off)
        return ms, int(offsets[-1]), n_tiles
    finally:
        for p in (d_src, d_out, d_off, d_siz):
            ctx.dev_free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--tile', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3, help='timed write_tiff calls on the device path')
    ap.add_argument('--kernel-reps', type=int, default=10)
    ap.add_argument('--predictor', type=int, choices=(1, 2, 3), default=1, help='TIFF predictor of both paths (2: integer rasters, 3: float rasters)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hk.default_context()
    lines = [f'# tools/deflate_timing.py --size {a.size} --tile {a.tile} --predictor {a.predictor}: write_tiff with host zlib level 6 against Context.deflate_tiles',
             f'# device path: one warm-up, median of {a.reps}; kernels: two warm-ups, median of {max(10, a.kernel_reps)} event pairs']
    with tempfile.TemporaryDirectory() as tmp:
        for name, arr, nodata in rasters(a.size):
            if (a.predictor == 2 and arr.dtype.kind == 'f') or (a.predictor == 3 and arr.dtype.kind != 'f'):
                continue
            host_file, dev_file = os.path.join(tmp, 'host.tif'), os.path.join(tmp, 'dev.tif')
            t0 = time.perf_counter()
            write_tiff(host_file, arr, TF, CRS('EPSG:32735'), nodata=nodata, tile=a.tile, predictor=a.predictor)
            host_s = time.perf_counter() - t0
            dev_s = []
            for k in range(a.reps + 1):
                t0 = time.perf_counter()
                write_tiff(dev_file, arr, TF, CRS('EPSG:32735'), nodata=nodata, tile=a.tile, compressor=ctx.deflate_tiles,
                           predictor=a.predictor)
                dev_s.append(time.perf_counter() - t0)
            dev_med = float(np.median(dev_s[1:]))
            same = read_tiff(dev_file).array.tobytes() == arr.tobytes()
            ms, stream_bytes, n_tiles = kernels_ms(ctx, arr, a.tile, max(10, a.kernel_reps), a.predictor)
            host_size, dev_size = os.path.getsize(host_file), os.path.getsize(dev_file)
            lines += [
                f'{name}: {arr.shape}, {arr.nbytes / 1e6:.1f} MB raw, {n_tiles} tiles',
                f'  write_tiff host zlib level 6   {host_s:8.2f} s   ({arr.nbytes / 1e6 / host_s:7.1f} MB/s)   file {host_size} bytes',
                f'  write_tiff device DEFLATE      {dev_med:8.2f} s   ({arr.nbytes / 1e6 / dev_med:7.1f} MB/s)   file {dev_size} bytes'
                f'   runs {" ".join(f"{s:.2f}" for s in dev_s[1:])}; first (cold) {dev_s[0]:.2f}; reads back equal: {same}',
                f'  kernels alone (device-resident)  median {np.median(ms):8.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}'
                f'   ({arr.nbytes / 1e6 / np.median(ms):7.1f} GB/s of raw bytes)',
                f'  PCIe: {arr.nbytes} bytes to the device, {stream_bytes + 16 * n_tiles + 8} back ({stream_bytes} of streams, 16 per tile of offsets and sizes)',
                f'  size: device / level 6 = {dev_size / host_size:.4f}',
            ]
            if a.predictor != 1:
                ms1, bytes1, _ = kernels_ms(ctx, arr, a.tile, max(10, a.kernel_reps), 1)
                lines.append(f'  kernels alone at predictor 1       median {np.median(ms1):8.3f} ms, min {min(ms1):.3f}, max {max(ms1):.3f}'
                             f'   ({bytes1} bytes of streams; predictor {a.predictor}: {stream_bytes}); predicted / predictor 1 = '
                             f'{np.median(ms) / np.median(ms1):.3f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
