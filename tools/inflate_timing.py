#!/usr/bin/env python3
""" Timing of the device INFLATE path (hk_inflate.hip) beside zlib on the host, the default of ``tiff.read_tiff``.

The two rasters of tools/deflate_timing.py: ``--size``^2 float32 in 4 bands (uniform values inside a NaN frame) and ``--size``^2
uint8 in 3 bands (a real-imagery fixture tiled up).  Each is written twice at ``--tile``-pixel tiles: with host zlib level 6 (what
this package and GDAL write by default) and with the device compressor (``Context.deflate_tiles``).  Per file:
  * wall time of ``read_tiff`` on the host path (``inflater=None``; median of ``--reps``) and on the device path
    (``inflater=Context.inflate_image``; one warm-up, then the median of ``--reps``), both from the file's name to the array;
  * the two kernels alone on device-resident streams (``hk_inflate_image_dev`` between two events; warm-ups, median of >= 10),
    as decoded GB/s;
  * whether the two arrays are equal.
``--predictor`` 2 or 3 writes the files with that TIFF predictor (tag 317): the rasters whose samples it applies to -- for 3 the
float32 one and a 3-band float32 parameter raster (``param_raster``) -- and the host path then is zlib + the predictor in numpy.
The kernels of the predictor-1 twin of the same raster are timed in the same run, so that a ``rocprofv3 --kernel-trace --stats``
run of this script (a run of its own) shows the second stage with and without the predictor side by side.
The host time of the same file on the same box is what the device time is compared with.  The report goes to stdout and to
``--out``. """
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homonim_amd import _hk  # noqa: E402
from homonim_amd.geo import CRS  # noqa: E402
from homonim_amd.tiff import read_tiff, write_tiff  # noqa: E402
from tools.deflate_timing import TF, rasters  # noqa: E402


def param_raster(size):
    """ a parameter image as the product writes it: gains, offsets and r2 of one band, float32, NaN where nothing was fitted """
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    gain = 1.0 + 0.2 * np.sin(x / 97.0) * np.cos(y / 131.0) + rng.normal(0, 0.01, (size, size))
    offset = 5.0 + 3.0 * np.cos(x / 211.0) + rng.normal(0, 0.05, (size, size))
    r2 = np.clip(0.8 + rng.normal(0, 0.1, (size, size)), 0, 1)
    p = np.stack([gain, offset, r2]).astype(np.float32)
    frame = max(1, size // 32)
    p[:, :frame] = p[:, -frame:] = np.nan
    p[:, :, :frame] = p[:, :, -frame:] = np.nan
    return 'float32 3 bands, parameter raster', p, float('nan')


def rasters_for(size, predictor):
    """ the rasters of tools/deflate_timing.py that ``predictor`` applies to; with 3 the parameter raster too """
    for name, arr, nodata in rasters(size):
        if predictor == 1 or (predictor == 3) == (arr.dtype.kind == 'f'):
            yield name, arr, nodata
    if predictor == 3:
        yield param_raster(size)


def file_blocks(path):
    """ (streams, layout) of a file, as read_tiff hands them to its hook """
    seen = []

    def grab(streams, layout):
        seen.append((streams, layout))
        raise StopIteration

    grab.predictors = _hk.PREDICTORS   # (asked for predictor-3 files too)
    try:
        read_tiff(path, inflater=grab)
    except StopIteration:
        pass
    return seen[0]


def kernels_ms(ctx, streams, lay, reps):
    sizes = np.array([len(s) for s in streams], np.int64)
    padded = (sizes + 15) // 16 * 16
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    buf = np.zeros(int(padded.sum()), np.uint8)
    for o, s in zip(offsets.tolist(), streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    n_blocks, _, work_bytes = _hk.inflate_bound(lay)
    out_bytes = lay.spp * lay.height * lay.width * lay.sample_bytes
    ptrs = [ctx.dev_alloc(n) for n in (buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, out_bytes, 4 * n_blocks)]
    d_buf, d_off, d_siz, d_work, d_out, d_st = ptrs
    try:
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)

        def launch():
            ctx.inflate_image_dev(lay, d_buf, d_off, d_siz, d_work, d_out, lay.width, lay.height * lay.width, d_st, stream=0)

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
        status = np.empty(n_blocks, np.int32)
        ctx.d2h(status, d_st)
        return ms, int(buf.nbytes), not status.any()
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--tile', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3, help='timed read_tiff calls per path')
    ap.add_argument('--kernel-reps', type=int, default=10)
    ap.add_argument('--predictor', type=int, default=1, choices=(1, 2, 3), help='TIFF predictor of the files (2: the integer rasters, 3: the float ones)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hk.default_context()
    k_reps = max(10, a.kernel_reps)
    lines = [f'# tools/inflate_timing.py --size {a.size} --tile {a.tile} --predictor {a.predictor}: read_tiff with host zlib against Context.inflate_image',
             f'# host path: median of {a.reps}; device path: one warm-up, median of {a.reps}; kernels: two warm-ups, median of {k_reps} event pairs']
    with tempfile.TemporaryDirectory() as tmp:
        for name, arr, nodata in rasters_for(a.size, a.predictor):
            lines.append(f'{name}: {arr.shape}, {arr.nbytes / 1e6:.1f} MB raw')
            if a.predictor != 1:   # the predictor-1 twin's kernels: the same raster through the second stage without a predictor
                twin = os.path.join(tmp, 'twin.tif')
                write_tiff(twin, arr, TF, CRS('EPSG:32735'), nodata=nodata, tile=a.tile, compressor=ctx.deflate_tiles)
                ms, _, all_ok = kernels_ms(ctx, *file_blocks(twin), k_reps)
                lines.append(f'  predictor-1 twin (the device compressor): kernels alone  median {np.median(ms):8.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}'
                             f'   ({arr.nbytes / 1e6 / np.median(ms):7.2f} GB/s decoded; every status 0: {all_ok})')
            for written, compressor in (('host zlib level 6', None), ('the device compressor', ctx.deflate_tiles)):
                path = os.path.join(tmp, 'f.tif')
                write_tiff(path, arr, TF, CRS('EPSG:32735'), nodata=nodata, tile=a.tile, compressor=compressor, predictor=a.predictor)
                host_s, dev_s = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    host = read_tiff(path).array
                    host_s.append(time.perf_counter() - t0)
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    dev = read_tiff(path, inflater=ctx.inflate_image).array
                    dev_s.append(time.perf_counter() - t0)
                same = host.dtype == dev.dtype and host.tobytes() == dev.tobytes() == arr.tobytes()
                host_med, dev_med = float(np.median(host_s)), float(np.median(dev_s[1:]))
                streams, lay = file_blocks(path)
                ms, stream_bytes, all_ok = kernels_ms(ctx, streams, lay, k_reps)
                lines += [
                    f'  written with {written}: file {os.path.getsize(path)} bytes, {len(streams)} tiles',
                    f'    read_tiff host zlib            {host_med:8.2f} s   ({arr.nbytes / 1e6 / host_med:7.1f} MB/s)   runs {" ".join(f"{s:.2f}" for s in host_s)}',
                    f'    read_tiff device INFLATE       {dev_med:8.2f} s   ({arr.nbytes / 1e6 / dev_med:7.1f} MB/s)   runs {" ".join(f"{s:.2f}" for s in dev_s[1:])};'
                    f' first (cold) {dev_s[0]:.2f}; equal to the host path and to the raster: {same}',
                    f'    host / device = {host_med / dev_med:.2f}',
                    f'    kernels alone (device-resident)  median {np.median(ms):8.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}'
                    f'   ({arr.nbytes / 1e6 / np.median(ms):7.2f} GB/s decoded; every status 0: {all_ok})',
                    f'    PCIe: {stream_bytes} bytes of streams to the device, {arr.nbytes} back',
                ]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
