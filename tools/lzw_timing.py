#!/usr/bin/env python3
""" Timing of the two LZW decoders of the library (hk_lzw.hip on the device, its host build hk_lzw_image_host) beside host zlib
on the DEFLATE twin of the same raster.

The two rasters of tools/deflate_timing.py: ``--size``^2 float32 in 4 bands (uniform values inside a NaN frame) and ``--size``^2
uint8 in 3 bands (a real-imagery fixture tiled up), written at ``--tile``-pixel tiles with host zlib level 6, and the same file
with every tile re-coded as LZW by the test encoder (tests/_lzw_streams.py: Clear at entry 4094 like libtiff; in a process pool,
it is plain Python).  Per raster:
  * wall time of ``read_tiff`` from the file's name to the array: the LZW file through ``Context.lzw_image`` (one warm-up, then
    the median of ``--reps``) and through ``_hk.lzw_image_host`` (median of ``--reps``), the DEFLATE twin through host zlib
    (``inflater=None``; median of ``--reps``);
  * the kernels alone on device-resident streams (``hk_lzw_image_dev`` between two events; warm-ups, median of >= 10), as decoded
    GB/s -- per-kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of this script, a run of its own;
  * whether all arrays are equal.
``--predictor`` 2 or 3 writes both files with that TIFF predictor (tag 317; the re-coding keeps it): the rasters whose samples it
applies to, as in tools/inflate_timing.py.  ``--python-crop N``: the plain-Python reader (``tiff.lzw_decode``, what reads an LZW
file where no hook takes it) is timed once on the LZW file of the N x N pixels in the middle of the first band.
The report goes to stdout and to ``--out``. """
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import _lzw_streams as st  # noqa: E402
from homonim_amd import _hk  # noqa: E402
from homonim_amd.geo import CRS  # noqa: E402
from homonim_amd.tiff import read_tiff, write_tiff  # noqa: E402
from tools.deflate_timing import TF  # noqa: E402
from tools.inflate_timing import rasters_for  # noqa: E402


def file_blocks(path):
    """ (streams, layout) of an LZW file, as read_tiff hands them to its hook """
    seen = []

    def grab(streams, layout):
        seen.append((streams, layout))
        raise StopIteration

    grab.predictors = _hk.PREDICTORS   # (asked for predictor-3 files too)
    try:
        read_tiff(path, lzw=grab)
    except StopIteration:
        pass
    return seen[0]


def kernels_ms(ctx, streams, lay, reps):
    buf, offsets, sizes = _hk._pack_streams(streams)
    n_blocks, _, work_bytes = _hk.inflate_bound(lay)
    out_bytes = lay.spp * lay.height * lay.width * lay.sample_bytes
    ptrs = [ctx.dev_alloc(n) for n in (buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, out_bytes, 4 * n_blocks)]
    d_buf, d_off, d_siz, d_work, d_out, d_st = ptrs
    try:
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)

        def launch():
            ctx.lzw_image_dev(lay, d_buf, d_off, d_siz, d_work, d_out, lay.width, lay.height * lay.width, d_st, stream=0)

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


def middle(arr, n):
    """ the n x n pixels in the middle of the first band """
    y0, x0 = (arr.shape[1] - n) // 2, (arr.shape[2] - n) // 2
    return np.ascontiguousarray(arr[:1, y0:y0 + n, x0:x0 + n])


def timed(f, reps):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        runs.append(time.perf_counter() - t0)
    return out, runs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--tile', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3, help='timed read_tiff calls per path')
    ap.add_argument('--kernel-reps', type=int, default=10)
    ap.add_argument('--workers', type=int, default=16, help='processes of the test encoder')
    ap.add_argument('--predictor', type=int, default=1, choices=(1, 2, 3), help='TIFF predictor of the files (2: the integer rasters, 3: the float ones)')
    ap.add_argument('--python-crop', type=int, default=0, help='time the plain-Python reader on a crop of this many pixels a side (0: not)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    k_reps = max(10, a.kernel_reps)
    lines = [f'# tools/lzw_timing.py --size {a.size} --tile {a.tile} --predictor {a.predictor}: read_tiff of an LZW file through Context.lzw_image and through '
             '_hk.lzw_image_host, and of its DEFLATE twin through host zlib',
             f'# host paths: median of {a.reps}; device path: one warm-up, median of {a.reps}; kernels: two warm-ups, median of {k_reps} event pairs']
    with tempfile.TemporaryDirectory() as tmp, ProcessPoolExecutor(a.workers) as pool:
        # (the files first: the encoder's processes are forked before this one opens the device)
        made = []
        for k, (name, arr, nodata) in enumerate(rasters_for(a.size, a.predictor)):
            deflate, lzw = os.path.join(tmp, f'{k}_deflate.tif'), os.path.join(tmp, f'{k}_lzw.tif')
            write_tiff(deflate, arr, TF, CRS('EPSG:32735'), nodata=nodata, tile=a.tile, bigtiff='no', predictor=a.predictor)
            t0 = time.perf_counter()
            with open(deflate, 'rb') as f, open(lzw, 'wb') as g:
                g.write(st.lzw_copy(f.read(), mapper=lambda fn, items: pool.map(fn, items, chunksize=1)))
            crop = None
            if a.python_crop:
                crop = os.path.join(tmp, f'{k}_crop_lzw.tif')
                write_tiff(crop, middle(arr, a.python_crop), TF, CRS('EPSG:32735'), nodata=nodata, tile=min(a.tile, 256),
                           bigtiff='no', predictor=a.predictor)
                with open(crop, 'rb') as f:
                    data = st.lzw_copy(f.read(), mapper=lambda fn, items: pool.map(fn, items, chunksize=1))
                with open(crop, 'wb') as g:
                    g.write(data)
            made.append((name, arr, deflate, lzw, time.perf_counter() - t0, crop))
        ctx = _hk.default_context()
        for name, arr, deflate, lzw, enc_s, crop in made:
            zlib_out, zlib_s = timed(lambda: read_tiff(deflate).array, a.reps)
            host_out, host_s = timed(lambda: read_tiff(lzw, lzw=_hk.lzw_image_host).array, a.reps)
            dev_out, dev_s = timed(lambda: read_tiff(lzw, lzw=ctx.lzw_image).array, a.reps + 1)
            same = zlib_out.tobytes() == host_out.tobytes() == dev_out.tobytes() == arr.tobytes()
            z, h, d = float(np.median(zlib_s)), float(np.median(host_s)), float(np.median(dev_s[1:]))
            streams, lay = file_blocks(lzw)
            ms, stream_bytes, all_ok = kernels_ms(ctx, streams, lay, k_reps)
            mb = arr.nbytes / 1e6
            lines += [
                f'{name}: {arr.shape}, {mb:.1f} MB raw; DEFLATE file {os.path.getsize(deflate)} bytes, LZW streams {stream_bytes} bytes in '
                f'{len(streams)} tiles (encoded in {enc_s:.0f} s by {a.workers} processes)',
                f'    read_tiff LZW, device (Context.lzw_image)      {d:8.2f} s   ({mb / d:7.1f} MB/s)   runs {" ".join(f"{s:.2f}" for s in dev_s[1:])}; first (cold) {dev_s[0]:.2f}',
                f'    read_tiff LZW, host (_hk.lzw_image_host)       {h:8.2f} s   ({mb / h:7.1f} MB/s)   runs {" ".join(f"{s:.2f}" for s in host_s)}',
                f'    read_tiff DEFLATE twin, host zlib              {z:8.2f} s   ({mb / z:7.1f} MB/s)   runs {" ".join(f"{s:.2f}" for s in zlib_s)}',
                f'    LZW host / LZW device = {h / d:.2f}; host zlib / LZW device = {z / d:.2f}; host zlib / LZW host = {z / h:.2f}; all four arrays equal: {same}',
                f'    kernels alone (device-resident)  median {np.median(ms):8.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}'
                f'   ({mb / np.median(ms):7.2f} GB/s decoded; every status 0: {all_ok})',
            ]
            if crop:
                part = middle(arr, a.python_crop)
                py_out, py_s = timed(lambda: read_tiff(crop).array, 1)
                lines.append(f'    read_tiff LZW, plain Python (tiff.lzw_decode) on the crop {part.shape}, {part.nbytes / 1e6:.1f} MB raw: {py_s[0]:8.2f} s'
                             f'   ({part.nbytes / 1e6 / py_s[0]:7.2f} MB/s)   equal to the crop: {py_out.tobytes() == part.tobytes()}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
