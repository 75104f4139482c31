#!/usr/bin/env python3
""" Timing of the per-dataset mask (hk_dataset_mask.hip) on an MI355X.

  * device-resident: ``dataset_mask_kernel<uint8, BITS>`` and ``<uint8, ALPHA>`` on 3 x ``--size``^2 uint8 between two events
    (two warm-ups, ``--reps`` launches each, the two kinds and the yardstick alternating), beside the yardstick
    ``cast_in_kernel<uint8>`` on the same raster in the same process (hk_debug_cast_plane_dev on the three planes as one plane of
    3 x size rows; that entry synchronises the stream before the closing event is recorded, so its time carries one host round
    trip the others do not).  The bytes each moves, the rate, and the ratio to the yardstick beside the ratio of the byte counts:
    (3 + 1/8 + 12) / (3 + 12) for BITS, (4 + 12) / (3 + 12) for ALPHA.
  * end to end: ``read_tiff`` + ``fuse.dataset_masked`` of an RGBA uint8 file of ``--file-size``^2 written here (host zlib), wall
    clock, one warm-up and the median of ``--file-reps``.
The report goes to stdout and to ``--out``. """
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homonim_amd import _hk  # noqa: E402
from homonim_amd.fuse import dataset_masked  # noqa: E402
from homonim_amd.tiff import read_tiff  # noqa: E402


def timed(ctx, launch, reps):
    e0, e1 = ctx.event(), ctx.event()
    ctx.event_record(e0, 0)
    for _ in range(reps):
        launch()
    ctx.event_record(e1, 0)
    ctx.stream_sync(0)
    ms = ctx.event_elapsed_ms(e0, e1) / reps
    ctx.event_destroy(e0), ctx.event_destroy(e1)
    return ms


def device_resident(ctx, size, reps, rounds):
    nb = 3
    rng = np.random.default_rng(0)
    d_src, d_bits, d_alpha, d_out = (ctx.dev_alloc(n) for n in (nb * size * size, size * (size // 8), size * size, 4 * nb * size * size))
    try:
        row = rng.integers(0, 256, (1, size), dtype=np.uint8)
        plane = np.ascontiguousarray(np.bitwise_xor(row, np.arange(size, dtype=np.uint8)[:, None]))
        for b in range(nb):
            ctx.h2d(d_src + b * size * size, plane)
        ctx.h2d(d_alpha, np.where(plane > 40, plane, 0).astype(np.uint8))
        ctx.h2d(d_bits, np.packbits(plane > 40, axis=1))
        kinds = {
            'dataset_mask_kernel<uint8, BITS>': lambda: ctx.dataset_mask_dev(d_src, 'uint8', nb, size, size, size, size * size, d_bits, _hk.MASK_BITS,
                                                                           size // 8, d_out, size, size * size),
            'dataset_mask_kernel<uint8, ALPHA>': lambda: ctx.dataset_mask_dev(d_src, 'uint8', nb, size, size, size, size * size, d_alpha,
                                                                            _hk.MASK_ALPHA, size, d_out, size, size * size),
            'cast_in_kernel<uint8> (yardstick)': lambda: ctx.cast_plane_dev(False, 'uint8', d_src, size, d_out, size, nb * size, size),
        }
        px = nb * size * size
        moved = {'dataset_mask_kernel<uint8, BITS>': px * 5 + size * size // 8, 'dataset_mask_kernel<uint8, ALPHA>': px * 5 + size * size,
                 'cast_in_kernel<uint8> (yardstick)': px * 5}
        ms = {k: [] for k in kinds}
        for k, launch in kinds.items():   # warm-up
            launch(), launch()
        ctx.stream_sync(0)
        for _ in range(rounds):   # alternating
            for k, launch in kinds.items():
                ms[k].append(timed(ctx, launch, 1 if 'cast' in k else reps))
        return ms, moved
    finally:
        for p in (d_src, d_bits, d_alpha, d_out):
            ctx.dev_free(p)


def end_to_end(ctx, size, reps):
    from PIL import Image
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:size, 0:size]
    rgba = np.empty((size, size, 4), np.uint8)
    for b in range(3):
        rgba[:, :, b] = (x // 7 + y // 5 + 40 * b) % 251 + rng.integers(0, 3, (size, size))
    rgba[:, :, 3] = np.where((x - size / 2) ** 2 + (y - size / 2) ** 2 < (0.48 * size) ** 2, 255, 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rgba.tif')
        Image.fromarray(rgba, 'RGBA').save(path, compression='tiff_adobe_deflate')
        times = {'read_tiff': [], 'mask': []}
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            tif = read_tiff(path)
            t1 = time.perf_counter()
            array, nodata, _ = dataset_masked(tif)
            t2 = time.perf_counter()
            times['read_tiff'].append(t1 - t0), times['mask'].append(t2 - t1)
        valid = rgba[:, :, 3] != 0
        same = np.array_equal(np.isnan(array[0]), ~valid) and np.array_equal(array[1][valid], rgba[:, :, 1][valid].astype(np.float32))
        return os.path.getsize(path), {k: v[1:] for k, v in times.items()}, same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=16384, help='a multiple of 8')
    ap.add_argument('--reps', type=int, default=10, help='launches between two events')
    ap.add_argument('--rounds', type=int, default=7, help='event pairs per kernel')
    ap.add_argument('--file-size', type=int, default=4096)
    ap.add_argument('--file-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = _hk.default_context()
    lines = [f'# tools/dataset_mask_timing.py --size {a.size} --reps {a.reps} --rounds {a.rounds} --file-size {a.file_size} --file-reps {a.file_reps}',
             f'# device-resident, 3 x {a.size} x {a.size} uint8 -> float32: two warm-ups, then {a.rounds} rounds alternating the three; a round is '
             f'{a.reps} launches between two events (the yardstick: 1, its entry synchronises)']
    ms, moved = device_resident(ctx, a.size, a.reps, a.rounds)
    yard = float(np.median(ms['cast_in_kernel<uint8> (yardstick)']))
    expect = {'dataset_mask_kernel<uint8, BITS>': (3 + 1 / 8 + 12) / 15, 'dataset_mask_kernel<uint8, ALPHA>': (4 + 12) / 15}
    for k, v in ms.items():
        med = float(np.median(v))
        line = f'  {k:36s} median {med:7.3f} ms  min {min(v):7.3f}  max {max(v):7.3f}   {moved[k] / 1e9:6.3f} GB moved, {moved[k] / 1e6 / med:7.1f} GB/s'
        if k in expect:
            line += f'   / yardstick = {med / yard:.3f} (byte counts: {expect[k]:.3f})'
        lines.append(line)
    size, times, same = end_to_end(ctx, a.file_size, a.file_reps)
    rd, mk = float(np.median(times['read_tiff'])), float(np.median(times['mask']))
    lines += [f'# end to end, RGBA uint8 {a.file_size} x {a.file_size} (Pillow, DEFLATE strips, {size} bytes): one warm-up, median of {a.file_reps}; wall clock',
              f'  read_tiff (host zlib)            {rd:7.3f} s   runs {" ".join(f"{t:.3f}" for t in times["read_tiff"])}',
              f'  dataset_masked (host entry)      {mk:7.3f} s   runs {" ".join(f"{t:.3f}" for t in times["mask"])}   '
              f'({3 * a.file_size ** 2 * 5 / 1e6 / mk:7.1f} MB/s over PCIe both ways); the statement holds: {same}']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
