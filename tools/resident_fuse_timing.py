""" Times ``RasterFuse.process`` across two grids with the rasters on the host (the default route) and resident on the device
(``device_config`` ``resident=True``) and writes the result to profiles/resident_fuse.txt.  Recorded, not gated: the yardstick is
the default route on the same box, whose code the resident mode does not touch.

Case: 4 bands, a uint8 source of 8190 x 8190 against a float32 reference at 2.5:1 (3276 x 3276), gain-blk-offset 5 x 5, float32
output, the default ``max_block_mem``, ``proc_crs`` ref and src, mask_partial off and on; ``process()`` to arrays (no file).

    python tools/resident_fuse_timing.py [--out profiles/resident_fuse.txt] [--reps 5] [--size 8190] [--stats-dir DIR]

In one process, per configuration and route: one warm-up call, then the median and the best wall time of `reps` calls.  The
resident time is split into upload (planning, allocation, source and reference up, the prefills), loop, overviews (none here: no
``.tif`` is written) and download (``ResidentRun.timings``).

The kernel summary of one resident call comes from a run of its own under the profiler, the program after `--`:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/resident_fuse_timing.py --trace ref:0

(`--trace PROC_CRS:MASK_PARTIAL` makes TRACE_CALLS resident calls and leaves the statistics to the profiler; the table assumes
ref:0, the first configuration.)  With --stats-dir the table of every kernel's time per ``process`` call is added.  The two kernels of
the resident mode are also timed alone on resident planes, between events: the bytes per second they achieve against the bytes of
the planes they read and write (from the shapes: every sample once).  One pass, no retries. """
import argparse
import csv
import glob
import json
import os
import sys
import time
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from homonim_amd import CRS, Model, RasterFuse, resident  # noqa: E402
from homonim_amd.geo import Affine  # noqa: E402

BANDS, RATIO = 4, 2.5
TRACE_CALLS = 2   # resident calls of a --trace run (the first one warms up; the profiler sees both)
CONFIGS = [(proc_crs, mask_partial) for proc_crs in ('ref', 'src') for mask_partial in (False, True)]


def make_pair(n):
    """ the rasters of tools/two_grid_timing.py: 10 .. 200 with a nodata frame and holes; the reference = 1.3 x the source + 5 + noise """
    r = int(np.ceil(n / RATIO))
    rng = np.random.default_rng(1)
    src, ref = np.empty((BANDS, n, n), np.uint8), np.empty((BANDS, r, r), np.float32)
    for b in range(BANDS):
        s = rng.integers(10, 201, (n, n), dtype=np.uint8)
        s[:3] = s[:, -4:] = 0
        s[rng.random((n, n)) < 0.002] = 0
        src[b] = s
        at = (np.arange(r) * RATIO).astype(np.int64)
        ref[b] = 1.3 * s[at][:, at].astype(np.float32) + 5. + rng.normal(0., 1., (r, r)).astype(np.float32)
        ref[b, 100:140, 200:260] = np.nan
    return src, ref


def make_fuse(src, ref, proc_crs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')   # proc_crs=src on a finer source is "not recommended"
        return RasterFuse(src, ref, src_nodata=0, ref_nodata=float('nan'), proc_crs=proc_crs, crs=CRS('EPSG:32735'),
                          transform=Affine(10., 0., 500000., 0., -10., 7000000.),
                          ref_transform=Affine(10. * RATIO, 0., 500000., 0., -10. * RATIO, 7000000.))


def process(rf, mask_partial, resident_mode):
    return rf.process(model=Model.gain_blk_offset, kernel_shape=(5, 5), model_config=dict(mask_partial=mask_partial),
                      device_config=dict(resident=resident_mode))


def timed(call, reps):
    call()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        s.append(time.perf_counter() - t0)
    return float(np.median(s)), min(s)


C_NAMES = {'uint8': 'unsigned char', 'float32': 'float'}


def count_gathers(into):
    """ wrap Context.boundless_window_dev: bytes read + written by the gathers, by the raster's dtype, summed into `into` """
    from homonim_amd import _hk
    real = _hk.Context.boundless_window_dev

    def counting(self, raster, window, out_dptr, *a, **kw):
        out = real(self, raster, window, out_dptr, *a, **kw)
        n = raster.shape[0] * int(window[2]) * int(window[3])
        into[raster.dtype.name] = into.get(raster.dtype.name, 0) + n * (raster.dtype.itemsize + out.dtype.itemsize)
        return out

    _hk.Context.boundless_window_dev = counting


def kernel_table(stats_dir, n, r, lines, gather_bytes):
    found = sorted(glob.glob(os.path.join(stats_dir, '**', '*kernel_stats.csv'), recursive=True))
    if not found:
        lines.append(f'kernels: no profiler run found under {stats_dir}')
        return
    with open(found[-1], newline='') as f:
        rows = list(csv.DictReader(f))
    # the planes the two new kernels move per call: the prefill writes the corrected raster (float32); the gathers' bytes depend on the
    # edge blocks and are not stated from the shapes alone
    fill_bytes = BANDS * n * n * 4
    lines.append(f'kernels of one resident process() (rocprofv3 --kernel-trace --stats, a run of its own, {TRACE_CALLS} calls): ms per call, '
                 'launches per call')
    total = 0.
    for row in sorted(rows, key=lambda x: -float(x['TotalDurationNs'])):
        name, calls, ns = row['Name'], int(row['Calls']), float(row['TotalDurationNs'])
        per_call_ms = ns / TRACE_CALLS / 1e6
        total += per_call_ms
        note = ''
        if 'fill_planes_kernel<float>' in name:
            note = f'   {fill_bytes * TRACE_CALLS / (ns * 1e-9) / 1e12:.2f} TB/s against the {fill_bytes / 1e6:.0f} MB of the corrected raster'
        for dtype, nbytes in gather_bytes.items():
            if f'boundless_window_kernel<{C_NAMES[dtype]}>' in name:
                note = (f'   {nbytes * TRACE_CALLS / (ns * 1e-9) / 1e12:.2f} TB/s against the {nbytes / 1e6:.0f} MB the edge windows of a call '
                        'read and write')
        short = name if len(name) <= 100 else name[:97] + '...'
        lines.append(f'  {per_call_ms:9.3f} ms  {calls / TRACE_CALLS:7.1f}  {short}{note}')
    lines.append(f'  {total:9.3f} ms  sum of the kernels per process() call')


def kernels_alone(n, reps, lines):
    """ the two kernels of the resident mode alone on resident planes, between two events on stream 0: the prefill of the corrected
    raster, and the gather of a window that overhangs the source by a halo of 3 on every side (no in-block of the case above reaches
    beyond its raster -- the reference covers the source exactly -- so the block loop itself launches no gather) """
    from homonim_amd import _hk
    ctx = _hk.default_context()
    m = n + 6
    d_src, d_f32, d_win = ctx.dev_alloc(BANDS * n * n), ctx.dev_alloc(BANDS * n * n * 4), ctx.dev_alloc(BANDS * m * m * 4)
    start, stop = ctx.event(), ctx.event()

    def ms_of(launch):
        launch()
        ctx.stream_sync(0)
        out = []
        for _ in range(reps):
            ctx.event_record(start, 0)
            launch()
            ctx.event_record(stop, 0)
            out.append(ctx.event_elapsed_ms(start, stop))
        return float(np.median(out))

    try:
        ctx.fill_planes_dev(d_src, 'uint8', BANDS, n, n, n, n * n, 100)
        cases = [('fill_planes_kernel<float>, the corrected raster', BANDS * n * n * 4,
                  lambda: ctx.fill_planes_dev(d_f32, 'float32', BANDS, n, n, n, n * n, float('nan')))]
        for nodata, out_size, what in ((0, 1, 'numeric nodata: uint8 out'), (None, 4, 'no nodata: float32 out')):
            raster = _hk.DeviceRaster(d_src, 'uint8', (BANDS, n, n), nodata=nodata)
            cases.append((f'boundless_window_kernel<unsigned char>, {what}', BANDS * (n * n + m * m * out_size),
                          lambda raster=raster: ctx.boundless_window_dev(raster, (-3, -3, m, m), d_win)))
        lines.append(f'the two kernels alone, {BANDS} bands of {n} x {n}, median of {reps} launches between events; bytes = every sample read '
                     'once and written once')
        for what, nbytes, launch in cases:
            ms = ms_of(launch)
            lines.append(f'  {ms:8.3f} ms  {nbytes / 1e6:8.1f} MB  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s  {what}')
    finally:
        ctx.event_destroy(start), ctx.event_destroy(stop)
        for p in (d_src, d_f32, d_win):
            ctx.dev_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resident_fuse.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--size', type=int, default=8190)
    ap.add_argument('--stats-dir', default=None, help='directory of the profiler run')
    ap.add_argument('--trace', default=None, help='PROC_CRS:MASK_PARTIAL -- resident calls alone (under rocprofv3)')
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    src, ref = make_pair(args.size)
    n, r = src.shape[-1], ref.shape[-1]
    if args.trace:
        proc_crs, mp = args.trace.split(':')
        rf = make_fuse(src, ref, proc_crs)
        for _ in range(TRACE_CALLS):
            process(rf, bool(int(mp)), True)
        print(json.dumps({'proc_crs': proc_crs, 'mask_partial': int(mp), 'calls': TRACE_CALLS}))
        return
    runs = []
    real_run = resident.ResidentRun.run

    def recording_run(self):
        out = real_run(self)
        runs.append((self.timings, len(self.calls), self.n_workers))
        return out

    resident.ResidentRun.run = recording_run
    gathered = {}
    count_gathers(gathered)
    lines = [f'# tools/resident_fuse_timing.py, {time.strftime("%Y-%m-%d")}: RasterFuse.process() to arrays, rasters on the host (default) and '
             'resident on the device',
             f'# {BANDS} bands, uint8 source {n} x {n}, float32 reference {r} x {r} ({RATIO}:1), gain-blk-offset 5 x 5, float32 output, default '
             f'max_block_mem and threads; median / best seconds of {args.reps} calls after a warm-up call, wall clock',
             '# resident split (median call): upload = planning + allocation + source and reference up + prefills; loop; overviews (none: '
             'no .tif); download', '']
    for proc_crs, mask_partial in CONFIGS:
        rf = make_fuse(src, ref, proc_crs)
        default = timed(lambda: process(rf, mask_partial, False), args.reps)
        del runs[:]
        gathered.clear()
        res = timed(lambda: process(rf, mask_partial, True), args.reps)
        a, b = process(rf, mask_partial, False)[0], process(rf, mask_partial, True)[0]
        if (proc_crs, mask_partial) == CONFIGS[0]:   # the configuration of the profiler run: bytes of one call
            gather_bytes = {k: v // (args.reps + 1) for k, v in gathered.items()}
        same = np.array_equal(a.view(np.uint8), b.view(np.uint8))
        del a, b
        split = {k: float(np.median([t[k] for t, _, _ in runs[1:args.reps + 1]])) for k in ('upload', 'loop', 'overviews', 'download')}
        lines.append(f'proc_crs={proc_crs} mask_partial={int(mask_partial)}   default {default[0]:7.3f} / {default[1]:7.3f} s   resident {res[0]:7.3f} / '
                     f'{res[1]:7.3f} s   default / resident {default[0] / res[0]:5.2f}   same bytes: {same}')
        lines.append(f'    resident: {runs[0][1]} call(s) on {runs[0][2]} stream(s); upload {split["upload"]:.3f} s, loop {split["loop"]:.3f} s, overviews '
                     f'{split["overviews"]:.3f} s, download {split["download"]:.3f} s')
    lines.append('')
    kernels_alone(n, args.reps, lines)
    if args.stats_dir:
        lines.append('')
        kernel_table(args.stats_dir, n, r, lines, gather_bytes)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
