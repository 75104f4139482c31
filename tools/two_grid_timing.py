""" Times the two-grid chains on device-resident rasters (hk_refspace_fit_apply_dev, hk_srcspace_fit_apply_dev) beside their
host-pointer forms and writes the result to profiles/two_grid_dev.txt.  Recorded, not gated: the kernels are the ones the host forms
run, so the host form's time on the same box is the yardstick.

Case: 4 bands, a uint8 source of 8190 x 8190 against a float32 reference at 2.5:1 (3276 x 3276), the default model configuration
(gain-blk-offset 5 x 5, `average` down, `cubic_spline` up), float32 output, mask_partial off and on, both families.

    python tools/two_grid_timing.py [--out profiles/two_grid_dev.txt] [--reps 7] [--size 8190] [--stats-dir DIR]

In one process, after a warm-up call of each form, it takes the median of `reps` calls of
  * the device form on resident rasters, between two events on the job's stream;
  * the host-pointer form on page-locked arrays, band by band, by the host clock (each call ends in a stream synchronise).
Bytes over PCIe: none for the device form; source + reference up and the corrected block down for the host form.

The per-kernel split comes from runs of their own under the profiler, one per configuration, the program after `--`:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/refspace_0 -- python tools/two_grid_timing.py --trace refspace:0

(`--trace FAMILY:MASK_PARTIAL` runs the device form alone and leaves DIR's kernel statistics to the profiler.)  With --stats-dir the
table of every kernel's time per call of the entry is added, and for the kernels whose algorithmic bytes this file states (from the
shapes: what the kernel must read and write, once) the share of the 8 TB/s HBM peak those bytes give.  One pass, no retries. """
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from homonim_amd import _hk  # noqa: E402

BANDS, RATIO = 4, 2.5
HBM_PEAK = 8e12   # bytes / s
AVERAGE, CUBIC_SPLINE = 5, 3
FAMILIES = ('refspace', 'srcspace')
TRACE_CALLS = 3   # calls of the entry in a --trace run (the first one warms up; the profiler sees all of them)


class Case:
    """ the rasters of the case on the device and page-locked on the host, and the two forms of one family """

    def __init__(self, ctx, n):
        self.ctx, self.n, self.r = ctx, n, int(np.ceil(n / RATIO))
        rng = np.random.default_rng(1)
        n, r = self.n, self.r
        self.src = ctx.pinned_empty((BANDS, n, n), np.uint8)
        self.ref = ctx.pinned_empty((BANDS, r, r), np.float32)
        self.corr = ctx.pinned_empty((BANDS, n, n), np.float32)
        for b in range(BANDS):   # 10 .. 200 with a nodata frame and holes; the reference = 1.3 x the source + 5 + noise
            s = rng.integers(10, 201, (n, n), dtype=np.uint8)
            s[:3] = s[:, -4:] = 0
            s[rng.random((n, n)) < 0.002] = 0
            self.src[b] = s
            at = (np.arange(r) * RATIO).astype(np.int64)     # (a pixel of every cell stands in for the cell's mean)
            ref = 1.3 * s[at][:, at].astype(np.float32) + 5. + rng.normal(0., 1., (r, r)).astype(np.float32)
            ref[100:140, 200:260] = np.nan
            self.ref[b] = ref
        self.stride = (n + 63) // 64 * 64
        self.d_src = ctx.dev_alloc(BANDS * n * self.stride)
        self.d_ref = ctx.dev_alloc(self.ref.nbytes)
        self.d_corr = ctx.dev_alloc(BANDS * n * self.stride * 4)
        padded = np.zeros((BANDS, n, self.stride), np.uint8)
        padded[:, :, :n] = self.src
        ctx.h2d(self.d_src, padded)
        ctx.h2d(self.d_ref, self.ref)
        self.desc = _hk.make_desc('gain-blk-offset', (5, 5), False, None, 0., float('nan'))
        self.io = _hk.make_io_desc('uint8', 'float32', 'float32', None)
        self.down, self.up = (RATIO, 0., RATIO, 0.), (1. / RATIO, 0., 1. / RATIO, 0.)

    def job(self, scratch=(0, 0)):
        n, r = self.n, self.r
        raster = _hk.DeviceRaster
        return _hk.make_two_grid_job(raster(self.d_src, 'uint8', (BANDS, n, n), self.stride), raster(self.d_ref, 'float32', (BANDS, r, r)),
                                     raster(self.d_corr, 'float32', (BANDS, n, n), self.stride), scratch=scratch[0], scratch_bytes=scratch[1])

    def space(self, family, mask_partial):
        if family == 'refspace':
            return (self.down, self.up, AVERAGE, CUBIC_SPLINE, mask_partial)
        return (self.up, CUBIC_SPLINE, mask_partial)     # the reference is the coarser raster: it is up-sampled to the source grid

    def dev(self, family, mask_partial):
        fn = self.ctx.refspace_fit_apply_dev if family == 'refspace' else self.ctx.srcspace_fit_apply_dev
        return lambda: fn(self.desc, *self.space(family, mask_partial), self.job(), self.io)

    def host(self, family, mask_partial):
        fn = self.ctx.refspace_fit_apply if family == 'refspace' else self.ctx.srcspace_fit_apply

        def call():
            for b in range(BANDS):
                fn(self.desc, self.src[b], self.ref[b], *self.space(family, mask_partial), 2, False, out_dtype='float32', out_nodata=None,
                   out_corr=self.corr[b])
        return call

    def pcie_bytes_host(self):
        return self.src.nbytes + self.ref.nbytes + self.corr.nbytes

    def free(self):
        for d in (self.d_src, self.d_ref, self.d_corr):
            self.ctx.dev_free(d)


def time_dev(ctx, launch, reps):
    """ median and best milliseconds of `reps` calls between two events on stream 0, after one warm-up call """
    start, stop = ctx.event(), ctx.event()
    launch()
    ctx.stream_sync(0)
    ms = []
    for _ in range(reps):
        ctx.event_record(start, 0)
        launch()
        ctx.event_record(stop, 0)
        ms.append(ctx.event_elapsed_ms(start, stop))
    ctx.event_destroy(start), ctx.event_destroy(stop)
    return float(np.median(ms)), min(ms)


def time_host(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()   # (every band's call ends in a stream synchronise)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def kernel_bytes(family, mask_partial, n, r):
    """ {part of a kernel's name: the bytes ONE band's launches of it must move}, from the shapes alone: every input read once, every
    output written once.  Kernels that are not listed (block statistics, mask_partial's erosion, the row table) get no share. """
    N, R = n * n, r * r
    if family == 'refspace':
        out = {'cast_in_kernel<unsigned char>': 5 * N + (5 * R if mask_partial else 0),   # the source; mask_partial: the mask bytes too
               'resample_kernel<5>': (4 * N + 4 * R) * (2 if mask_partial else 1),         # source down; mask_partial: its valid plane too
               'fit_apply_kernel': 16 * R,                                                 # source + reference in, gain + offset out
               'upsample_apply_kernel<3>': 8 * N + 8 * R + (4 * N if mask_partial else 0)}
        if mask_partial:
            out.update({'valid_plane_kernel': 8 * N, 'resample_kernel<0>': 4 * R + 4 * N})
        return out
    out = {'cast_in_kernel<unsigned char>': 5 * N,
           'resample_kernel<3>': 4 * R + 4 * N,                                            # the reference up to the source grid
           'fit_apply_kernel': 8 * N + (8 * N if mask_partial else 12 * N)}                # ... + the corrected plane without mask_partial
    if mask_partial:
        out.update({'valid_plane_kernel': 8 * R, 'resample_kernel<5>': 4 * R + 4 * N})
    return out


def kernel_table(stats_dir, family, mask_partial, n, r, lines):
    found = sorted(glob.glob(os.path.join(stats_dir, f'{family}_{int(mask_partial)}', '**', '*kernel_stats.csv'), recursive=True))
    if not found:
        lines.append(f'    kernels: no profiler run found under {stats_dir}/{family}_{int(mask_partial)}')
        return
    with open(found[-1], newline='') as f:
        rows = list(csv.DictReader(f))
    bytes_of = kernel_bytes(family, mask_partial, n, r)
    lines.append(f'    kernels (rocprofv3 --kernel-trace --stats, a run of its own, {TRACE_CALLS} calls of the entry): ms per call of the entry, '
                 f'launches per call, share of the {HBM_PEAK / 1e12:.0f} TB/s peak its algorithmic bytes give')
    total = 0.
    for row in sorted(rows, key=lambda x: -float(x['TotalDurationNs'])):
        name, calls, ns = row['Name'], int(row['Calls']), float(row['TotalDurationNs'])
        per_call_ms = ns / TRACE_CALLS / 1e6
        total += per_call_ms
        hits = [part for part in bytes_of if part in name]
        assert len(hits) <= 1, f'{name}: matched by {hits}'    # (a name is matched by one entry of kernel_bytes or by none)
        share = f'{bytes_of[hits[0]] * BANDS * TRACE_CALLS / (ns * 1e-9) / HBM_PEAK:6.3f}' if hits else '     -'
        short = name if len(name) <= 96 else name[:93] + '...'
        lines.append(f'      {per_call_ms:9.3f} ms  {calls / TRACE_CALLS:7.1f}  {share}  {short}')
    lines.append(f'      {total:9.3f} ms  sum of the kernels per call of the entry ("-": no byte count stated for the kernel; its time is in the sum)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'two_grid_dev.txt'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--size', type=int, default=8190)
    ap.add_argument('--stats-dir', default=None, help='directory of the profiler runs (one sub-directory FAMILY_MASKPARTIAL each)')
    ap.add_argument('--trace', default=None, help='FAMILY:MASK_PARTIAL -- run the device form alone (under rocprofv3)')
    args = ap.parse_args()
    ctx = _hk.default_context()
    case = Case(ctx, args.size)
    try:
        if args.trace:
            family, mp = args.trace.split(':')
            launch = case.dev(family, bool(int(mp)))
            for _ in range(TRACE_CALLS):
                launch()
                ctx.stream_sync(0)
            print(json.dumps({'family': family, 'mask_partial': int(mp), 'calls': TRACE_CALLS}))
            return
        n, r = case.n, case.r
        lines = [f'# tools/two_grid_timing.py, {time.strftime("%Y-%m-%d")}: the two-grid chains on device-resident rasters beside their host-pointer forms',
                 f'# {BANDS} bands, uint8 source {n} x {n} (row stride {case.stride}), float32 reference {r} x {r} ({RATIO}:1), gain-blk-offset 5 x 5, '
                 f'average down, cubic_spline up, float32 output; median / best ms of {args.reps} calls after a warm-up call',
                 f'# device form: events on the job\'s stream, 0 bytes over PCIe; host form: page-locked arrays, band by band, host clock, '
                 f'{case.pcie_bytes_host() / 1e6:.1f} MB over PCIe per call of all bands', '']
        for family in FAMILIES:
            for mask_partial in (False, True):
                dev = time_dev(ctx, case.dev(family, mask_partial), args.reps)
                host = time_host(case.host(family, mask_partial), args.reps)
                need = (ctx.refspace_dev_scratch_bytes if family == 'refspace' else ctx.srcspace_dev_scratch_bytes)(
                    case.desc, *case.space(family, mask_partial), case.job(), case.io)
                lines.append(f'{family:<9} mask_partial={int(mask_partial)}   device form {dev[0]:9.3f} / {dev[1]:9.3f} ms   host form {host[0]:9.3f} / '
                             f'{host[1]:9.3f} ms   host / device {host[0] / dev[0]:6.2f}   scratch {need / 1e6:8.1f} MB')
                if args.stats_dir:
                    kernel_table(args.stats_dir, family, mask_partial, n, r, lines)
        text = '\n'.join(lines) + '\n'
        print(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    finally:
        case.free()


if __name__ == '__main__':
    main()
