""" Times the warps of hk_warp.hip on device-resident rasters and writes times, ratios and achieved GB/s to profiles/warp.txt.

(1) The cross-CRS warp (hk_reproject_crs_dev, bilinear, Transverse Mercator lon0 25 -> UTM 35S) on device-resident rasters at
4 x 8192^2 and 4 x 16384^2 destination pixels against (a) the same-CRS affine re-sampler on the same shapes (hk_reproject_dev:
resample_kernel<1>, one launch for the 4 bands) and (b) the coordinate kernel alone (hk_warp_coords_dev), and writes times, ratios
and achieved GB/s.  The comparison shows whether the launch is bound by float64 arithmetic or by the gather.

(2) Rotated grids (hk_reproject_affine_dev, bilinear, 10 m -> 5 m like (1)): a source turned by 0, 30 and 90 degrees within one CRS,
and a Transverse Mercator source turned by 30 degrees onto the UTM grid of (1) -- for every candidate thread tile of the affine
builds (HK_WARP_TILE, read once per process: each candidate runs in a fresh child process, one after the other).  The tile that is
fastest at 90 degrees without slowing 0 degrees beyond the spread of the repeats is the library's default (hk_warp.hip warp_tile).

    python tools/warp_timing.py [--out profiles/warp.txt] [--reps 5] [--sizes 8192 16384] [--tiles 256x1 64x4 32x8 16x16 8x32]

One pass, no retries: any failing step ends the script.  Bytes counted per destination pixel: 4 B written per band
plus 4 B read per band (the up-sampled source is read once through the caches); the coordinate kernel writes 16 B. """
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from homonim_amd import Affine, CRS, _hk, crs  # noqa: E402
from homonim_amd.raster_array import warp_scale  # noqa: E402

TM25 = CRS('unnamed [1024=1; 2048=4326; 2057=6378137.0; 2059=298.257223563; 3075=1; 3080=25.0; 3081=0.0; 3082=0.0; 3083=0.0; 3092=1.0]')
UTM35S = CRS('EPSG:32735')
BANDS = 4


def timed(ctx, launch, reps):
    """ best and median milliseconds of `reps` launches between two events on stream 0 (one warm-up launch first) """
    start, stop = ctx.event(), ctx.event()
    launch()
    ctx.stream_sync(0)
    ms = []
    for _ in range(reps):
        ctx.event_record(start, 0)
        launch()
        ctx.event_record(stop, 0)
        ms.append(ctx.event_elapsed_ms(start, stop))
    ctx.event_destroy(start)
    ctx.event_destroy(stop)
    return min(ms), float(np.median(ms))


def run(ctx, n, reps, lines):
    # destination: n x n UTM pixels of 5 m; source: a Transverse Mercator raster of 10 m pixels that covers it (up-sampling 2 x,
    # the fast bilinear kernel on both paths)
    dst_tf = Affine(5., 0., 250000., 0., -5., 6280000.)
    cols, rows = np.array([0., n, n, 0.]), np.array([0., 0., n, n])
    xs, ys = crs.transform_coords(UTM35S, TM25, dst_tf.c + cols * dst_tf.a, dst_tf.f + rows * dst_tf.e)
    src_tf = Affine(10., 0., float(xs.min()) - 50., 0., -10., float(ys.max()) + 50.)
    sw, sh = int((xs.max() - xs.min()) / 10.) + 12, int((ys.max() - ys.min()) / 10.) + 12
    warp = _hk.make_warp_desc(crs.parse(TM25), src_tf, crs.parse(UTM35S), dst_tf)
    scale = warp_scale(UTM35S, dst_tf, (n, n), TM25, src_tf)
    s_stride, d_stride = (sw + 63) // 64 * 64, (n + 63) // 64 * 64
    src = np.random.default_rng(1).uniform(0.05, 1., (BANDS, sh, s_stride)).astype(np.float32)
    d_src, d_dst = ctx.dev_alloc(src.nbytes), ctx.dev_alloc(BANDS * n * d_stride * 4)
    d_xy = ctx.dev_alloc(2 * n * d_stride * 8)
    try:
        ctx.h2d(d_src, src)
        t_warp = timed(ctx, lambda: ctx.reproject_crs_dev(warp, d_src, BANDS, (sh, sw), s_stride, sh * s_stride, None, scale, 1,
                                                          d_dst, (n, n), d_stride, n * d_stride, 0.), reps)
        t_one = timed(ctx, lambda: ctx.reproject_crs_dev(warp, d_src, 1, (sh, sw), s_stride, sh * s_stride, None, scale, 1,
                                                         d_dst, (n, n), d_stride, n * d_stride, 0.), reps)
        mapping = (0.5, 3., 0.5, 3.)     # the affine kernel at the same up-sampling factor, inside the same source
        t_aff = timed(ctx, lambda: ctx.reproject_dev(d_src, BANDS, (sh, sw), s_stride, sh * s_stride, None, mapping, 1, d_dst, (n, n),
                                                     d_stride, n * d_stride, 0.), reps)
        t_xy = timed(ctx, lambda: ctx.warp_coords_dev(warp, (n, n), d_xy, d_xy + n * d_stride * 8, d_stride), reps)
    finally:
        for d in (d_src, d_dst, d_xy):
            ctx.dev_free(d)
    px = n * n
    gbs = lambda ms, nbytes: nbytes / ms / 1e6   # noqa: E731
    lines += [
        f'{BANDS} x {n}^2 destination pixels, source {sh} x {sw} (10 m -> 5 m), scale ({scale[0]:.4f}, {scale[1]:.4f}), best / median ms of {reps}',
        f'  warp      hk_reproject_crs_dev, {BANDS} bands  {t_warp[0]:9.3f} / {t_warp[1]:9.3f} ms   {gbs(t_warp[0], px * BANDS * 8):8.1f} GB/s   '
        f'{t_warp[0] / BANDS:8.3f} ms per band',
        f'  warp      hk_reproject_crs_dev, 1 band   {t_one[0]:9.3f} / {t_one[1]:9.3f} ms   {gbs(t_one[0], px * 8):8.1f} GB/s',
        f'  affine    hk_reproject_dev,     {BANDS} bands  {t_aff[0]:9.3f} / {t_aff[1]:9.3f} ms   {gbs(t_aff[0], px * BANDS * 8):8.1f} GB/s   '
        f'{t_aff[0] / BANDS:8.3f} ms per band',
        f'  coords    hk_warp_coords_dev            {t_xy[0]:9.3f} / {t_xy[1]:9.3f} ms   {gbs(t_xy[0], px * 16):8.1f} GB/s',
        f'  ratios    warp / affine per band at {BANDS} bands {t_warp[0] / t_aff[0]:6.2f}; warp, 1 band / coords {t_one[0] / t_xy[0]:6.2f}; '
        f'each further band {(t_warp[0] - t_one[0]) / (BANDS - 1):8.3f} ms',
        '',
    ]


KEEP_MARKER = '# ---- below: not written by tools/warp_timing.py'
ROTATED = ('0 deg', '30 deg', '90 deg', 'TM 30 deg -> UTM')


def _turned_source(centre, degrees, n):
    """ a 10 m source grid turned by `degrees` about `centre` that covers an n x n destination of 5 m pixels centred there """
    r = math.radians(degrees)
    m = int(math.ceil(n / 2 * (abs(math.cos(r)) + abs(math.sin(r))))) + 12
    tf = Affine.translation(*centre) * Affine.rotation(degrees) * Affine.scale(10., -10.) * Affine.translation(-m / 2, -m / 2)
    return tf, m


def run_rotated(ctx, n, reps):
    """ {case: (best ms, median ms)} of the four rotated cases at 4 x n^2 destination pixels, with the tile this process was given """
    dst_tf = Affine(5., 0., 250000., 0., -5., 6280000.)
    centre = dst_tf * (n / 2, n / 2)
    tm_centre = [float(v) for v in crs.transform_coords(UTM35S, TM25, *centre)]
    cases = [(name, None, None, *_turned_source(centre, deg, n)) for name, deg in zip(ROTATED, (0., 30., 90.))]
    cases.append((ROTATED[3], crs.parse(TM25), crs.parse(UTM35S), *_turned_source(tm_centre, 30., n + 64)))
    d_stride = (n + 63) // 64 * 64
    out = {}
    for name, src_def, dst_def, src_tf, m in cases:
        warp = _hk.make_affine_warp_desc(src_def, src_tf, dst_def, dst_tf)
        scale = warp_scale(UTM35S, dst_tf, (n, n), TM25 if src_def is not None else UTM35S, src_tf)
        s_stride = (m + 63) // 64 * 64
        src = np.random.default_rng(1).uniform(0.05, 1., (BANDS, m, s_stride)).astype(np.float32)
        d_src, d_dst = ctx.dev_alloc(src.nbytes), ctx.dev_alloc(BANDS * n * d_stride * 4)
        try:
            ctx.h2d(d_src, src)
            out[name] = timed(ctx, lambda: ctx.reproject_affine_dev(warp, d_src, BANDS, (m, m), s_stride, m * s_stride, None, scale, 1,
                                                                    d_dst, (n, n), d_stride, n * d_stride, 0.), reps)
        finally:
            ctx.dev_free(d_src)
            ctx.dev_free(d_dst)
    return out


def sweep_tiles(tiles, n, reps, lines):
    """ run_rotated once per candidate tile, each in a fresh process; the table, and the tile the rule picks """
    rows = {}
    for tile in tiles:
        env = dict(os.environ, HK_WARP_TILE=tile)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--sizes', str(n), '--reps', str(reps)], env=env,
                             stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit(f'tile {tile}: the child process ended with status {res.returncode}')
        rows[tile] = json.loads(res.stdout.strip().splitlines()[-1])
    gbs = lambda ms: n * n * BANDS * 8 / ms / 1e6   # noqa: E731
    lines += [f'rotated grids, hk_reproject_affine_dev, bilinear, {BANDS} x {n}^2 destination pixels (10 m -> 5 m): best / median ms of '
              f'{reps} and GB/s at the best, per thread tile (width x height of destination pixels, 256 threads)',
              '  tile     ' + ''.join(f'{c:>34}' for c in ROTATED)]
    for tile, r in rows.items():
        lines.append(f'  {tile:<8} ' + ''.join(f'{r[c][0]:10.3f} /{r[c][1]:9.3f} {gbs(r[c][0]):8.1f} GB/s' for c in ROTATED))
    # fastest at 90 degrees among those that do not slow 0 degrees beyond the run-to-run spread (median - best) of the fastest there
    best0 = min(rows.values(), key=lambda r: r[ROTATED[0]][0])[ROTATED[0]]
    allowed = {t: r for t, r in rows.items() if r[ROTATED[0]][0] <= best0[0] + max(best0[1] - best0[0], 0.01 * best0[0])}
    pick = min(allowed, key=lambda t: allowed[t][ROTATED[2]][0])
    lines += [f'  rule: fastest at 90 deg among the tiles within the spread of the fastest at 0 deg -> {pick}', '']
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'warp.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[8192, 16384])
    ap.add_argument('--tiles', nargs='+', default=['256x1', '64x4', '32x8', '16x16', '8x32'])
    ap.add_argument('--child', action='store_true', help='(internal) time the rotated cases with this process\'s HK_WARP_TILE')
    args = ap.parse_args()
    ctx = _hk.default_context()
    if args.child:
        print(json.dumps(run_rotated(ctx, args.sizes[0], args.reps)))
        return
    lines = [f'# tools/warp_timing.py, {time.strftime("%Y-%m-%d")}: bilinear warps of hk_warp.hip on device-resident rasters', '',
             'TM(lon0 25) -> UTM 35S, axis-aligned grids (hk_reproject_crs_dev):', '']
    for n in args.sizes:
        run(ctx, n, args.reps, lines)
    sweep_tiles(args.tiles, args.sizes[0], args.reps, lines)
    text = '\n'.join(lines)
    print(text)
    kept = ''
    if os.path.exists(args.out):   # what the file holds below the marker is not this tool's: accuracy figures, notes
        with open(args.out) as f:
            old = f.read()
        kept = old[old.index(KEEP_MARKER):] if KEEP_MARKER in old else ''
    with open(args.out, 'w') as f:
        f.write(text + ('\n' + kept if kept else ''))


if __name__ == '__main__':
    main()
