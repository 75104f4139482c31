""" Times the cross-CRS warp (hk_reproject_crs_dev, bilinear, Transverse Mercator lon0 25 -> UTM 35S) on device-resident rasters at
4 x 8192^2 and 4 x 16384^2 destination pixels against (a) the same-CRS affine re-sampler on the same shapes (hk_reproject_dev:
resample_kernel<1>, one launch for the 4 bands) and (b) the coordinate kernel alone (hk_warp_coords_dev), and writes times, ratios
and achieved GB/s to profiles/warp.txt.  The comparison shows whether the launch is bound by float64 arithmetic or by the gather.

    python tools/warp_timing.py [--out profiles/warp.txt] [--reps 5]

One process, one pass, no retries: any failing step ends the script.  Bytes counted per destination pixel: 4 B written per band
plus 4 B read per band (the up-sampled source is read once through the caches); the coordinate kernel writes 16 B. """
import argparse
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'warp.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[8192, 16384])
    args = ap.parse_args()
    ctx = _hk.default_context()
    lines = [f'# tools/warp_timing.py, {time.strftime("%Y-%m-%d")}: bilinear warp TM(lon0 25) -> UTM 35S on device-resident rasters', '']
    for n in args.sizes:
        run(ctx, n, args.reps, lines)
    text = '\n'.join(lines)
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
