""" The measurements of profiles/internal_mask.txt, on an MI355X.
    python tools/internal_mask_timing.py events OUT.txt     (b) the masked overview kernel beside the unmasked one, device events;
                                                            (c) process() with nodata=None against nodata=0, wall clock
    rocprofv3 --kernel-trace --stats ... -- python tools/internal_mask_timing.py cast
                                                            (a) launches cast_out_kernel<uint8> and cast_out_valid_kernel<uint8> on
                                                            the same 16384^2 block, alternating: the trace gives their kernel times """
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from homonim_amd import Affine, RasterFuse, _hk   # noqa: E402

ctx = _hk.default_context()


def measure_overviews(out):
    nb, h, w, n = 3, 16384, 16384, 6
    rng = np.random.default_rng(1)
    a = rng.integers(1, 200, (nb, h, w), dtype=np.uint8)
    valid = (rng.random((h, w)) >= 0.25).astype(np.uint8) * np.uint8(255)
    a[:, valid == 0] = 255
    shapes = _hk.overview_shapes(h, w, n)
    d_src, d_valid = ctx.dev_alloc(a.nbytes), ctx.dev_alloc(valid.nbytes)
    d_outs = [ctx.dev_alloc(nb * lh * lw) for lh, lw in shapes]
    d_vouts = [ctx.dev_alloc(lh * lw) for lh, lw in shapes]
    ctx.h2d(d_src, a)
    ctx.h2d(d_valid, valid)
    strides, bstrides = [lw for _, lw in shapes], [lh * lw for lh, lw in shapes]

    def plain():
        ctx.overviews_dev(d_src, 'uint8', nb, h, w, w, h * w, 255, d_outs, strides, bstrides)

    def masked():
        ctx.overviews_valid_dev(d_src, 'uint8', nb, h, w, w, h * w, d_valid, w, d_outs, strides, bstrides, d_vouts, strides)

    e0, e1 = ctx.event(), ctx.event()
    times = {'plain': [], 'masked': []}
    for _ in range(3):
        plain(), masked()
    ctx.stream_sync(0)
    for rep in range(10):           # alternating, 10 launches per timed window
        for name, fn in (('plain', plain), ('masked', masked)):
            ctx.event_record(e0, 0)
            for _ in range(10):
                fn()
            ctx.event_record(e1, 0)
            ctx.stream_sync(0)
            times[name].append(ctx.event_elapsed_ms(e0, e1) / 10)
    for d in [d_src, d_valid] + d_outs + d_vouts:
        ctx.dev_free(d)
    px = nb * h * w
    for name in times:
        t = np.array(times[name])
        out.write(f'(b) overview_kernel<uint8> {name}: 3 x 16384^2, 6 levels, device events, 10 windows of 10 launches: '
                  f'median {np.median(t):.3f} ms (min {t.min():.3f}, max {t.max():.3f}); {px * 4 / 3 / np.median(t) / 1e6:.0f} GB/s of '
                  f'sample bytes (read 1 + written 1/3 per sample)\n')
    out.write(f'(b) ratio masked / plain (medians): {np.median(times["masked"]) / np.median(times["plain"]):.3f}\n')


def measure_process(out):
    nb, h, w = 3, 4096, 4096
    rng = np.random.default_rng(2)
    src = rng.uniform(20.0, 200.0, (nb, h, w)).astype(np.float32)
    ref = (1.1 * src + 5.0 + rng.normal(0, 2.0, src.shape).astype(np.float32)).astype(np.float32)
    src[:, :50, :] = np.nan
    src[:, 1000:1400, 2000:2600] = np.nan
    src8, ref8 = np.nan_to_num(src, nan=0).astype(np.uint8), np.clip(ref, 1, 255).astype(np.uint8)
    tf = Affine(10., 0., 300000., 0., -10., 6200000.)
    times = {'nodata=0': [], 'nodata=None': []}
    for rep in range(4):            # the first round warms up and is dropped
        for name, nodata in (('nodata=0', 0), ('nodata=None', None)):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fuse = RasterFuse(src8, ref8, src_nodata=0, ref_nodata=None, transform=tf)
                t0 = time.perf_counter()
                fuse.process(f'/tmp/internal_mask_{rep}.tif', 'gain-blk-offset', (5, 5), overwrite=True,
                             out_profile=dict(dtype='uint8', nodata=nodata))
                dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
    for name, t in times.items():
        out.write(f'(c) process 3 x 4096^2 uint8 -> .tif, {name}: wall {", ".join(f"{x:.2f}" for x in t)} s (median {np.median(t):.2f})\n')
    out.write(f'(c) ratio nodata=None / nodata=0 (medians): {np.median(times["nodata=None"]) / np.median(times["nodata=0"]):.3f}\n')


def launch_casts():
    h = w = 16384
    rng = np.random.default_rng(3)
    src = rng.uniform(20.0, 200.0, (h, w)).astype(np.float32)
    ref = (1.1 * src + 5.0).astype(np.float32)
    src[rng.random((h, w)) < 0.1] = np.nan
    desc = _hk.make_desc('gain', (5, 5), False, None, np.nan, np.nan)
    corr, valid = np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)
    for _ in range(4):              # alternating; the trace names the two cast kernels
        ctx.fit_apply_block(desc, src, ref, (0, 0, h, w), corr, out_nodata=None)
        ctx.fit_apply_block(desc, src, ref, (0, 0, h, w), corr, out_nodata=None, valid_dst=valid)


if __name__ == '__main__':
    if sys.argv[1] == 'events':
        with open(sys.argv[2], 'w') as out:
            measure_overviews(out)
            out.flush()
            measure_process(out)
    else:
        launch_casts()
