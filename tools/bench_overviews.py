#!/usr/bin/env python3
""" Timing of the internal overviews (hk_overview.hip).

default     device-resident: ``--bands`` x ``--size``^2 float32 (NaN nodata) and uint8 (nodata 0), all ``overview_factors`` levels
            in one ``hk_overviews_dev`` call, timed with events; achieved bytes/s over the algorithmic bytes (one read of the
            raster + every level written once) beside the library's flat-stream probe (``hk_stream_probe_dev``) in the same call.
``--host``  a host raster through ``Context.overviews`` (pageable and page-locked) beside the only way to the same pixels without
            it -- chained ``Context.reproject(average)`` calls, which re-upload every level -- and a numpy 2 x 2 nanmean pyramid
            for scale; alternating rounds.
``--product``  ``RasterFuse.process`` to memory on a 4-band gain-offset 5 x 5 tile (BASELINE.json configs[4]) and the overview
            build of its results (corrected + parameters) as ``process(build_ovw=True)`` does it before the file is written. """
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homonim_amd import RasterFuse, Resampling, _hk, overview_factors  # noqa: E402


def algorithmic_bytes(bands, h, w, itemsize, n_levels):
    return bands * itemsize * (h * w + sum(lh * lw for lh, lw in _hk.overview_shapes(h, w, n_levels)))


def device_resident(a):
    ctx = _hk.Context(0, n_streams=1)
    H = W = a.size
    n = len(overview_factors((H, W)))
    probe_bytes = 1 << 30
    d_probe = [ctx.dev_alloc(probe_bytes) for _ in range(3)]
    for d in d_probe:
        ctx.memset(d, 0, probe_bytes)
    for dtype, nodata in (('float32', float('nan')), ('uint8', 0)):
        it = np.dtype(dtype).itemsize
        stride = (W + 63) // 64 * 64
        band_stride = stride * H
        d_src = ctx.dev_alloc(it * band_stride * a.bands)
        if dtype == 'float32':
            d_ref = ctx.dev_alloc(it * band_stride * a.bands)
            ctx.synth_fill_dev(d_src, d_ref, a.bands, H, W, stride, band_stride, seed=1, nodata_variant=1, stream=0)
            ctx.stream_sync(0)
            ctx.dev_free(d_ref)
        else:
            band = np.random.default_rng(1).integers(0, 255, (H, stride), dtype=np.uint8, endpoint=True)
            for b in range(a.bands):
                ctx.h2d(d_src + b * band_stride, band)
        shapes = _hk.overview_shapes(H, W, n)
        strides = [(lw + 63) // 64 * 64 for _, lw in shapes]
        d_out = [ctx.dev_alloc(it * a.bands * lh * s) for (lh, _), s in zip(shapes, strides)]

        def launch():
            ctx.overviews_dev(d_src, dtype, a.bands, H, W, stride, band_stride, nodata, d_out, strides,
                              [lh * s for (lh, _), s in zip(shapes, strides)], stream=0)

        def probe():
            ctx.stream_probe_dev(d_probe[0], d_probe[1], d_probe[2], probe_bytes, 0)

        def timed(fn, reps):
            ev = [(ctx.event(), ctx.event()) for _ in range(reps)]
            for e0, e1 in ev:
                ctx.event_record(e0, 0)
                fn()
                ctx.event_record(e1, 0)
            ctx.stream_sync(0)
            ms = [ctx.event_elapsed_ms(e0, e1) for e0, e1 in ev]
            for e0, e1 in ev:
                ctx.event_destroy(e0), ctx.event_destroy(e1)
            return ms

        for _ in range(max(1, a.warmup)):
            launch(), probe()
        ctx.stream_sync(0)
        one = float(np.median(timed(launch, 5)))
        reps = max(20, int(1000.0 / max(one, 1e-3)) // 4)      # four alternating rounds fill about a second
        ov_ms, pr_ms = [], []
        for _ in range(4):
            ov_ms += timed(launch, reps)
            pr_ms += timed(probe, 20)
        ms, pms = float(np.median(ov_ms)), float(np.median(pr_ms))
        gb = algorithmic_bytes(a.bands, H, W, it, n) / 1e9
        tbps, probe_tbps = gb / ms, 3 * probe_bytes / 1e9 / pms
        print(json.dumps(dict(kernel=f'overview_kernel<{dtype}>', size=a.size, bands=a.bands, levels=n, reps=len(ov_ms), ms=round(ms, 4),
                              algorithmic_GB=round(gb, 3), TBps=round(tbps, 3), stream_probe_TBps=round(probe_tbps, 3),
                              ratio_to_stream_probe=round(tbps / probe_tbps, 3))), flush=True)
        for d in [d_src] + d_out:
            ctx.dev_free(d)


def numpy_pyramid(arr, n):
    if arr.shape[0] > 1:   # band by band: the float64 copy of one band at a time
        per_band = [numpy_pyramid(arr[b:b + 1], n) for b in range(arr.shape[0])]
        return [np.concatenate([pb[m] for pb in per_band]) for m in range(n)]
    out, cur = [], arr
    for _ in range(n):
        nb, h, w = cur.shape
        pad = np.full((nb, (h + 1) // 2 * 2, (w + 1) // 2 * 2), np.nan, np.float32)
        pad[:, :h, :w] = cur
        with np.errstate(all='ignore'):
            cells = pad.reshape(nb, pad.shape[1] // 2, 2, pad.shape[2] // 2, 2).transpose(0, 1, 3, 2, 4).reshape(nb, pad.shape[1] // 2, pad.shape[2] // 2, 4)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                cur = np.nanmean(cells.astype(np.float64), axis=-1).astype(np.float32)
        out.append(cur)
    return out


def host_path(a):
    ctx = _hk.default_context()
    H = W = a.size
    n = len(overview_factors((H, W)))
    rng = np.random.default_rng(2)
    arr = np.empty((a.bands, H, W), np.float32)
    arr[0] = rng.random((H, W), dtype=np.float32)
    arr[0][rng.random((H, W), dtype=np.float32) < 0.1] = np.nan
    for b in range(1, a.bands):
        arr[b] = arr[0] + np.float32(b)
    nan = float('nan')

    def chained():
        out, cur = [], arr
        for _ in range(n):
            cur = ctx.reproject(cur, nan, (2, 0, 2, 0), ((cur.shape[1] + 1) // 2, (cur.shape[2] + 1) // 2), int(Resampling.average), nan)
            out.append(cur)
        return out

    def wall(fn):
        t0 = time.perf_counter()
        res = fn()
        return time.perf_counter() - t0, res

    ctx.overviews(arr, nan, n), chained()                  # warm-up: staging ring, slabs
    t = dict(pageable=[], pinned=[], chained_reproject=[])
    for _ in range(a.rounds):
        s, new = wall(lambda: ctx.overviews(arr, nan, n))
        t['pageable'].append(s)
        s, old = wall(chained)
        t['chained_reproject'].append(s)
        ctx.pin(arr)
        try:
            s, pinned = wall(lambda: ctx.overviews(arr, nan, n))
        finally:
            ctx.unpin(arr)
        t['pinned'].append(s)
        for x, y, z in zip(new, old, pinned):
            assert x.tobytes() == z.tobytes() and np.array_equal(x, y, equal_nan=True)
    numpy_s, ref = wall(lambda: numpy_pyramid(arr, n))
    same_as_numpy = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(new, ref))
    moved = algorithmic_bytes(a.bands, H, W, 4, n) / 1e9
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps(dict(what='Context.overviews on a host raster', size=a.size, bands=a.bands, levels=n, rounds=a.rounds,
                          pageable_s=round(med['pageable'], 3), pinned_s=round(med['pinned'], 3),
                          chained_reproject_s=round(med['chained_reproject'], 3), numpy_nanmean_pyramid_s=round(numpy_s, 3),
                          pcie_GBps_pageable=round(moved / med['pageable'], 1), pcie_GBps_pinned=round(moved / med['pinned'], 1),
                          speedup_over_chained=round(med['chained_reproject'] / med['pageable'], 2),
                          bit_identical_to_chained=True, equal_to_numpy=bool(same_as_numpy))), flush=True)


def product(a):
    ctx = _hk.default_context()
    H = W = a.size
    rng = np.random.default_rng(3)
    src = rng.uniform(0.1, 1.0, (a.bands, H, W)).astype(np.float32)
    ref = (1.5 * src + 0.1 + rng.normal(0, 0.05, src.shape).astype(np.float32)).astype(np.float32)
    src[:, :8, :] = np.nan
    fuse = RasterFuse(src, ref)
    runs, ovw = [], []
    for _ in range(a.rounds + 1):
        t0 = time.perf_counter()
        corr, params = fuse.process(None, 'gain-offset', (5, 5), param_filename=True)
        runs.append(time.perf_counter() - t0)
        pinned = RasterFuse._pin(ctx, [corr, params])
        t0 = time.perf_counter()
        RasterFuse._overviews(ctx, corr, float('nan')), RasterFuse._overviews(ctx, params, float('nan'))
        ovw.append(time.perf_counter() - t0)
        for p in pinned:
            ctx.unpin(p)
    p_s, o_s = float(np.median(runs[1:])), float(np.median(ovw[1:]))
    print(json.dumps(dict(what='RasterFuse.process to memory, and the overviews of its results', size=a.size, bands=a.bands,
                          levels=len(overview_factors((H, W))), param_bands=int(params.shape[0]), process_s=round(p_s, 3),
                          overviews_s=round(o_s, 3), added=round(o_s / p_s, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--bands', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--product', action='store_true')
    a = ap.parse_args()
    if a.host:
        return host_path(a)
    if a.product:
        return product(a)
    return device_resident(a)


if __name__ == '__main__':
    main()
