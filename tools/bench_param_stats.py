#!/usr/bin/env python3
""" Device-resident timing of the parameter statistics reduction (hk_param_stats_dev): 4 B read per pixel*band.
``--e2e``: instead, the wall time of ``ParamStats.from_arrays(params).stats()`` on a host array (PCIe-bound: every byte crosses
the bus once) beside numpy doing the reference's five float64 passes (homonim/stats.py:220-229) on the same host. """
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homonim_amd import _hk  # noqa: E402


def e2e(a):
    from homonim_amd import Model, ParamStats
    rng = np.random.default_rng(1)
    band = rng.normal(1, 0.3, (a.size, a.size)).astype(np.float32)
    band[0, :] = band[-1, :] = np.nan
    band[:, 0] = band[:, -1] = np.nan
    params = np.empty((a.bands, a.size, a.size), np.float32)
    for b in range(a.bands):
        params[b] = band
        params[b, :, 1] += np.float32(b)   # bands differ
    runs = []
    for _ in range(a.steps + 1):   # the first run allocates the staging ring and the slabs: not counted
        ps = ParamStats.from_arrays(params, Model.gain_offset, r2_inpaint_thresh=a.thresh)
        t0 = time.perf_counter()
        stats_list = ps.stats(threads=a.threads)
        runs.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = []
    for b in range(a.bands):   # stats.py:220-229: the band as a masked float64 array, five passes (+ the threshold count)
        array = np.ma.masked_invalid(params[b].astype(np.float64))
        ref.append(dict(min=array.min(), max=array.max(), sum=array.sum(), sum2=(array ** 2).sum(), n=array.count(),
                        inpaint_sum=(array < a.thresh).sum()))
    numpy_s = time.perf_counter() - t0
    assert all(s['n'] == r['n'] and s['min'] == r['min'] and s['max'] == r['max'] for s, r in zip(stats_list, ref))
    gb = params.nbytes / 1e9
    print(json.dumps(dict(what='ParamStats.from_arrays(params).stats()', size=a.size, bands=a.bands, threads=a.threads,
                          runs_s=[round(r, 3) for r in runs[1:]], median_s=round(float(np.median(runs[1:])), 3),
                          host_GBps=round(gb / float(np.median(runs[1:])), 2), numpy_five_passes_s=round(numpy_s, 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--bands', type=int, default=4)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--nodata', type=int, default=1, help='synthetic nodata variant (1: NaN frame; 0: none)')
    ap.add_argument('--thresh', type=float, default=0.25)
    ap.add_argument('--e2e', action='store_true', help='time ParamStats.from_arrays(...).stats() on a host array and numpy beside it')
    ap.add_argument('--threads', type=int, default=4)
    a = ap.parse_args()
    if a.e2e:
        return e2e(a)
    ctx = _hk.Context(0, n_streams=1)
    H = W = a.size
    stride = (W + 63) // 64 * 64
    band_stride = stride * H
    d = {k: ctx.dev_alloc(4 * band_stride * a.bands) for k in ('src', 'ref')}
    d['stats'] = ctx.dev_alloc(8 * _hk.PARAM_STATS_N * a.bands)
    ctx.synth_fill_dev(d['src'], d['ref'], a.bands, H, W, stride, band_stride, seed=1, nodata_variant=a.nodata, stream=0)
    ctx.dev_free(d.pop('ref'))
    nd = np.nan if a.nodata in (1, 2) else None

    def launch():
        ctx.param_stats_dev(d['src'], a.bands, H, W, stride, band_stride, d['stats'], nd, a.thresh, stream=0)

    for _ in range(max(1, a.warmup)):
        launch()
    ev = [(ctx.event(), ctx.event()) for _ in range(max(20, a.steps))]
    for e0, e1 in ev:
        ctx.event_record(e0, 0)
        launch()
        ctx.event_record(e1, 0)
    ctx.stream_sync(0)
    ms = float(np.median([ctx.event_elapsed_ms(e0, e1) for e0, e1 in ev]))
    stats = np.zeros((a.bands, _hk.PARAM_STATS_N))
    ctx.d2h(stats, d['stats'])
    gb = 4.0 * H * W * a.bands / 1e9
    print(json.dumps(dict(kernel='param_stats', size=a.size, bands=a.bands, steps=len(ev), ms=round(ms, 4),
                          GBps=round(gb / ms * 1e3, 1), frac_of_8TBps=round(gb / ms * 1e3 / 8000, 4),
                          n_valid=int(stats[:, 4].sum()), n_below=int(stats[:, 5].sum()))))


if __name__ == '__main__':
    main()
