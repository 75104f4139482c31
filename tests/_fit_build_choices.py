"""
Which builds of the fused kernel the library launches, case by case, over the decision space of tests/test_gpu_build_sweep.py: its
CONFIGS over HEIGHTS x WIDTHS, the paired widths, the forced rings with their heights, force-general and the batched jobs, on that
file's 44 x 300 raster and through its entry kinds (parameters out; corrected only; device job + in-painting where the sweep runs
it).  No pixel is compared here: the result is, per case, the fused-kernel records of the launch ledger that were hit and how often
-- differences of `_hk.build_ledger()`, never a reset, so the session ledger of tests/conftest.py is not disturbed.

tools/record_fit_builds.py writes the result of a tree to tests/golden/fit_build_choices.json; tests/test_gpu_fit_build_choices.py
holds the tree under test to that record.  Every (section, configuration) runs on a context of its own, so that what one call
leaves in the context (whether the last fit met r2-mask failures decides which planes the next one is handed) is the same
whatever ran before.
"""
import warnings

import numpy as np
import pytest

from _launch_env import launch_context
from homonim_amd import _hk
from test_gpu_build_sweep import CONFIGS, H, HEIGHTS, W, WIDTHS, _dev_job_corrected_only, _pair

BATCHED = [(0, None), (1, None), (1, '1')]   # (nodata variant, forced ring) of test_batched_builds_of_every_width_vs_oracle
BATCHED_CONFIG = ('gain-blk-offset', False, None, np.nan)   # the configuration their case ids are filed under


def config_id(model, find_r2, thresh, nodata):
    return f'{model} r2={int(find_r2)} thresh={thresh} nodata={nodata}'


def _short(name):
    return name.replace('fit_apply_kernel', 'apply').replace('fit_list_kernel', 'list')


class _Hits:
    """ the fused-kernel records hit between two readings of the ledger, in the record's short spelling (apply<...> / list<...>) """

    def __init__(self):
        self.last = _hk.build_ledger()

    def take(self):
        now = _hk.build_ledger()
        hits = {_short(k): v - self.last.get(k, 0) for k, v in now.items() if k.startswith('fit_') and v != self.last.get(k, 0)}
        self.last = now
        return dict(sorted(hits.items()))


def _run_shape(c, model, find_r2, thresh, nodata, kshape, src, ref):
    """ the launches of test_gpu_build_sweep._check_shape, without the oracle """
    open_rows = thresh is not None and kshape[0] in (3, 5, 9)
    if open_rows:
        ref = ref.copy()
        ref[18:23, 90:131] = np.random.default_rng(5).uniform(-3, -1, (5, 41)).astype(np.float32)
    desc = _hk.make_desc(model, kshape, find_r2, thresh, nodata, nodata)
    n_params = 3 if (find_r2 or thresh is not None) else 2
    c.fit_apply(desc, src, ref, n_params, want_params=True, want_corr=True)
    if not find_r2:
        c.fit_apply(desc, src, ref, n_params, want_params=False, want_corr=True)
        if open_rows:
            _dev_job_corrected_only(c, desc, src, ref)


def _batched(hits, out, nodata_variant, ring):
    with pytest.MonkeyPatch.context() as mp:   # (hk_ctx_create reads the switch)
        if ring is not None:
            mp.setenv('HK_USE_RING', ring)
        ctx = _hk.Context(0, n_streams=2)
    B, shapes = 2, [(H, W), (H - 7, W - 36)]
    nd = np.nan if nodata_variant else None
    stride = (W + 3) // 4 * 4
    plane = stride * H
    bufs = [{k: ctx.dev_alloc(4 * plane * B) for k in ('src', 'ref', 'corr')} for _ in shapes]
    norm = ctx.dev_alloc(16 * B * len(shapes))
    try:
        jobs = []
        for j, (h, w) in enumerate(shapes):
            ctx.synth_fill_dev(bufs[j]['src'], bufs[j]['ref'], B, h, w, stride, plane, seed=300 + j, nodata_variant=nodata_variant, stream=0)
            job = _hk.DevJob()
            job.src, job.ref, job.corr = bufs[j]['src'], bufs[j]['ref'], bufs[j]['corr']
            job.gain = job.offset = job.r2 = job.fail_count = None
            job.norm = norm + 16 * B * j
            job.n_bands, job.height, job.width, job.stride, job.band_stride = B, h, w, stride, plane
            job.seg_rows, job.stream = 0, 1
            jobs.append(job)
        ctx.stream_sync(0)
        arr = ctx.job_array(jobs)
        hits.take()
        for kh in ((1, 5, 7, 9, 11, 15, 17, 41) if ring is None else (5, 11)):
            for kw in WIDTHS + ((31, 33, 35, 37) if ring is None and kh in (5, 17) else ()):
                desc = _hk.make_desc('gain-blk-offset', (kh, kw), False, None, nd, nd)
                ctx.block_norm_batch_dev(desc, arr, norm)
                ctx.fit_apply_batch_dev(desc, arr)
                ctx.stream_sync(1)
                out[f'batched variant={nodata_variant} ring={ring} {kh}x{kw}'] = hits.take()
    finally:
        for d in bufs:
            for p in d.values():
                ctx.dev_free(p)
        ctx.dev_free(norm)
        ctx.close()


def choices(config) -> dict:
    """ {case id: {fused-kernel record: launches}} of one of CONFIGS """
    model, find_r2, thresh, nodata = config
    numeric = -3.0 if (nodata is not None and model != 'gain-blk-offset') else None
    sections = [('sweep', {}, 7, None, [(kh, kw) for kh in HEIGHTS for kw in WIDTHS]),
                ('paired', {}, 17, None, [(kh, kw) for kh in (3, 9, 17) for kw in (31, 33, 35, 37)])]
    for ring, heights in (('0', (5, 17)), ('1', (3, 11, 17)), ('2', (1, 5, 65)), ('3', (7, 11, 15))):
        sections.append((f'ring {ring}', {'HK_USE_RING': ring}, 11, numeric, [(kh, kw) for kh in heights for kw in WIDTHS]))
    if nodata is None:
        sections.append(('general', {'HK_FORCE_GENERAL': '1'}, 13, None, [(kh, kw) for kh in (3, 5, 9, 17) for kw in WIDTHS]))
    out, hits = {}, _Hits()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for section, env, seed, num, shapes in sections:
            src, ref = _pair(seed, nodata, num)
            nd = nodata if num is None else num
            base = _hk.Context(0, n_streams=1)
            try:
                with launch_context(base, env) as c:
                    hits.take()
                    for kh, kw in shapes:
                        if model == 'gain-offset' and kh * kw < 2:
                            continue
                        _run_shape(c, model, find_r2, thresh, nd, (kh, kw), src, ref)
                        out[f'{section} {kh}x{kw}'] = hits.take()
            finally:
                base.close()
        if config_id(*config) == config_id(*BATCHED_CONFIG):
            for nodata_variant, ring in BATCHED:
                _batched(hits, out, nodata_variant, ring)
    return out
