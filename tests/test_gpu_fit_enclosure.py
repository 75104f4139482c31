"""
The fused fit + apply on the GPU against the enclosures of oracle/exact_window.py: exact window sums and sound bounds for any
row-segment partition and any order of the horizontal combination, propagated through the contract's expressions (DESIGN.md
section 2).  On data where the float64 sums are inexact (bright outliers, six decades of dynamic range, saturated DN pixels,
subnormal float32 products) every parameter and corrected pixel must lie inside its enclosure, and match it bit for bit wherever
the enclosure is a single value; the r2-mask failure count must lie between the certain and the possible failures.
"""
import numpy as np
import pytest

from oracle import exact_window as ew

pytestmark = pytest.mark.gpu

from _launch_env import launch_context  # noqa: E402
from homonim_amd import _hk  # noqa: E402

H, W = 160, 600
SHAPES = [(1, 1), (3, 3), (5, 5), (3, 7), (7, 3), (15, 15), (31, 31)]
UNDECIDED = {}


@pytest.fixture(scope='module')
def ctx():
    c = _hk.default_context()
    c.selftest()
    return c


@pytest.fixture(scope='module')
def oc():
    from homonim_amd import build
    build.build_oracle(verbose=False)
    from oracle import oracle_c
    return oracle_c


def _pair(kind, shape, nodata, seed):
    src, ref = ew.raster_pair(kind, shape, seed)
    if nodata is not None:                       # a NaN frame with holes
        rng = np.random.default_rng(seed + 1)
        for a in (src, ref):
            a[:2], a[-2:], a[:, :3], a[:, -3:] = np.nan, np.nan, np.nan, np.nan
            a[rng.random(shape) < 0.002] = np.nan
        src[40:44, 100:130] = np.nan
    return src, ref


def _assert_in(iv, got, sel, what):
    bad = ~iv.contains(got) & sel
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f'{what}: {int(bad.sum())} outside the enclosure, e.g. ({y}, {x}) got {got[y, x]!r} in '
                             f'[{iv.lo[y, x]!r}, {iv.hi[y, x]!r}] und={bool(iv.und[y, x])}')


def check(enc, params, corr, what, thresh=None, n_fail=None, oc=None, src=None):
    """ params / corr (either may be None) of one launch against the enclosure; with a threshold: the count, the first-pass values
    where the r2 mask certainly passes, R2 everywhere, and -- where nothing is undecided -- the in-painting (GDAL's fill of the
    launch's own offsets, kernel_model.py:366-371) """
    everywhere = np.ones(enc.mask.shape, bool)
    sel = everywhere
    if thresh is not None:
        d = ew.decide(enc, thresh)
        n_cf, n_und = int(d.certain_fail.sum()), int(d.undecided.sum())
        assert n_cf <= n_fail <= n_cf + n_und, f'{what}: n_fail {n_fail} outside [{n_cf}, {n_cf + n_und}]'
        sel = ~d.certain_fail & ~d.undecided
        UNDECIDED.setdefault(what.split()[0], []).append(d.undecided_fraction())
    if params is not None:
        for i in range(params.shape[0]):
            _assert_in(enc.params[i], params[i], everywhere if i == 2 else sel, f'{what}: param {i}')
    if corr is not None:
        _assert_in(enc.corr, corr, sel, f'{what}: corrected')
    if thresh is not None and params is not None and n_fail and not d.undecided.any():
        redo = d.certain_fail
        o_fill = oc.fill_nodata(params[1], d.certain_pass)
        assert (o_fill[redo].view(np.uint32) == params[1][redo].view(np.uint32)).all(), f'{what}: in-painted offsets'
        g_iv, c_iv = ew.redo_gain(enc, params[1], src)
        _assert_in(g_iv, params[0], redo, f'{what}: gain of failing pixels')
        if corr is not None:
            _assert_in(c_iv, corr, redo, f'{what}: corrected failing pixels')


def _fit(ctx, model, kshape, find_r2, thresh, nodata, src, ref, norm=None, want_params=True):
    desc = _hk.make_desc(model, kshape, find_r2, thresh, nodata, nodata)
    n = 3 if (find_r2 or thresh is not None) else 2
    params, corr, _, n_fail = ctx.fit_apply(desc, src, ref, n, want_params=want_params, want_corr=True, norm_in=norm)
    return params, corr, n_fail


def _run_all_models(ctx, oc, kind, kshape, nodata, src, ref, thresholds=(0.25, 0.9)):
    what = f'{kind} {kshape} nodata={nodata}'
    # gain
    enc = ew.enclose('gain', src, nodata, ref, nodata, kshape, True)
    for find_r2 in (False, True):
        p, c, _ = _fit(ctx, 'gain', kshape, find_r2, None, nodata, src, ref)
        check(enc, p, c, f'{what} gain r2={find_r2}')
    # gain-blk-offset with injected statistics (with R2: normalised pixels; without: the normalised window sum)
    norm = oc.fit_block_norm(src, nodata, ref, nodata)
    for find_r2 in (False, True):
        enc = ew.enclose('gain-blk-offset', src, nodata, ref, nodata, kshape, find_r2, None, norm)
        p, c, _ = _fit(ctx, 'gain-blk-offset', kshape, find_r2, None, nodata, src, ref, norm)
        check(enc, p, c, f'{what} gain-blk-offset r2={find_r2}')
    # gain-offset: parameters with and without R2, then the r2 mask through the parameter path and the corrected-only path
    if kshape == (1, 1):
        return
    enc = ew.enclose('gain-offset', src, nodata, ref, nodata, kshape, True)
    for find_r2 in (False, True):
        p, c, _ = _fit(ctx, 'gain-offset', kshape, find_r2, None, nodata, src, ref)
        check(enc, p, c, f'{what} gain-offset r2={find_r2}')
    for t in thresholds:
        p, c, n_fail = _fit(ctx, 'gain-offset', kshape, False, t, nodata, src, ref)
        check(enc, p, c, f'{kind} {kshape} nodata={nodata} gain-offset thresh={t}', t, n_fail, oc, src)
        _, c_only, n_only = _fit(ctx, 'gain-offset', kshape, False, t, nodata, src, ref, want_params=False)
        check(enc, None, c_only, f'{kind} {kshape} nodata={nodata} gain-offset thresh={t} (corrected only)', t, n_only, oc, src)
        if not ew.decide(enc, t).undecided.any():
            assert n_only == n_fail
            assert (c_only.view(np.uint32) == c.view(np.uint32)).all(), f'{what} thresh={t}: certificate vs parameter path'


def _cases():
    for i, kind in enumerate(ew.KINDS):
        for j, kshape in enumerate(sorted({(5, 5), SHAPES[i % len(SHAPES)], SHAPES[(i + 3) % len(SHAPES)]})):
            yield pytest.param(kind, kshape, [None, np.nan][(i + j) % 2], id=f'{kind}-{kshape[0]}x{kshape[1]}')


@pytest.mark.oracle
@pytest.mark.parametrize('kind, kshape, nodata', list(_cases()))
def test_fit_lies_in_its_enclosure(ctx, oc, kind, kshape, nodata):
    """ Every model, R2 on and off, thresholds None / 0.25 / 0.9, parameter and corrected-only paths. """
    src, ref = _pair(kind, (H, W), nodata, seed=len(kind) + kshape[0])
    _run_all_models(ctx, oc, kind, kshape, nodata, src, ref)
    for k, v in UNDECIDED.items():
        if k == kind:
            print(f'undecided fraction of {kind}: max {max(v):.2e} over {len(v)} r2-mask decisions')


VARIANTS = [('ring0', {'HK_USE_RING': '0'}), ('ring1', {'HK_USE_RING': '1'}), ('ring2', {'HK_USE_RING': '2'}),
            ('ring3', {'HK_USE_RING': '3'}), ('general', {'HK_FORCE_GENERAL': '1'}),
            ('segments-a', {'HK_WAVE_SLOTS': '4', 'HK_SEG_BIG': '96', 'HK_SEG_TAIL': '8'}),
            ('segments-b', {'HK_WAVE_SLOTS': '4', 'HK_SEG_BIG': '40', 'HK_SEG_TAIL': '16'})]


@pytest.mark.oracle
@pytest.mark.parametrize('kind, kshape', [('bright-65535', (5, 5)), ('bright-1e4', (15, 15)), ('dn-saturated', (9, 11))])
@pytest.mark.parametrize('variant', [v[0] for v in VARIANTS])
def test_launch_variants_lie_in_the_enclosure(ctx, oc, kind, kshape, variant):
    """ Ring modes, the NaN-aware builds on dense rasters and two segment policies on rasters tall enough for several row
    segments: the running sums restart elsewhere, the enclosure holds all the same. """
    src, ref = _pair(kind, (420, 300), None, seed=5)
    with launch_context(ctx, dict(VARIANTS)[variant]) as c:
        _run_all_models(c, oc, f'{kind}/{variant}', kshape, None, src, ref, thresholds=(0.25,))


def _dev_plane(c, arr, stride, d, name):
    h, w = arr.shape
    d[name] = c.dev_alloc(4 * stride * h)
    c.h2d(d[name], np.pad(arr, ((0, 0), (0, stride - w))).astype(np.float32))
    return d[name]


@pytest.mark.oracle
def test_device_resident_and_batched_entries_lie_in_the_enclosure(ctx, oc):
    """ hk_fit_apply_dev (gain-offset, r2 mask, parameter planes: the first pass before any in-painting) and
    hk_fit_apply_batch_dev (gain-blk-offset, two jobs with injected statistics) on inexact data. """
    h, w = 200, 520
    stride = (w + 63) // 64 * 64
    src, ref = _pair('bright-65535', (h, w), np.nan, seed=9)
    src2, ref2 = _pair('log-uniform', (h, w), np.nan, seed=10)
    d = {}
    try:
        job = _hk.DevJob()
        job.src, job.ref = _dev_plane(ctx, src, stride, d, 'src'), _dev_plane(ctx, ref, stride, d, 'ref')
        for k in ('gain', 'offset', 'r2', 'corr'):
            setattr(job, k, _dev_plane(ctx, np.zeros((h, w), np.float32), stride, d, k))
        d['fail'] = ctx.dev_alloc(8)
        ctx.memset(d['fail'], 0, 8)
        job.fail_count, job.norm = d['fail'], None
        job.n_bands, job.height, job.width, job.stride, job.band_stride = 1, h, w, stride, stride * h
        job.seg_rows, job.stream = 0, 0
        desc = _hk.make_desc('gain-offset', (5, 5), False, 0.25, np.nan, np.nan)
        ctx.fit_apply_dev(desc, job)
        ctx.stream_sync(0)
        out = {}
        for k in ('gain', 'offset', 'r2', 'corr'):
            a = np.empty((h, stride), np.float32)
            ctx.d2h(a, d[k])
            out[k] = a[:, :w].copy()
        cnt = np.zeros(1, np.uint64)
        ctx.d2h(cnt, d['fail'])
        enc = ew.enclose('gain-offset', src, np.nan, ref, np.nan, (5, 5), True)
        dec = ew.decide(enc, 0.25)
        n_cf, n_und = int(dec.certain_fail.sum()), int(dec.undecided.sum())
        assert n_cf <= int(cnt[0]) <= n_cf + n_und
        params = np.stack([out['gain'], out['offset'], out['r2']])
        check(enc, params, out['corr'], 'bright-65535 device job')      # (first pass: every pixel, no in-painting yet)
        ctx.inpaint_dev(desc, job)
        ctx.stream_sync(0)

        # two gain-blk-offset jobs in one batched launch, their statistics injected through job.norm
        norms = [oc.fit_block_norm(s, np.nan, r, np.nan) for s, r in ((src, ref), (src2, ref2))]
        d['norm'] = ctx.dev_alloc(32)
        ctx.h2d(d['norm'], np.concatenate(norms).astype(np.float64))
        jobs = []
        for i, (s, r) in enumerate(((src, ref), (src2, ref2))):
            j = _hk.DevJob()
            j.src, j.ref = _dev_plane(ctx, s, stride, d, f'bs{i}'), _dev_plane(ctx, r, stride, d, f'br{i}')
            j.corr = _dev_plane(ctx, np.zeros((h, w), np.float32), stride, d, f'bc{i}')
            j.gain = j.offset = j.r2 = j.fail_count = None
            j.norm = d['norm'] + 16 * i
            j.n_bands, j.height, j.width, j.stride, j.band_stride = 1, h, w, stride, stride * h
            j.seg_rows, j.stream = 0, 0
            jobs.append(j)
        bdesc = _hk.make_desc('gain-blk-offset', (7, 7), False, None, np.nan, np.nan)
        ctx.fit_apply_batch_dev(bdesc, jobs)
        ctx.stream_sync(0)
        for i, (s, r) in enumerate(((src, ref), (src2, ref2))):
            a = np.empty((h, stride), np.float32)
            ctx.d2h(a, d[f'bc{i}'])
            enc = ew.enclose('gain-blk-offset', s, np.nan, r, np.nan, (7, 7), False, None, norms[i])
            check(enc, None, a[:, :w], f'batched gain-blk-offset job {i}')
    finally:
        for v in d.values():
            ctx.dev_free(v)

