""" The device-resident entries on rasters whose bands, or rows, lie 2^32 + delta elements apart (tests/_far_layout.py): every
offset `plane + band * band_stride + y * stride + x` a kernel forms is then one that no 32-bit number holds, in elements and in
bytes.  Each case runs its entry once on a compact layout and once on every far layout it takes, and asserts, in this order,

  (a) the compact result meets the reference the entry's own test file uses (imported from there: nothing new is stated here);
  (b) every far result equals the compact one byte for byte;
  (c) the sum of the used arena's 32-bit words is the expected one: canary everywhere but on the inputs, which are unchanged, and
      on the expected output pixels.

A kernel that narrows an offset reads the canary or another array, or writes into the canary: (b) or (c) fails; by the choice of
the distance the access stays inside the arena (tests/test_far_layout_cpu.py).  'band' layouts have 2 bands F apart, 'row' layouts
one band of 3 rows F apart (2 rows for 8-byte samples); delta 'odd' leaves no far row or plane 16-byte aligned and is run wherever
the entry accepts such strides -- hk_dev_job, the casts and the in-painting demand strides that are multiples of 4 elements and
take the aligned delta only. """
import contextlib
import zlib

import numpy as np
import pytest

import _far_layout as fl
import _format_edges as fe
import _inpaint_masks as M
import _lzw_streams as lz
import _masked_tiffs as mt
import _resample_exact as rx
import _rotated_grids as rg
from homonim_amd import _hk
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

F32 = np.float32
BOTH = list(fl.DELTAS)          # 'aligned', 'odd'
ALIGNED = ['aligned']


@pytest.fixture(scope='module')
def ctx():
    """ a context of the module's own: the slot scratch the in-painting grows to at a stride of 2^23 goes when the module ends """
    c = _hk.Context(0, n_streams=2)
    yield c
    c.close()


@pytest.fixture(scope='module')
def arena(ctx):
    a = fl.Arena(ctx)   # (a failed allocation is an error of the tests that use it)
    try:
        yield a
    finally:
        a.free()


@pytest.fixture(scope='module')
def oc():
    from oracle import oracle_c
    assert oracle_c.available(), 'the oracle library is not built (python -m homonim_amd.build)'
    return oracle_c


def memset_now(ctx, dptr, value, nbytes):
    """ a fill that is over when this returns (hk_memset queues it on the device's default stream, which the context's own streams
    do not wait for) """
    ctx.memset(dptr, value, nbytes)
    ctx.sync()


@contextlib.contextmanager
def dev_bufs(ctx, *sizes):
    """ small device buffers outside the arena (statistics, streams, counters), zeroed """
    ptrs = []
    try:
        for n in sizes:
            ptrs.append(ctx.dev_alloc(max(int(n), 16)))
            memset_now(ctx, ptrs[-1], 0, max(int(n), 16))
        yield ptrs
    finally:
        for p in ptrs:
            ctx.dev_free(p)


class Placed:
    """ array k of a case: a (bands, h, w) raster of ``dtype`` laid out 'compact', 'band'-far or 'row'-far in the arena """

    def __init__(self, arena, kind, delta, k, shape, dtype, pitch=None, band_pad=0):
        self.arena, self.shape, self.dtype = arena, tuple(shape), np.dtype(dtype)
        self.lay = fl.Layout(kind, delta)
        pitch = shape[2] if pitch is None else pitch
        self.base = fl.slot(k, delta)
        self.stride, self.band_stride = self.lay.strides(shape[1], pitch, band_pad)
        self.ptr = arena.at(self.base, self.dtype.itemsize)
        self.end_bytes = self.lay.extent(k, shape, pitch, band_pad) * self.dtype.itemsize

    def put(self, arr):
        arr = np.asarray(arr).reshape(self.shape)
        assert arr.dtype == self.dtype
        self.arena.put(arr, self.base, self.stride, self.band_stride)

    def expect(self, arr):
        self.arena.expect(np.asarray(arr).reshape(self.shape).astype(self.dtype, copy=False), self.base, self.stride, self.band_stride)

    def get(self):
        return self.arena.get(self.shape, self.dtype, self.base, self.stride, self.band_stride)


def run(arena, ins, outs, launch, expected=None):
    """ One run of a case.  ``ins``: [(Placed, array)] uploaded; ``outs``: {name: Placed} read back afterwards (a Placed may be both:
    it is worked on in place); ``launch()`` queues the entry and waits, and may return more results.  ``expected``: the compact
    run's outputs -- what the model expects at the output pixels; without it (the compact run itself) the run's own outputs.
    -> (outputs, launch's results, the device's checksum, the expected one) """
    arena.begin(max(p.end_bytes for p in [p for p, _ in ins] + list(outs.values())))
    for p, arr in ins:
        p.put(arr)
    extra = launch()
    got = {name: p.get() for name, p in outs.items()}
    for name, p in outs.items():
        p.expect(got[name] if expected is None else expected[name])
    dev, want = arena.checksum()
    return got, extra, dev, want


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hold_far(what, compact, far):
    """ (b) and (c) of a far run against the compact one, and (c) of the compact run itself """
    got_c, extra_c, dev_c, want_c = compact
    got_f, extra_f, dev_f, want_f = far
    for name in got_c:
        assert same_bytes(got_f[name], got_c[name]), f'{what}: `{name}` differs from the compact run'
    if extra_c is not None:
        for x, y in zip(extra_f, extra_c):
            assert same_bytes(np.asarray(x), np.asarray(y)), f'{what}: a result outside the arena differs from the compact run'
    assert dev_f == want_f, f'{what}: arena checksum {dev_f:#x}, expected {want_f:#x}: bytes outside the expected pixels were written'


def hold_compact(what, compact):
    assert compact[2] == compact[3], f'{what}: compact run: arena checksum {compact[2]:#x}, expected {compact[3]:#x}'


def far_kinds(shape_band, shape_row, deltas):
    """ [(kind, delta name, shape)]: the far layouts of a case that has both strides """
    return [(kind, d, shape_band if kind == 'band' else shape_row) for kind in ('band', 'row') for d in deltas]


# ---- checksum_dev itself, first: the other cases rest on it -------------------------------------------------------------------------
def test_checksum_dev_over_the_whole_arena_and_over_a_far_window(ctx, arena):
    arena.begin(fl.ARENA_BYTES)
    n_words = fl.ARENA_BYTES // 4
    dev, want = arena.checksum()
    assert want == (n_words * fl.CANARY_WORD) % (1 << 64)
    assert dev == want, 'the canary-only arena'
    word = np.array([0x12345679], '<u4')
    ctx.h2d(arena.ptr + (1 << 34) + 4, word)
    arena.model.write((1 << 34) + 4, word)
    dev2, want2 = arena.checksum()
    assert (want2 - want) % (1 << 64) == (0x12345679 - fl.CANARY_WORD) % (1 << 64)
    assert dev2 == want2, 'one word changed at byte offset 2^34 + 4'
    rng = np.random.default_rng(1)
    for name, delta in fl.DELTAS.items():   # a window of 3 rows F apart holding known words
        rows = rng.integers(0, 1 << 32, (3, 70), dtype=np.uint64).astype('<u4')
        base = fl.slot(2 + list(fl.DELTAS).index(name), delta)   # (the slots of the two deltas coincide: one each)
        arena.put(rows.view(F32), base, fl.far(delta))
        got = ctx.checksum_dev(arena.at(base, 4), fl.far(delta), 3, 70)
        assert got == int(rows.sum(dtype=np.uint64)), f'far window, delta {name}'
    dev3, want3 = arena.checksum()
    assert dev3 == want3 != want2, 'the whole arena with the far windows in it'


# ---- compare_sums_dev and param_stats_dev ------------------------------------------------------------------------------------------
def _stat_planes(shape, nodata, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(1.0, 0.3, shape).astype(F32)
    hole = F32('nan') if np.isnan(nodata) else F32(nodata)
    a[:, 0, :7] = hole
    a[:, -1, 30:41] = hole
    a[rng.random(shape) < 0.1] = hole
    return a


@pytest.mark.parametrize('nodata', [float('nan'), -9999.0], ids=['nan', 'value'])
def test_param_stats_dev(ctx, arena, nodata):
    from test_gpu_stats import check_vector
    thresh = 0.9
    for kind, dname, shape in far_kinds((2, 5, 70), (1, 3, 70), BOTH):
        planes = _stat_planes(shape, nodata, seed=shape[1])
        nb, h, w = shape
        with dev_bufs(ctx, 80 * nb) as (d_stats,):
            def one(kind_, delta):
                p = Placed(arena, kind_, delta, 0, shape, F32, pitch=72, band_pad=8)

                def launch():
                    memset_now(ctx, d_stats, 0, 80 * nb)
                    ctx.param_stats_dev(p.ptr, nb, h, w, p.stride, p.band_stride, d_stats, nodata, thresh, stream=0)
                    ctx.stream_sync(0)
                    got = np.zeros((nb, 10))
                    ctx.d2h(got, d_stats)
                    return [got]
                return run(arena, [(p, planes)], {}, launch)
            compact = one('compact', fl.DELTAS[dname])
            for b in range(nb):
                check_vector(compact[1][0][b], planes[b], nodata, thresh, f'compact {shape} band {b}')
            hold_compact(f'param_stats {shape}', compact)
            hold_far(f'param_stats {kind}-far {dname}', compact, one(kind, fl.DELTAS[dname]))


def _job(**kw):
    job = _hk.DevJob()
    for k, v in kw.items():
        setattr(job, k, v)
    return job


@pytest.mark.parametrize('nodata', [float('nan'), -9999.0], ids=['nan', 'value'])
def test_compare_sums_dev(ctx, arena, nodata):
    from test_gpu_parity import _exact_compare_sums
    for kind, dname, shape in far_kinds((2, 5, 70), (1, 3, 70), ALIGNED):
        src = _stat_planes(shape, nodata, seed=11 + shape[1])
        ref = (0.7 * _stat_planes(shape, nodata, seed=12 + shape[1]) + 0.2).astype(F32)
        if not np.isnan(nodata):
            ref[0, 1, 3:9] = nodata
        nb, h, w = shape
        with dev_bufs(ctx, 56 * nb) as (d_sums,):
            def one(kind_, delta):
                ps, pr = (Placed(arena, kind_, delta, k, shape, F32, pitch=72, band_pad=8) for k in (0, 1))
                job = _job(src=ps.ptr, ref=pr.ptr, n_bands=nb, height=h, width=w, stride=ps.stride, band_stride=ps.band_stride)

                def launch():
                    memset_now(ctx, d_sums, 0, 56 * nb)
                    ctx.compare_sums_dev(job, nodata, nodata, d_sums)
                    ctx.stream_sync(0)
                    got = np.zeros((nb, 7))
                    ctx.d2h(got, d_sums)
                    return [got]
                return run(arena, [(ps, src), (pr, ref)], {}, launch)
            compact = one('compact', fl.DELTAS[dname])
            for b in range(nb):
                exp = _exact_compare_sums(src[b], nodata, ref[b], nodata)
                assert exp[6] > 0 and np.allclose(compact[1][0][b], exp, rtol=1e-12, atol=0), (shape, b, compact[1][0][b], exp)
            hold_compact(f'compare_sums {shape}', compact)
            hold_far(f'compare_sums {kind}-far {dname}', compact, one(kind, fl.DELTAS[dname]))


# ---- the fused fit ----------------------------------------------------------------------------------------------------------------
FIT_SHAPE, FIT_ROW_SHAPE, FIT_PITCH, FIT_W = (2, 37, 261), (1, 3, 261), 264, 261
# A lane of the fused kernel stores its four columns as one 16-byte word (rows are padded to quads: hk_dev_job's strides), so the
# quad that holds the last column is written to its end.  The output planes are therefore read back, compared and expected 264
# wide: the three columns behind the width hold whatever the compact run left there, and nothing else may differ.


def _fit_pair(shape, seed, variant, defect=False):
    srcs, refs = [], []
    for b in range(shape[0]):
        s, r = onp.synth_pair(shape[1], shape[2], seed + b, variant)
        r = r.copy()
        if defect and b == shape[0] - 1:   # what the fit cannot explain: pixels fail the r2 mask
            r[18:24, 100:112] = -3.0
            r[30, 200] = 9.0
        srcs.append(s), refs.append(r)
    return np.stack(srcs).astype(F32), np.stack(refs).astype(F32)


def _fit_run(ctx, arena, kind, delta, shape, desc, src, ref, outs, first_slot=0, norm=None, fail=None):
    """ places src, ref and the planes named in ``outs`` from slot ``first_slot`` on -> (job, ins, outs as {name: Placed}) """
    nb, h, w = shape
    names = ['src', 'ref'] + list(outs)
    p = {n: Placed(arena, kind, delta, first_slot + k, (nb, h, w if k < 2 else FIT_PITCH), F32, pitch=FIT_PITCH) for k, n in enumerate(names)}
    job = _job(src=p['src'].ptr, ref=p['ref'].ptr, n_bands=nb, height=h, width=w, stride=p['src'].stride,
               band_stride=p['src'].band_stride, stream=0, norm=norm, fail_count=fail)
    for n in outs:
        setattr(job, n, p[n].ptr)
    return job, [(p['src'], src), (p['ref'], ref)], {n: p[n] for n in outs}


def test_fit_apply_dev_gain_3x3(ctx, arena, oc):
    from test_gpu_parity import assert_close_ulp
    desc = _hk.make_desc('gain', (3, 3), False, None, np.nan, np.nan)
    for kind, dname, shape in far_kinds(FIT_SHAPE, FIT_ROW_SHAPE, ALIGNED):
        src, ref = _fit_pair(shape, 70, 'frame+holes' if kind == 'band' else 'none')

        def one(kind_):
            job, ins, outs = _fit_run(ctx, arena, kind_, fl.DELTAS[dname], shape, desc, src, ref, ['corr', 'gain', 'offset'])

            def launch():
                ctx.fit_apply_dev(desc, job)
                ctx.stream_sync(0)
            return run(arena, ins, outs, launch)
        compact = one('compact')
        for b in range(shape[0]):
            exp_params, exp_corr, _ = oc.fit_apply('gain', src[b], np.nan, ref[b], np.nan, (3, 3), False, None)
            assert_close_ulp(compact[0]['corr'][b][:, :FIT_W], exp_corr, f'gain 3x3 {shape} band {b} corrected')
            assert_close_ulp(np.stack([compact[0]['gain'][b][:, :FIT_W], compact[0]['offset'][b][:, :FIT_W]]), exp_params,
                             f'gain 3x3 {shape} band {b} params')
            assert np.isfinite(exp_corr).any()
        hold_compact(f'gain 3x3 {shape}', compact)
        hold_far(f'gain 3x3 {kind}-far', compact, one(kind))


def test_fit_apply_dev_gain_blk_offset_5x5_with_block_norm_dev_and_the_batched_entries(ctx, arena, oc):
    from test_gpu_parity import assert_close_ulp
    desc = _hk.make_desc('gain-blk-offset', (5, 5), False, None, np.nan, np.nan)
    delta = fl.DELTA_ALIGNED
    for kind, shape in (('band', FIT_SHAPE), ('row', FIT_ROW_SHAPE)):
        nb = shape[0]
        pairs = [_fit_pair(shape, 80 + 10 * j, 'frame+holes' if kind == 'band' else 'none') for j in range(2)]
        with dev_bufs(ctx, 16 * nb * 2) as (d_norm,):
            def one(kind_, batched):
                jobs, ins, outs = [], [], {}
                for j, (src, ref) in enumerate(pairs if batched else pairs[:1]):
                    job, i, o = _fit_run(ctx, arena, kind_, delta, shape, desc, src, ref, ['corr'], first_slot=3 * j,
                                         norm=d_norm + 16 * nb * j)
                    jobs.append(job), ins.extend(i), outs.update({f'corr{j}': o['corr']})

                def launch():
                    memset_now(ctx, d_norm, 0, 16 * nb * 2)
                    if batched:
                        arr = ctx.job_array(jobs)
                        ctx.block_norm_batch_dev(desc, arr, d_norm)
                        ctx.fit_apply_batch_dev(desc, arr)
                    else:
                        ctx.block_norm_dev(desc, jobs[0], jobs[0].norm)
                        ctx.fit_apply_dev(desc, jobs[0])
                    ctx.stream_sync(0)
                    norm = np.zeros((2, nb, 2))
                    ctx.d2h(norm, d_norm)
                    return [norm]
                return run(arena, ins, outs, launch)
            single, batch = one('compact', False), one('compact', True)
            for j, (src, ref) in enumerate(pairs):
                for b in range(nb):
                    norm = batch[1][0][j, b]
                    assert np.allclose(norm, oc.fit_block_norm(src[b], np.nan, ref[b], np.nan), rtol=2e-6, atol=1e-9), (kind, j, b, norm)
                    _, exp_corr, _ = oc.fit_apply('gain-blk-offset', src[b], np.nan, ref[b], np.nan, (5, 5), False, None, norm_model=norm,
                                                  want_params=False)
                    assert_close_ulp(batch[0][f'corr{j}'][b][:, :FIT_W], exp_corr, f'gain-blk-offset {shape} job {j} band {b}')
            # a job's statistics and corrected planes do not depend on the launch it travels in (tests/test_gpu_batch.py)
            assert same_bytes(single[0]['corr0'], batch[0]['corr0']) and same_bytes(single[1][0][0], batch[1][0][0])
            hold_compact(f'gain-blk-offset {shape}', single), hold_compact(f'gain-blk-offset batch {shape}', batch)
            hold_far(f'gain-blk-offset {kind}-far', single, one(kind, False))
            hold_far(f'gain-blk-offset batch {kind}-far', batch, one(kind, True))


def test_fit_apply_dev_gain_offset_5x5_r2_threshold_and_inpaint_dev(ctx, arena, oc):
    """ every output plane asked for, pixels that fail the r2 mask in the last band, hk_inpaint_dev behind the fit; the job carries
    no scratch (hk_dev_job_scratch_bytes spans the bands: 5 bytes per pixel of 2^32 of them).  Band-far only: the in-painting's own
    workspace is sized by height x stride. """
    from test_gpu_parity import assert_close_ulp
    desc = _hk.make_desc('gain-offset', (5, 5), True, 0.25, np.nan, np.nan)
    shape = FIT_SHAPE
    nb = shape[0]
    src, ref = _fit_pair(shape, 40, 'frame+holes', defect=True)
    with dev_bufs(ctx, 8 * nb) as (d_fail,):
        def one(kind_):
            job, ins, outs = _fit_run(ctx, arena, kind_, fl.DELTA_ALIGNED, shape, desc, src, ref, ['corr', 'gain', 'offset', 'r2'],
                                      fail=d_fail)

            def launch():
                memset_now(ctx, d_fail, 0, 8 * nb)
                ctx.fit_apply_dev(desc, job)
                ctx.stream_sync(0)
                counts = np.zeros(nb, np.uint64)
                ctx.d2h(counts, d_fail)
                n_fail = ctx.inpaint_dev(desc, job)
                ctx.stream_sync(0)
                return [counts, np.array([n_fail], np.uint64)]
            return run(arena, ins, outs, launch)
        compact = one('compact')
        total = 0
        for b in range(nb):
            exp_params, exp_corr, exp_fail = oc.fit_apply('gain-offset', src[b], np.nan, ref[b], np.nan, (5, 5), True, 0.25)
            total += exp_fail
            assert (exp_fail > 0) == (b == nb - 1) and int(compact[1][0][b]) == exp_fail
            assert_close_ulp(compact[0]['corr'][b][:, :FIT_W], exp_corr, f'band {b} corrected', max_frac=1e-3)
            got = np.stack([compact[0][n][b][:, :FIT_W] for n in ('gain', 'offset', 'r2')])
            assert_close_ulp(got, exp_params, f'band {b} params', max_frac=1e-3)
        assert int(compact[1][1][0]) == total
        hold_compact('gain-offset r2 in-painting', compact)
        hold_far('gain-offset r2 in-painting band-far', compact, one('band'))


# ---- the re-projections -------------------------------------------------------------------------------------------------------------
RS_SRC_SHAPE = (2, 24, 70)


def _rs_source():
    a = rx.source(RS_SRC_SHAPE[1:], np.nan)
    return np.stack([a, (-a * F32(1.5)).astype(F32)])


def _resample_case(ctx, arena, what, dst_shape, call, check):
    """ a re-sampler from a 2-band 24 x 70 source: compact, then source far / destination compact and the other way round, both
    deltas.  ``call(src Placed, dst Placed)`` queues the entry; ``check(band, plane)`` holds a compact plane to its reference. """
    src = _rs_source()
    d_shape = (2, *dst_shape)

    def one(src_kind, dst_kind, delta):
        ps = Placed(arena, src_kind, delta, 0, RS_SRC_SHAPE, F32, pitch=72, band_pad=8)
        pd = Placed(arena, dst_kind, delta, 1, d_shape, F32, pitch=dst_shape[1] + 3, band_pad=5)

        def launch():
            call(ps, pd)
            ctx.stream_sync(0)
        return run(arena, [(ps, src)], {'dst': pd}, launch)
    compact = one('compact', 'compact', fl.DELTA_ALIGNED)
    for b in range(2):
        check(src[b], compact[0]['dst'][b])
    hold_compact(what, compact)
    for dname, delta in fl.DELTAS.items():
        hold_far(f'{what}: source band-far {dname}', compact, one('band', 'compact', delta))
        hold_far(f'{what}: destination band-far {dname}', compact, one('compact', 'band', delta))


@pytest.mark.parametrize('method, mapping, dst_shape', [('average', (2., 0., 2., 0.), (12, 35)), ('cubic_spline', (.5, 0., .5, 0.), (48, 140)),
                                                        ('nearest', (1., .5, 1., .5), (24, 70))], ids=['average-2to1', 'cubic_spline-1to2', 'nearest'])
def test_reproject_dev(ctx, arena, method, mapping, dst_shape):
    code = onp.RESAMPLING_CODES[method]

    def call(ps, pd):
        ctx.reproject_dev(ps.ptr, 2, RS_SRC_SHAPE[1:], ps.stride, ps.band_stride, np.nan, mapping, code, pd.ptr, dst_shape, pd.stride,
                          pd.band_stride, np.nan)

    def check(src, got):
        rx.assert_held(rx.enclosure_failures(got, src, np.nan, mapping, dst_shape, method), f'reproject_dev {method}',
                       0.4 * dst_shape[0] * dst_shape[1])
    _resample_case(ctx, arena, f'reproject_dev {method}', dst_shape, call, check)


def test_reproject_crs_dev_bilinear(ctx, arena):
    from test_gpu_warp import small_case
    c = small_case('unit')   # (a 24 x 36 source grid: the 24 x 70 source overhangs it on the right, which the warp does not mind)
    sx, sy = ctx.warp_coords(c.warp, c.dst_shape)

    def call(ps, pd):
        ctx.reproject_crs_dev(c.warp, ps.ptr, 2, RS_SRC_SHAPE[1:], ps.stride, ps.band_stride, np.nan, c.scale, 1, pd.ptr, c.dst_shape,
                              pd.stride, pd.band_stride, np.nan)

    def check(src, got):
        inside = (sx >= 0) & (sx < RS_SRC_SHAPE[2]) & (sy >= 0) & (sy < RS_SRC_SHAPE[1])
        rx.assert_held(rx.enclosure_failures_at(got, src, np.nan, sx, sy, c.scale[0], c.scale[1], 'bilinear'), 'reproject_crs_dev',
                       0.3 * inside.sum())
    _resample_case(ctx, arena, 'reproject_crs_dev bilinear', c.dst_shape, call, check)


def test_reproject_affine_dev_bilinear_on_a_rotated_grid(ctx, arena):
    from test_gpu_rotated import WEB, Case, _centred
    src_tf = rg.rotated(254000., 6278000., 30., 30.)
    dst_shape = (40, 75)
    dst_tf = _centred(src_tf, 30., dst_shape, RS_SRC_SHAPE[1:])
    c = Case(WEB, src_tf, WEB, dst_tf, dst_shape, RS_SRC_SHAPE[1:])
    warp, scale = c.warp, c.scale
    sx, sy = ctx.warp_coords_affine(warp, dst_shape)
    nx, ny = rg.coords_np(src_tf, dst_tf, dst_shape, 0.5)
    assert np.array_equal(sx, nx) and np.array_equal(sy, ny)

    def call(ps, pd):
        ctx.reproject_affine_dev(warp, ps.ptr, 2, RS_SRC_SHAPE[1:], ps.stride, ps.band_stride, np.nan, scale, 1, pd.ptr, dst_shape,
                                 pd.stride, pd.band_stride, np.nan)

    def check(src, got):
        inside = (sx >= 0) & (sx < RS_SRC_SHAPE[2]) & (sy >= 0) & (sy < RS_SRC_SHAPE[1])
        assert inside.sum() > 0.3 * inside.size and (~inside).any()
        rx.assert_held(rx.enclosure_failures_at(got, src, np.nan, sx, sy, scale[0], scale[1], 'bilinear'), 'reproject_affine_dev',
                       0.3 * inside.sum())
    _resample_case(ctx, arena, 'reproject_affine_dev bilinear', dst_shape, call, check)


# ---- the coordinate planes: float64, 2 rows F apart -----------------------------------------------------------------------------------
def _coords_case(ctx, arena, what, entry, warp, check):
    shape = (1, 2, 70)

    def one(kind, delta):
        px, py = (Placed(arena, kind, delta, k, shape, np.float64, pitch=73) for k in (0, 1))
        assert px.stride == py.stride

        def launch():
            entry(warp, shape[1:], px.ptr, py.ptr, px.stride)
            ctx.stream_sync(0)
        return run(arena, [], {'x': px, 'y': py}, launch)
    compact = one('compact', fl.DELTA_ALIGNED)
    check(compact[0]['x'][0], compact[0]['y'][0])
    hold_compact(what, compact)
    for dname, delta in fl.DELTAS.items():
        hold_far(f'{what} row-far {dname}', compact, one('row', delta))


def test_warp_coords_affine_dev(ctx, arena):
    src_tf, dst_tf = rg.PAIRS['shear3-and-minus40deg-30m']
    warp = _hk.make_affine_warp_desc(None, src_tf, None, dst_tf)

    def check(gx, gy):
        nx, ny = rg.coords_np(src_tf, dst_tf, (2, 70), 0.5)
        assert np.array_equal(gx, nx) and np.array_equal(gy, ny), 'not the stated association'
    _coords_case(ctx, arena, 'warp_coords_affine_dev', ctx.warp_coords_affine_dev, warp, check)


def test_warp_coords_dev(ctx, arena):
    import _crs_mp
    from test_gpu_warp import BAR_M, COORD_PAIRS, M_PER_DEG, Case
    src_crs, src_tf, dst_crs, dst_tf = COORD_PAIRS['tm25-from-utm35s']
    c = Case(src_crs, src_tf, dst_crs, dst_tf, (2, 70))

    def check(gx, gy):
        rows, cols = np.mgrid[0:2, 0:70].astype(np.float64)
        X, Y = dst_tf.c + (cols + 0.5) * dst_tf.a, dst_tf.f + (rows + 0.5) * dst_tf.e
        exact = _crs_mp.transform_many(tuple(c.dst_def), tuple(c.src_def), X.ravel(), Y.ravel())
        with _crs_mp.mp.workdps(_crs_mp.DPS):
            exact_px = [((ex - src_tf.c) / src_tf.a, (ey - src_tf.f) / src_tf.e) for ex, ey in exact]
        m_per_unit = M_PER_DEG if c.src_def.is_geographic else 1.
        err = _crs_mp.max_error(gx.ravel(), gy.ravel(), exact_px, abs(src_tf.a) * m_per_unit, abs(src_tf.e) * m_per_unit)
        assert err < BAR_M, f'{err} m'
    _coords_case(ctx, arena, 'warp_coords_dev', ctx.warp_coords_dev, c.warp, check)


# ---- overviews -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32', 'float64'])
def test_overviews_dev(ctx, arena, dtype):
    from test_overviews_cpu import oracle_levels, overview_levels
    from test_gpu_overviews import assert_same_bits
    shape, n = (2, 9, 70), 3
    rng = np.random.default_rng(9)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        a = rng.normal(100.0, 30.0, shape).astype(dt)
        a[rng.random(shape) < 0.3] = np.nan
        nodata = float('nan')
    else:
        a = rng.integers(0, np.iinfo(dt).max, shape, dtype=dt, endpoint=True)
        a[rng.random(shape) < 0.3] = 0
        nodata = 0
    shapes = [(2, lh, lw) for lh, lw in _hk.overview_shapes(9, 70, n)]

    def one(src_kind, level1_kind, delta):
        ps = Placed(arena, src_kind, delta, 0, shape, dt, pitch=73, band_pad=5)
        pl = [Placed(arena, level1_kind if m == 0 else 'compact', delta, 1 + m, s, dt, pitch=s[2] + 5, band_pad=3) for m, s in enumerate(shapes)]

        def launch():
            ctx.overviews_dev(ps.ptr, dtype, 2, 9, 70, ps.stride, ps.band_stride, nodata, [p.ptr for p in pl], [p.stride for p in pl],
                              [p.band_stride for p in pl])
            ctx.stream_sync(0)
        return run(arena, [(ps, a)], {f'level{m + 1}': p for m, p in enumerate(pl)}, launch)
    compact = one('compact', 'compact', fl.DELTA_ALIGNED)
    for b in range(2):
        exp = oracle_levels(a[b], nodata, n) if dtype == 'float32' else overview_levels(a[b], nodata, n)
        for m in range(n):
            assert_same_bits(compact[0][f'level{m + 1}'][b], exp[m], f'{dtype} band {b} level {m + 1}')
    hold_compact(f'overviews {dtype}', compact)
    for dname, delta in fl.DELTAS.items():
        hold_far(f'overviews {dtype}: source band-far {dname}', compact, one('band', 'compact', delta))
        hold_far(f'overviews {dtype}: level 1 band-far {dname}', compact, one('compact', 'band', delta))


# ---- the dataset mask ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype, how', [('uint8', 'alpha'), ('uint16', 'bits'), ('float32', 'bits')])
def test_dataset_mask_dev(ctx, arena, dtype, how):
    """ planes band-far, the mask's rows F apart (bytes for the bits, elements for the alpha plane), the output band-far """
    from test_gpu_dataset_mask import mask_source, pixels, validity
    shape = (2, 3, 1100)   # two whole waves of 64 groups (the path that exchanges a wave's halves) and a part of one
    a = pixels(dtype, shape, seed=31)
    valid = validity('random', 3, 1100, seed=32)
    _, m = mask_source(how, valid, dtype, seed=33)
    exp = mt.masked_f32(a, valid)
    kind_code = _hk.MASK_BITS if how == 'bits' else _hk.MASK_ALPHA

    def one(plane_kind, mask_kind, delta):
        ps = Placed(arena, plane_kind, delta, 0, shape, a.dtype, pitch=1104, band_pad=16)
        pm = Placed(arena, mask_kind, delta, 1, (1, *m.shape), m.dtype, pitch=m.shape[1] + 3)
        po = Placed(arena, plane_kind, delta, 2, shape, F32, pitch=1104, band_pad=16)

        def launch():
            ctx.dataset_mask_dev(ps.ptr, dtype, 2, 3, 1100, ps.stride, ps.band_stride, pm.ptr, kind_code, pm.stride, po.ptr, po.stride,
                                 po.band_stride)
            ctx.stream_sync(0)
        return run(arena, [(ps, a), (pm, m)], {'out': po}, launch)
    compact = one('compact', 'compact', fl.DELTA_ALIGNED)
    assert mt.same_bytes(compact[0]['out'], exp), f'hk_dataset_mask_dev {dtype} {how}'
    hold_compact(f'dataset_mask {dtype} {how}', compact)
    for dname, delta in fl.DELTAS.items():
        hold_far(f'dataset_mask {dtype} {how} far {dname}', compact, one('band', 'row', delta))


# ---- DEFLATE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype, predictor', [('uint8', 1), ('uint16', 1), ('float32', 1), ('uint8', 2), ('uint16', 2), ('float32', 3)])
def test_deflate_tiles_dev(ctx, arena, dtype, predictor):
    from test_gpu_deflate import raw_tiles
    from test_out_profile_cpu import predicted_tiles
    shape, tile = (2, 20, 40), 16
    rng = np.random.default_rng(17)
    a = np.round(rng.normal(100, 30, shape)).astype(dtype)
    a[:, :, :13] = 0
    raws = raw_tiles(a, tile) if predictor == 1 else predicted_tiles(a, tile, predictor)
    n_tiles, cap = _hk.deflate_bound(dtype, *shape, tile)
    assert n_tiles == len(raws) == 2 * 2 * 3
    with dev_bufs(ctx, cap, 8 * (n_tiles + 1), 8 * n_tiles) as (d_out, d_off, d_siz):
        def one(kind, delta):
            ps = Placed(arena, kind, delta, 0, shape, a.dtype, pitch=43, band_pad=7)

            def launch():
                memset_now(ctx, d_out, 0, cap)
                ctx.deflate_tiles_dev(ps.ptr, dtype, *shape, ps.stride, ps.band_stride, tile, d_out, cap, d_off, d_siz, stream=0,
                                      predictor=predictor)
                ctx.stream_sync(0)
                off, siz, out = np.empty(n_tiles + 1, np.int64), np.empty(n_tiles, np.int64), np.empty(cap, np.uint8)
                ctx.d2h(off, d_off), ctx.d2h(siz, d_siz), ctx.d2h(out, d_out)
                return [off, siz, out[:off[-1]].copy()]
            return run(arena, [(ps, a)], {}, launch)
        compact = one('compact', fl.DELTA_ALIGNED)
        off, siz, out = compact[1]
        for t, raw in enumerate(raws):
            d = zlib.decompressobj()
            assert d.decompress(out[off[t]:off[t] + siz[t]].tobytes()) == raw and d.eof, f'tile {t} does not inflate to its bytes'
        hold_compact(f'deflate {dtype} predictor {predictor}', compact)
        for dname, delta in fl.DELTAS.items():
            hold_far(f'deflate {dtype} predictor {predictor} band-far {dname}', compact, one('band', delta))


# ---- INFLATE and LZW -----------------------------------------------------------------------------------------------------------------
BLOCK_LAYOUTS = [   # (layout of tests/_lzw_streams.py, far kind): the smallest tiled and stripped ones, and one-band ones of 3 rows
    (lz.LAYOUTS[8], 'band'),                                                     # tiles16-separate-u32: 2 bands 33 x 31
    (lz.LAYOUTS[6], 'band'),                                                     # strips-contig3-u8: 3 bands 41 x 29
    (lz.Layout('tiles16-u16-3rows', 'u2', 1, 3, 45, 16, 0, 0, 1), 'row'),
    (lz.Layout('strips2-u8-3rows-pred2', 'u1', 1, 3, 29, 0, 2, 0, 2), 'row'),
]


def _blocks_case(ctx, arena, what, entry, lay, kind, streams, pixels):
    from homonim_amd.tiff import BlockLayout
    bl = BlockLayout(*lz.block_layout(lay))
    n_blocks, _, work_bytes = _hk.inflate_bound(bl)
    assert n_blocks == len(streams)
    buf, offsets, sizes = _hk._pack_streams(streams)
    shape = pixels.shape
    with dev_bufs(ctx, buf.nbytes, offsets.nbytes, sizes.nbytes, work_bytes, 4 * n_blocks) as (d_buf, d_off, d_siz, d_work, d_st):
        ctx.h2d(d_buf, buf), ctx.h2d(d_off, offsets), ctx.h2d(d_siz, sizes)

        def one(kind_, delta):
            po = Placed(arena, kind_, delta, 0, shape, pixels.dtype, pitch=shape[2] + 7, band_pad=5)

            def launch():
                memset_now(ctx, d_st, 0xff, 4 * n_blocks)
                entry(bl, d_buf, d_off, d_siz, d_work, po.ptr, po.stride, po.band_stride, d_st, stream=0)
                ctx.stream_sync(0)
                status = np.empty(n_blocks, np.int32)
                ctx.d2h(status, d_st)
                return [status]
            return run(arena, [], {'out': po}, launch)
        compact = one('compact', fl.DELTA_ALIGNED)
        assert not compact[1][0].any()
        assert compact[0]['out'].tobytes() == pixels.tobytes(), f'{what}: not the pixels the streams were made from'
        hold_compact(what, compact)
        for dname, delta in fl.DELTAS.items():
            if kind == 'band' and shape[0] > 2 and pixels.dtype.itemsize > 1:
                continue
            hold_far(f'{what} {kind}-far {dname}', compact, one(kind, delta))


@pytest.mark.parametrize('lay, kind', BLOCK_LAYOUTS, ids=[lay.name for lay, _ in BLOCK_LAYOUTS])
def test_inflate_image_dev(ctx, arena, lay, kind):
    a = lz.layout_array(lay)
    streams = [zlib.compress(b, 6) for b in lz.raw_blocks(a, lay)]
    _blocks_case(ctx, arena, f'inflate_image_dev {lay.name}', ctx.inflate_image_dev, lay, kind, streams, a)


@pytest.mark.parametrize('lay, kind', BLOCK_LAYOUTS, ids=[lay.name for lay, _ in BLOCK_LAYOUTS])
def test_lzw_image_dev(ctx, arena, lay, kind):
    a, streams = lz.layout_streams(lay)
    _blocks_case(ctx, arena, f'lzw_image_dev {lay.name}', ctx.lzw_image_dev, lay, kind, streams, a)


# ---- the casts: 3 x 1025, rows F apart on both sides ----------------------------------------------------------------------------------
@pytest.mark.parametrize('to_typed', [False, True], ids=['cast_in', 'cast_out'])
@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'float64'])
def test_cast_plane_dev(ctx, arena, dtype, to_typed):
    """ Both kernels work on whole groups of four columns (tests/test_gpu_format_edges.py): the rows are 1028 wide here, the last
    three columns the zero padding of the source and its conversion, zero. """
    from test_gpu_format_edges import _fill, _same
    rows = 2 if dtype == 'float64' else 3   # (three float64 rows F apart do not fit the arena)
    w, w4 = 1025, 1028
    if to_typed:
        fam = fe.cast_out_families(dtype)
        vals = _fill(np.concatenate(list(fam.values())), (rows, w), 17).astype(F32)
        nodata = fe.held_nodata(dtype)[0]
        exp = fe.cast_out_exact(vals, dtype, nodata)
        src_dt, dst_dt = F32, np.dtype(dtype)
        has, value = _hk.out_nodata_code(dtype, nodata)
    else:
        vals = _fill(fe.cast_in_family(dtype), (rows, w), 19).astype(dtype)
        exp = fe.cast_in_exact(vals, dtype)
        src_dt, dst_dt = np.dtype(dtype), F32
        has, value = False, 0.0
    padded = np.zeros((1, rows, w4), src_dt)
    padded[0, :, :w] = vals

    def one(kind, delta):
        ps = Placed(arena, kind, delta, 0, padded.shape, src_dt, pitch=w4 + 60)
        pd = Placed(arena, kind, delta, 1, padded.shape, dst_dt, pitch=w4 + 60)

        def launch():
            ctx.cast_plane_dev(to_typed, dtype, ps.ptr, ps.stride, pd.ptr, pd.stride, rows, w, has, value)
        return run(arena, [(ps, padded)], {'dst': pd}, launch)
    compact = one('compact', fl.DELTA_ALIGNED)
    got = compact[0]['dst'][0]
    _same(np.ascontiguousarray(got[:, :w]), exp, f'cast {dtype} to_typed {to_typed}')
    assert not got[:, w:].view(np.uint8).any(), 'the padding inside the last group of four is not zero'
    hold_compact(f'cast {dtype} to_typed {to_typed}', compact)
    hold_far(f'cast {dtype} to_typed {to_typed} row-far', compact, one('row', fl.DELTA_ALIGNED))


# ---- the synthetic fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', [0, 1])
def test_synth_fill_dev(ctx, arena, variant):
    """ (the fill has no reference of its own in the suite: the far runs are held to the compact one) """
    shape = (2, 37, 261)

    def one(kind, delta):
        ps, pr = (Placed(arena, kind, delta, k, shape, F32, pitch=264, band_pad=8) for k in (0, 1))

        def launch():
            ctx.synth_fill_dev(ps.ptr, pr.ptr, *shape, ps.stride, ps.band_stride, seed=7, nodata_variant=variant, stream=0)
            ctx.stream_sync(0)
        return run(arena, [], {'src': ps, 'ref': pr}, launch)
    compact = one('compact', fl.DELTA_ALIGNED)
    src, ref = compact[0]['src'], compact[0]['ref']
    assert np.isnan(src).any() == (variant == 1) and np.isfinite(src[:, 3:-3, 3:-3]).mean() > 0.99 and not same_bytes(src[0], src[1])
    assert np.isfinite(ref[:, 3:-3, 3:-3]).mean() > 0.99 and not same_bytes(src, ref)
    hold_compact(f'synth_fill {variant}', compact)
    for dname, delta in fl.DELTAS.items():
        hold_far(f'synth_fill {variant} band-far {dname}', compact, one('band', delta))


# ---- the in-painting step across the stride at which the packed search is left out ---------------------------------------------------
def test_inpaint_plane_dev_across_the_stride_limit_of_the_packed_search(ctx, arena, oc):
    """ 70 x 300 at strides 2^23 - 4, 2^23 and 2^23 + 4 (70 rows then span 2.2 GiB): all three give the compact bytes and those of
    the run with the packed search off, and the ledger shows inpaint_fill_fast_kernel launched below 2^23 only. """
    from test_gpu_inpaint_exact import _same
    h, w = 70, 300
    img, flags = M._image((h, w), 5), M._random_flags((h, w), 0.1, 6)
    exp = oc.fill_nodata(img, flags == 1)
    assert (flags == 0).sum() > 0.5 * h * w

    def fast_launches():
        return sum(n for b, n in _hk.build_ledger().items() if 'inpaint_fill_fast_kernel' in b)

    def one(stride, mode):
        pb, fb = 0, fl.slot(1, fl.DELTA_ALIGNED)   # the plane at the base, the flags (bytes) behind its first row
        arena.begin(max(((h - 1) * stride + w) * 4, fb + (h - 1) * stride + w))
        arena.put(img, pb, stride)
        arena.put(flags, fb, stride)
        before = fast_launches()
        ctx.inpaint_plane_dev(arena.at(pb, 4), arena.at(fb, 1), None, None, 0.0, h, w, stride, mode)
        launched = fast_launches() - before
        got = arena.get((1, h, w), F32, pb, stride)[0]
        return got, launched

    def held(stride, mode, want):
        got, launched = one(stride, mode)
        if want is not None:
            assert same_bytes(got, want), f'stride {stride} mode {mode}: differs from the compact run'
            for y in range(h):   # the plane is worked on in place: its expected bytes replace the input's
                arena.model.write((y * stride) * 4, want[y])
            dev, model = arena.checksum()
            assert dev == model, f'stride {stride} mode {mode}: arena checksum {dev:#x}, expected {model:#x}'
        return got, launched
    compact, launched = held(w, 0, None)
    _same(compact, exp, img, flags, 'compact, mode 0')
    assert launched == 1
    general, launched = held(w, 3, compact)
    assert launched == 0
    for stride in ((1 << 23) - 4, 1 << 23, (1 << 23) + 4):
        _, launched = held(stride, 0, compact)
        assert launched == (1 if stride < (1 << 23) else 0), f'stride {stride}: inpaint_fill_fast_kernel launched {launched} times'
        _, launched = held(stride, 3, compact)
        assert launched == 0
