""" RasterFuse.process and RasterCompare.process across two grids, held to the references of tests/_process_blocks.py -- every
comparison on the bits, NaN equal to NaN, no tolerance.

(1) Closed form (reference (B)): model gain, kernel (1, 1), a source of ones, a reference of position codes, `nearest` up-sampling:
    every corrected pixel and every gain is a code that says where it came from, so a block written a pixel off, clipped wrongly,
    read with the wrong fill, given the wrong transform or put in the wrong plane shows.  Threads 1 and 4, two ranks (round-robin
    and contiguous), a caller's ``corr_out``, uint16 output.
(2) Placement with real kernels (reference (A)): ``process`` against one ``fit_apply`` per block that the test makes itself through
    the helper's own reader, transforms and placement: gain 5 x 5, gain-blk-offset 3 x 7, gain-offset 5 x 5 in-painting; mask_partial
    off and on; both proc_crs; NaN, numeric and absent nodata; uint16 and uint8 rasters; three source bands under a five-band
    reference.  (The single-block calls are held to the oracle by test_gpu_refspace_exact.py / test_gpu_srcspace.py.)
(3) RasterCompare: with `nearest` both ways the seven sums of every partition and thread count equal the whole-image sums in integer
    arithmetic; with the default re-sampling ``process`` equals the block-order accumulation of ``Context.compare_sums`` over windows the
    helper cut and re-projected through the public ``RasterArray.reproject``.
(4) The rasters ``fit_apply`` returns: count, dtype, nodata, transform and shape of the corrected block and of the parameters, for the
    three model classes on one grid and across two.

Shapes: at most 72 x 38 and 62 x 102 reference pixels under 70 x 90 and 24 x 40 source pixels, 16 blocks per band.  The last test
prints the file's total time and its slowest test. """
import time
import warnings

import numpy as np
import pytest

import _process_blocks as pb
from conftest import assert_same_f32
from homonim_amd import CRS, KernelModel, Model, RasterArray, RasterCompare, RasterFuse, RefSpaceModel, SrcSpaceModel, _hk
from homonim_amd.enums import Resampling
from homonim_amd.geo import Affine

pytestmark = pytest.mark.gpu

TIMES = {}


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


@pytest.fixture(scope='module')
def ctx():
    c = _hk.default_context()
    c.selftest()
    return c


def _fuse(case, src, ref, src_nodata=float('nan'), ref_nodata=float('nan')):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # proc_crs=src on a finer source is "not recommended"
        return RasterFuse(src.copy(), ref.copy(), src_nodata=src_nodata, ref_nodata=ref_nodata, proc_crs=case.proc_crs, crs=CRS(),
                          transform=case.src_tf, ref_transform=case.ref_tf)


def _process(rf, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # the small-block ConfigWarning
        return rf.process(**kw)


# -- 1: the closed form ----------------------------------------------------------------------------------------------------------
def _closed_form_run(case_name, threads=1, bands=(1, 1), **kw):
    case = pb.CASES[case_name]
    src, ref = pb.closed_form_pair(case_name, *bands)
    rf = _fuse(case, src, ref)
    assert rf.proc_crs.name == case.proc_crs
    mem = pb.block_mem(case_name, (1, 1))
    assert len(pb.blocks_of(case, 1, (1, 1), mem)) >= 9
    return _process(rf, model=Model.gain, kernel_shape=(1, 1), model_config=pb.CLOSED_FORM_CONFIG[case.proc_crs],
                    block_config=dict(threads=threads, max_block_mem=mem), **kw)


def _assert_closed_form_params(case_name, params, n_src=1):
    _, exp_gain = pb.closed_form_expected(case_name, n_src)
    assert params.shape == (3 * n_src, *exp_gain.shape[-2:])          # the gains, the offsets, the r2 of the bands
    assert_same_f32(params[:n_src], exp_gain, f'{case_name} gains')
    assert_same_f32(params[n_src:2 * n_src], np.where(np.isnan(exp_gain), np.nan, 0).astype(np.float32), f'{case_name} offsets')


@pytest.mark.oracle
@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_process_meets_the_closed_form(ctx, case_name, threads):
    corr, params = _closed_form_run(case_name, threads, param_filename=True)
    exp_corr, _ = pb.closed_form_expected(case_name)
    assert_same_f32(corr, exp_corr, f'{case_name} corrected')
    _assert_closed_form_params(case_name, params)


@pytest.mark.oracle
@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('case_name', ['3x-ref', '2.5x-ref', '12-under-30-src'])
def test_two_bands_under_three_meet_the_closed_form_in_their_own_planes(ctx, case_name, threads):
    """ two source bands against a three-band reference whose codes run on from band to band: a parameter plane in another band's
    slot, or a band corrected against the wrong reference band, shows """
    corr, params = _closed_form_run(case_name, threads, bands=(2, 3), param_filename=True)
    exp_corr, _ = pb.closed_form_expected(case_name, 2)
    assert_same_f32(corr, exp_corr, f'{case_name} corrected')
    _assert_closed_form_params(case_name, params, 2)


@pytest.mark.oracle
@pytest.mark.parametrize('contiguous', [False, True], ids=['round-robin', 'contiguous'])
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_two_ranks_fill_their_own_blocks_and_together_the_closed_form(ctx, case_name, contiguous):
    case = pb.CASES[case_name]
    exp_corr, exp_gain = pb.closed_form_expected(case_name)
    bps = pb.blocks_of(case, 1, (1, 1), pb.block_mem(case_name, (1, 1)))
    union_corr = np.full(exp_corr.shape, np.nan, np.float32)
    union_gain = np.full(exp_gain.shape[-2:], np.nan, np.float32)
    for rank in range(2):
        corr, params = _closed_form_run(case_name, 1, param_filename=True,
                                        device_config=dict(rank=rank, world_size=2, contiguous=contiguous))
        own = pb.written_mask(case, pb.own_shard(bps, rank, 2, contiguous))
        assert own.any() and not own.all()
        assert np.isnan(corr[0][~own]).all(), f'rank {rank} wrote outside its blocks'
        assert_same_f32(corr[0][own], exp_corr[0][own], f'{case_name} rank {rank}')
        assert not (np.isfinite(union_corr[0]) & np.isfinite(corr[0])).any()
        union_corr[0][own] = corr[0][own]
        union_gain[np.isfinite(params[0])] = params[0][np.isfinite(params[0])]
    assert_same_f32(union_corr, exp_corr, f'{case_name} union')
    assert_same_f32(union_gain, exp_gain[0], f'{case_name} union of the gains')


@pytest.mark.oracle
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_corr_out_and_uint16_output_meet_the_closed_form(ctx, case_name):
    exp_corr, _ = pb.closed_form_expected(case_name)
    # a caller's array, not pre-filled by process: every source pixel is written, so nothing of the sentinel stays
    mine = np.full(exp_corr.shape, -7., np.float32)
    corr, params = _closed_form_run(case_name, 4, corr_out=mine)
    assert corr is mine and params is None
    assert_same_f32(mine, exp_corr, f'{case_name} corr_out')
    # uint16 with nodata 0: the codes fit
    assert np.nanmax(exp_corr) < 65535
    exp16 = np.where(np.isnan(exp_corr), 0, exp_corr).astype(np.uint16)
    corr16, params = _closed_form_run(case_name, 1, param_filename=True, out_profile=dict(dtype='uint16', nodata=0))
    assert corr16.dtype == np.uint16 and np.array_equal(corr16, exp16)
    _assert_closed_form_params(case_name, params)


# -- 2: placement with real kernels ------------------------------------------------------------------------------------------------
MODELS = {
    'gain': (Model.gain, (5, 5), {}),
    'gain-blk-offset': (Model.gain_blk_offset, (3, 7), {}),
    'gain-offset-inpaint': (Model.gain_offset, (5, 5), dict(r2_inpaint_thresh=0.25)),
}


def _placement_cases():
    """ (id, case, model, mask_partial, nodata key, bands (source, reference), typed, parameters asked) """
    cases, k = [], {'ref': 0, 'src': 0}
    for model in MODELS:
        for mp in (False, True):
            for ni, nd in enumerate(pb.NODATA):
                for proc, names in (('ref', pb.REF_CASES), ('src', pb.SRC_CASES)):
                    name = names[k[proc] % len(names)]
                    k[proc] += 1
                    cases.append((name, model, mp, nd, (1, 1), None, bool((mp * 3 + ni) % 2)))
    for name in ('2.5x-ref', '2.5x-src'):    # edge blocks read beyond the source, interior blocks do not (test_process_blocks_cpu.py)
        cases.append((name, 'gain-blk-offset', name.endswith('src'), 'numeric', (1, 1), 'uint16', name.endswith('ref')))
        cases.append((name, 'gain', name.endswith('ref'), 'none', (1, 1), 'uint8', name.endswith('src')))
    cases.append(('3x-ref', 'gain-blk-offset', False, 'nan', (3, 5), None, True))
    cases.append(('12-under-30-src', 'gain-offset-inpaint', True, 'nan', (3, 5), None, True))
    return cases


def _placement_id(c):
    name, model, mp, nd, bands, typed, want = c
    return '-'.join([name, model, 'partial' if mp else 'whole', nd, typed or 'float32', f'{bands[0]}of{bands[1]}', 'params' if want else 'corr'])


_expected = {}


def _placement_setup(c):
    name, model_key, mp, nd, (n_src, n_ref), typed, want = c
    case = pb.CASES[name]
    model, kernel, config = MODELS[model_key]
    src, ref = pb.kernel_pair(name, nd, n_src, n_ref, typed)
    nodata = pb.NODATA[nd]
    out_profile = dict(dtype='uint16', nodata=0) if typed == 'uint16' else dict(dtype='float32', nodata=float('nan'))
    overlap = tuple(-(-k // 2) for k in kernel)
    mem = pb.block_mem(name, overlap)
    return case, model, kernel, dict(config, mask_partial=mp), src, ref, nodata, out_profile, overlap, mem


def _placement_expected(c):
    if c not in _expected:
        name, model_key, mp, nd, (n_src, n_ref), typed, want = c
        case, model, kernel, config, src, ref, nodata, out_profile, overlap, mem = _placement_setup(c)
        bps = pb.blocks_of(case, n_src, overlap, mem)
        assert len(bps) >= 9 * n_src
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            km = (RefSpaceModel if case.proc_crs == 'ref' else SrcSpaceModel)(model, kernel, find_r2=want, **config)
        _expected[c] = pb.expected_by_blocks(src, ref, nodata, nodata, case.src_tf, case.ref_tf, case.proc_crs, bps,
                                             pb.model_block_fn(km, want, out_profile['dtype'], out_profile['nodata']),
                                             n_param=3 if want else 0, out_dtype=out_profile['dtype'], out_nodata=out_profile['nodata'])
    return _expected[c]


@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('c', _placement_cases(), ids=_placement_id)
def test_process_equals_its_blocks_placed_by_the_helper(ctx, c, threads):
    name, model_key, mp, nd, (n_src, n_ref), typed, want = c
    case, model, kernel, config, src, ref, nodata, out_profile, overlap, mem = _placement_setup(c)
    exp_corr, exp_params = _placement_expected(c)
    rf = _fuse(case, src, ref, nodata, nodata)
    corr, params = _process(rf, model=model, kernel_shape=kernel, param_filename=True if want else None, model_config=config,
                            out_profile=out_profile, block_config=dict(threads=threads, max_block_mem=mem))
    assert corr.dtype == exp_corr.dtype and corr.shape == exp_corr.shape == (n_src, *case.src_shape)
    assert np.array_equal(corr, exp_corr, equal_nan=corr.dtype.kind == 'f')
    if want:
        assert params.shape == (3 * n_src, *(case.ref_shape if case.proc_crs == 'ref' else case.src_shape))
        assert_same_f32(params, exp_params, 'parameters')
        assert np.isfinite(params[:n_src]).any()
        # the band offsets matter: no two planes are alike (bands under one model that has offsets, or one band's three parameters)
        if n_src == 1 or model_key != 'gain':
            assert len({params[i].tobytes() for i in range(params.shape[0])}) == params.shape[0]
        if model_key == 'gain-offset-inpaint' and not mp:
            r2 = params[2 * n_src:]
            assert (r2[np.isfinite(r2)] < 0.25).any(), 'no pixel failed the r2 mask: the in-painting did not run'
    else:
        assert params is None and exp_params is None
    valid = np.isfinite(corr) if corr.dtype.kind == 'f' else corr != out_profile['nodata']
    assert valid.mean() > (0.2 if mp else 0.8)


# -- 3: RasterCompare ----------------------------------------------------------------------------------------------------------------
COMPARE_CASES = [('2.5x-ref', 'ref'), ('3x-ref', 'ref'), ('2x-aligned-ref', 'ref'), ('x-only-ref', 'ref'), ('12-under-30-src', 'src'),
                 ('2.5x-src', 'src')]


def _compare(case_name, proc_crs):
    case = pb.CASES[case_name]
    src, ref = pb.compare_pair(case_name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RasterCompare(src.copy(), ref.copy(), proc_crs=proc_crs, crs=CRS(), transform=case.src_tf, ref_transform=case.ref_tf)


def _accumulate_block_sums(rc, ctx, config):
    acc = dict.fromkeys(pb.onp.COMPARE_KEYS, 0.)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bps = list(rc.block_pairs(max_block_mem=config['max_block_mem']))
    for bp in bps:
        for k, v in rc._block_sums(bp, ctx, config).items():
            acc[k] += v
    return acc, len(bps)


@pytest.mark.oracle
@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('at_least', [1, 4, 9])
@pytest.mark.parametrize('case_name, proc_crs', COMPARE_CASES)
def test_compare_sums_of_every_partition_equal_the_whole_image(ctx, case_name, proc_crs, at_least, threads):
    exact = pb.compare_exact_sums(case_name, proc_crs)
    rc = _compare(case_name, proc_crs)
    config = dict(threads=threads, max_block_mem=pb.compare_mem(case_name, proc_crs, at_least), upsampling=Resampling.nearest,
                  downsampling=Resampling.nearest)
    acc, n_blocks = _accumulate_block_sums(rc, ctx, rc.create_config(**config))
    assert n_blocks == 1 if at_least == 1 else n_blocks >= at_least
    assert acc == exact, f'{n_blocks} blocks'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        stats = rc.process(**config)
    exp = pb.band_stats(**exact)
    assert stats['Ref. band 1'] == exp and stats['Mean'] == exp
    assert 0 < exp['r2'] < 1 and exp['rmse'] > 0 and exp['n'] > 100


@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('case_name, proc_crs', COMPARE_CASES)
def test_compare_with_default_resampling_equals_its_blocks(ctx, case_name, proc_crs, threads):
    def through_reproject(arr, nodata, tf, dst_tf, dst_shape, down):
        ra = RasterArray(np.ascontiguousarray(arr, dtype=np.float32), CRS(), tf, nodata=nodata)
        return ra.reproject(transform=dst_tf, shape=dst_shape, resampling=Resampling.average if down else Resampling.cubic_spline,
                            context=ctx).array

    def sums(s, s_nd, r, r_nd):
        return ctx.compare_sums(np.ascontiguousarray(s, dtype=np.float32), s_nd, np.ascontiguousarray(r, dtype=np.float32), r_nd)

    mem = pb.compare_mem(case_name, proc_crs, 9)
    exp = pb.band_stats(**pb.compare_by_blocks(case_name, proc_crs, mem, through_reproject, sums))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        stats = _compare(case_name, proc_crs).process(threads=threads, max_block_mem=mem)
    assert stats['Ref. band 1'] == exp
    assert exp['n'] > 100 and 0 < exp['r2'] < 1


# -- 4: the rasters fit_apply returns ------------------------------------------------------------------------------------------------
WRAP_SRC_TF = Affine(1., 0., 100., 0., -1., 200.)      # 24 x 24 source pixels of 1.0
WRAP_REF_TF = Affine(2., 0., 100., 0., -2., 200.)      # 12 x 12 reference pixels of 2.0 over them
WRAP_CASES = [(KernelModel, 'same')] + [(cls, grid) for cls in (RefSpaceModel, SrcSpaceModel) for grid in ('same', 'two')]


@pytest.mark.parametrize('out_dtype, out_nodata', [('float32', float('nan')), ('uint16', 0)])
@pytest.mark.parametrize('model_cls, grid', WRAP_CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_fit_apply_returns_rasters_with_the_stated_profiles(ctx, model_cls, grid, out_dtype, out_nodata):
    """ the corrected block: one band of the output dtype and nodata on the source block's grid; the parameters: gain and offset,
    float32 with NaN nodata, on the reference block's grid for RefSpaceModel across two grids and on the source block's otherwise """
    rng = np.random.default_rng(7)
    src = rng.uniform(50, 150, (24, 24)).astype(np.float32)
    ref_shape, ref_tf = ((24, 24), WRAP_SRC_TF) if grid == 'same' else ((12, 12), WRAP_REF_TF)
    ref = rng.uniform(60, 180, ref_shape).astype(np.float32)
    km = model_cls(Model.gain, (3, 3))
    corr_ra, param_ra = km.fit_apply(RasterArray(src, CRS(), WRAP_SRC_TF), RasterArray(ref, CRS(), ref_tf), want_params=True,
                                     out_dtype=out_dtype, out_nodata=out_nodata)
    assert (corr_ra.count, corr_ra.dtype, corr_ra.transform, corr_ra.shape) == (1, out_dtype, WRAP_SRC_TF, (24, 24))
    assert corr_ra.array.dtype == np.dtype(out_dtype) and corr_ra.profile['dtype'] == out_dtype and corr_ra.profile['count'] == 1
    assert corr_ra.nodata == 0 if out_dtype == 'uint16' else np.isnan(corr_ra.nodata)
    on_ref = model_cls is RefSpaceModel and grid == 'two'
    assert (param_ra.count, param_ra.dtype) == (2, 'float32') and np.isnan(param_ra.nodata)
    assert param_ra.profile['count'] == 2 and param_ra.profile['dtype'] == 'float32'
    assert (param_ra.transform, param_ra.shape) == ((WRAP_REF_TF, (12, 12)) if on_ref else (WRAP_SRC_TF, (24, 24)))
    assert param_ra.array.shape == (2, *param_ra.shape) and np.isfinite(param_ra.array).any()
    assert (np.isfinite(corr_ra.array) if out_dtype == 'float32' else corr_ra.array != 0).any()


# -- timings ---------------------------------------------------------------------------------------------------------------------
def test_zz_print_timings():
    if TIMES:
        slowest = max(TIMES, key=TIMES.get)
        print(f'[process-blocks] {len(TIMES)} tests in {sum(TIMES.values()):.1f} s; slowest: {slowest} {TIMES[slowest]:.2f} s')
        assert TIMES[slowest] < 10, f'{slowest} took {TIMES[slowest]:.1f} s'
