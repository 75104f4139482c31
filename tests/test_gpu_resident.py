""" ``RasterFuse.process`` on device-resident rasters (``device_config`` ``resident=True``, homonim_amd/resident.py) and the two
kernels it adds -- every comparison on the bits, no tolerance anywhere.

(1) ``fill_planes_kernel<T>``: every sample type, planes on a stride inside poisoned memory, against ``numpy.full``; padding and
    guards keep the poison.
(2) ``boundless_window_kernel<T>``: every sample type, no / NaN / numeric nodata, windows inside, overhanging, larger than, touching
    and missing the raster, against ``read_window`` of tests/_process_blocks.py (dtype included); guards keep the poison.
(3) Both kernels at uint8 with the bands 2^32 + 4096 elements apart, in an arena as tests/test_gpu_far_planes.py builds it.
(4) The closed form, reference (B) of tests/_process_blocks.py, met by the resident route: threads, bands, ranks, ``corr_out``.
(5) Resident equals default: arrays of real-kernel runs, byte for byte.
(6) ... and the ``.tif`` files with their overviews and masks.
(7) No device allocation outlives a resident ``process``, returned or raised.
(8) Rasters that do not fit the free memory are refused with both sizes and nothing is launched. """
import filecmp
import warnings

import numpy as np
import pytest

import _far_layout as fl
import _process_blocks as pb
from conftest import assert_same_f32
from homonim_amd import CRS, Model, RasterFuse, RefSpaceModel, SrcSpaceModel, _hk
from homonim_amd.fuse import default_devices
from homonim_amd.geo import Affine, Window
from homonim_amd.resident import window_inside

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DTYPES = list(_hk.DTYPE_CODES)
POISON = 0xA5


@pytest.fixture(scope='module')
def ctx():
    c = _hk.get_context(default_devices()[0])
    c.selftest()
    return c


class Poisoned:
    """ a device buffer of ``n`` elements of ``dtype`` whose every byte is the poison, and its host picture """

    def __init__(self, ctx, dtype, n):
        self.ctx, self.dtype = ctx, np.dtype(dtype)
        self.host = np.full(n * self.dtype.itemsize, POISON, np.uint8)
        self.dptr = ctx.dev_alloc(self.host.nbytes)
        ctx.h2d(self.dptr, self.host)

    def at(self, elem):
        return self.dptr + elem * self.dtype.itemsize

    def place(self, planes, lead, stride, band_stride):
        """ the picture after `planes` (bands, h, w) were written at element `lead` on the strides """
        view = self.host.view(self.dtype)
        for b in range(planes.shape[0]):
            for y in range(planes.shape[1]):
                o = lead + b * band_stride + y * stride
                view[o:o + planes.shape[2]] = planes[b, y]

    def download(self):
        got = np.empty_like(self.host)
        self.ctx.d2h(got, self.dptr)
        return got

    def free(self):
        self.ctx.dev_free(self.dptr)


def _extremes(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        info = np.finfo(dtype)
        return [float('nan'), 0., float(info.max), float(info.min)]
    info = np.iinfo(dtype)
    return [0, int(info.max), int(info.min)]


# -- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_fill_planes_equals_numpy_full_and_leaves_padding_and_guards(ctx, dtype):
    nb, h, w, stride, lead = 2, 19, 45, 48, 1
    band_stride = h * stride + 7
    for value in _extremes(dtype):
        buf = Poisoned(ctx, dtype, lead + nb * band_stride + 64)
        try:
            ctx.fill_planes_dev(buf.at(lead), dtype, nb, h, w, stride, band_stride, value)
            ctx.stream_sync(0)
            buf.place(np.full((nb, h, w), value, dtype), lead, stride, band_stride)
            assert buf.download().tobytes() == buf.host.tobytes(), f'{dtype} {value!r}'
        finally:
            buf.free()
    if np.dtype(dtype).kind != 'f':     # a value the type does not hold is refused, NaN included
        for bad in (float('nan'), float(np.iinfo(dtype).max) + 1, 0.5):
            with pytest.raises(ValueError):
                ctx.fill_planes_dev(0x1000, dtype, 1, 1, 1, 1, 1, bad)


# -- 2 ---------------------------------------------------------------------------------------------------------------------------------
RASTER = (2, 37, 53)
RASTER_STRIDE = 56
WINDOWS = {                                     # (row_off, col_off, height, width)
    'inside': (5, 7, 20, 30),
    'over-top-left': (-3, -5, 20, 30),
    'over-bottom-right': (20, 30, 37 - 20 + 4, 53 - 30 + 2),
    'larger': (-2, -3, 37 + 5, 53 + 7),
    'one-row': (36, 10, 5, 20),
    'outside': (40, 60, 6, 9),
    'outside-above': (-9, -20, 5, 8),
}


def _raster_of(dtype, seed=3):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        arr = (rng.normal(0., 1e3, RASTER) * (1 + 1e-7 * rng.normal(size=RASTER))).astype(dtype)   # float64: values float32 rounds
        arr[:, 4, 9] = np.nan
    else:
        info = np.iinfo(dtype)
        arr = rng.integers(info.min, info.max, RASTER, dtype=dtype, endpoint=True)
    return arr


@pytest.mark.parametrize('dtype', DTYPES)
def test_boundless_window_equals_the_helpers_reader(ctx, dtype):
    arr = _raster_of(dtype)
    nb, h, w = RASTER
    band_stride = h * RASTER_STRIDE + 3
    src = Poisoned(ctx, dtype, 1 + nb * band_stride)
    src.place(arr, 1, RASTER_STRIDE, band_stride)
    ctx.h2d(src.dptr, src.host)
    nodatas = [None, 7] + ([float('nan')] if np.dtype(dtype).kind == 'f' else [])
    try:
        for nodata in nodatas:
            raster = _hk.DeviceRaster(src.at(1), dtype, RASTER, RASTER_STRIDE, band_stride, nodata=nodata)
            for name, (r0, c0, wh, ww) in WINDOWS.items():
                exp = [pb.read_window(arr[b], nodata, Window(c0, r0, ww, wh)) for b in range(nb)]
                exp_arr = np.stack([e[0] for e in exp])
                stride, lead = ww + 3, 2
                out_band = wh * stride + 5
                out = Poisoned(ctx, exp_arr.dtype, lead + nb * out_band + 32)
                try:
                    got = ctx.boundless_window_dev(raster, (r0, c0, wh, ww), out.at(lead), stride, out_band)
                    ctx.stream_sync(0)
                    what = f'{dtype} nodata {nodata!r} window {name}'
                    assert got.dtype == exp_arr.dtype and got.shape == exp_arr.shape, what
                    exp_nd = exp[0][1]
                    assert (got.nodata is None and exp_nd is None) or got.nodata == exp_nd or (got.nodata != got.nodata and exp_nd != exp_nd), what
                    out.place(exp_arr, lead, stride, out_band)
                    assert out.download().tobytes() == out.host.tobytes(), what
                finally:
                    out.free()
    finally:
        src.free()


# -- 3 ---------------------------------------------------------------------------------------------------------------------------------
FAR = (1 << 32) + 4096


@pytest.fixture(scope='module')
def arena(ctx):
    a = fl.Arena(ctx, FAR + (64 << 20))
    try:
        yield a
    finally:
        a.free()


def test_fill_planes_on_bands_2_32_apart(ctx, arena):
    nb, h, w, stride, base = 2, 19, 45, 48, 1
    arena.begin(base + FAR + h * stride)
    ctx.fill_planes_dev(arena.at(base, 1), 'uint8', nb, h, w, stride, FAR, 201)
    ctx.stream_sync(0)
    arena.expect(np.full((nb, h, w), 201, np.uint8), base, stride, FAR)
    assert np.array_equal(arena.get((nb, h, w), np.uint8, base, stride, FAR), np.full((nb, h, w), 201, np.uint8))
    dev, want = arena.checksum()
    assert dev == want, 'bytes outside the filled pixels were written: an index was narrowed'


def test_boundless_window_on_bands_2_32_apart(ctx, arena):
    arr = _raster_of('uint8', seed=5)
    nb, h, w = RASTER
    r0, c0, wh, ww = WINDOWS['larger']
    out_base, out_stride = 1 << 16, ww + 3
    arena.begin(out_base + FAR + wh * out_stride)
    arena.put(arr, 0, RASTER_STRIDE, FAR)
    raster = _hk.DeviceRaster(arena.at(0, 1), 'uint8', RASTER, RASTER_STRIDE, FAR, nodata=9)
    ctx.boundless_window_dev(raster, (r0, c0, wh, ww), arena.at(out_base, 1), out_stride, FAR)
    ctx.stream_sync(0)
    exp = np.stack([pb.read_window(arr[b], 9, Window(c0, r0, ww, wh))[0] for b in range(nb)])
    assert exp.dtype == np.uint8 and len({exp[0].tobytes(), exp[1].tobytes()}) == 2
    assert np.array_equal(arena.get(exp.shape, np.uint8, out_base, out_stride, FAR), exp)
    arena.expect(exp, out_base, out_stride, FAR)
    dev, want = arena.checksum()
    assert dev == want, 'bytes outside the window were written: an index was narrowed'


# -- 4 ---------------------------------------------------------------------------------------------------------------------------------
def _fuse(case, src, ref, src_nodata=float('nan'), ref_nodata=float('nan')):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RasterFuse(src.copy(), ref.copy(), src_nodata=src_nodata, ref_nodata=ref_nodata, proc_crs=case.proc_crs, crs=CRS(),
                          transform=case.src_tf, ref_transform=case.ref_tf)


def _process(rf, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return rf.process(**kw)


def _closed_form_run(case_name, threads=1, bands=(1, 1), device_config=None, **kw):
    case = pb.CASES[case_name]
    src, ref = pb.closed_form_pair(case_name, *bands)
    rf = _fuse(case, src, ref)
    mem = pb.block_mem(case_name, (1, 1))
    return _process(rf, model=Model.gain, kernel_shape=(1, 1), model_config=pb.CLOSED_FORM_CONFIG[case.proc_crs],
                    block_config=dict(threads=threads, max_block_mem=mem), device_config=dict(device_config or {}, resident=True), **kw)


def _assert_closed_form_params(case_name, params, n_src=1):
    _, exp_gain = pb.closed_form_expected(case_name, n_src)
    assert params.shape == (3 * n_src, *exp_gain.shape[-2:])
    assert_same_f32(params[:n_src], exp_gain, f'{case_name} gains')
    assert_same_f32(params[n_src:2 * n_src], np.where(np.isnan(exp_gain), np.nan, 0).astype(np.float32), f'{case_name} offsets')


@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_resident_process_meets_the_closed_form(ctx, case_name, threads):
    corr, params = _closed_form_run(case_name, threads, param_filename=True)
    assert_same_f32(corr, pb.closed_form_expected(case_name)[0], f'{case_name} corrected')
    _assert_closed_form_params(case_name, params)


@pytest.mark.parametrize('threads', [1, 4])
def test_resident_two_bands_under_three_meet_the_closed_form(ctx, threads):
    corr, params = _closed_form_run('2.5x-ref', threads, bands=(2, 3), param_filename=True)
    assert_same_f32(corr, pb.closed_form_expected('2.5x-ref', 2)[0], 'corrected')
    _assert_closed_form_params('2.5x-ref', params, 2)


@pytest.mark.parametrize('contiguous', [False, True], ids=['round-robin', 'contiguous'])
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_resident_ranks_fill_their_own_blocks_and_together_the_closed_form(ctx, case_name, contiguous):
    case = pb.CASES[case_name]
    exp_corr, exp_gain = pb.closed_form_expected(case_name)
    bps = pb.blocks_of(case, 1, (1, 1), pb.block_mem(case_name, (1, 1)))
    union_corr = np.full(exp_corr.shape, np.nan, np.float32)
    union_gain = np.full(exp_gain.shape[-2:], np.nan, np.float32)
    for rank in range(2):
        corr, params = _closed_form_run(case_name, 1, param_filename=True, device_config=dict(rank=rank, world_size=2, contiguous=contiguous))
        own = pb.written_mask(case, pb.own_shard(bps, rank, 2, contiguous))
        assert own.any() and not own.all()
        assert np.isnan(corr[0][~own]).all(), f'rank {rank} wrote outside its blocks'
        assert_same_f32(corr[0][own], exp_corr[0][own], f'{case_name} rank {rank}')
        assert not (np.isfinite(union_corr[0]) & np.isfinite(corr[0])).any()
        union_corr[0][own] = corr[0][own]
        union_gain[np.isfinite(params[0])] = params[0][np.isfinite(params[0])]
    assert_same_f32(union_corr, exp_corr, f'{case_name} union')
    assert_same_f32(union_gain, exp_gain[0], f'{case_name} union of the gains')


@pytest.mark.parametrize('case_name', ['3x-ref', '12-under-30-src'])
def test_resident_runs_of_some_of_the_bands_put_their_parameters_in_their_own_planes(ctx, case_name):
    """ three bands in two contiguous shards: each rank holds blocks with two of the three bands, whose parameters go band by band """
    from homonim_amd.fuse import group_block_calls
    case = pb.CASES[case_name]
    exp_corr, exp_gain = pb.closed_form_expected(case_name, 3)
    bps = pb.blocks_of(case, 3, (1, 1), pb.block_mem(case_name, (1, 1)))
    union_corr, union_gain = np.full(exp_corr.shape, np.nan, np.float32), np.full(exp_gain.shape, np.nan, np.float32)
    for rank in range(2):
        assert any(c.n_bands == 2 for c in group_block_calls(pb.own_shard(bps, rank, 2, True)))
        corr, params = _closed_form_run(case_name, 4, bands=(3, 3), param_filename=True,
                                        device_config=dict(rank=rank, world_size=2, contiguous=True))
        assert not (np.isfinite(union_corr) & np.isfinite(corr)).any()
        union_corr[np.isfinite(corr)] = corr[np.isfinite(corr)]
        union_gain[np.isfinite(params[:3])] = params[:3][np.isfinite(params[:3])]
        offsets = params[3:6]
        assert (offsets[np.isfinite(offsets)] == 0).all() and (np.isfinite(offsets) == np.isfinite(params[:3])).all()
    assert_same_f32(union_corr, exp_corr, f'{case_name} union')
    assert_same_f32(union_gain, exp_gain, f'{case_name} union of the gains')


@pytest.mark.parametrize('contiguous', [False, True], ids=['round-robin', 'contiguous'])
@pytest.mark.parametrize('case_name', ['3x-ref', '2.5x-src'])
def test_resident_corr_out_keeps_its_sentinel_outside_the_ranks_blocks(ctx, case_name, contiguous):
    """ two source bands, so that a contiguous shard holds runs of some, not all, bands """
    case = pb.CASES[case_name]
    exp_corr, _ = pb.closed_form_expected(case_name, 2)
    bps = pb.blocks_of(case, 2, (1, 1), pb.block_mem(case_name, (1, 1)))
    for rank in range(2):
        mine = np.full(exp_corr.shape, -7., np.float32)
        corr, params = _closed_form_run(case_name, 4, bands=(2, 2), corr_out=mine,
                                        device_config=dict(rank=rank, world_size=2, contiguous=contiguous))
        assert corr is mine and params is None
        shard = pb.own_shard(bps, rank, 2, contiguous)
        for b in range(2):
            own = pb.written_mask(case, [bp._replace(band_i=0) for bp in shard if bp.band_i == b])
            assert (mine[b][~own] == -7.).all(), f'rank {rank} band {b}: the sentinel did not survive outside the blocks'
            assert_same_f32(mine[b][own], exp_corr[b][own], f'rank {rank} band {b}')


# -- 5 ---------------------------------------------------------------------------------------------------------------------------------
MODELS = {
    'gain': (Model.gain, (5, 5), {}),
    'gain-blk-offset': (Model.gain_blk_offset, (3, 7), {}),
    'gain-offset-r2': (Model.gain_offset, (5, 5), dict(r2_inpaint_thresh=0.25)),
}
RASTERS = {'uint8-none': ('uint8', 'none'), 'uint16-numeric': ('uint16', 'numeric'), 'float32-nan': (None, 'nan')}
OUTPUTS = {'float32-nan': (dict(dtype='float32', nodata=float('nan')), False), 'uint8-0': (dict(dtype='uint8', nodata=0), False),
           'int16-none-valid': (dict(dtype='int16', nodata=None), True)}
EQUAL_RUNS = [                                   # (pair, model, mask_partial, rasters, output, threads)
    ('2.5x-ref', 'gain', False, 'uint8-none', 'float32-nan', 1),
    ('3x-ref', 'gain-blk-offset', True, 'uint16-numeric', 'uint8-0', 4),
    ('12-under-30-src', 'gain-offset-r2', False, 'float32-nan', 'int16-none-valid', 4),
    ('12-under-30-src', 'gain', True, 'uint8-none', 'float32-nan', 1),
    ('2.5x-ref', 'gain-offset-r2', True, 'float32-nan', 'uint8-0', 1),
    ('3x-ref', 'gain-blk-offset', False, 'uint16-numeric', 'int16-none-valid', 4),
    ('2.5x-ref', 'gain-offset-r2', False, 'uint16-numeric', 'float32-nan', 4),
    ('12-under-30-src', 'gain-blk-offset', True, 'uint16-numeric', 'uint8-0', 1),
]


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


@pytest.mark.parametrize('run', EQUAL_RUNS, ids=lambda r: '-'.join(map(str, r)))
def test_resident_equals_default(ctx, run):
    name, model_key, mask_partial, rasters, output, threads = run
    case = pb.CASES[name]
    model, kernel, config = MODELS[model_key]
    typed, nd = RASTERS[rasters]
    out_profile, return_valid = OUTPUTS[output]
    src, ref = pb.kernel_pair(name, nd, 3, 5, typed)
    nodata = pb.NODATA[nd]
    overlap = tuple(-(-k // 2) for k in kernel)
    mem = pb.block_mem(name, overlap)
    bps = pb.blocks_of(case, 3, overlap, mem)
    assert len(bps) == 3 * 16 and max(case.src_shape) <= 90
    # both routes of the in-blocks run: some reach outside their raster and are gathered, some lie inside and are addressed in place
    inside = [window_inside(w, *shape) for bp in bps for w, shape in ((bp.src_in_block, case.src_shape), (bp.ref_in_block, case.ref_shape))]
    assert any(inside) and not all(inside)
    kw = dict(model=model, kernel_shape=kernel, param_filename=True, model_config=dict(config, mask_partial=mask_partial),
              out_profile=out_profile, block_config=dict(threads=threads, max_block_mem=mem), return_valid=return_valid)
    default = _process(_fuse(case, src, ref, nodata, nodata), **kw)
    resident = _process(_fuse(case, src, ref, nodata, nodata), device_config=dict(resident=True), **kw)
    assert len(default) == len(resident) == (3 if return_valid else 2)
    for what, a, b in zip(('corrected', 'parameters', 'validity'), default, resident):
        _same_bytes(a, b, f'{run}: {what}')
    corr, params = default[:2]
    assert np.isfinite(params[:3]).any() and (np.isfinite(corr) if corr.dtype.kind == 'f' else corr != 0).any()
    if return_valid:
        assert 0 < (default[2] == 255).sum() < default[2].size
    if model_key == 'gain-offset-r2' and not mask_partial:
        r2 = params[6:]
        assert (r2[np.isfinite(r2)] < 0.25).any(), 'no pixel failed the r2 mask: the in-painting did not run'


# -- 6 ---------------------------------------------------------------------------------------------------------------------------------
FILE_SRC_TF = Affine(10., 0., 1000., 0., -10., 9000.)
FILE_REF_TF = Affine(30., 0., 1000. - 45., 0., -30., 9000. + 20.)


def _file_pair():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:520, 0:530]
    src = np.stack([(60 + 40 * np.sin(x / 37.) * np.cos(y / 23.) + rng.uniform(0, 20, (520, 530)) + 9 * b) for b in range(2)])
    src = np.clip(np.round(src), 1, 255).astype(np.uint8)
    src[:, 100:130, 200:260] = 0
    ry, rx = np.mgrid[0:180, 0:182]
    ref = np.stack([(500. + 300. * np.sin(rx / 11.) * np.cos(ry / 7.) + rng.normal(0, 5, (180, 182)) + 30 * b) for b in range(2)]).astype(np.float32)
    return src, ref


@pytest.mark.parametrize('nodata', [0, None], ids=['nodata-0', 'internal-mask'])
def test_resident_writes_the_same_files(ctx, tmp_path, nodata):
    src, ref = _file_pair()
    paths = {}
    for route in ('default', 'resident'):
        rf = RasterFuse(src.copy(), ref.copy(), src_nodata=0, ref_nodata=float('nan'), crs=CRS('EPSG:32735'), transform=FILE_SRC_TF,
                        ref_transform=FILE_REF_TF)
        assert rf.proc_crs.name == 'ref'
        paths[route] = (tmp_path / f'{route}_corr.tif', tmp_path / f'{route}_param.tif')
        _process(rf, corr_filename=paths[route][0], param_filename=paths[route][1], model=Model.gain, kernel_shape=(3, 3),
                 build_ovw=True, out_profile=dict(dtype='uint8', nodata=nodata), block_config=dict(threads=2, max_block_mem=0.05),
                 device_config=dict(resident=route == 'resident'))
    from homonim_amd.tiff import read_tiff
    tif = read_tiff(paths['default'][0])
    assert tif.array.shape == (2, 520, 530) and (tif.mask is not None) == (nodata is None)
    for d, r in zip(paths['default'], paths['resident']):
        assert filecmp.cmp(d, r, shallow=False), f'{d.name} and {r.name} differ'


# -- 7 ---------------------------------------------------------------------------------------------------------------------------------
def _counted(ctx, monkeypatch):
    live = []
    alloc, free = ctx.dev_alloc, ctx.dev_free

    def dev_alloc(nbytes):
        p = alloc(nbytes)
        live.append(p)
        return p

    def dev_free(p):
        live.remove(p)
        free(p)

    monkeypatch.setattr(ctx, 'dev_alloc', dev_alloc)
    monkeypatch.setattr(ctx, 'dev_free', dev_free)
    return live


@pytest.mark.parametrize('case_name, model_cls', [('3x-ref', RefSpaceModel), ('12-under-30-src', SrcSpaceModel)])
def test_no_device_allocation_outlives_a_resident_process(ctx, monkeypatch, case_name, model_cls):
    live = _counted(ctx, monkeypatch)
    seen = []
    corr, params = _closed_form_run(case_name, 1, param_filename=True)
    assert not live, f'{len(live)} device allocations outlive a resident process'
    assert_same_f32(corr, pb.closed_form_expected(case_name)[0], 'corrected')
    real = model_cls.fit_apply_dev

    def third_raises(self, *a, **kw):
        seen.append(len(live))
        if len(seen) == 3:
            raise RuntimeError('the third block fails')
        return real(self, *a, **kw)

    monkeypatch.setattr(model_cls, 'fit_apply_dev', third_raises)
    with pytest.raises(RuntimeError, match='the third block fails'):
        _closed_form_run(case_name, 1, param_filename=True)
    assert len(seen) == 3 and min(seen) > 0
    assert not live, f'{len(live)} device allocations outlive a resident process that raised'


# -- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rasters_beyond_the_free_memory_are_refused_with_both_sizes(ctx, monkeypatch):
    monkeypatch.setattr(_hk.Context, 'mem_info', lambda self: (1 << 20, 1 << 30))
    live = _counted(ctx, monkeypatch)
    src, ref = _file_pair()
    rf = RasterFuse(src, ref, src_nodata=0, crs=CRS('EPSG:32735'), transform=FILE_SRC_TF, ref_transform=FILE_REF_TF)
    before = _hk.build_ledger()
    with pytest.raises(ValueError, match=r'need (\d+) bytes of device memory.* has 1048576 bytes free') as e:
        _process(rf, model=Model.gain, kernel_shape=(3, 3), device_config=dict(resident=True))
    need = int(str(e.value).split(' need ')[1].split(' bytes')[0])
    assert need >= src.nbytes + ref.nbytes + src.size * 4 > (1 << 20)
    assert _hk.build_ledger() == before, 'a refused call launched a kernel'
    assert not live
