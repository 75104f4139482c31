""" The two forms of an operation are one operation: hk_reproject / hk_reproject_dev, hk_reproject_affine / _dev, hk_compare_sums /
_dev and hk_param_stats / _dev run the same check and build the same kernel arguments, whether the rasters come as host arrays (the
library stages them into rows padded to 64 elements) or lie on the device already.

1. The results of the two forms on the same input are the same BYTES.  The reference of a form is the other form, which other tests
   hold to the oracle; no tolerance is involved.  Input: 2 bands of 9 x 13 float32 -- neither a multiple of 4 nor of the padded row --
   with one nodata pixel per band, nodata being NaN or a number; the device form gets rows 16 elements apart, the host form pads to 64.
2. One bad argument at a time is refused by both forms with the same status and, where the forms share the check, the same text --
   before anything is launched, so a valid call on the same context right afterwards succeeds.  Every size that is declared is a size
   the buffers have (a destination of 65536 rows is 65536 x 1, 65536 bands are 65536 planes of 1 x 1).

(hk_refspace_fit_apply's mask_partial refusal of a kernel with more than 65535 window pixels cannot be reached: hk_fit_desc's own
limits, kh <= 255 and kw <= 193, come first.  Nothing is tested for it.) """
import ctypes as C

import numpy as np
import pytest

from homonim_amd import Affine, _hk
from homonim_amd.errors import DeviceError
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

NB, H, W = 2, 9, 13
STRIDE, BAND = 16, 160            # the device form's rows and planes, elements: multiples of 4 (hk_dev_job), not of 64
DH, DW, DSTRIDE, DBAND = 5, 7, 8, 48
AVERAGE, BILINEAR = onp.RESAMPLING_CODES['average'], onp.RESAMPLING_CODES['bilinear']
BIG = 2 * 65536                   # elements of the buffers of the refusals: whatever a case declares fits
VP = C.c_void_p


@pytest.fixture(scope='module')
def ctx():
    return _hk.default_context()


@pytest.fixture(scope='module', params=['nan', 'numeric'])
def rasters(request):
    """ (src, ref, nodata): 2 x 9 x 13 each, one nodata pixel per band in the source and one in the reference """
    rng = np.random.default_rng(913)
    src = rng.uniform(50., 200., (NB, H, W)).astype(np.float32)
    ref = (1.2 * src + 10. + rng.normal(0., 1., src.shape)).astype(np.float32)
    nodata = float('nan') if request.param == 'nan' else -9999.
    src[0, 4, 6] = src[1, 0, 12] = ref[0, 8, 0] = ref[1, 3, 3] = nodata
    for a in (src, ref):
        a.setflags(write=False)
    return src, ref, nodata


class DevBuf:
    """ a device buffer holding `array` laid out with the given row / band stride (elements), the gaps poisoned; read(shape) -> array """

    def __init__(self, ctx, n_bands, rows, stride, band, array=None, dtype=np.float32):
        self.ctx, self.host = ctx, np.full((n_bands, band), 12345, dtype)
        self.view = self.host[:, :rows * stride].reshape(n_bands, rows, stride)
        if array is not None:
            self.view[:, :, :array.shape[2]] = array
        self.ptr = ctx.dev_alloc(self.host.nbytes)
        ctx.h2d(self.ptr, self.host)

    def read(self, width):
        self.ctx.d2h(self.host, self.ptr)
        return np.ascontiguousarray(self.view[:, :, :width])

    def free(self):
        self.ctx.dev_free(self.ptr)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# -- 1. one operation, two forms ----------------------------------------------------------------------------------------------------
def test_reproject_average_host_and_device_forms_give_the_same_bytes(ctx, rasters):
    src, _, nodata = rasters
    mapping = (2., -.5, 2., 0.)
    host = ctx.reproject(src, nodata, mapping, (DH, DW), AVERAGE, float('nan'))
    d_src, d_dst = DevBuf(ctx, NB, H, STRIDE, BAND, src), DevBuf(ctx, NB, DH, DSTRIDE, DBAND)
    try:
        ctx.reproject_dev(d_src.ptr, NB, (H, W), STRIDE, BAND, nodata, mapping, AVERAGE, d_dst.ptr, (DH, DW), DSTRIDE, DBAND, float('nan'))
        ctx.stream_sync(0)
        dev = d_dst.read(DW)
    finally:
        d_src.free(), d_dst.free()
    assert same_bytes(host, dev) and np.isfinite(host).sum() > 0.8 * host.size


def test_reproject_affine_bilinear_host_and_device_forms_give_the_same_bytes(ctx, rasters):
    src, _, nodata = rasters
    warp = _hk.make_affine_warp_desc(None, Affine(1., 0., 0., 0., -1., 9.), None, Affine(1., .2, 1.5, .1, -1., 8.))
    host = ctx.reproject_affine(src, nodata, warp, (1., 1.), (DH, DW), BILINEAR, float('nan'))
    d_src, d_dst = DevBuf(ctx, NB, H, STRIDE, BAND, src), DevBuf(ctx, NB, DH, DSTRIDE, DBAND)
    try:
        ctx.reproject_affine_dev(warp, d_src.ptr, NB, (H, W), STRIDE, BAND, nodata, (1., 1.), BILINEAR, d_dst.ptr, (DH, DW), DSTRIDE, DBAND,
                                 float('nan'))
        ctx.stream_sync(0)
        dev = d_dst.read(DW)
    finally:
        d_src.free(), d_dst.free()
    assert same_bytes(host, dev) and np.isfinite(host).sum() > 0.5 * host.size


def test_compare_sums_host_and_device_forms_give_the_same_bytes(ctx, rasters):
    src, ref, nodata = rasters
    host = np.stack([ctx.compare_sums(src[b], nodata, ref[b], nodata) for b in range(NB)])
    d_src, d_ref = DevBuf(ctx, NB, H, STRIDE, BAND, src), DevBuf(ctx, NB, H, STRIDE, BAND, ref)
    d_sums = DevBuf(ctx, 1, NB, 7, NB * 7, dtype=np.float64)
    try:
        job = _hk.DevJob(src=d_src.ptr, ref=d_ref.ptr, n_bands=NB, height=H, width=W, stride=STRIDE, band_stride=BAND, stream=0)
        ctx.compare_sums_dev(job, nodata, nodata, d_sums.ptr)
        ctx.stream_sync(0)
        dev = d_sums.read(7)[0]
    finally:
        d_src.free(), d_ref.free(), d_sums.free()
    assert same_bytes(host, dev) and (host[:, 6] == H * W - 2).all()


def test_param_stats_host_and_device_forms_give_the_same_bytes(ctx, rasters):
    src, _, nodata = rasters
    host = np.stack([ctx.param_stats(src[b], nodata, 100.) for b in range(NB)])
    d_src, d_stats = DevBuf(ctx, NB, H, STRIDE, BAND, src), DevBuf(ctx, 1, NB, 10, NB * 10, dtype=np.float64)
    try:
        ctx.param_stats_dev(d_src.ptr, NB, H, W, STRIDE, BAND, d_stats.ptr, nodata, 100.)
        ctx.stream_sync(0)
        dev = d_stats.read(10)[0]
    finally:
        d_src.free(), d_stats.free()
    assert same_bytes(host, dev) and np.isfinite(host).all()


# -- 2. one refusal, two forms ------------------------------------------------------------------------------------------------------
def refusal(fn, args):
    """ (exception class, text) of a call that must be refused """
    with pytest.raises((ValueError, DeviceError)) as info:
        _hk._check(fn(*args))
    return type(info.value), str(info.value)


@pytest.fixture(scope='module')
def buffers(ctx):
    """ host and device buffers of BIG float32 for the refused calls (and the valid ones that follow them) """
    h_src, h_dst = np.ones(BIG, np.float32), np.zeros(BIG, np.float32)
    d_src, d_dst = ctx.dev_alloc(4 * BIG), ctx.dev_alloc(4 * BIG)
    ctx.h2d(d_src, h_src)
    yield h_src, h_dst, d_src, d_dst
    ctx.dev_free(d_src), ctx.dev_free(d_dst)


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# argument, its value in the refused call, the class of the refusal, which forms have the argument
REPROJECT_REFUSALS = [
    ('sw', 0, ValueError, 'both'), ('nb', 0, ValueError, 'both'), ('dh', 0, ValueError, 'both'),            # empty raster
    ('s_stride', W - 1, ValueError, 'dev'), ('d_stride', DW - 1, ValueError, 'dev'),                         # row stride below width
    ('s_band', -1, ValueError, 'dev'), ('d_band', -4, ValueError, 'dev'),                                    # negative band stride
    ('mode', 7, ValueError, 'both'), ('mode', -1, ValueError, 'both'), ('mode', 3, ValueError, 'both'),
    ('resampling', 7, DeviceError, 'both'), ('resampling', 15, DeviceError, 'both'),
    ('tall', None, DeviceError, 'both'),            # a destination of 65536 rows, 65536 x 1
    ('stream', 99, ValueError, 'dev'),
]


def _reproject_calls(ctx, buffers, affine, **bad):
    """ -> (host form's (fn, args), device form's) for 2 x 9 x 13 -> 2 x 5 x 7 with the arguments named in `bad` replaced """
    h_src, h_dst, d_src, d_dst = buffers
    a = dict(nb=NB, sh=H, sw=W, s_stride=STRIDE, s_band=BAND, mode=_hk.NODATA_NAN, dh=DH, dw=DW,
             d_stride=DSTRIDE, d_band=DBAND, resampling=BILINEAR if affine else AVERAGE, stream=0)
    if 'tall' in bad:
        a.update(nb=1, dh=65536, dw=1, d_stride=1, d_band=65536)
    a.update({k: v for k, v in bad.items() if k != 'tall'})
    lib, h = ctx._lib, ctx.handle
    if affine:
        warp = _hk.make_affine_warp_desc(None, Affine(1., 0., 0., 0., -1., 9.), None, Affine(1., .2, 1.5, .1, -1., 8.))
        host = (lib.hk_reproject_affine, (h, C.byref(warp), _f32p(h_src), a['nb'], a['sh'], a['sw'], a['mode'], 0., 1., 1., a['resampling'],
                                          _f32p(h_dst), a['dh'], a['dw'], 0.))
        dev = (lib.hk_reproject_affine_dev, (h, C.byref(warp), VP(d_src), a['nb'], a['sh'], a['sw'], a['s_stride'], a['s_band'], a['mode'], 0.,
                                             1., 1., a['resampling'], VP(d_dst), a['dh'], a['dw'], a['d_stride'], a['d_band'], 0., a['stream']))
    else:
        host = (lib.hk_reproject, (h, _f32p(h_src), a['nb'], a['sh'], a['sw'], a['mode'], 0., 2., 0., 2., 0., a['resampling'], _f32p(h_dst),
                                   a['dh'], a['dw'], 0.))
        dev = (lib.hk_reproject_dev, (h, VP(d_src), a['nb'], a['sh'], a['sw'], a['s_stride'], a['s_band'], a['mode'], 0., 2., 0., 2., 0.,
                                      a['resampling'], VP(d_dst), a['dh'], a['dw'], a['d_stride'], a['d_band'], 0., a['stream']))
    return host, dev


@pytest.mark.parametrize('affine', [False, True], ids=['scaled', 'affine'])
def test_reproject_refusals_are_the_same_from_both_forms(ctx, buffers, affine):
    good_host, good_dev = _reproject_calls(ctx, buffers, affine)
    for name, value, cls, forms in REPROJECT_REFUSALS:
        host, dev = _reproject_calls(ctx, buffers, affine, **{name: value})
        got_dev = refusal(*dev)
        assert got_dev[0] is cls, (name, value, got_dev)
        if forms == 'both':
            got_host = refusal(*host)
            # hk_reproject says more about a resampling that is not built than hk_reproject_dev; everything else word for word
            if name == 'resampling' and not affine:
                assert got_host[0] is cls and got_host[1].startswith(got_dev[1]) and 'GRA_*' in got_host[1], (name, value, got_host)
            else:
                assert got_host == got_dev, (name, value)
        for fn, args in (good_host, good_dev):
            assert fn(*args) == 0, (name, value, ctx._lib.hk_last_error())
        ctx.stream_sync(0)


def test_too_many_bands_are_refused_by_both_forms_of_the_scaled_reproject(ctx, buffers):
    """ the band count is the launch's gridDim.z: 65536 planes of 1 x 1, which the buffers hold, are refused as an argument by both """
    host, dev = _reproject_calls(ctx, buffers, False, nb=65536, sh=1, sw=1, s_stride=1, s_band=1, dh=1, dw=1, d_stride=1, d_band=1)
    got = refusal(*host)
    assert got == refusal(*dev) and got == (ValueError, 'too many bands for one launch (65536 > 65535)')
    for fn, args in _reproject_calls(ctx, buffers, False):
        assert fn(*args) == 0, ctx._lib.hk_last_error()
    ctx.stream_sync(0)


def test_param_stats_and_compare_sums_refusals(ctx, buffers):
    h_src, h_dst, d_src, d_dst = buffers
    lib, h = ctx._lib, ctx.handle
    out = np.zeros(16, np.float64)
    f64p = out.ctypes.data_as(C.POINTER(C.c_double))

    def stats(n_bands=1, height=H, width=W, stride=STRIDE, band_stride=BAND, mode=1, stream=0):
        return ((lib.hk_param_stats, (h, _f32p(h_src), stride, mode, 0., 0., height, width, f64p)),
                (lib.hk_param_stats_dev, (h, VP(d_src), n_bands, height, width, stride, band_stride, stream, mode, 0., 0., VP(d_dst))))

    def compare(height=H, width=W, stride=STRIDE, src_mode=1, ref_mode=1):
        job = _hk.DevJob(src=d_src, ref=d_src, n_bands=1, height=height, width=width, stride=stride, band_stride=BAND, stream=0)
        return ((lib.hk_compare_sums, (h, _f32p(h_src), stride, src_mode, 0., _f32p(h_src), stride, ref_mode, 0., height, width, f64p)),
                (lib.hk_compare_sums_dev, (h, C.byref(job), src_mode, 0., ref_mode, 0., VP(d_dst))))

    # the statistics share check_param_stats: the same words from both forms
    for bad in (dict(width=0), dict(height=0), dict(stride=W - 1), dict(mode=7), dict(mode=3)):
        host, dev = stats(**bad)
        got = refusal(*host)
        assert got[0] is ValueError and got == refusal(*dev), bad
        for fn, args in stats():
            assert fn(*args) == 0, (bad, lib.hk_last_error())
    for bad, text in ((dict(band_stride=-1), 'band_stride is negative'), (dict(stream=99), 'bad stream index'),
                      (dict(n_bands=65536, height=1, width=1, stride=1, band_stride=1), 'too many bands for one launch (65536 > 65535)')):
        assert refusal(*stats(**bad)[1]) == (ValueError, text), bad
        assert all(fn(*args) == 0 for fn, args in stats()), (bad, lib.hk_last_error())
    # the comparison's device form takes a job and refuses its shape in a job's words; the nodata modes are one check
    for bad in (dict(src_mode=7), dict(ref_mode=-2)):
        host, dev = compare(**bad)
        got = refusal(*host)
        assert got[0] is ValueError and 'nodata mode' in got[1] and got == refusal(*dev), bad
        assert all(fn(*args) == 0 for fn, args in compare()), (bad, lib.hk_last_error())
    for bad in (dict(width=0), dict(stride=W - 1)):
        for call in compare(**bad):
            assert refusal(*call)[0] is ValueError, bad
        assert all(fn(*args) == 0 for fn, args in compare()), (bad, lib.hk_last_error())
    ctx.stream_sync(0)


def test_partial_mask_refuses_an_unknown_nodata_mode(ctx):
    """ 0 .. 2 are the nodata modes, 3 says `in` is a coverage fraction; anything else is an argument error, and nothing is launched """
    rng = np.random.default_rng(5)
    cover = np.ones((H, W), np.float32)
    params = rng.uniform(.5, 2., (2, H, W)).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)

    def call(mode):
        return ctx._lib.hk_partial_mask(ctx.handle, _f32p(cover), W, mode, 0., _f32p(params), 2, None, 0, H, W, 3, 3, None, None,
                                        mask.ctypes.data_as(C.POINTER(C.c_uint8)))

    for mode in (4, 7, -1):
        with pytest.raises(ValueError, match=f'bad nodata mode {mode}'):
            _hk._check(call(mode))
        assert call(3) == 0, ctx._lib.hk_last_error()
    exp = np.zeros((H, W), np.uint8)
    exp[2:-2, 2:-2] = 1     # full coverage and parameters everywhere: the (3+2) x (3+2) erosion with a zero border leaves the core
    assert np.array_equal(mask, exp)
    _, _, by_wrapper = ctx.partial_mask(cover, None, params, (3, 3), want_mask=True, coverage=True)
    assert np.array_equal(by_wrapper, exp)
