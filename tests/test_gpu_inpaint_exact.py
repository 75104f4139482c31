"""
GPU test: the in-painting kernels (hk_inpaint.hip) alone, on source masks chosen for what the search can get wrong
(tests/_inpaint_masks.py; tests/test_inpaint_masks_cpu.py shows that each family holds what it is named for), against the C
oracle's restatement of GDALFillNodata -- bit for bit, at every pixel, in every mode of hk_debug_inpaint_plane_dev:

    0  what a fit would get (the targets counted, the packed search's order picked by their share)
    1  packed search, a tile's targets in row order        2  ... in column order
    3  no packed search: the general search takes every target

There is no tolerance: the kernels take the same decisions on integers and form the float64 weight sums in the oracle's order.
Through the fit (test_r2_inpainting_* of test_gpu_parity.py, test_gpu_srcspace.py, test_gpu_batch.py) the step only sees the
mask of a noisy pair, where a failing pixel has passing ones a few pixels away in every quadrant.
"""
import numpy as np
import pytest

import _inpaint_masks as M
from homonim_amd import _hk
from oracle import oracle_c as oc

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

CASES = M.cases()
MODES = (0, 1, 2, 3)
_EXPECTED = {}


@pytest.fixture(scope='module')
def ctx():
    assert oc.available(), 'the oracle library is not built (python -m homonim_amd.build)'
    return _hk.default_context()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _expected(name):
    """ oracle_c.fill_nodata of a named case, computed once: its mask is flags == 1 """
    if name not in _EXPECTED:
        img, flags = CASES[name]
        exp = oc.fill_nodata(img, flags == 1)
        exp.setflags(write=False)
        _EXPECTED[name] = exp
    return _EXPECTED[name]


def _same(got, exp, img, flags, what, dist=None):
    """ equal bit patterns wherever the kernels may write (flag 0), the input's bit patterns everywhere else """
    want = np.where(flags == 0, _bits(exp), _bits(img))
    bad = _bits(got) != want
    if bad.any():
        dist = dist if dist is not None else M.quadrant_distances(flags)
        lines = [M.describe(flags, dist, y, x) + f': got {got[y, x]!r} ({_bits(got)[y, x]:#010x}), expected '
                 f'{want.view(np.float32)[y, x]!r} ({want[y, x]:#010x}), input {img[y, x]!r}' for y, x in np.argwhere(bad)[:8]]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} pixels differ '
                             f'({int((bad & (flags == 0)).sum())} targets, {int((bad & (flags == 1)).sum())} sources, '
                             f'{int((bad & (flags > 1)).sum())} flag-2 pixels); first:\n  ' + '\n  '.join(lines))


@pytest.mark.parametrize('name', list(CASES))
def test_inpaint_plane_equals_the_oracle_in_every_mode(ctx, name):
    img, flags = CASES[name]
    exp = _expected(name)
    results = {}
    for mode in MODES:
        results[mode] = ctx.inpaint_plane(img, flags=flags, mode=mode)
        _same(results[mode], exp, img, flags, f'{name}, mode {mode}')
    for mode in (2, 3):   # (follows from the above; said on its own because it is what a faster search must keep)
        assert (_bits(results[mode]) == _bits(results[1])).all(), f'{name}: modes 1 and {mode} differ'


@pytest.mark.parametrize('name', ['lattice'] + [n for n in CASES if n.startswith('dense[70x257,')])
def test_row_padding_never_acts(ctx, name):
    """ stride > width: the flag plane is read four columns at a time and the table sixteen bytes at a time.  The padding holds
    source flags and 1e30: neither may reach a target.  (Strides are multiples of 4, the kernels' own requirement: width + 4 and
    width + 60, rounded up.) """
    img, flags = CASES[name]
    exp = _expected(name)
    w = flags.shape[1]
    for stride in ((w + 4 + 3) // 4 * 4, (w + 60 + 3) // 4 * 4):
        for mode in MODES:
            got = ctx.inpaint_plane(img, flags=flags, mode=mode, stride=stride, pad_value=1e30, pad_flag=1)
            _same(got, exp, img, flags, f'{name}, stride {stride}, mode {mode}')


def test_flag_route(ctx):
    """ the mask from gain / r2 / thresh (inpaint_flag_kernel): NaN, r2 == thresh, +-0 and negative gains, infinities """
    img, gain, r2, thresh = M.flag_route_planes()
    src = (r2 > np.float32(thresh)) & (gain > 0)
    flags = src.astype(np.uint8)
    exp = oc.fill_nodata(img, src)
    dist = M.quadrant_distances(flags)
    for mode in MODES:
        got = ctx.inpaint_plane(img, gain=gain, r2=r2, thresh=thresh, mode=mode)
        _same(got, exp, img, flags, f'flag route, mode {mode}', dist)
    got = ctx.inpaint_plane(img, gain=gain, r2=r2, thresh=thresh, stride=img.shape[1] + 8, pad_value=1.0)   # (a padding of sources)
    _same(got, exp, img, flags, 'flag route, padded', dist)


def test_scratch_of_an_earlier_plane_is_not_seen(ctx):
    """ the stream's scratch (bit planes, table, the plane of targets the packed search left over) keeps what the last call wrote:
    a smaller plane right after a larger one must come out as on its own """
    for big, small in (('dense[130x301,0.01]', 'dense[70x257,0.9]'), ('edges[row0]', 'narrow[65x3]'), ('lattice', 'circle[25]'),
                       ('all', 'none'), ('reach', 'narrow[130x1]')):
        for mode in MODES:
            ctx.inpaint_plane(CASES[big][0], flags=CASES[big][1], mode=mode)
            img, flags = CASES[small]
            _same(ctx.inpaint_plane(img, flags=flags, mode=mode), _expected(small), img, flags, f'{small} after {big}, mode {mode}')


def test_refusals_launch_nothing(ctx):
    h, w, stride = 8, 12, 12
    n = h * stride
    buf = ctx.dev_alloc(4 * n * 4)
    try:
        ctx.memset(buf, 0, 4 * n * 4)
        plane, flags, gain, r2 = buf, buf + 4 * n, buf + 8 * n, buf + 12 * n
        before = _hk.build_ledger()
        bad = [
            dict(plane_dptr=None),                                  # no plane
            dict(flags_dptr=None),                                  # neither input
            dict(gain_dptr=gain, r2_dptr=r2),                       # both inputs
            dict(flags_dptr=None, gain_dptr=gain),                  # half of the second input
            dict(flags_dptr=None, r2_dptr=r2),
            dict(height=0), dict(width=0), dict(height=-3), dict(width=-1),
            dict(stride=w - 4), dict(stride=w + 1), dict(stride=w + 2), dict(stride=0), dict(stride=-12),
            dict(plane_dptr=plane + 2), dict(flags_dptr=flags + 1), dict(flags_dptr=flags + 2),
            dict(flags_dptr=None, gain_dptr=gain + 2, r2_dptr=r2), dict(flags_dptr=None, gain_dptr=gain, r2_dptr=r2 + 1),
            dict(mode=-1), dict(mode=4), dict(stream=-1), dict(stream=10 ** 6),
            dict(mode=1, stride=1 << 23), dict(mode=2, stride=1 << 23),   # (no packed search at such a stride)
        ]
        for change in bad:
            args = dict(plane_dptr=plane, flags_dptr=flags, gain_dptr=None, r2_dptr=None, thresh=0.25, height=h, width=w,
                        stride=stride, mode=0, stream=0)
            args.update(change)
            with pytest.raises(ValueError):
                ctx.inpaint_plane_dev(**args)
        assert _hk.build_ledger() == before, 'a refused call launched a kernel'
        # ... and the same planes are taken when nothing is wrong with the call
        ctx.inpaint_plane_dev(plane, flags, None, None, 0.25, h, w, stride)
        ctx.inpaint_plane_dev(plane, None, gain, r2, 0.25, h, w, stride)
        assert _hk.build_ledger() != before
    finally:
        ctx.dev_free(buf)
    img = np.zeros((4, 6), np.float32)
    for kw in (dict(flags=np.zeros((4, 6), np.uint8), stride=4), dict(flags=np.zeros((4, 6), np.uint8), stride=10), dict(),
               dict(flags=np.zeros((4, 6), np.uint8), gain=img, r2=img, thresh=0.5), dict(flags=np.zeros((4, 5), np.uint8)),
               dict(gain=img, thresh=0.5), dict(gain=img, r2=img), dict(flags=np.zeros((4, 6), np.uint8), thresh=0.5)):
        with pytest.raises(ValueError):
            ctx.inpaint_plane(img, **kw)
