"""
GPU tests: the block statistics of gain-blk-offset (hk_norm.hip; reference KernelModel._fit_block_norm,
homonim/kernel_model.py:216-229) against the EXACT statistics of oracle/exact_stats.py, through every way the library computes
them -- host arrays (hk_block_norm), multi-band device planes with padded rows (hk_block_norm_dev), a batched launch between
jobs of other shapes (hk_block_norm_batch_dev), the fused fit's own statistics (fit_apply with norm_in=None) and the split
protocol over 2-4 slabs (homonim_amd/split_norm.py).

* Antisymmetric pairs (ref = -src, numeric nodata mirrored): the kernel's shift and moments of ref are the exact negation /
  copy of those of src, so norm[0] == 1.0 exactly and norm[1] must be BIT-equal to p1(-src) - p1(src) from the exact order
  statistics -- on every entry point.
* General pairs: n0 within exact_stats.n0_rel_bound of the exact std ratio (never looser than 1e-11), norm1 within
  NormExact.norm1_tol; a rank-sensitive case checks on itself that k0 +- 1 or a float32 lerp would fall outside that tolerance.
* The single-device entry points agree bit for bit; the split one has the same order statistics.
"""
import math
import zlib

import numpy as np
import pytest

from homonim_amd import _hk, split_norm
from oracle import exact_stats as ex
from oracle import oracle_np as onp

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

F32 = np.float32
ENTRY = ('host', 'dev', 'batch', 'fit_apply', 'split')


@pytest.fixture(scope='module')
def ctx():
    c = _hk.default_context()
    c.selftest()
    return c


def _desc(snd, rnd):
    return _hk.make_desc('gain-blk-offset', (5, 5), False, None, snd, rnd)


def _job(c, planes_s, planes_r, stride, stream=0, fill=F32(-3e38)):
    """ a device job of len(planes) bands, rows padded to `stride` with `fill` (never valid data of a plane) """
    nb, (h, w) = len(planes_s), planes_s[0].shape
    bufs = []
    for planes in (planes_s, planes_r):
        a = np.full((nb, max(h, 1), stride), fill, F32)
        for b, p in enumerate(planes):
            a[b, :h, :w] = p
        d = c.dev_alloc(a.nbytes)
        c.h2d(d, a)
        bufs.append(d)
    job = _hk.DevJob()
    job.src, job.ref = bufs
    job.corr = job.gain = job.offset = job.r2 = job.norm = job.fail_count = None
    job.n_bands, job.height, job.width, job.stride, job.band_stride = nb, h, w, stride, stride * max(h, 1)
    job.seg_rows, job.stream = 0, stream
    return job, bufs


def _stride(w, extra=64):
    return (w + 3) // 4 * 4 + extra


def _run_dev(ctx, desc, src, ref, bands):
    """ the case as band 1 of a multi-band job (the other bands: other data of the same shape) """
    rng = np.random.default_rng(1)
    other = [(rng.uniform(-5, 5, src.shape).astype(F32), rng.uniform(0, 9, src.shape).astype(F32)) for _ in range(2)]
    ps, pr = ([src], [ref]) if bands == 1 else ([other[0][0], src, other[1][0]], [other[0][1], ref, other[1][1]])
    job, bufs = _job(ctx, ps, pr, _stride(src.shape[1]))
    norm = ctx.dev_alloc(16 * len(ps))
    try:
        ctx.block_norm_dev(desc, job, norm)
        ctx.stream_sync(0)
        out = np.zeros((len(ps), 2))
        ctx.d2h(out, norm)
        return out[0 if bands == 1 else 1]
    finally:
        ctx.dev_free(norm), ctx.dev_free(bufs[0]), ctx.dev_free(bufs[1])


def _run_batch(ctx, desc, src, ref):
    """ the case between jobs of other shapes (one taller and wider, one smaller) in one batched launch """
    rng = np.random.default_rng(2)
    h, w = src.shape
    shapes = [(h + 37, w + 129), (max(h // 3, 1), max(w // 2, 1) + 1)] if h * w < 10 ** 7 else [(1000, 1111), (333, 77)]
    o = [(rng.normal(0, 3, s).astype(F32), rng.normal(5, 1, s).astype(F32)) for s in shapes]
    specs = [([o[0][0]], [o[0][1]]), ([src], [ref]), ([o[1][0]], [o[1][1]])]
    jobs, allb = [], []
    for ps, pr in specs:
        j, b = _job(ctx, ps, pr, _stride(ps[0].shape[1], 8), stream=0)
        jobs.append(j), allb.extend(b)
    norm = ctx.dev_alloc(16 * 3)
    try:
        ctx.block_norm_batch_dev(desc, jobs, norm)
        ctx.stream_sync(0)
        out = np.zeros((3, 2))
        ctx.d2h(out, norm)
        return out[1]
    finally:
        ctx.dev_free(norm)
        for b in allb:
            ctx.dev_free(b)


def _split_edges(h, k):
    """ k slabs of rows; the second of three or more is empty (a rank without rows) """
    if k == 2:
        return [0, h // 3, h]
    if k == 3:
        return [0, h // 2, h // 2, h]
    return [0, 1, h // 4 + 1, h // 2, h] if h >= 8 else [0, 0, 1, h, h]


def _run_split(ctx, desc, src, ref, k, edges=None):
    edges = edges or _split_edges(src.shape[0], k)
    ctxs = [_hk.Context(0, n_streams=1) for _ in range(k)]
    parts, bufs = [], []
    try:
        for c, r0, r1 in zip(ctxs, edges[:-1], edges[1:]):
            job, b = _job(c, [src[r0:r1]], [ref[r0:r1]], _stride(src.shape[1], 16))
            parts.append((c, job)), bufs.append((c, b))
        norms = split_norm.block_norm_split_local(parts, desc)
        for n in norms[1:]:
            assert n.tobytes() == norms[0].tobytes()        # identical on every rank
        return norms[0][0], edges
    finally:
        for c, (a, b) in bufs:
            c.dev_free(a), c.dev_free(b)
        for c in ctxs:
            c.close()


def _all_entry_points(ctx, src, ref, snd, rnd, bands=3, split_k=3):
    desc = _desc(snd, rnd)
    got = {'host': ctx.block_norm(desc, src, ref), 'dev': _run_dev(ctx, desc, src, ref, bands),
           'batch': _run_batch(ctx, desc, src, ref)}
    _, _, got['fit_apply'], _ = ctx.fit_apply(desc, src, ref, 2, want_params=False, want_corr=True)
    got['split'], edges = _run_split(ctx, desc, src, ref, split_k)
    return got, edges


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same_bits_single_device(got, what):
    ref_bits = _bits(got['dev'])
    for name in ('host', 'batch', 'fit_apply'):
        assert _bits(got[name]) == ref_bits, f'{what}: {name} {got[name]!r} != dev {got["dev"]!r}'


# ---- cases --------------------------------------------------------------------------------------------------------------
def _holes(rng, shape, frac):
    return rng.random(shape) < frac


def _antisym_case(name):
    """ -> (src, src_nodata, ref_nodata); the pair is (src, -src) """
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    nd = None
    if name == 'negative':
        src = -rng.uniform(1, 2, (700, 333))
    elif name == 'mixed_sign_p1_near_zero':
        src = rng.normal(0.1165, 0.05, (513, 1021))       # 1st percentile ~ 0: the pivot window crosses zero
        nd = np.nan
        src[_holes(rng, src.shape, 0.01)] = np.nan
    elif name == 'signed_zeros':
        src = rng.uniform(0, 1, (400, 601))
        z = _holes(rng, src.shape, 0.03)
        src[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    elif name == 'zero_sign_at_the_pivot':
        src = ex.signed_zero_raster(512, 512, seed=3)
    elif name == 'nodata_zero_with_minus_zero':
        src = rng.uniform(-1, 1, (300, 404))
        h = _holes(rng, src.shape, 0.3)
        src[h] = np.where(rng.random(int(h.sum())) < 0.5, 0.0, -0.0)
        nd = 0.0
    elif name == 'subnormals':
        src = rng.integers(-2 ** 23, 2 ** 23, (300, 257)) * 2.0 ** -149     # float32 subnormals ...
        h = _holes(rng, src.shape, 0.2)
        src[h] = rng.normal(0, 1e-37, int(h.sum()))                         # ... among the smallest normal values
    elif name == 'span_1e-30_1e30':
        src = rng.choice([-1, 1], (333, 300)) * 10.0 ** rng.uniform(-30, 30, (333, 300))
    elif name == 'dn_ties_numeric_nodata':
        src = (rng.integers(0, 256, (517, 623)) * 257).astype(float)      # 256 distinct DN up to 65535
        src[_holes(rng, src.shape, 0.3)] = -9999
        nd = -9999.0
    elif name == 'offset_100':
        src = 100 + 1e-3 * rng.normal(size=(400, 500))
    elif name == 'offset_1e6':
        src = 1e6 + rng.normal(size=(400, 500))
    elif name == 'two_valued':
        src = np.where(rng.random((300, 300)) < 0.5, 3.0, 7.0)
    elif name == 'tied_7pct_at_p1':
        src = rng.uniform(1, 2, (600, 700))
        src[_holes(rng, src.shape, 0.07)] = 1.0101                        # the overflow branch
    elif name.startswith('holes_'):
        frac = float(name.split('_')[1]) / 100
        src = rng.normal(2, 1, (700, 900))
        src[_holes(rng, src.shape, frac)] = np.nan
        nd = np.nan
    elif name == 'width_1':
        src = rng.normal(0, 1, (5000, 1))
    elif name == 'height_1':
        src = rng.normal(0, 1, (1, 5001))
    elif name == 'width_1023':
        src = rng.normal(0, 1, (123, 1023))
    elif name.startswith('miss_'):
        src = ex.pivot_miss_raster(256, 320, name.split('_')[1], seed=1)
    else:
        raise ValueError(name)
    src = src.astype(F32)
    rnd = None if nd is None else (nd if math.isnan(nd) else -nd)
    return src, nd, rnd


ANTISYM = ['negative', 'mixed_sign_p1_near_zero', 'signed_zeros', 'zero_sign_at_the_pivot', 'nodata_zero_with_minus_zero',
           'subnormals', 'span_1e-30_1e30', 'dn_ties_numeric_nodata', 'offset_100', 'offset_1e6', 'two_valued',
           'tied_7pct_at_p1', 'holes_0', 'holes_1', 'holes_30', 'holes_99.9', 'width_1', 'height_1', 'width_1023', 'miss_low',
           'miss_high']


def _check_antisym(got, src, snd, what):
    """ norm[0] == 1 exactly and norm[1] == p1(-src) - p1(src) bit for bit, on every entry point """
    s, _ = ex.joint_values(src, snd, src, snd)
    ss = ex.sort_exact(s)
    k0, k1, t = ex.rank_info(ss.size)
    ps = ex.lerp(float(ss[k0]), float(ss[k1]), t)
    rs = ex.sort_exact(-s)
    pr = ex.lerp(float(rs[k0]), float(rs[k1]), t)
    exp = np.array([1.0, pr - ps])
    for name in ENTRY:
        assert got[name][0] == 1.0 and _bits(got[name][1]) == _bits(exp[1]), \
            f'{what} [{name}]: {got[name]!r}, exact [1, {exp[1]!r}] (p1 src {ps!r}, p1 ref {pr!r})'


@pytest.mark.parametrize('name', ANTISYM)
def test_antisymmetric_pairs_are_bit_exact(ctx, name):
    src, snd, rnd = _antisym_case(name)
    ref = -src
    if name.startswith('miss_'):     # the constructed rasters take the miss branch (tests/test_exact_stats_cpu.py)
        assert all(d['miss'] and not d['overflow'] for d in ex.pivot_decision(src, snd, ref, rnd))
    if name == 'tied_7pct_at_p1':    # ... and this one the overflow branch
        assert any(d['overflow'] for d in ex.pivot_decision(src, snd, ref, rnd))
    got, _ = _all_entry_points(ctx, src, ref, snd, rnd, split_k=2 + len(name) % 3)
    _same_bits_single_device(got, name)
    _check_antisym(got, src, snd, name)


@pytest.mark.parametrize('n', [100, 3000])
def test_antisymmetric_lerp_branch_where_t_is_at_least_half(ctx, n):
    """ t = 0.99 (n = 100, 3000): values at k0, k1 on which numpy's b - (b - a)(1 - t) and a + (b - a) t round differently --
    the test checks on itself that dropping the t >= 0.5 branch would change the bits """
    h, w = (50, 60) if n < 3000 else (100, 100)
    k0, k1, t = ex.rank_info(n)
    assert t >= 0.5
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        v = rng.normal(0, 1, n).astype(F32)
        srt = ex.sort_exact(v)
        lo, hi = float(srt[k0]), float(srt[k1])
        if ex.lerp(lo, hi, t) != lo + (hi - lo) * t:
            break
    else:
        raise AssertionError('no branch-sensitive order statistics found')
    src = np.full(h * w, np.nan, F32)
    src[rng.choice(h * w, n, replace=False)] = v
    src = src.reshape(h, w)
    got, _ = _all_entry_points(ctx, src, -src, np.nan, np.nan, split_k=3)
    _same_bits_single_device(got, f'n={n}')
    _check_antisym(got, src, np.nan, f'lerp branch n={n}')


@pytest.mark.parametrize('n', [2, 100, 101, 102, 201, 5000])
@pytest.mark.parametrize('shape', [(50, 60), (100, 100)])     # 3000 pixels (sample step 1) / 10000 (step 2)
def test_antisymmetric_valid_counts(ctx, n, shape):
    """ n valid pixels among NaN: t = 0 (n = 101, 201), t ~ 0.99 (n = 100), k0 steps (100 -> 101 -> 102) """
    h, w = shape
    if n > h * w:
        n = h * w - 7
    rng = np.random.default_rng(n + h)
    src = np.full(h * w, np.nan, F32)
    src[rng.choice(h * w, n, replace=False)] = rng.normal(1, 2, n).astype(F32)
    src = src.reshape(h, w)
    got, _ = _all_entry_points(ctx, src, -src, np.nan, np.nan, split_k=2)
    _same_bits_single_device(got, f'n={n}')
    _check_antisym(got, src, np.nan, f'n={n} {shape}')


def test_antisymmetric_8192_block(ctx):
    """ 8192 x 8192 valid pixels: an off-by-one rank moves norm[1] by ~1e-7 relative here, invisible at the 2e-6 of the
    float32 comparisons; bit equality sees it """
    rng = np.random.default_rng(8192)
    src = rng.normal(0.3, 0.1, (8192, 8192)).astype(F32)
    got, _ = _all_entry_points(ctx, src, -src, None, None, bands=1, split_k=2)
    _same_bits_single_device(got, '8192')
    _check_antisym(got, src, None, '8192 x 8192')


# ---- general pairs: bounds ----------------------------------------------------------------------------------------------
def _general_case(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    nd = None
    if name == 'synth_1024':
        src, ref = onp.synth_pair(1024, 1024, 4, 'frame+holes')
        nd = np.nan
    elif name == 'mixed_sign':
        src = rng.normal(0.1165, 0.05, (601, 777))
        ref = 0.8 * src - 0.01 + 0.02 * rng.normal(size=src.shape)
    elif name == 'dn_ties':
        src = rng.integers(0, 65536, (400, 555)).astype(float)
        ref = np.minimum(np.round(src * 0.5 + rng.integers(0, 3, src.shape)), 65535)
        src[_holes(rng, src.shape, 0.01)] = -9999
        nd = -9999.0
    elif name == 'offset_100_vs_1e6':
        src = 100 + 1e-3 * rng.normal(size=(500, 511))
        ref = 1e6 + rng.normal(size=src.shape)
    elif name in ('miss_low', 'miss_high'):
        src = ex.pivot_miss_raster(256, 320, name.split('_')[1], seed=2).astype(float)
        ref = 2 * src + 1
    elif name == 'span':
        src = rng.choice([-1, 1], (300, 301)) * 10.0 ** rng.uniform(-30, 3, (300, 301))
        ref = 3 * src + rng.normal(size=src.shape)
    else:
        raise ValueError(name)
    return src.astype(F32), ref.astype(F32), nd


# (rank-sensitive: the order statistics next to k0, k1 differ enough that a wrong rank moves norm1 outside its tolerance; on
# float32-quantised "100 + noise" data and the high-miss raster's sparse tail they do not)
GENERAL = [('synth_1024', True), ('mixed_sign', True), ('dn_ties', True), ('offset_100_vs_1e6', False), ('miss_low', True),
           ('miss_high', False), ('span', True)]


def _offsets(src, ref, nd, edges, e):
    """ |mean - shift| per raster, the shift as the kernel takes it (the sample mean; for a split block the mean of the
    slabs' sample means over the slabs whose sample found valid pixels), with slack for its summation order """
    shifts, cnt = np.zeros(2), 0
    for r0, r1 in zip(edges[:-1], edges[1:]):
        if r1 > r0:
            sm = ex.sample_restated(src[r0:r1], nd, ref[r0:r1], nd)
            if sm[0]['m']:
                shifts += [sm[0]['shift'], sm[1]['shift']]
                cnt += 1
    shifts = shifts / cnt if cnt else shifts
    mean = (float(e.src_moments.mean()), float(e.ref_moments.mean()))
    return tuple(abs(m - c) + 1e-12 * abs(c) for m, c in zip(mean, shifts))


@pytest.mark.parametrize('name, rank_sensitive', GENERAL)
def test_general_pairs_within_the_float64_bound(ctx, name, rank_sensitive):
    src, ref, nd = _general_case(name)
    got, edges = _all_entry_points(ctx, src, ref, nd, nd, split_k=4)
    _same_bits_single_device(got, name)
    e = ex.norm_exact(src, nd, ref, nd)
    h, w = src.shape
    whole = [0, h]
    for entry in ENTRY:
        n0, n1 = got[entry]
        if entry == 'split':
            depth = max(ex.sum_depth(r1 - r0, w) for r0, r1 in zip(edges[:-1], edges[1:])) + len(edges)
            bound = ex.n0_rel_bound(e.n, e.spread(), _offsets(src, ref, nd, edges, e), depth)
        else:
            bound = ex.n0_rel_bound(e.n, e.spread(), _offsets(src, ref, nd, whole, e), ex.sum_depth(h, w))
        assert abs(n0 - e.n0) <= bound * e.n0, f'{name} [{entry}]: n0 {n0!r}, exact {e.n0!r}, bound {bound:.3g}'
        tol = e.norm1_tol(n0)
        assert abs(n1 - e.norm1) <= tol, f'{name} [{entry}]: norm1 {n1!r}, exact {e.norm1!r}, tol {tol:.3g}'
    if rank_sensitive:   # the tolerance must be able to see the bugs it is meant for
        n0 = got['dev'][0]
        tol = e.norm1_tol(n0)
        for dk in (-1, 1):
            assert abs(e.norm1_with(n0, dk) - e.norm1) > tol, f'{name}: tolerance cannot see k0 {dk:+d}'
        assert abs(e.norm1_with(n0, use_lerp32=True) - e.norm1) > tol, f'{name}: tolerance cannot see a float32 lerp'


def test_split_shift_ignores_slabs_without_valid_pixels(ctx):
    """ "1e6 + noise" over three slabs: the first has rows but no valid pixel, the second none at all.  The split shift is the
    mean of the sample means of the slabs that found valid pixels; averaging in the others' zeros would put it ~7e5 from the
    data and the float64 moments about it would lose ~10 digits. """
    rng = np.random.default_rng(6)
    src = (1e6 + rng.normal(size=(600, 500))).astype(F32)
    ref = (-3 + 0.25 * rng.normal(size=src.shape)).astype(F32)
    src[:20] = np.nan
    edges = [0, 20, 20, 600]
    got, _ = _run_split(ctx, _desc(np.nan, np.nan), src, ref, 3, edges)
    e = ex.norm_exact(src, np.nan, ref, np.nan)
    depth = max(ex.sum_depth(r1 - r0, 500) for r0, r1 in zip(edges[:-1], edges[1:])) + len(edges)
    bound = ex.n0_rel_bound(e.n, e.spread(), _offsets(src, ref, np.nan, edges, e), depth)
    assert abs(got[0] - e.n0) <= bound * e.n0, (got, e.norm, bound)
    assert abs(got[1] - e.norm1) <= e.norm1_tol(got[0]), (got, e.norm)


# ---- degenerate blocks --------------------------------------------------------------------------------------------------
def _class(v):
    return 'nan' if math.isnan(v) else ('+inf' if v == math.inf else ('-inf' if v == -math.inf else 'finite'))


@pytest.mark.parametrize('kind', ['no_valid', 'one_valid', 'constant', 'constant_src', 'constant_ref', 'constant_sparse'])
def test_degenerate_blocks(ctx, kind):
    rng = np.random.default_rng(len(kind))
    h, w = 300, 301
    src = rng.normal(0.5, 0.2, (h, w)).astype(F32)
    ref = rng.normal(2, 1, (h, w)).astype(F32)
    nd = np.nan
    if kind == 'no_valid':
        src[:] = np.nan
    elif kind == 'one_valid':
        src[:] = np.nan
        src[123, 45] = 0.7
    elif kind == 'constant':
        src[:], ref[:] = F32(0.1), F32(-3.3)
    elif kind == 'constant_src':
        src[:] = F32(0.1)
    elif kind == 'constant_ref':
        ref[:] = F32(-3.3)
    elif kind == 'constant_sparse':   # 500 valid pixels, none of them in the sample: the shift is 0
        src, ref = np.full((2000, 2000), np.nan, F32), np.full((2000, 2000), F32(0.1), F32)
        free = np.setdiff1d(np.arange(src.size), ex.sample_positions(2000, 2000))
        src.ravel()[rng.choice(free, 500, replace=False)] = F32(0.1)
    got, _ = _all_entry_points(ctx, src, ref, nd, nd, split_k=2)
    e = ex.norm_exact(src, nd, ref, nd)
    for name in ENTRY:
        g = got[name]
        if kind == 'no_valid':
            assert (g == 0).all(), (name, g)          # kernel_model.py:223-226
            continue
        assert [_class(x) for x in g] == [_class(x) for x in e.norm], f'{kind} [{name}]: {g!r}, exact {e.norm!r}'
        if np.isfinite(e.norm).all():
            assert g[0] == e.n0 == 0.0 and g[1] == e.norm1, (name, g, e.norm)
