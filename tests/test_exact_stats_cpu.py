"""
CPU tests of the exact block statistics (oracle/exact_stats.py) -- the reference the GPU's block normalisation
(hk_norm.hip) is held to in tests/test_gpu_block_norm_exact.py -- and of the CPU statements of those statistics against it:
the C oracle (oracle/hk_oracle.c) and the numpy statement of the split protocol (oracle_np.split_norm_*).  The last tests
restate the sample of norm_sample_kernel and prove that the constructed rasters the GPU tests use take the branch they
are built for.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_stats as ex
from oracle import oracle_np as onp

F32 = np.float32


def _frac_stats(vals):
    """ mean, population variance and 1st percentile of float32 values in Fractions (the lerp as a Fraction too) """
    fr = [Fraction(float(v)) for v in vals]
    n = len(fr)
    mean = sum(fr) / n
    var = sum((v - mean) ** 2 for v in fr) / n
    srt = sorted(fr)
    k0, k1, t = ex.rank_info(n)
    return mean, var, srt[k0] + (srt[k1] - srt[k0]) * Fraction(t)


def _data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        v = rng.normal(0.3, 2.0, n)
    elif kind == 'subnormal':
        v = rng.integers(-2 ** 23, 2 ** 23, n) * 2.0 ** -149           # float32 subnormals (and zeros)
    elif kind == 'zeros':
        v = rng.choice([0.0, -0.0, 1.5, -2.25, 1e-3], n)
    elif kind == 'span':
        v = rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-30, 30, n)    # magnitudes 1e-30 ... 1e30
    elif kind == 'offset':
        v = 100 + 1e-3 * rng.normal(size=n)
    else:
        raise ValueError(kind)
    return v.astype(F32)


KINDS = ['normal', 'subnormal', 'zeros', 'span', 'offset']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 2, 7, 64, 301])
def test_moments_and_percentile_equal_fractions(kind, n):
    v = _data(kind, n, seed=n + len(kind))
    mean, var, pct = _frac_stats(v)
    m = ex.exact_moments(v)
    assert m.n == n and m.mean() == mean and m.var() == var
    # p1 = the float64 lerp on the exact order statistics: within 2 roundings of the exact lerp of those statistics
    got = ex.p1(v)
    assert abs(Fraction(got) - pct) <= 2 * ex.EPS64 * max(abs(float(x)) for x in v[np.isfinite(v)])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 2, 3, 100, 101, 102, 201, 1000, 4099])
def test_p1_is_numpy_percentile_of_float64_copies_bit_for_bit(kind, n):
    v = _data(kind, n, seed=3 * n + len(kind))
    exp = np.percentile(v.astype(np.float64), 1)
    got = ex.p1(v)
    # (np.percentile orders -0.0 and +0.0 as equal, the key sort puts -0.0 first: a zero may differ in its sign only)
    assert got == exp and (got != 0 or kind == 'zeros' or math.copysign(1, got) == math.copysign(1, exp))
    assert np.float64(got).tobytes() == np.float64(exp).tobytes() or got == exp == 0


@pytest.mark.parametrize('n, k0, k1, t', [
    (1, 0, 0, 0.0), (2, 0, 1, 0.01), (3, 0, 1, 0.02), (100, 0, 1, 0.99), (101, 1, 2, 0.0), (102, 1, 2, 0.01),
    (201, 2, 3, 0.0),
])
def test_rank_known_answers(n, k0, k1, t):
    got = ex.rank_info(n)
    assert got[:2] == (k0, k1) and got[2] == pytest.approx(t, abs=1e-15)
    assert (got[2] == 0.0) == (t == 0.0)          # t = 0 exactly where 0.01 (n - 1) is an integer
    v = np.arange(n, dtype=F32)[::-1] * F32(3)     # order statistic k = 3 k
    exp = 3.0 * (k0 + t) if t < 0.5 else 3.0 * k1 - 3.0 * (k1 - k0) * (1 - t)
    assert ex.p1(v) == exp
    assert ex.p1(v) == np.percentile(v.astype(np.float64), 1)


def test_rank_t_branch_and_k0_steps():
    """ k0 steps exactly at n = 100 j + 1; the lerp takes its b - (b - a)(1 - t) branch where t >= 0.5 """
    for n in range(1, 1002):
        k0, k1, t = ex.rank_info(n)
        assert k0 == (n - 1) // 100 and k1 == min(k0 + 1, n - 1) and 0 <= t < 1
    assert ex.lerp(1.0, 2.0, 0.5) == 2.0 - 1.0 * 0.5 and ex.lerp(1.0, 2.0, 0.25) == 1.25


def test_signed_zeros_sort_by_key():
    v = np.array([0.0, -0.0, 1.0, -0.0, -1.0], F32)
    s = ex.sort_exact(v)
    assert [math.copysign(1, x) for x in s] == [-1, -1, -1, 1, 1] and list(s) == [-1, 0, 0, 0, 1]
    k = ex.f2key(np.array([-np.inf, -1, -0.0, 0.0, 1e-45, np.inf], F32))
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (ex.key2f(k).view(np.uint32) == np.array([-np.inf, -1, -0.0, 0.0, 1e-45, np.inf], F32).view(np.uint32)).all()


def test_exact_moments_extremes():
    # sums that overflow int64 and float64 cancellation alike: 2**26 copies of the largest mantissa
    v = np.full(1 << 16, F32(np.nextafter(F32(2), F32(0))), F32)
    m = ex.exact_moments(v)
    assert m.var() == 0 and m.mean() == Fraction(float(v[0]))
    w = np.array([1e30, -1e30, 1e-30, 3e-45], F32)
    mean, var, _ = _frac_stats(w)
    assert ex.exact_moments(w).mean() == mean and ex.exact_moments(w).var() == var


def test_std_ratio_rounds_once_and_degenerate_classes():
    rng = np.random.default_rng(1)
    s, r = rng.normal(size=999).astype(F32), rng.normal(3, 7, size=999).astype(F32)
    n0 = ex.std_ratio(ex.exact_moments(s), ex.exact_moments(r))
    q = ex.exact_moments(r).var() / ex.exact_moments(s).var()
    lo, hi = Fraction(np.nextafter(n0, 0)), Fraction(np.nextafter(n0, np.inf))
    assert ((lo + Fraction(n0)) / 2) ** 2 <= q <= ((hi + Fraction(n0)) / 2) ** 2     # n0 is sqrt(q) correctly rounded
    c = np.full(10, F32(0.1))
    assert math.isnan(ex.std_ratio(ex.exact_moments(c), ex.exact_moments(c)))
    assert ex.std_ratio(ex.exact_moments(c), ex.exact_moments(s[:10])) == math.inf
    assert ex.std_ratio(ex.exact_moments(s[:10]), ex.exact_moments(c)) == 0.0
    e = ex.norm_exact(np.full((3, 3), np.nan, F32), np.nan, np.zeros((3, 3), F32), None)
    assert e.n == 0 and (e.norm == 0).all()


def test_n0_bound_never_looser_than_1e_11():
    assert ex.n0_rel_bound(10 ** 6, 1.0, 0.0, depth=600) < 1e-12
    assert ex.n0_rel_bound(10 ** 6, (1.0, 2.0), (0.01, 3.0), depth=600) < 1e-11
    with pytest.raises(ValueError):
        ex.n0_rel_bound(10 ** 8, 1.0, 0.0)                 # a plain running sum of 1e8 values: ~1e-8
    with pytest.raises(ValueError):
        ex.n0_rel_bound(10 ** 6, 1e-3, 100.0, depth=600)   # an unshifted "100 + 1e-3 noise"
    # the bound holds for an actual float64 shifted one-pass evaluation with a plain running sum
    rng = np.random.default_rng(5)
    s = (1e6 + rng.normal(size=20000)).astype(F32)
    r = (-3 + 0.25 * rng.normal(size=20000)).astype(F32)
    var = []
    for v, c in ((s, 1e6 + 0.5), (r, -3.01)):
        m1 = m2 = 0.0
        for x in v.astype(np.float64).tolist():
            d = x - c
            m1 += d
            m2 += d * d
        dd = m1 / v.size
        var.append(m2 / v.size - dd * dd)
    n0 = math.sqrt(var[1]) / math.sqrt(var[0])
    e = ex.norm_exact_values(s, r)
    sp = e.spread()
    off = (abs(float(e.src_moments.mean()) - (1e6 + 0.5)), abs(float(e.ref_moments.mean()) + 3.01))
    bound = ex.n0_rel_bound(s.size, sp, off)          # depth n: the plain running sum above
    assert abs(n0 - e.n0) <= bound * e.n0
    # ... and it is not vacuous: float32 sums miss it by orders of magnitude
    v32 = [float(np.var(v, dtype=F32)) for v in (s - F32(1e6), r)]
    assert abs(math.sqrt(v32[1] / v32[0]) - e.n0) > 1e3 * bound * e.n0


def test_norm1_tolerance_sees_off_by_one_and_float32_lerp():
    """ at 1024 x 1024 the tolerance of the GPU tests excludes k0 +- 1 and a float32 lerp """
    src, ref = onp.synth_pair(1024, 1024, 4)
    e = ex.norm_exact(src, None, ref, None)
    tol = e.norm1_tol(e.n0)
    assert abs(e.norm1_with(e.n0) - e.norm1) == 0
    for dk in (-1, 1):
        assert abs(e.norm1_with(e.n0, dk) - e.norm1) > tol
    assert abs(e.norm1_with(e.n0, use_lerp32=True) - e.norm1) > tol


# ---- the C oracle and the numpy split protocol against the exact reference ---------------------------------------------
@pytest.fixture(scope='module')
def oc():
    from homonim_amd import build
    build.build_oracle(verbose=False)
    from oracle import oracle_c
    assert oracle_c.available()
    return oracle_c


def _pairs():
    rng = np.random.default_rng(11)
    out = []
    s, r = onp.synth_pair(300, 401, 2, 'frame+holes')
    out.append(('synth', s, r, np.nan))
    s = (rng.normal(0.01, 0.05, (200, 333))).astype(F32)                    # mixed sign, p1 near zero
    out.append(('mixed', s, (0.8 * s + 0.02 * rng.normal(size=s.shape)).astype(F32), None))
    s = rng.integers(0, 65536, (150, 257)).astype(F32)                       # DN with ties
    r = np.minimum(s * 0.5 + rng.integers(0, 3, s.shape), 65535).astype(F32)
    s[rng.random(s.shape) < 0.3] = -9999
    out.append(('dn', s, r, -9999.0))
    s = (100 + 1e-3 * rng.normal(size=(97, 211))).astype(F32)
    out.append(('offset', s, (1e6 + rng.normal(size=s.shape)).astype(F32), None))
    return out


@pytest.mark.parametrize('case', range(4))
def test_c_oracle_is_exact(oc, case):
    name, src, ref, nd = _pairs()[case]
    e = ex.norm_exact(src, nd, ref, nd)
    got = oc.fit_block_norm(src, nd, ref, nd)
    assert abs(got[0] - e.n0) <= 1e-13 * e.n0, name
    assert abs(got[1] - e.norm1) <= e.norm1_tol(got[0]), name


def _split_protocol(vals_per_rank):
    """ the phases of the split statistics on numpy (as tests/test_split_norm_cpu.py), returning norm and the prefixes """
    x = np.sum([np.array([v[0].mean(), v[1].mean(), 1.0]) if v[0].size else np.zeros(3) for v in vals_per_rank], axis=0)
    shift = x[:2] / x[2] if x[2] > 0 else np.zeros(2)
    mom = np.sum([onp.split_norm_moments(v, shift) for v in vals_per_rank], axis=0)
    n = int(mom[0])
    ranks, prefixes = onp.split_norm_ranks(n), [[0, 0], [0, 0]]
    for level in range(3):
        hist = np.sum([onp.split_norm_hist(v, level, prefixes) for v in vals_per_rank], axis=0)
        prefixes, ranks = onp.split_norm_select(hist, level, prefixes, ranks)
    return onp.split_norm_finish(mom, shift, prefixes), prefixes, shift


@pytest.mark.parametrize('case', range(4))
@pytest.mark.parametrize('edges', [(0, None), (0, 0, None), (0, 40, 40, None), (0, 1, 50, 0, None)])
def test_split_protocol_is_exact(case, edges):
    """ 1-4 slabs (one of them empty, one a single row): the radix select returns the sorted order statistics exactly, the
    std ratio is within the float64 bound of the exact one """
    name, src, ref, nd = _pairs()[case]
    h = src.shape[0]
    cuts = [0] + sorted(min(c, h) for c in edges[1:-1]) + [h]
    vals = [onp.split_norm_slab_values(src[a:b], nd, ref[a:b], nd) for a, b in zip(cuts[:-1], cuts[1:])]
    norm, prefixes, shift = _split_protocol(vals)
    e = ex.norm_exact(src, nd, ref, nd)
    for q, k in ((0, e.src_k), (1, e.ref_k)):
        got = [onp._key2f(prefixes[q][i]) for i in range(2)]
        assert [g.tobytes() for g in got] == [F32(x).tobytes() for x in k], name
    mean = (float(e.src_moments.mean()), float(e.ref_moments.mean()))
    off = tuple(abs(m - c) for m, c in zip(mean, shift))
    bound = ex.n0_rel_bound(e.n, e.spread(), off, depth=160 + len(vals))    # numpy's pairwise sums
    assert abs(norm[0] - e.n0) <= bound * e.n0, name
    assert abs(norm[1] - e.norm1) <= e.norm1_tol(norm[0]), name


# ---- the sample of norm_sample_kernel restated: the constructed rasters take their branch --------------------------------
@pytest.mark.parametrize('side', ['low', 'high'])
@pytest.mark.parametrize('shape', [(256, 320), (1000, 999)])
def test_pivot_miss_construction(side, shape):
    """ The restatement (oracle/exact_stats.py sample_positions, sample_ranks, sample_restated, pivot_decision) mirrors
    hk_norm.hip norm_sample_kernel -- `step`, the three `hsh` lines and `p` (one hashed pixel per stratum), `ia` / `ib` and
    the pivots `ws.lo` / `ws.hi` -- and norm_stats_kernel's decision `nm > mid_cap || k0 < below || k1 >= below + nm` with
    mid_capacity() = H W / 25 + 8192.  Both constructions MISS, and neither overflows: the miss alone routes the band to the
    full-raster select. """
    h, w = shape
    src = ex.pivot_miss_raster(h, w, side, seed=1)
    ref = (F32(2) * src + F32(1)).astype(F32)
    n = h * w
    k0, k1, _ = ex.rank_info(n)
    for d in ex.pivot_decision(src, None, ref, None):
        assert d['m'] == min(4096, n) and 10 <= d['lo'] <= d['hi'] <= 21 + 1, d
        assert d['mid'] <= d['capacity'] == n // 25 + 8192 and not d['overflow'], d
        assert d['miss'], d
        if side == 'low':
            assert k0 < d['below'], d                     # more than k0 values below the low pivot
        else:
            assert d['below'] <= k0 and k1 >= d['below'] + d['mid'], d
    # the regular path would have resolved the ranks: a plain raster of the same shape does not miss
    plain = np.random.default_rng(2).uniform(10, 11, (h, w)).astype(F32)
    assert not any(d['miss'] or d['overflow'] for d in ex.pivot_decision(plain, None, plain, None))


def test_sample_positions_one_per_stratum():
    for h, w in ((1, 1), (3, 5), (64, 64), (65, 64), (1, 70000), (7000, 3)):
        pos = ex.sample_positions(h, w)
        total = h * w
        step = max(total // 4096, 1)
        assert (pos < total).all() and (np.diff(pos) > 0).all()
        assert ((pos // step) == np.arange(pos.size)).all()          # stratum j holds sample j
        assert pos.size == min(4096, total)


def test_signed_zero_construction_puts_plus_zero_at_the_low_pivot():
    """ The raster of the GPU test for the pivots' zero sign: the sample's order statistic at rank ia is +0.0, -0.0 values
    lie at the block's 1st percentile (and are not below +0.0 as floats), and the window reaches past the zeros. """
    src = ex.signed_zero_raster(512, 512, seed=3)
    pos = ex.sample_positions(512, 512)
    samp = ex.sort_exact(src.ravel()[pos])
    ia, ib, need_lo, need_hi = ex.sample_ranks(pos.size)
    assert need_lo and need_hi
    assert samp[ia] == 0 and math.copysign(1, samp[ia]) == 1 and samp[ib] > 0
    e = ex.norm_exact(src, None, -src, None)
    assert [math.copysign(1, x) for x in e.src_k] == [-1, -1] and e.src_k == (0, 0)
