"""
ORACLE -- TEST INFRASTRUCTURE ONLY.  The block statistics of gain-blk-offset (kernel_model.py:216-229)

    norm[0] = std(ref) / std(src),   norm[1] = p1(ref) - p1(src) * norm[0]

computed EXACTLY, with numpy and Python integers only (no float32 arithmetic anywhere), to hold hk_norm.hip to the claim
of its header: exact order statistics and float64 moments.

* Jointly valid values follow the reference's mask rules (oracle_np.mask_of).
* Order statistics come from a sort of the float32 values, which is exact.  The sort key is the order-preserving uint32
  image of the float (``f2key``, as in hk_norm.hip), so -0.0 sorts before +0.0 as it does in the kernel's radix select.
* ``p1`` is numpy's 'linear' method written out in float64 on those order statistics: virtual index ``0.01 * (n - 1)``,
  ``k0 = floor``, ``k1 = min(k0 + 1, n - 1)``, ``t = vi - k0`` and numpy's ``_lerp`` with its ``t >= 0.5`` branch -- the formula
  of hk_norm.hip (norm_select_kernel) and oracle/hk_oracle.c (percentile1).  np.percentile on the float32 values
  themselves differs from it BY DESIGN: numpy casts ``t`` and runs the lerp in float32; on float64 copies it is
  this formula bit for bit.
* The moments are exact: every float32 is an integer mantissa (|m| < 2**24) times a power of two; mantissas and squared
  mantissas (split into 12-bit halves so that no int64 sum can overflow) are summed per exponent in int64 and combined
  in Python ints, which gives ``n * sum(v**2) - sum(v)**2`` exactly.  The std ratio is then rounded once to float64 (through
  ``decimal`` with 60 significant digits).

The module also restates the sample of norm_sample_kernel (its positions, pivots and shift) so that tests can build rasters
that take a given branch of the kernel's decision, and it bounds the error of a float64 shifted one-pass evaluation of the
moments (``n0_rel_bound``).
"""
import decimal
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from oracle.oracle_np import mask_of

F32 = np.float32
EPS64 = float(np.finfo(np.float64).eps)  # 2**-52
U64 = EPS64 / 2                          # unit roundoff of float64 round-to-nearest
SAMPLE_N = 4096                          # hk_norm.hip SAMPLE_N
PASS_WAVES = 2048                        # hk_norm.hip PASS_WAVES
WAVE, PX = 64, 4


# ---- values and order ------------------------------------------------------------------------------------------------
def f2key(v) -> np.ndarray:
    """ order-preserving float32 -> uint32 (hk_norm.hip f2key) """
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k) -> np.ndarray:
    k = np.asarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.view(F32)


def joint_values(src, src_nodata, ref, ref_nodata):
    """ the jointly valid (src, ref) values of a block, as float32 """
    mask = mask_of(ref, ref_nodata) & mask_of(src, src_nodata)
    return np.asarray(src, F32)[mask], np.asarray(ref, F32)[mask]


def sort_exact(v) -> np.ndarray:
    """ the float32 values in the kernel's total order (by key: -0.0 before +0.0) """
    return key2f(np.sort(f2key(v)))


def rank_info(n: int):
    """ (k0, k1, t) of numpy's linear 1st percentile of n values: vi = 0.01 (n - 1) in float64 """
    vi = 0.01 * float(n - 1)
    k0 = int(math.floor(vi))
    return k0, min(k0 + 1, n - 1), vi - k0


def lerp(lo: float, hi: float, t: float) -> float:
    """ numpy's _lerp in float64 (lib/_function_base_impl.py) """
    d = hi - lo
    return hi - d * (1.0 - t) if t >= 0.5 else lo + d * t


def lerp32(lo: float, hi: float, t: float) -> float:
    """ the same lerp carried out in float32 (what a float32 percentile does; tests use it as a wrong value) """
    lo, hi, t = F32(lo), F32(hi), F32(t)
    d = F32(hi - lo)
    return float(F32(hi - F32(d * F32(F32(1) - t)))) if t >= 0.5 else float(F32(lo + F32(d * t)))


def p1(values) -> float:
    """ the 1st percentile of float32 values by the exact order statistics and numpy's float64 lerp """
    srt = sort_exact(values)
    k0, k1, t = rank_info(srt.size)
    return lerp(float(srt[k0]), float(srt[k1]), t)


# ---- exact moments ---------------------------------------------------------------------------------------------------
@dataclass
class Moments:
    """ sum(v) = s1 * 2**e and sum(v**2) = s2 * 2**(2 e), exactly (Python ints) """
    n: int
    s1: int
    s2: int
    e: int

    def mean(self) -> Fraction:
        return Fraction(self.s1) * Fraction(2) ** self.e / self.n

    def m2n(self) -> int:
        """ n * sum(v**2) - sum(v)**2, in units of 2**(2 e): n**2 times the population variance """
        return self.n * self.s2 - self.s1 * self.s1

    def var(self) -> Fraction:
        return Fraction(self.m2n()) * Fraction(2) ** (2 * self.e) / (self.n * self.n)


def exact_moments(values) -> Moments:
    v = np.asarray(values, F32).astype(np.float64)
    n = int(v.size)
    if n == 0:
        return Moments(0, 0, 0, 0)
    m, ex = np.frexp(v)                             # v = m * 2**ex, 0.5 <= |m| < 1 (float32 values: 24 bits of mantissa)
    mi = np.ldexp(m, 24).astype(np.int64)           # exact: |mi| < 2**24
    ex = ex.astype(np.int64) - 24
    ex[mi == 0] = ex[mi != 0].min() if (mi != 0).any() else 0
    order = np.argsort(ex, kind='stable')
    mi, ex = mi[order], ex[order]
    starts = np.flatnonzero(np.r_[True, ex[1:] != ex[:-1]])
    hi, lo = mi >> 12, mi & 0xfff                   # mi = hi * 2**12 + lo, |hi|, lo < 2**12: every product < 2**24
    a = np.add.reduceat(mi, starts)                 # int64 sums: < 2**24 * n, < 2**24 * 2**39 fits
    hh, hl, ll = (np.add.reduceat(x, starts) for x in (hi * hi, hi * lo, lo * lo))
    e0 = int(ex[0])
    s1 = s2 = 0
    for i, st in enumerate(starts):
        sh = int(ex[st]) - e0
        s1 += int(a[i]) << sh
        s2 += ((int(hh[i]) << 24) + (int(hl[i]) << 13) + int(ll[i])) << (2 * sh)
    return Moments(n, s1, s2, e0)


def _ratio_sqrt(num: int, den: int, scale2: int) -> float:
    """ sqrt(num / den * 2**scale2) rounded once to float64 (num, den > 0) """
    with decimal.localcontext() as c:
        c.prec = 60
        q = decimal.Decimal(num) / decimal.Decimal(den)
        q = q * (decimal.Decimal(2) ** scale2) if scale2 >= 0 else q / (decimal.Decimal(2) ** -scale2)
        return float(q.sqrt())


def std_ratio(ms: Moments, mr: Moments) -> float:
    """ std(ref) / std(src) rounded once to float64; 0 / 0 -> nan, x / 0 -> inf (numpy's classes) """
    a, b = mr.m2n(), ms.m2n()
    if b == 0:
        return float('nan') if a == 0 else float('inf')
    if a == 0:
        return 0.0
    return _ratio_sqrt(a, b, 2 * (mr.e - ms.e))


# ---- the exact block statistics -----------------------------------------------------------------------------------------
@dataclass
class NormExact:
    n: int
    n0: float                       # std ratio, rounded once
    norm1: float                    # p1(ref) - p1(src) * n0 in float64
    k0: int = 0
    k1: int = 0
    t: float = 0.0
    src_k: tuple = (0.0, 0.0)       # order statistics k0, k1 of src / ref (float32 values)
    ref_k: tuple = (0.0, 0.0)
    p1_src: float = 0.0
    p1_ref: float = 0.0
    src_sorted: Optional[np.ndarray] = None
    ref_sorted: Optional[np.ndarray] = None
    src_moments: Optional[Moments] = None
    ref_moments: Optional[Moments] = None

    @property
    def norm(self) -> np.ndarray:
        return np.array([self.n0, self.norm1])

    def spread(self):
        """ (std(src), std(ref)) as floats """
        return tuple(math.sqrt(float(m.var())) for m in (self.src_moments, self.ref_moments))

    def norm1_with(self, n0: float, dk: int = 0, use_lerp32: bool = False) -> float:
        """ norm1 with the given std ratio, with both ranks moved by ``dk`` (clipped to [0, n - 1]) and/or with the lerp
        carried out in float32 -- the values a subtly wrong kernel would return """
        k0 = min(max(self.k0 + dk, 0), self.n - 1)
        k1 = min(k0 + 1, self.n - 1)
        f = lerp32 if use_lerp32 else lerp
        ps = f(float(self.src_sorted[k0]), float(self.src_sorted[k1]), self.t)
        pr = f(float(self.ref_sorted[k0]), float(self.ref_sorted[k1]), self.t)
        return pr - ps * n0

    def norm1_tol(self, n0: float) -> float:
        """ |norm1 - norm1*| allowed for a kernel whose std ratio is ``n0``: four float64 roundings of the two terms plus
        what the std ratio's own error moves the product by """
        return 4 * EPS64 * (abs(self.p1_ref) + abs(self.p1_src * n0)) + abs(self.p1_src) * abs(n0 - self.n0)


def norm_exact(src, src_nodata, ref, ref_nodata) -> NormExact:
    s, r = joint_values(src, src_nodata, ref, ref_nodata)
    return norm_exact_values(s, r)


def norm_exact_values(s, r) -> NormExact:
    n = int(s.size)
    if n == 0:                                     # kernel_model.py:223-226
        return NormExact(0, 0.0, 0.0)
    ms, mr = exact_moments(s), exact_moments(r)
    n0 = std_ratio(ms, mr)
    ss, rs = sort_exact(s), sort_exact(r)
    k0, k1, t = rank_info(n)
    ps = lerp(float(ss[k0]), float(ss[k1]), t)
    pr = lerp(float(rs[k0]), float(rs[k1]), t)
    with np.errstate(all='ignore'):
        norm1 = float(np.float64(pr) - np.float64(ps) * np.float64(n0))
    return NormExact(n, n0, norm1, k0, k1, t, (ss[k0], ss[k1]), (rs[k0], rs[k1]), ps, pr, ss, rs, ms, mr)


# ---- error bound of a float64 shifted one-pass evaluation --------------------------------------------------------------
def sum_depth(height: int, width: int, slabs: int = 1) -> int:
    """ Longest chain of float64 additions behind one moment sum of hk_norm.hip for a height x width plane: a lane adds its
    values one by one (PX per 1 KB chunk, one chunk in every G of the plane -- pass_waves), then a 64-lane butterfly,
    PASS_WAVES / 256 partials per thread of norm_stats_kernel, another butterfly, four wave sums (+ the ranks' sum of a split
    block).  Mirrors pass_waves(). """
    wq = (width + PX - 1) // PX
    chunks = height * ((wq + WAVE - 1) // WAVE)
    g = min(max(chunks // 16, 64), PASS_WAVES)
    per_lane = PX * ((chunks + g - 1) // g)
    return per_lane + 6 + PASS_WAVES // 256 + 6 + 4 + slabs


def n0_rel_bound(n: int, spread, offset, depth: Optional[int] = None) -> float:
    """
    Bound on |n0 - n0*| / n0* for n0 = sqrt(var_ref) / sqrt(var_src), where each variance is evaluated in float64 as
    ``m2 / n - (m1 / n)**2`` with m1 = sum(d), m2 = sum(d * d) (fma), d = v - c for a shift c.

    ``n``: the values summed; ``spread``: std of (src, ref) (a scalar applies to both); ``offset``: |mean - c| of (src, ref);
    ``depth``: the longest chain of additions of the sums (``sum_depth``; default ``n``, a plain running sum).

    With Q = sum(d**2) = n (s**2 + a**2) (s = spread, a = offset) and gamma_k = k u / (1 - k u):
      |m2^ - Q|      <= gamma_{D+3} Q                          (d rounded once, squared-and-added once per node)
      |m1^/n - a|    <= gamma_{D+2} sqrt(s**2 + a**2) + u |a|   (Cauchy-Schwarz on sum |d|)  =: e1
      |var^ - s**2|  <= gamma_{D+5} (s**2 + a**2) + (2 |a| + e1) e1 + 2 u (a**2 + s**2)
    so rho = that / s**2 per raster, and n0 = sqrt(var_r) / sqrt(var_s) (two square roots and a division, rounded):
      |n0 / n0* - 1| <= sqrt((1 + rho_r) / (1 - rho_s)) (1 + u)**3 - 1.
    A case whose bound would exceed 1e-11 raises ValueError: the bound is never looser than that, so a test has to use
    data on which a float32 moment (or any error above 1e-11) is visible.
    """
    sp = tuple(spread) if np.ndim(spread) else (spread, spread)
    of = tuple(offset) if np.ndim(offset) else (offset, offset)
    d = int(n if depth is None else depth)
    u = U64

    def gamma(k):
        return k * u / (1 - k * u)

    rho = []
    for s, a in zip(sp, of):
        s, a = float(s), abs(float(a))
        if not s > 0:
            raise ValueError('n0_rel_bound: zero spread')
        big = s * s + a * a
        e1 = gamma(d + 2) * math.sqrt(big) + u * a
        err = gamma(d + 5) * big + (2 * a + e1) * e1 + 2 * u * big
        rho.append(err / (s * s))
    rho_s, rho_r = rho
    if rho_s >= 0.5:
        raise ValueError(f'n0_rel_bound: ill-conditioned (rho {rho_s:.3g})')
    b = math.sqrt((1 + rho_r) / (1 - rho_s)) * (1 + u) ** 3 - 1
    b = b * (1 + 1e-6) + 4 * u   # margin for the float64 evaluation of this formula
    if b > 1e-11:
        raise ValueError(f'n0_rel_bound: {b:.3g} is looser than 1e-11 (n {n}, spread {sp}, offset {of}, depth {d})')
    return b


# ---- the sample of norm_sample_kernel ----------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def sample_positions(height: int, width: int) -> np.ndarray:
    """ Flat pixel indices the sample of a height x width plane reads, in the order of j (hk_norm.hip norm_sample_kernel,
    the `step` / `hsh` / `p` lines): one pixel per stratum of step = total // 4096 pixels (1 when the plane has fewer),
    at a 64-bit hash of the stratum index; indices at or past the plane's end are skipped. """
    total = height * width
    step = total // SAMPLE_N if total // SAMPLE_N > 0 else 1
    out = []
    for j in range(SAMPLE_N):
        h = ((j + 0x9e3779b97f4a7c15) * 0xbf58476d1ce4e5b9) & _M64
        h = ((h ^ (h >> 29)) * 0x94d049bb133111eb) & _M64
        h ^= h >> 32
        p = j * step + h % step
        if p < total:
            out.append(p)
    return np.array(out, np.int64)


def sample_ranks(m: int):
    """ (ia, ib, need_lo, need_hi): the sample ranks that bracket the 1st percentile (norm_sample_kernel, `ia` / `ib`) """
    c = 0.01 * m
    sd = math.sqrt(c) if c > 0 else 0.0
    ia, ib = int(math.floor(c - 4.0 * sd)) - 2, int(math.ceil(c + 4.0 * sd)) + 3
    return ia, ib, not (m == 0 or ia <= 0), not (m == 0 or ib >= m - 1)


def mid_capacity(n_px: int) -> int:
    """ hk_norm.hip mid_capacity: the compaction buffer of one raster """
    return n_px // 25 + 8192


def sample_restated(src, src_nodata, ref, ref_nodata):
    """ What norm_sample_kernel derives for one plane: per raster (src, ref) the sample count m, the shift (the sample mean;
    summed here in another order, so equal up to float64 rounding) and the pivots lo / hi (+-inf when not needed). """
    h, w = src.shape
    pos = sample_positions(h, w)
    s, r = np.asarray(src, F32).ravel()[pos], np.asarray(ref, F32).ravel()[pos]
    ok = mask_of(s, src_nodata) & mask_of(r, ref_nodata)
    out = []
    for v in (s[ok], r[ok]):
        m = int(v.size)
        ia, ib, need_lo, need_hi = sample_ranks(m)
        srt = sort_exact(v)
        mean = float(np.sum(v.astype(np.float64))) / m if m else 0.0
        out.append(dict(m=m, shift=mean if math.isfinite(mean) else 0.0, ia=ia, ib=ib,
                        lo=F32(srt[ia]) if need_lo else F32(-np.inf), hi=F32(srt[ib]) if need_hi else F32(np.inf)))
    return out


def pivot_decision(src, src_nodata, ref, ref_nodata):
    """ The streaming pass and norm_stats_kernel's decision restated for one plane: per raster the count below the low
    pivot, the count compacted (lo <= v <= hi in float compares), whether the pivots MISS (k0 < below or k1 >= below + mid)
    and whether the buffer OVERFLOWS (mid > mid_capacity(H W)). """
    samp = sample_restated(src, src_nodata, ref, ref_nodata)
    s, r = joint_values(src, src_nodata, ref, ref_nodata)
    n = int(s.size)
    k0, k1, _ = rank_info(n) if n else (0, 0, 0.0)
    cap = mid_capacity(src.shape[0] * src.shape[1])
    out = []
    for v, sm in zip((s, r), samp):
        below = int(np.count_nonzero(v < sm['lo']))
        mid = int(np.count_nonzero((v <= sm['hi']) & ~(v < sm['lo'])))
        out.append(dict(sm, below=below, mid=mid, capacity=cap, miss=bool(k0 < below or k1 >= below + mid),
                        overflow=bool(mid > cap)))
    return out


# ---- rasters built on the sample: each one takes a chosen branch of the kernel's decision ----------------------------------
def pivot_miss_raster(height: int, width: int, side: str, seed: int = 0) -> np.ndarray:
    """ A plane whose sampled pixels all lie in U[10, 11] while the unsampled ones do not follow them, so that the pivots
    bracket the sample's 1st percentile but not the plane's.  side='low': 6 % of the unsampled pixels in U[0, 1] (below the
    low pivot: more than k0 values), the rest in U[20, 21]; side='high': 0.5 % low, the rest high (fewer than k0 values below
    the low pivot, and the window holds only sampled pixels).  Needs step > 1 (more than 2 * 4096 pixels). """
    rng = np.random.default_rng(seed)
    total = height * width
    assert total // SAMPLE_N >= 2, 'the construction needs unsampled pixels in every stratum'
    v = rng.uniform(20, 21, total)
    sampled = np.zeros(total, bool)
    sampled[sample_positions(height, width)] = True
    un = np.flatnonzero(~sampled)
    frac = {'low': 0.06, 'high': 0.005}[side]
    v[rng.choice(un, int(frac * un.size), replace=False)] = rng.uniform(0, 1, int(frac * un.size))
    v[sampled] = rng.uniform(10, 11, int(sampled.sum()))
    return v.astype(F32).reshape(height, width)


def signed_zero_raster(height: int, width: int, seed: int = 0) -> np.ndarray:
    """ A plane whose sample holds +0.0 at the low pivot's rank while the plane's 1st percentile lies among -0.0 values:
    ~0.7 % of the sampled pixels are +0.0, 2 % of the unsampled ones -0.0, the rest U[1, 2].  Sorted by key, -0.0 comes
    first, so the exact order statistics at k0, k1 are -0.0. """
    rng = np.random.default_rng(seed)
    total = height * width
    v = rng.uniform(1, 2, total).astype(F32)
    pos = sample_positions(height, width)
    sampled = np.zeros(total, bool)
    sampled[pos] = True
    un = np.flatnonzero(~sampled)
    v[rng.choice(pos, int(0.007 * pos.size), replace=False)] = F32(0.0)
    v[rng.choice(un, int(0.02 * un.size), replace=False)] = F32(-0.0)
    return v.reshape(height, width)
