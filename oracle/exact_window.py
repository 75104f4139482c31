"""
ORACLE -- TEST INFRASTRUCTURE ONLY.  Exact window sums of the fused fit (csrc/hk_fit_kernel.h) and sound enclosures of
what any admissible float64 summation of them -- and everything the contract computes from them -- may give.

The window sums
---------------
The contract (HISTORY.md section 2) fixes every rounding of the fit except the order of the float64
window summation.  ``oracle_np.box_sum`` sums each window directly (rows of ``kw`` left to right, then ``kh`` rows top to
bottom); the kernel keeps RUNNING column sums (add the entering row, subtract the leaving one) restarted at the top of every
row segment, and combines ``kw`` column sums across lanes in a prefix / suffix order.  The two agree bit for bit only where
every partial sum is exact.  This module computes the exact sums and bounds the distance of either summation from them.

Exact sums.  Every float32 is an integer multiple of 2^-149, every float64 product of two float32 values a multiple of
2^-298, every float64 a multiple of 2^-1074.  The summed values are therefore scaled to Python integers (by the smallest
lowest-set-bit exponent present), summed with 2-D prefix sums (zero border) and rounded once to float64: CPython's integer
true division and int -> float conversion round correctly, in the subnormal range as well.

Bound ``B(y, x)`` on |float64 window sum - exact sum|, for ANY row-segment partition and any order of the horizontal
combination.  ``u = 2^-53``, ``a = |value|``.

* Vertical.  A segment's running sum starts from 0 at the segment's first priming row; the worst start is the top of the
  raster (a later start performs a subset of the same operations on the same values).  Between an add and a subtract the
  accumulator holds at most ``kh + 1`` consecutive rows, so every partial sum is bounded by
  ``A_t = sum of a over rows t - kh .. t`` of its column, and each of the two roundings of step ``t`` errs by at most
  ``u * A_t`` (times ``1 + O(n u)`` for the error already carried, absorbed in a final factor).  Column ``x`` at output row
  ``y`` carries ``Ev <= 2 u * sum_{t <= y + rh} A_t``.
* Horizontal.  ``kw`` column sums combined in any order take ``kw - 1`` additions, each erring by at most ``u`` times a
  partial sum, bounded by the window's ``sum a`` plus the column errors: ``Eh <= (kw - 1) u (sum_window a + sum Ev)``.
* The direct sums of the oracles (numpy and C, same order) err by at most ``(kw + kh - 2) u * sum_window a``.
* ``B = 1.001 * max(sum_window Ev + Eh, direct bound)`` plus 2^-1074 per operation for the subnormal range.
* Exactness rule: a running sum is exact when all its values are multiples of 2^e and every partial sum is below
  2^(53 + e).  With ``e`` the smallest lowest-set-bit exponent of the values of a column from the top of the raster down to
  the window's last row, the column sum is exact when ``max A_t < 2^(53 + e)``; the window is exact when its ``kw`` columns
  are and ``sum_window a < 2^(53 + min e)``.  That also makes every partial sum of the direct summation exact.  There
  ``B = 0``: integer rasters and narrow-range data (e.g. values in [1, 2)) collapse to single values.
* gain-blk-offset without R2 normalises the window sum of the RAW source instead of summing normalised pixels (DESIGN.md
  section 2, deviation iii): ``S' = RN(RN(n0 * S) + RN(n1 * N))``.  Its enclosure is the hull of that expression over the
  enclosure of ``S`` and of the enclosure of the direct sum of normalised pixels.

Interval evaluation
-------------------
Every quantity is carried as ``Iv(lo, hi, und)``.  Each IEEE operation is evaluated in its own dtype and order (the numpy
expressions of ``oracle_np``, hence its promotion rules) at the corners of its input intervals: rounded +, -, x and / are
monotone in each argument, so the corners bound every result.  A division whose divisor interval contains 0 (unless it is
the single value 0 and the dividend interval excludes 0) is undetermined (``und``): any value, inf or NaN; so is a product
of an interval holding 0 with one reaching infinity.  So is a result whose corners are partly NaN.  A result
whose corners are all NaN is NaN.  On data whose sums are exact every interval collapses to the oracle's single value.
"""
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from oracle.oracle_np import mask_of, nan_equals

F32, F64 = np.float32, np.float64
U = 2.0 ** -53
TINY = 2.0 ** -1074
_BIG = 1 << 20  # lowest-set-bit exponent of 0


# ---- exact sums ---------------------------------------------------------------------------------------------------------
def lsb_exp(v: np.ndarray) -> np.ndarray:
    """ exponent of the lowest set bit of each float64 (``_BIG`` for 0): v = odd integer * 2^lsb_exp(v) """
    m, e = np.frexp(np.asarray(v, F64))
    mi = (m * 2.0 ** 53).astype(np.int64)  # exact: 53-bit integer mantissa
    low = mi & -mi
    out = np.full(mi.shape, _BIG, np.int64)
    nz = mi != 0
    out[nz] = e[nz].astype(np.int64) - 53 + np.log2(low[nz].astype(F64)).astype(np.int64)
    return out


def _scaled_ints(v: np.ndarray):
    """ (object array of Python ints I, e0) with v == I * 2^e0 exactly """
    v = np.asarray(v, F64)
    m, e = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    ex = e.astype(np.int64) - 53
    nz = mi != 0
    e0 = int(ex[nz].min()) if nz.any() else 0
    sh = np.where(nz, ex - e0, 0)
    flat = [(a << b) if a >= 0 else -((-a) << b) for a, b in zip(mi.ravel().tolist(), sh.ravel().tolist())]
    out = np.empty(v.size, dtype=object)
    out[:] = flat
    return out.reshape(v.shape), e0


def _round_f64(i: int, e0: int) -> float:
    """ RN64(i * 2^e0) """
    try:
        return float(i << e0) if e0 >= 0 else i / (1 << -e0)
    except OverflowError:
        return float('inf') if i > 0 else float('-inf')


def exact_window_sum(v: np.ndarray, kernel_shape):
    """ the exact zero-border ``kh x kw`` window sums of the float64 values ``v``: (object array of ints, e0, RN64 of them) """
    kh, kw = int(kernel_shape[0]), int(kernel_shape[1])
    rh, rw = kh // 2, kw // 2
    h, w = v.shape
    ints, e0 = _scaled_ints(v)
    pre = np.zeros((h + 1, w + 1), dtype=object)
    pre[:] = 0
    if h and w:
        pre[1:, 1:] = np.cumsum(np.cumsum(ints, axis=0), axis=1)
    y0 = np.clip(np.arange(h) - rh, 0, h)[:, None]
    y1 = np.clip(np.arange(h) + rh + 1, 0, h)[:, None]
    x0 = np.clip(np.arange(w) - rw, 0, w)[None, :]
    x1 = np.clip(np.arange(w) + rw + 1, 0, w)[None, :]
    win = pre[y1, x1] - pre[y0, x1] - pre[y1, x0] + pre[y0, x0]
    rn = np.array([_round_f64(i, e0) for i in win.ravel().tolist()], F64).reshape(h, w)
    return win, e0, rn


def _box_nonneg(a: np.ndarray, kh: int, kw: int) -> np.ndarray:
    """ direct zero-border window sums of non-negative values (relative error <= (kh + kw) u: no cancellation) """
    h, w = a.shape
    rh, rw = kh // 2, kw // 2
    pad = np.zeros((h + 2 * rh, w + 2 * rw))
    pad[rh:rh + h, rw:rw + w] = a
    rows = np.zeros((h + 2 * rh, w))
    for dx in range(kw):
        rows += pad[:, dx:dx + w]
    out = np.zeros((h, w))
    for dy in range(kh):
        out += rows[dy:dy + h]
    return out


def _hbox(a: np.ndarray, kw: int) -> np.ndarray:
    """ zero-border horizontal window sums of non-negative values """
    h, w = a.shape
    rw = kw // 2
    pad = np.zeros((h, w + 2 * rw))
    pad[:, rw:rw + w] = a
    out = np.zeros((h, w))
    for dx in range(kw):
        out += pad[:, dx:dx + w]
    return out


def _hmin(a: np.ndarray, kw: int) -> np.ndarray:
    h, w = a.shape
    rw = kw // 2
    pad = np.full((h, w + 2 * rw), _BIG, np.int64)
    pad[:, rw:rw + w] = a
    out = np.full((h, w), _BIG, np.int64)
    for dx in range(kw):
        out = np.minimum(out, pad[:, dx:dx + w])
    return out


def _pow2(e: np.ndarray) -> np.ndarray:
    with np.errstate(over='ignore'):
        return np.ldexp(1.0, np.clip(e, -1100, 1100).astype(np.int32))


def sum_bound(v: np.ndarray, kernel_shape):
    """ (B, exact): the bound of the module docstring on |float64 window sum - exact sum| and where it is 0 """
    kh, kw = int(kernel_shape[0]), int(kernel_shape[1])
    rh = kh // 2
    h, w = v.shape
    a = np.abs(np.asarray(v, F64))
    # rows t = 0 .. h - 1 + rh (the window's last row may lie below the raster: zero rows)
    ap = np.zeros((h + rh, w))
    ap[:h] = a
    ep = np.full((h + rh, w), _BIG, np.int64)
    ep[:h] = lsb_exp(v)
    # A_t = sum of a over rows t - kh .. t, summed directly (a difference of running totals could cancel below the truth)
    A = ap.copy()
    for d in range(1, kh + 1):
        A[d:] += ap[:-d] if d < h + rh else 0.0
    A = A * (1 + 1e-9) + TINY
    ev = 2 * U * np.cumsum(A, axis=0)                          # column error at the step of row t
    e_cum = np.minimum.accumulate(ep, axis=0)
    a_max = np.maximum.accumulate(A, axis=0)
    v_exact = a_max < _pow2(53 + e_cum)
    # output row y reads the column state after row y + rh
    ev_y, vex_y, e_y = ev[rh:rh + h], v_exact[rh:rh + h], e_cum[rh:rh + h]
    win_a = _box_nonneg(a, kh, kw) * (1 + 1e-9)
    sum_ev = _hbox(ev_y, kw)
    bk = sum_ev + (kw - 1) * U * (win_a + sum_ev)
    bd = (kw + kh - 2) * U * win_a
    n_ops = 2.0 * (h + 2 * rh + 1) * kw + kh * kw
    b = 1.001 * np.maximum(bk, bd) + n_ops * TINY
    all_vex = _hbox((~vex_y).astype(F64), kw) == 0
    exact = all_vex & (win_a < _pow2(53 + _hmin(e_y, kw)))
    return np.where(exact, 0.0, b), exact


def window_enclosure(v: np.ndarray, kernel_shape) -> 'Iv':
    """ float64 enclosure of every admissible float64 window sum of ``v`` (a single value where the sums are exact) """
    _, _, rn = exact_window_sum(v, kernel_shape)
    b, exact = sum_bound(v, kernel_shape)
    with np.errstate(all='ignore'):
        lo = np.nextafter(np.nextafter(rn - b, -np.inf), -np.inf)
        hi = np.nextafter(np.nextafter(rn + b, np.inf), np.inf)
    lo = np.where(exact, rn, lo)
    hi = np.where(exact, rn, hi)
    return Iv(lo, hi)


# ---- intervals ----------------------------------------------------------------------------------------------------------
class Iv:
    """ [lo, hi] per element; ``und``: undetermined (any value, inf or NaN); lo = hi = NaN: exactly NaN """
    __slots__ = ('lo', 'hi', 'und')

    def __init__(self, lo, hi=None, und=None):
        self.lo = np.asarray(lo)
        self.hi = self.lo if hi is None else np.asarray(hi)
        self.und = np.zeros(np.broadcast(self.lo, self.hi).shape, bool) if und is None else np.asarray(und, bool)

    def astype(self, dt) -> 'Iv':
        with np.errstate(all='ignore'):
            return Iv(self.lo.astype(dt), self.hi.astype(dt), self.und)

    @property
    def point(self) -> np.ndarray:
        """ where the enclosure is one value (NaN included) """
        same = (self.lo == self.hi) | (np.isnan(self.lo) & np.isnan(self.hi))
        return ~self.und & same

    def where(self, cond, other: 'Iv') -> 'Iv':
        other = _iv(other)
        return Iv(np.where(cond, self.lo, other.lo), np.where(cond, self.hi, other.hi), np.where(cond, self.und, other.und))

    def contains(self, x) -> np.ndarray:
        """ per element: ``x`` is admissible (bit for bit where the enclosure is a single value, NaN pattern included) """
        x = np.asarray(x)
        xn, ln = np.isnan(x), np.isnan(self.lo) & np.isnan(self.hi)
        with np.errstate(all='ignore'):
            inside = ~xn & ~ln & (self.lo <= x) & (x <= self.hi)
        ok = self.und | (xn & ln) | inside
        # single values: the bits too (the sign of a zero); NaN already matched above
        if self.lo.dtype == x.dtype:
            lo = np.broadcast_to(self.lo, x.shape)
            bits_eq = lo.view(_uint(x.dtype)) == x.view(_uint(x.dtype))
            ok = ok & ~(self.point & ~ln & ~bits_eq)
        return ok


def _uint(dt):
    return np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64


def _iv(x) -> Iv:
    return x if isinstance(x, Iv) else Iv(np.asarray(x))


def _has0(a: Iv) -> np.ndarray:
    with np.errstate(invalid='ignore'):
        return (a.lo <= 0) & (a.hi >= 0)


def _has_inf(a: Iv) -> np.ndarray:
    return np.isinf(a.lo) | np.isinf(a.hi)


def _corners(f, a, b, div=False, mul=False) -> Iv:
    a, b = _iv(a), _iv(b)
    with np.errstate(all='ignore'):
        c = np.stack(np.broadcast_arrays(f(a.lo, b.lo), f(a.lo, b.hi), f(a.hi, b.lo), f(a.hi, b.hi)))
    nan = np.isnan(c)
    all_nan, any_nan = nan.all(0), nan.any(0)
    with np.errstate(all='ignore'):
        lo = np.where(any_nan, np.nan, c.min(0)).astype(c.dtype)
        hi = np.where(any_nan, np.nan, c.max(0)).astype(c.dtype)
    und = a.und | b.und | (any_nan & ~all_nan)
    # an interior point may give NaN where no corner does: x / 0 for x of either sign, 0 * inf
    if div:
        und = und | (_has0(b) & (~(b.lo == b.hi) | _has0(a)))
    if mul:
        und = und | (_has0(a) & _has_inf(b)) | (_has0(b) & _has_inf(a))
    return Iv(lo, hi, und)


def add(a, b):
    return _corners(np.add, a, b)


def sub(a, b):
    return _corners(np.subtract, a, b)


def mul(a, b):
    return _corners(np.multiply, a, b, mul=True)


def div(a, b):
    return _corners(np.divide, a, b, div=True)


# ---- the contract's expressions (oracle_np, dtype by dtype) -------------------------------------------------------------
def _f32(x):
    return _iv(x).astype(F32)


def _f64(x):
    return _iv(x).astype(F64)


def r2_iv(N, R, R2, S, S2, P, g, o=None, p_f64=False) -> Iv:
    """ oracle_np.r2_array (kernel_model.py:142-214) on enclosures; ``o`` None: the one-parameter form.  ``p_f64``: the
    gain-blk-offset flavour, whose S and P are float64 """
    sstot = sub(mul(_f64(N), R2), _f64(mul(R, R)))
    gg = mul(g, g)
    if o is not None:
        B = mul(mul(F32(2), mul(g, o)), S)                        # f32(f32(2 f32(g o)) S)
        C = mul(mul(F32(2), g), P)
        D = mul(mul(F32(2), o), R)
        F = mul(N, mul(o, o))
        ssres = add(sub(sub(add(mul(_f64(gg), S2), _f64(B)), _f64(C)), _f64(D)), R2)
        ssres = add(ssres, _f64(F))
    else:
        C = mul(_f64(mul(F32(2), g)), P) if p_f64 else _f64(mul(mul(F32(2), g), P))
        ssres = add(sub(mul(_f64(gg), S2), C), R2)
    ssres = mul(ssres, _f64(N))
    q = _f32(div(ssres, sstot))
    return sub(F32(1), q)


@dataclass
class Enclosure:
    mask: np.ndarray
    params: list                      # Iv per parameter band (gain, offset[, r2]); NaN outside the mask
    corr: Iv                          # the corrected pixels from the first-pass parameters
    sums: Dict[str, Iv] = field(default_factory=dict)
    certain_pass: Optional[np.ndarray] = None   # r2 mask (gain-offset with a threshold): certainly True ...
    certain_fail: Optional[np.ndarray] = None   # ... certainly False (valid pixels only)
    undecided: Optional[np.ndarray] = None      # ... either

    def undecided_fraction(self) -> float:
        n = int(self.mask.sum())
        return 0.0 if self.undecided is None or n == 0 else float(self.undecided.sum()) / n


def _nan_outside(iv: Iv, mask) -> Iv:
    return iv.where(mask, Iv(np.full(mask.shape, np.nan, iv.lo.dtype)))


def _sums(vals: Dict[str, np.ndarray], kernel_shape) -> Dict[str, Iv]:
    return {k: window_enclosure(v, kernel_shape) for k, v in vals.items()}


def enclose(model: str, src, src_nodata, ref, ref_nodata, kernel_shape=(5, 5), find_r2=False, r2_inpaint_thresh=None,
            norm_model=None) -> Enclosure:
    """ Enclosures of ``oracle_np.fit`` + ``apply`` (kernel_model.py:231-373, 442-463) for every admissible float64 window
    summation.  ``r2_inpaint_thresh`` (gain-offset only) decides the r2 mask: certain pass / certain fail / undecided; the
    in-painting of failing pixels is not enclosed (``corr`` and the parameters hold there only where the mask passes). """
    src = np.array(src, F32)
    ref = np.array(ref, F32)
    kh, kw = int(kernel_shape[0]), int(kernel_shape[1])
    thresh = r2_inpaint_thresh if model == 'gain-offset' else None
    want_r2 = find_r2 or thresh is not None
    with np.errstate(all='ignore'):
        if model == 'gain-blk-offset':
            n = np.asarray(norm_model, F64)
            s_nd = src.copy()
            if src_nodata is not None and not nan_equals(np.nan, src_nodata):
                s_nd[~mask_of(src, src_nodata)] = np.nan
            sd = (s_nd * n[0]) + n[1]
            mask = mask_of(sd, np.nan) & mask_of(ref, ref_nodata)
        else:
            mask = mask_of(ref, ref_nodata) & mask_of(src, src_nodata)
        s0 = np.where(mask, src, F32(0))
        r0 = np.where(mask, ref, F32(0))
        vals = {'R': r0.astype(F64)}
        if model == 'gain-blk-offset':
            sd0 = np.where(mask, sd, 0.0)
            vals['S'] = sd0
            if want_r2:
                vals['P'] = sd0 * r0.astype(F64)
                vals['S2'] = sd0 * sd0
            else:
                vals['Sraw'] = s0.astype(F64)
        else:
            vals['S'] = s0.astype(F64)
            if want_r2 or model == 'gain-offset':
                vals['P'] = (s0 * r0).astype(F64)
                vals['S2'] = s0.astype(F64) ** 2
        if want_r2:
            vals['R2'] = r0.astype(F64) ** 2
    sums = _sums(vals, kernel_shape)
    N = Iv(_box_nonneg(mask.astype(F64), kh, kw).astype(F32))  # counts: exact in any order
    sums['N'] = N
    R = _f32(sums['R'])
    if model == 'gain-blk-offset':
        S = sums['S']
        if not want_r2:
            # the kernel's form RN(RN(n0 * S) + RN(n1 * N)), hulled with the direct sum of normalised pixels
            k = add(mul(sums['Sraw'], F64(n[0])), mul(F64(n[1]), _f64(N)))
            S = Iv(np.fmin(S.lo, k.lo), np.fmax(S.hi, k.hi), S.und | k.und)
            sums['S'] = S
        g = _f32(div(_f64(R), S))
        params = [g]
        if want_r2:
            params.append(r2_iv(N, R, sums['R2'], S, sums['S2'], sums['P'], g, None, p_f64=True))
        o = _f32(mul(g, F64(n[1])))
        g_out = _f32(mul(g, F64(n[0])))
        params = [g_out, o] + params[1:]
    else:
        S = _f32(sums['S'])
        if model == 'gain':
            g = div(R, S)
            o = Iv(np.zeros(src.shape, F32))
            params = [g, o]
            if want_r2:
                params.append(r2_iv(N, R, sums['R2'], S, sums['S2'], _f32(sums['P']), g))
        elif model == 'gain-offset':
            P = _f32(sums['P'])
            num = sub(mul(N, P), mul(S, R))
            den = sub(mul(_f64(N), sums['S2']), _f64(mul(S, S)))
            g = _f32(div(_f64(num), den))
            o = div(sub(R, mul(g, S)), N)
            params = [g, o]
            if want_r2:
                params.append(r2_iv(N, R, sums['R2'], S, sums['S2'], P, g, o))
        else:
            raise ValueError(model)
    params = [_nan_outside(p, mask) for p in params]
    corr = add(mul(params[0], src), params[1])
    enc = Enclosure(mask=mask, params=params, corr=corr, sums=sums)
    return decide(enc, thresh) if thresh is not None else enc


def decide(enc: Enclosure, thresh: float) -> Enclosure:
    """ the r2 mask of kernel_model.py:363, ``r2 > thresh and gain > 0`` (numpy's comparison of the float32 planes), on the
    enclosures of a gain-offset fit with R2: certain pass / certain fail / undecided per valid pixel """
    r2, gq, mask = enc.params[2], enc.params[0], enc.mask
    with np.errstate(invalid='ignore'):
        det = ~r2.und & ~gq.und
        certain_pass = mask & det & (r2.lo > thresh) & (gq.lo > 0)
        fail_r2 = ~r2.und & ~(r2.hi > thresh) & ~(r2.lo > thresh)
        fail_g = ~gq.und & ~(gq.hi > 0) & ~(gq.lo > 0)
        certain_fail = mask & (fail_r2 | fail_g)
    return Enclosure(mask=mask, params=enc.params, corr=enc.corr, sums=enc.sums, certain_pass=certain_pass,
                     certain_fail=certain_fail, undecided=mask & ~certain_pass & ~certain_fail)


def redo_gain(enc: Enclosure, offset: np.ndarray, src) -> (Iv, Iv):
    """ kernel_model.py:371 on enclosures: the gain of failing pixels from a given (in-painted) offset, and their corrected
    value: ``g = f32(f32(R - f32(N o)) / S)``, ``corr = f32(f32(g s) + o)`` """
    s = enc.sums
    N, R, S = s['N'], _f32(s['R']), _f32(s['S'])
    o = Iv(np.asarray(offset, F32))
    g = div(sub(R, mul(N, o)), S)
    return g, add(mul(g, np.asarray(src, F32)), o)


# ---- rasters where the summation order matters ----------------------------------------------------------------------------
ADVERSARIAL_KINDS = ('flat-dn', 'marginal', 'integer', 'tiny', 'huge', 'small-gain')
KINDS = ADVERSARIAL_KINDS + ('bright-1e2', 'bright-1e4', 'bright-65535', 'log-uniform', 'dn-saturated', 'subnormal-products',
                             'narrow')


def raster_pair(kind: str, shape, seed: int):
    """ (src, ref) float32.  The six ADVERSARIAL_KINDS sit where the r2-mask certificate is tight: tiny variance on a large mean
    (flat DN imagery), R2 spread around the threshold, integer data, magnitudes outside the certificate's windows.  The others
    make the float64 sums inexact: U[0.05, 1) with finite bright pixels, rows and columns (``bright-<value>``), log-uniform
    values over six decades, DN-like data with saturated pixels, values near 1e-20 whose float32 products are subnormal; and
    ``narrow`` (values in [1, 2): every sum exact). """
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'flat-dn':
        sd = 10 ** (-2 + 3.5 * xx / w)                               # std 0.01 .. 30 on a mean of 5000
        src = 5000 + sd * rng.normal(size=shape)
        ref = 0.8 * src + 300 + sd * 10 ** (-1.5 + 2 * yy / h) * rng.normal(size=shape)
    elif kind == 'marginal':
        src = rng.normal(100, 10, shape)
        ref = src + (3 + 40 * xx / w) * rng.normal(size=shape)       # R2 from ~0.9 down to ~0.05 across the columns
    elif kind == 'integer':
        src = rng.integers(0, 255, shape).astype(float)
        ref = np.round(src * (0.5 + yy / h)) + rng.integers(0, 6, shape)
    elif kind == 'tiny':
        src = 1e-17 * rng.uniform(0.05, 1, shape)
        ref = 1.2 * src + 1e-18 + 1e-19 * rng.normal(size=shape)
    elif kind == 'huge':
        src = 1e14 * rng.uniform(0.05, 1, shape)
        ref = 1.2 * src + 1e13 + 1e12 * rng.normal(size=shape)
    elif kind == 'small-gain':
        src = 1e4 * rng.uniform(0.05, 1, shape)
        ref = 10 ** (-8 + 7 * xx / w) * src + 1e-3 * rng.normal(size=shape)   # gains 1e-8 .. 0.1 (window edge 2^-20)
    elif kind.startswith('bright-'):
        big = float(kind.split('-')[1])
        src = rng.uniform(0.05, 1, shape)
        ref = 1.3 * src + 0.05 + rng.normal(0, 0.02, shape)
        for a in (src, ref):
            a[rng.integers(0, h, 2), :] = big                        # bright rows ...
            a[:, rng.integers(0, w, 2)] = big                        # ... columns ...
            a[rng.random(shape) < 0.002] = big                       # ... and pixels
    elif kind == 'log-uniform':
        src = 10 ** rng.uniform(-3, 3, shape)
        ref = src * 10 ** rng.normal(0, 0.05, shape)
    elif kind == 'dn-saturated':
        src = rng.normal(1000, 150, shape)
        ref = 1.1 * src + 40 + rng.normal(0, 5, shape)
        src[rng.random(shape) < 0.003] = 65535
        ref[rng.random(shape) < 0.003] = 65535
    elif kind == 'subnormal-products':
        src = 1e-20 * rng.uniform(0.05, 1, shape)
        ref = 1.5 * src + 2e-21 + 1e-22 * rng.normal(size=shape)     # f32(s * r) ~ 1e-40: subnormal
    elif kind == 'narrow':
        src = rng.uniform(1, 2, shape)
        ref = np.clip(0.5 * src + 0.7 + rng.normal(0, 0.05, shape), 1, 1.999)
    else:
        raise ValueError(kind)
    return src.astype(F32), ref.astype(F32)
