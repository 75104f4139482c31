""" Exact statements of the element-wise kernels every pixel passes on its way in and out -- the dtype conversions of
hk_convert.hip, the erosion of hk_mask.hip -- and the value families they are held to (tests/test_format_edges_cpu.py checks the
statements and the families on the host, tests/test_gpu_format_edges.py holds the kernels to them bit for bit).

The statements are plain Python on exact integers and fractions; they share nothing with the kernels and do not lean on numpy's
own conversions (the CPU test compares them with those).  The families are built with numpy: they only choose inputs. """
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
INT_DTYPES = ('uint8', 'uint16', 'int16', 'uint32', 'int32')
OUT_DTYPES = ('float32',) + INT_DTYPES + ('float64',)   # in the order of hk_dtype
IN_DTYPES = INT_DTYPES + ('float64',)
FLT_MAX = float(np.finfo(F32).max)
DENORM_MIN = math.ldexp(1.0, -149)


# ----------------------------------------------------------------------------------------------------------------------
# statements
def _int_to_f32(n: int) -> float:
    """ The float32 nearest to the integer n, ties to the neighbour with the even significand; as a Python float (exact). """
    a = abs(n)
    bits = a.bit_length()
    if bits <= 24:
        return float(n)
    shift = bits - 24                      # the two float32 neighbours of a are multiples of 2^shift
    lo = (a >> shift) << shift
    hi = lo + (1 << shift)
    if a - lo < hi - a:
        r = lo
    elif a - lo > hi - a:
        r = hi
    else:
        r = lo if (lo >> shift) % 2 == 0 else hi
    return float(-r if n < 0 else r)       # at most 24 significant bits: exact in a double


def _fraction_to_f32(x: Fraction) -> float:
    """ The float32 nearest to the non-zero rational x (round half to even; gradual underflow; overflow to inf). """
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                   # now 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23                                        # the spacing of float32 there is 2^q
    n = a / Fraction(2) ** q
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
        k += 1
    r = math.ldexp(k, q) if k * Fraction(2) ** q < Fraction(2) ** 128 else math.inf
    return -r if x < 0 else r


def cast_in_exact(values, dtype) -> np.ndarray:
    """ float32 of every element of `values` (dtype: an integer type or float64) under round-to-nearest-even: what a read with
    out_dtype float32 gives (homonim/raster_array.py:178-188). """
    dtype = np.dtype(dtype)
    flat = np.asarray(values, dtype).ravel().tolist()           # Python ints / floats: exact
    out = []
    if dtype.kind in 'iu':
        out = [_int_to_f32(v) for v in flat]
    else:
        for v in flat:
            if v != v or v in (math.inf, -math.inf) or v == 0.0:
                out.append(v)                                   # NaN, +-inf and +-0.0 are themselves
            else:
                r = _fraction_to_f32(Fraction(v))
                out.append(math.copysign(r, v))                 # (an underflow to zero keeps the sign)
    # every entry is a float32 value held in a double: the conversion below is exact
    return np.array(out, np.float64).astype(F32).reshape(np.shape(values))


def cast_out_exact(values_f32, dtype, nodata) -> np.ndarray:
    """ RasterArray._convert_array_dtype (homonim/raster_array.py:353-387) element by element: integer types round the exact
    value half to even and clip to the type's range (+-inf to its bounds), float types keep the value (float64: widened
    exactly); NaN becomes `nodata`, or without one stays NaN in a float type and becomes 0 in an integer type (the library's
    choice, hk_convert.hip; the reference leaves that conversion to the platform). """
    dtype = np.dtype(dtype)
    vals = np.asarray(values_f32)
    assert vals.dtype == F32
    if dtype.kind == 'f':
        out = vals.astype(dtype)                                # float32 -> float32 / float64 is exact
        if nodata is not None:
            out[vals != vals] = nodata
        return out
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    nd = 0 if nodata is None else int(nodata)
    assert nodata is None or (nd == nodata and lo <= nd <= hi)
    out = []
    for v in vals.ravel().tolist():                             # float32 -> Python float is exact
        if v != v:
            out.append(nd)
        elif v == math.inf:
            out.append(hi)
        elif v == -math.inf:
            out.append(lo)
        else:
            out.append(min(max(round(v), lo), hi))              # round(float) -> int: exact, half to even
    return np.array(out, dtype).reshape(vals.shape)


def valid_exact(in_arr, mode, nodata, params) -> np.ndarray:
    """ The mask KernelModel._full_coverage_mask erodes (homonim/kernel_model.py:399-401): the input is valid under its nodata
    `mode` ('none', 'nan', 'value', 'coverage': a mask re-projected with `average`, valid where >= 1) and the parameter image is
    not masked there (two-band parameter array of :487: masked where gain and offset are both NaN). """
    a = np.asarray(in_arr, F32)
    if mode == 'none':
        ok = np.ones(a.shape, bool)
    elif mode == 'nan':
        ok = ~np.isnan(a)
    elif mode == 'value':
        ok = ~(a == F32(nodata))
    else:
        assert mode == 'coverage'
        with np.errstate(invalid='ignore'):
            ok = a >= F32(1)
    return ok & ~(np.isnan(params[0]) & np.isnan(params[1]))


def erode_exact(valid, kernel_shape) -> np.ndarray:
    """ cv.erode(valid, ones((kh + 2, kw + 2)), borderType=BORDER_CONSTANT, borderValue=0) (homonim/kernel_model.py:407-408), by
    brute force: a pixel survives when every pixel of the window around it lies in the raster and is valid. """
    valid = np.asarray(valid, bool)
    h, w = valid.shape
    eh, ew = int(kernel_shape[0]) + 2, int(kernel_shape[1]) + 2
    rh, rw = eh // 2, ew // 2
    pad = np.zeros((h + 2 * rh, w + 2 * rw), bool)
    pad[rh:rh + h, rw:rw + w] = valid
    out = np.ones((h, w), bool)
    for dy in range(eh):
        for dx in range(ew):
            out &= pad[dy:dy + h, dx:dx + w]
    return out


def apply_two_roundings(gain, src, offset) -> np.ndarray:
    """ KernelModel.apply (homonim/kernel_model.py:461) in float32: fl(fl(gain * src) + offset). """
    with np.errstate(all='ignore'):
        prod = np.multiply(np.asarray(gain, F32), np.asarray(src, F32), dtype=F32)
        return np.add(prod, np.asarray(offset, F32), dtype=F32)


def apply_fused(gain, src, offset) -> np.ndarray:
    """ What a fused multiply-add would give: fl(gain * src + offset).  The float64 product of two float32 is exact; the float64
    sum can round once more than an fma (double rounding), rarely: good enough to COUNT the pixels that tell the two apart. """
    with np.errstate(all='ignore'):
        return (np.asarray(gain, np.float64) * np.asarray(src, np.float64) + np.asarray(offset, np.float64)).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# families
def _bits(*patterns) -> np.ndarray:
    return np.array(patterns, np.uint32).view(F32)


def _around(k: np.ndarray) -> np.ndarray:
    """ For every integer k (float64): k - 0.5, k + 0.5 and their float32 neighbours on the side of k -- where float32 holds the
    half-integer at all. """
    out = []
    for half, toward in ((k - 0.5, k), (k + 0.5, k)):
        h32 = half.astype(F32)
        keep = h32.astype(np.float64) == half
        out += [h32[keep], np.nextafter(h32[keep], toward[keep].astype(F32))]
    return np.concatenate(out)


def out_ties(dtype) -> np.ndarray:
    """ uint8 / uint16 / int16: the rounding and clipping edges of every integer of the type and of the two just outside. """
    info = np.iinfo(dtype)
    assert info.bits <= 16
    return _around(np.arange(int(info.min) - 1, int(info.max) + 2, dtype=np.float64))


def out_ties_wide() -> np.ndarray:
    """ int32 / uint32: half-integers around 0, +-2^23 (the last that float32 holds) and +-2^24, every float32 within 8 ulp of
    +-2^31 and of 2^32, and the neighbours of the clipping bounds by name. """
    ks = np.concatenate([np.arange(c - 64, c + 65, dtype=np.float64) for c in (0, 2 ** 23, -2 ** 23, 2 ** 24, -2 ** 24)])
    near = []
    for c in (2.0 ** 31, -2.0 ** 31, 2.0 ** 32):
        up = down = F32(c)
        near.append(up)
        for _ in range(8):
            up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
            near += [up, down]
    named = np.array([2147483520, 4294967040, 4294967296, -2147483904], np.float64).astype(F32)
    assert (named.astype(np.float64) == [2147483520, 4294967040, 4294967296, -2147483904]).all()
    # integers of the windows themselves too: above 2^23 every float32 is one
    return np.concatenate([_around(ks), ks.astype(F32), np.array(near, F32), named])


def out_specials() -> np.ndarray:
    """ +-0.0, +-inf, NaN with two payloads (and both signs), the smallest denormal and FLT_MAX in both signs. """
    return _bits(0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7fc00001, 0x00000001, 0x80000001,
                 0x7f7fffff, 0xff7fffff)


def out_random(dtype, n=4096, seed=7) -> np.ndarray:
    """ Integer types: uniform over the type's range widened to 1.5 times about its centre; float types: random finite float32
    bit patterns (every exponent). """
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        b = rng.integers(0, 2 ** 32, 2 * n, dtype=np.uint64).astype(np.uint32)
        b = b[(b & 0x7f800000) != 0x7f800000][:n]
        assert b.size == n
        return b.view(F32)
    info = np.iinfo(dtype)
    mid, half = (int(info.min) + int(info.max)) / 2, (int(info.max) - int(info.min)) / 2 * 1.5
    return rng.uniform(mid - half, mid + half, n).astype(F32)


def cast_out_families(dtype) -> dict:
    """ {name: 1-D float32 array} of the families `dtype`'s output conversion is held to. """
    dtype = np.dtype(dtype)
    fam = {}
    if dtype.kind in 'iu':
        fam['ties'] = out_ties(dtype) if dtype.itemsize <= 2 else out_ties_wide()
    fam['specials'] = out_specials()
    fam['random'] = out_random(dtype)
    return fam


def _window(c, lo, hi):
    return list(range(max(c - 8, lo), min(c + 40, hi) + 1))


def cast_in_family(dtype) -> np.ndarray:
    """ 1-D array of `dtype` the input conversion is held to. """
    dtype = np.dtype(dtype)
    if dtype.kind in 'iu' and dtype.itemsize <= 2:
        info = np.iinfo(dtype)
        return np.arange(int(info.min), int(info.max) + 1, dtype=np.int64).astype(dtype)   # every value of the type
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        lo, hi = int(info.min), int(info.max)
        vals = [lo, hi]
        centres = (2 ** 24, 2 ** 25, 2 ** 30, 2 ** 31) if dtype.kind == 'u' else (2 ** 24, 2 ** 25, 2 ** 30)
        for c in centres:
            vals += _window(c, lo, hi)
            if dtype.kind == 'i':
                vals += [-v for v in _window(c, lo, hi)]
        if dtype.kind == 'u':
            vals += [2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 127]   # the last tie: 2^32 - 128 lies between 2^32 - 256 and 2^32
            vals += list(range(hi - 40, hi + 1))
        else:
            vals += list(range(lo, lo + 41)) + list(range(hi - 40, hi + 1))
        return np.array(vals, np.int64).astype(dtype)
    # float64: the midpoints of neighbouring float32 around 1.0, 2^24 and FLT_MAX, and the float64 either side of each
    vals = []
    for c in (1.0, 2.0 ** 24, FLT_MAX):
        seq = [F32(c)]
        for _ in range(16):
            seq.insert(0, np.nextafter(seq[0], F32(-np.inf)))
            if seq[-1] < F32(FLT_MAX):
                seq.append(np.nextafter(seq[-1], F32(np.inf)))
        for a, b in zip(seq[:-1], seq[1:]):
            m = (float(a) + float(b)) / 2        # exact: one more significant bit than float32
            vals += [m, np.nextafter(m, np.inf), np.nextafter(m, -np.inf)]
    tie_max = 3.4028235677973366e38              # halfway from FLT_MAX to 2^128: ties to even, which is infinity
    assert tie_max == float.fromhex('0x1.ffffffp127')
    vals += [tie_max, np.nextafter(tie_max, np.inf), np.nextafter(tie_max, 0.0), -tie_max, np.nextafter(-tie_max, 0.0)]
    vals += [1e39, -1e39, 1e-40, 1e-46, -1e-46, 2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), -2.0 ** -150,
             1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, -1e-40, 3e-42, 2.0 ** -127, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), 0.0, -0.0, np.inf, -np.inf, np.nan]
    vals += np.random.default_rng(11).uniform(-1e6, 1e6, 2048).tolist()
    return np.array(vals, np.float64)


def held_nodata(dtype):
    """ The nodata values the casts are run with: one the type can hold; float32 -9999.0 and NaN; float64 -1.5; uint8 also none. """
    return {'float32': (-9999.0, float('nan')), 'uint8': (255, None), 'uint16': (65535,), 'int16': (-32768,),
            'uint32': (4294967295,), 'int32': (-2147483648,), 'float64': (-1.5,)}[np.dtype(dtype).name]


def as_plane(values: np.ndarray, width: int = 1028, fill=0) -> np.ndarray:
    """ A 1-D family laid out row by row as a plane `width` columns wide (default 1025 + 3: a second x block of one lane), the
    last row filled up with `fill`. """
    values = np.asarray(values).ravel()
    rows = -(-values.size // width)
    out = np.full(rows * width, fill, values.dtype)
    out[:values.size] = values
    return out.reshape(rows, width)


def fma_values(shape, seed=0):
    """ (gain, src, offset) float32 planes on which fl(fl(g * s) + o) and fl(g * s + o) differ at a good share of the pixels:
    full-width significands, the offset of the product's size and opposite sign now and then. """
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, shape).astype(F32)
    s = rng.uniform(0.5, 2.0, shape).astype(F32)
    o = (rng.uniform(-1.0, 1.0, shape) * rng.choice([1.0, 4.0], shape)).astype(F32)
    return g, s, o
