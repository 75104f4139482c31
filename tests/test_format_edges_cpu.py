""" The exact statements of tests/_format_edges.py -- the dtype conversions either side of the path and the erosion of
mask_partial -- checked on the host before the kernels are held to them (tests/test_gpu_format_edges.py): against numpy's own
conversions, the host-side convert_dtype, the reference's recorded outputs and the oracle's mask; and the value families checked
for what they claim to contain, so that an empty family fails here. """
import os
import warnings

import numpy as np
import pytest

import _format_edges as fe
from conftest import GOLDEN_DIR, assert_same_f32
from homonim_amd import _hk, fuse
from oracle import oracle_np as onp

F32 = np.float32


def _numpy_cast_out(vals, dtype, nodata):
    """ numpy's own route: np.round (half to even) + np.clip in float64, astype; NaN -> nodata (0 without one). """
    dtype = np.dtype(dtype)
    nan = np.isnan(vals)
    if dtype.kind == 'f':
        out = vals.astype(dtype)
        if nodata is not None:
            out[nan] = nodata
        return out
    info = np.iinfo(dtype)
    with np.errstate(invalid='ignore'):
        out = np.clip(np.round(np.where(nan, 0, vals).astype(np.float64)), info.min, info.max).astype(dtype)
    out[nan] = 0 if nodata is None else nodata
    return out


def _same(got, exp, what):
    assert got.dtype == exp.dtype, what
    if got.dtype == F32:
        assert_same_f32(got, exp, what)
    else:
        np.testing.assert_array_equal(got, exp, err_msg=what)


@pytest.mark.parametrize('dtype', fe.IN_DTYPES)
def test_cast_in_exact_equals_numpy_astype(dtype):
    vals = fe.cast_in_family(dtype)
    with np.errstate(over='ignore'):
        exp = vals.astype(F32)
    got = fe.cast_in_exact(vals, dtype)
    _same(got, exp, f'cast_in_exact vs astype, {dtype}')
    if dtype == 'float64':   # the sign of zero and of an underflow is part of the statement
        np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))


@pytest.mark.parametrize('dtype', fe.OUT_DTYPES)
def test_cast_out_exact_equals_numpy_and_convert_dtype(dtype):
    for name, vals in fe.cast_out_families(dtype).items():
        for nodata in fe.held_nodata(dtype):
            exp = fe.cast_out_exact(vals, dtype, nodata)
            _same(_numpy_cast_out(vals, dtype, nodata), exp, f'numpy vs cast_out_exact, {dtype} {name} nodata {nodata}')
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                _same(fuse.convert_dtype(vals.copy(), dtype, nodata), exp, f'convert_dtype vs cast_out_exact, {dtype} {name} nodata {nodata}')
            if dtype == 'float64' or dtype == 'float32':
                np.testing.assert_array_equal(np.signbit(exp[~np.isnan(vals)]), np.signbit(vals[~np.isnan(vals)]))


def test_cast_out_exact_equals_the_reference_goldens():
    """ The outputs of the reference's own RasterArray._convert_array_dtype (tests/golden/convert_dtype.npz): every recorded case
    has a nodata, so every result is defined. """
    g = np.load(os.path.join(GOLDEN_DIR, 'convert_dtype.npz'))
    a = g['input']
    keys = [k for k in g.files if k != 'input']
    assert len(keys) >= 9
    for key in keys:
        dtype, nd = key.rsplit('_', 1)
        nodata = float('nan') if nd == 'nan' else float(nd)
        if np.isnan(nodata):
            assert np.dtype(dtype).kind == 'f'
            nodata = None   # NaN stays NaN
        _same(fe.cast_out_exact(a, dtype, nodata), g[key], key)


def test_erode_exact_equals_the_oracle_mask():
    rng = np.random.default_rng(5)
    for (h, w), k, p in (((40, 56), (3, 3), 0.01), ((33, 70), (1, 9), 0.01), ((70, 33), (9, 1), 0.02), ((64, 64), (15, 15), 0.001),
                         ((5, 7), (7, 9), 0.0), ((1, 1), (1, 1), 0.0), ((90, 40), (31, 5), 0.0005)):
        valid = rng.random((h, w)) >= p
        params = rng.normal(1, 0.1, (2, h, w)).astype(F32)
        params[:, rng.random((h, w)) < p] = np.nan
        params[0, rng.random((h, w)) < p] = np.nan    # one band NaN alone does not mask the parameters
        v = fe.valid_exact(np.where(valid, 1.0, np.nan).astype(F32), 'nan', None, params)
        np.testing.assert_array_equal(fe.erode_exact(v, k), onp.full_coverage_mask(valid, params, k), err_msg=f'{(h, w)} {k}')


def test_erode_exact_at_the_largest_structuring_element():
    """ kernel (253, 255) -> a 255 x 257 window, 65535 pixels: on an all-valid 260 x 262 raster exactly the central 6 x 6 pixels
    see no border. """
    valid = np.ones((260, 262), bool)
    exp = np.zeros_like(valid)
    exp[127:133, 128:134] = True
    np.testing.assert_array_equal(fe.erode_exact(valid, (253, 255)), exp)


def test_erode_exact_equals_cv2():
    cv2 = pytest.importorskip('cv2', reason='OpenCV is not installed: erode_exact is compared with the oracle mask only')
    rng = np.random.default_rng(6)
    for (h, w), k in (((40, 56), (3, 3)), ((33, 70), (1, 9)), ((70, 33), (9, 1)), ((64, 64), (15, 15)), ((5, 7), (7, 9))):
        valid = rng.random((h, w)) >= 0.01
        se = np.ones((k[0] + 2, k[1] + 2), np.uint8)
        exp = cv2.erode(valid.astype(np.uint8), se, borderType=cv2.BORDER_CONSTANT, borderValue=0).astype(bool)
        np.testing.assert_array_equal(fe.erode_exact(valid, k), exp, err_msg=f'{(h, w)} {k}')


def _is_tie(v):
    """ finite float32 exactly halfway between two integers """
    d = v.astype(np.float64)
    return np.isfinite(d) & (np.floor(d) != d) & (np.floor(d * 2) == d * 2)


def test_cast_out_families_contain_what_they_claim(capsys):
    lines = []
    for dtype in fe.OUT_DTYPES:
        fam = fe.cast_out_families(dtype)
        sp = fam['specials']
        assert np.isinf(sp).sum() == 2 and np.isnan(sp).sum() == 3 and len(set(sp[np.isnan(sp)].view(np.uint32).tolist())) == 3
        assert (sp == 0).sum() == 2 and np.signbit(sp[sp == 0]).sum() == 1
        assert (np.abs(sp) == fe.FLT_MAX).sum() == 2 and (np.abs(sp.astype(np.float64)) == fe.DENORM_MIN).sum() == 2
        rnd = fam['random']
        assert rnd.size == 4096 and np.isfinite(rnd).all()
        counts = dict(n=sum(v.size for v in fam.values()))
        if np.dtype(dtype).kind in 'iu':
            info = np.iinfo(dtype)
            ties = fam['ties']
            d = ties.astype(np.float64)
            counts.update(ties=int(_is_tie(ties).sum()), below=int((d < info.min - 0.5).sum() + (rnd < info.min).sum()),
                          above=int((d > info.max + 0.5).sum() + (rnd > info.max).sum()))
            assert (rnd < info.min).sum() > 300 and (rnd > info.max).sum() > 300   # a sixth each of the widened range
            if info.bits <= 16:
                n_k = int(info.max) - int(info.min) + 3
                assert ties.size == 4 * n_k and counts['ties'] == 2 * n_k         # k - 0.5 and k + 0.5 of every k
                # the neighbours are the float32 next to the tie on the side of k: they round to k, the ties do not all
                k = np.arange(int(info.min) - 1, int(info.max) + 2, dtype=np.float64)
                np.testing.assert_array_equal(np.round(ties[n_k:2 * n_k].astype(np.float64)), k)
                np.testing.assert_array_equal(np.round(ties[3 * n_k:].astype(np.float64)), k)
                assert (ties.astype(np.float64).min(), ties.astype(np.float64).max()) == (info.min - 1.5, info.max + 1.5)
            else:
                assert counts['ties'] >= 2 * 129 + 4 * 64        # all of the window at 0, the halves below +-2^23
                assert (np.abs(d) > 2.0 ** 24).sum() >= 2 * 64   # integers float32 holds only every other one of
                for c in (2.0 ** 31, -2.0 ** 31, 2.0 ** 32):
                    ulp_below, ulp_above = abs(c) / 2 ** 24, abs(c) / 2 ** 23
                    near = d[(d >= c - 8 * max(ulp_below, ulp_above)) & (d <= c + 8 * max(ulp_below, ulp_above))]
                    assert np.unique(near).size >= 17, c
                for named in (2147483520, 4294967040, 4294967296, -2147483904):
                    assert (d == named).any(), named
                assert counts['below'] > 0 and counts['above'] > 0
        lines.append(f'[families] cast_out {dtype}: ' + ', '.join(f'{k} {v}' for k, v in counts.items()) +
                     ', infinities 2, NaN payloads 3')
    with capsys.disabled():
        print('\n' + '\n'.join(lines))


def test_cast_in_families_contain_what_they_claim(capsys):
    lines = []
    for dtype in fe.IN_DTYPES:
        vals = fe.cast_in_family(dtype)
        dt = np.dtype(dtype)
        if dt.kind in 'iu' and dt.itemsize <= 2:
            assert np.unique(vals).size == 2 ** (8 * dt.itemsize)
            lines.append(f'[families] cast_in {dtype}: all {vals.size} values of the type')
            continue
        if dt.kind in 'iu':
            ints = [int(v) for v in vals.tolist()]
            info = np.iinfo(dt)
            assert int(info.min) in ints and int(info.max) in ints
            inexact = [v for v in ints if float(F32(v)) != v]
            # an exact tie: the integer lies halfway between its two float32 neighbours
            ties = [v for v in inexact if abs(v) % (1 << (abs(v).bit_length() - 24)) == 1 << (abs(v).bit_length() - 25)]
            for c in (2 ** 24, 2 ** 25, 2 ** 30) + ((2 ** 31,) if dt.kind == 'u' else ()):
                assert all(v in ints for v in range(c - 8, c + 41)), c
                if dt.kind == 'i':
                    assert all(-v in ints for v in range(c - 8, c + 41)), -c
            if dt.kind == 'u':
                assert all(v in ints for v in (2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 127))
            # odd integers of [2^24, 2^24 + 40]: 20 ties; 2 mod 4 of [2^25, 2^25 + 40]: 10; 2^30 + 32: 1; mirrored for a signed type
            assert len(ties) >= 31 * (2 if dt.kind == 'i' else 1) and len(inexact) >= 150
            assert dt.kind == 'i' or 2 ** 32 - 128 in ties
            lines.append(f'[families] cast_in {dtype}: n {len(ints)}, not float32 {len(inexact)}, exact ties {len(ties)}')
            continue
        d = vals
        with np.errstate(over='ignore'):
            f = d.astype(F32)
        fin = np.isfinite(d)
        with np.errstate(over='ignore'):
            lo = np.nextafter(f, F32(-np.inf)).astype(np.float64)
            hi = np.nextafter(f, F32(np.inf)).astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            ff = f.astype(np.float64)
            # ties among the normal results (float32 spacing is uniform either side unless f is a power of two: then both tests)
            tie = fin & np.isfinite(f) & (f != 0) & ((np.abs(d - ff) * 2 == np.abs(hi - ff)) | (np.abs(d - ff) * 2 == np.abs(ff - lo)))
        overflow = fin & np.isinf(f)
        denorm = fin & (f != 0) & (np.abs(f) < F32(2.0 ** -126))
        underflow = fin & (d != 0) & (f == 0)
        counts = dict(n=d.size, ties=int(tie.sum()), overflow=int(overflow.sum()), denormal=int(denorm.sum()),
                      underflow=int(underflow.sum()), inf=int(np.isinf(d).sum()), nan=int(np.isnan(d).sum()))
        assert counts['ties'] >= 3 * 16 and counts['overflow'] >= 5 and counts['denormal'] >= 5 and counts['underflow'] >= 3
        assert counts['inf'] == 2 and counts['nan'] == 1
        for named in (1e39, 3.4028235677973366e38, 1e-40, 1e-46, -1e-46, 2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0)):
            assert (d == named).any(), named
        assert np.signbit(d[d == 0]).sum() == 1
        lines.append('[families] cast_in float64: ' + ', '.join(f'{k} {v}' for k, v in counts.items()))
    with capsys.disabled():
        print('\n' + '\n'.join(lines))


def test_named_conversions():
    """ The single values the issue of this file was written around, by name. """
    assert fe.cast_in_exact(np.array([2 ** 32 - 1], np.uint32), 'uint32')[0] == F32(4294967296.0)
    assert fe.cast_in_exact(np.array([2 ** 24 + 1, 2 ** 24 + 3], np.int32), 'int32').tolist() == [2.0 ** 24, 2.0 ** 24 + 4]
    assert fe.cast_in_exact(np.array([2 ** 32 - 128, 2 ** 32 - 129, 2 ** 32 - 127], np.uint32), 'uint32').tolist() == \
        [2.0 ** 32, 2.0 ** 32 - 256, 2.0 ** 32]
    got = fe.cast_in_exact(np.array([3.4028235677973366e38, 1e39, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 1e-46, -1e-46]), 'float64')
    assert got[:2].tolist() == [np.inf, np.inf] and got[2] == 0 and float(got[3]) == 2.0 ** -149
    assert got[4] == 0 and not np.signbit(got[4]) and got[5] == 0 and np.signbit(got[5])
    v = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, np.nextafter(F32(0.5), F32(1)), 65534.5, 65535.5], F32)
    assert fe.cast_out_exact(v, 'uint8', 7).tolist() == [0, 2, 2, 254, 255, 0, 1, 255, 255]
    assert fe.cast_out_exact(v, 'uint16', 7).tolist() == [0, 2, 2, 254, 256, 0, 1, 65534, 65535]
    w = np.array([2147483520, 2147483648, 4294967040, 4294967296, -2147483904, np.nan], F32)
    assert fe.cast_out_exact(w, 'int32', None).tolist() == [2147483520, 2147483647, 2147483647, 2147483647, -2147483648, 0]
    assert fe.cast_out_exact(w, 'uint32', 9).tolist() == [2147483520, 2147483648, 4294967040, 4294967295, 0, 9]


def test_fma_values_tell_one_rounding_from_two():
    g, s, o = fe.fma_values((70, 257), seed=3)
    two, one = fe.apply_two_roundings(g, s, o), fe.apply_fused(g, s, o)
    share = float((two != one).mean())
    assert share >= 0.1, share
    assert_same_f32(two, onp.apply(s, np.stack([g, o])), 'apply_two_roundings vs the oracle')


@pytest.mark.parametrize('dtype, nodata', [('uint8', -9999), ('uint8', 256), ('uint8', 0.5), ('int16', 0.5), ('int16', 32768),
                                           ('uint16', -1), ('uint32', 4294967296), ('int32', -2147483649), ('uint8', float('inf')),
                                           ('int32', float('-inf')), ('float32', 1e39)])
def test_out_nodata_the_dtype_cannot_hold_is_refused(dtype, nodata):
    """ RasterArray._convert_array_dtype (homonim/raster_array.py:357-358), with its message. """
    with pytest.raises(ValueError, match=rf"'nodata' value: .* cannot be safely cast to '{dtype}'"):
        _hk.out_nodata_code(dtype, nodata)


def test_out_nodata_edge_values_are_accepted():
    assert _hk.out_nodata_code('uint8', 255) == (1, 255.0)
    assert _hk.out_nodata_code('int16', -32768) == (1, -32768.0)
    assert _hk.out_nodata_code('uint32', 4294967295) == (1, 4294967295.0)
    assert _hk.out_nodata_code('float32', -9999.0) == (1, -9999.0) and _hk.out_nodata_code('float32', float('inf'))[0] == 1
    assert _hk.out_nodata_code('float64', 1e300) == (1, 1e300)
    # None and NaN keep their meaning: NaN stays NaN in a float type, NaN for an integer type is 0
    assert _hk.out_nodata_code('uint8', None) == (0, 0.0) and _hk.out_nodata_code('float32', float('nan')) == (0, 0.0)
    assert _hk.out_nodata_code('uint8', float('nan')) == (1, 0.0) and _hk.out_nodata_code('int16', np.float32('nan')) == (1, 0.0)


def test_raster_fuse_refuses_a_nodata_the_output_dtype_cannot_hold():
    """ RasterFuse.process(out_profile=dict(dtype='uint8', nodata=-9999)) raises as the reference does, before any device work. """
    src = np.ones((1, 16, 16), F32)
    with pytest.raises(ValueError, match=r"'nodata' value: -9999 cannot be safely cast to 'uint8'"):
        fuse.RasterFuse(src, src.copy()).process(out_profile=dict(dtype='uint8', nodata=-9999))
