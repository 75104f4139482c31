"""
CPU tests of oracle/exact_window.py: the exact window sums against Fractions and oracle_np.box_sum, and the enclosures of the
fused fit -- SOUND (a numpy emulator of the kernel's summation under random row-segment partitions, the numpy oracle and the
C oracle all lie inside them), TIGHT (they reject emulator mutations that break the arithmetic contract) and EXACT (single
values equal to oracle_np where every sum is exact).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_window as ew
from oracle import oracle_np as onp

F32, F64 = np.float32, np.float64
MODELS = ('gain', 'gain-blk-offset', 'gain-offset')


@pytest.fixture(scope='module')
def oc():
    from homonim_amd import build
    build.build_oracle(verbose=False)
    from oracle import oracle_c
    assert oracle_c.available()
    return oracle_c


# ---- exact sums -------------------------------------------------------------------------------------------------------------
def _fraction_box(v, kernel_shape):
    kh, kw = kernel_shape
    h, w = v.shape
    out = np.empty((h, w), F64)
    for y in range(h):
        for x in range(w):
            acc = Fraction(0)
            for yy in range(max(0, y - kh // 2), min(h, y + kh // 2 + 1)):
                for xx in range(max(0, x - kw // 2), min(w, x + kw // 2 + 1)):
                    acc += Fraction(float(v[yy, xx]))
            out[y, x] = float(acc)   # Fraction -> float rounds correctly
    return out


@pytest.mark.parametrize('case', ['negative', 'mixed-exponents', 'subnormal', 'cancel', 'f32-squares'])
@pytest.mark.parametrize('kernel_shape', [(1, 1), (3, 3), (3, 5), (5, 3)])
def test_exact_sums_equal_fraction_sums(case, kernel_shape):
    rng = np.random.default_rng(len(case))
    shape = (9, 11)
    if case == 'negative':
        v = rng.normal(0, 1, shape).astype(F32).astype(F64)
    elif case == 'mixed-exponents':
        v = (rng.choice([-1, 1], shape) * 10.0 ** rng.uniform(-30, 30, shape)).astype(F32).astype(F64)
    elif case == 'subnormal':
        v = rng.integers(-2 ** 40, 2 ** 40, shape) * 2.0 ** -1074        # float64 subnormals, sums included
        v[0, 0] = 2.0 ** -1074
    elif case == 'cancel':
        v = rng.choice([1e300, -1e300, 1.0, 2.0 ** -60], shape)
    else:
        v = rng.uniform(0.05, 1, shape).astype(F32).astype(F64) ** 2
    _, _, rn = ew.exact_window_sum(v, kernel_shape)
    exp = _fraction_box(v, kernel_shape)
    assert (rn.view(np.uint64) == exp.view(np.uint64)).all()
    iv = ew.window_enclosure(v, kernel_shape)
    assert iv.contains(onp.box_sum(v, kernel_shape)).all()
    b, exact = ew.sum_bound(v, kernel_shape)
    direct = onp.box_sum(v, kernel_shape)
    assert (direct[exact].view(np.uint64) == rn[exact].view(np.uint64)).all()
    if case in ('subnormal',):
        assert exact.all()


def test_lsb_exponent():
    v = np.array([1.0, 3.0, 0.5, 0.75, 2.0 ** -1074, 3 * 2.0 ** -1074, -6.0, 0.0, 2.0 ** 1000])
    assert ew.lsb_exp(v)[:7].tolist() == [0, 0, -1, -2, -1074, -1074, 1]
    assert ew.lsb_exp(v)[7] > 2000 and ew.lsb_exp(v)[8] == 1000


# ---- the kernel's summation, emulated -----------------------------------------------------------------------------------
def running_col_sums(v, kh, starts, dtype=F64, leave_off=0):
    """ running column sums of hk_fit_kernel.h: per row segment [y0, y1) start from 0 at row y0 - rh, add the entering row,
    subtract the leaving one (``leave_off``: the leaving row that many rows too early -- a mutation) """
    h, w = v.shape
    rh = kh // 2
    v = v.astype(dtype)
    col = np.zeros((h, w), dtype)
    cuts = sorted(set([0, h] + [int(s) for s in starts if 0 < s < h]))
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        acc = np.zeros(w, dtype)
        for t in range(y0 - rh, y1 + rh):
            if 0 <= t < h:
                acc = acc + v[t]
            tl = t - kh - leave_off
            if tl >= y0 - rh and 0 <= tl < h:
                acc = acc - v[tl]
            if t - rh >= y0:
                col[t - rh] = acc
    return col


def lane_hsum(col, kw, px=4):
    """ the window's kw column sums in the lanes' order: the suffix of the left partial lane (right to left), the prefix sums
    of the whole lanes, the prefix of the right partial lane, added left to right """
    h, w = col.shape
    rw = kw // 2
    pad = np.zeros((h, w + 2 * rw + 2 * px), col.dtype)
    off = rw + px
    pad[:, off:off + w] = col
    out = np.zeros((h, w), col.dtype)
    for x in range(w):
        a, b = x - rw, x + rw                 # inclusive window columns
        chunks = []
        c = a
        while c <= b:
            lane_end = (c // px) * px + px - 1
            e = min(lane_end, b)
            chunks.append((c, e))
            c = e + 1
        total = None
        for i, (c0, c1) in enumerate(chunks):
            cols = [pad[:, off + c] for c in range(c0, c1 + 1)]
            if i == 0 and len(chunks) > 1:    # suffix sum
                s = cols[-1]
                for v in cols[-2::-1]:
                    s = v + s
            else:                             # prefix sum
                s = cols[0]
                for v in cols[1:]:
                    s = s + v
            total = s if total is None else total + s
        out[:, x] = total
    return out


def emulate(model, src, src_nodata, ref, ref_nodata, kernel_shape, find_r2, thresh, norm, starts, mutation=None):
    """ the fused fit with the kernel's summation and the contract's expressions (HISTORY.md section 2) written out per
    dtype; returns (params, corr) like oracle_np.fit + apply, before any in-painting """
    kh, kw = kernel_shape
    src, ref = np.array(src, F32), np.array(ref, F32)
    want_r2 = find_r2 or (model == 'gain-offset' and thresh is not None)
    with np.errstate(all='ignore'):
        if model == 'gain-blk-offset':
            s_nd = src.copy()
            if src_nodata is not None and not np.isnan(src_nodata):
                s_nd[~onp.mask_of(src, src_nodata)] = np.nan
            sd = s_nd * norm[0] + norm[1]
            mask = ~np.isnan(sd) & onp.mask_of(ref, ref_nodata)
        else:
            mask = onp.mask_of(src, src_nodata) & onp.mask_of(ref, ref_nodata)
        s0, r0 = np.where(mask, src, F32(0)), np.where(mask, ref, F32(0))
        csum = lambda v, dt=F64: lane_hsum(  # noqa: E731
            running_col_sums(v, kh, starts, dt, 1 if mutation == 'leave-off-by-one' else 0), kw)
        N = onp.box_sum(mask.astype(F32), kernel_shape)
        R = csum(r0.astype(F64)).astype(F32)
        R2 = csum(r0.astype(F64) ** 2) if want_r2 else None
        if model == 'gain-blk-offset':
            sd0 = np.where(mask, sd, 0.0)
            if want_r2:
                S, P, S2 = csum(sd0), csum(sd0 * r0), csum(sd0 * sd0)
            else:
                S = (csum(s0.astype(F64)) * norm[0]) + (norm[1] * N.astype(F64))
            g = (R / S).astype(F32)
            params = [g]
            if want_r2:
                ssres = ((g * g) * S2 - (F32(2) * g) * P + R2) * N
                params.append(F32(1) - (ssres / (N * R2 - (R * R).astype(F64))).astype(F32))
            params = [(g * norm[0]).astype(F32), (g * norm[1]).astype(F32)] + params[1:]
        else:
            S = csum(s0.astype(F64)).astype(F32)
            P = csum((s0 * r0).astype(F64)).astype(F32)
            S2 = csum(s0.astype(F64) ** 2, F32 if mutation == 's2-f32' else F64).astype(F64)
            if model == 'gain':
                g, o = R / S, np.zeros_like(R)
            else:
                num = (N.astype(F64) * P.astype(F64) - (S * R)) if mutation == 'np-unrounded' else (N * P - S * R)
                ss = S.astype(F64) * S.astype(F64) if mutation == 'den-f64-ss' else (S * S).astype(F64)
                den = N.astype(F64) * S2 - ss
                g = (num.astype(F64) / den).astype(F32)
                o = (R - g * S) / N
            params = [g, o]
            if want_r2:
                sstot = N.astype(F64) * R2 - (R * R).astype(F64)
                if model == 'gain':
                    ssres = (g * g) * S2 - ((F32(2) * g) * P).astype(F64) + R2
                else:
                    B = (F32(2) * (g * o)) * S
                    ssres = (g * g) * S2 + B - (F32(2) * g) * P - (F32(2) * o) * R + R2 + N * (o * o)
                ssres = ssres * N
                params.append(F32(1) - (ssres / sstot).astype(F32))
        params = np.stack([np.where(mask, p, F32(np.nan)).astype(F32) for p in params])
        if model == 'gain':
            params[1][mask] = 0
        corr = (params[0] * src + params[1]).astype(F32)
    return params, corr


def _starts(rng, h, n):
    return sorted(rng.integers(1, max(2, h), n).tolist())


def _configs():
    for model in MODELS:
        for find_r2 in (False, True):
            yield model, find_r2, (0.25 if model == 'gain-offset' else None)


def _in_enclosure(enc, params, corr, what, pass_only=True):
    sel = enc.certain_pass if (enc.certain_pass is not None and pass_only) else np.ones(enc.mask.shape, bool)
    for i, iv in enumerate(enc.params[:params.shape[0]]):
        bad = ~iv.contains(params[i]) & sel
        assert not bad.any(), f'{what}: param {i} outside its enclosure at {np.argwhere(bad)[:3].tolist()}'
    bad = ~enc.corr.contains(corr) & sel
    assert not bad.any(), f'{what}: corrected outside its enclosure at {np.argwhere(bad)[:3].tolist()}'


SOUND_KINDS = ew.KINDS
SHAPE = (72, 60)


@pytest.mark.parametrize('kind', SOUND_KINDS)
@pytest.mark.parametrize('kernel_shape', [(5, 5), (3, 7), (7, 3), (1, 1)])
def test_emulator_and_oracles_lie_in_the_enclosures(oc, kind, kernel_shape):
    """ Soundness: the kernel's summation under random row-segment partitions, oracle_np and the C oracle -- every parameter,
    corrected pixel and r2-mask decision lies in the enclosure (failure counts between the certain and the possible ones). """
    src, ref = ew.raster_pair(kind, SHAPE, seed=7)
    src[5, 3:9] = np.nan
    ref[40, 20] = np.nan
    rng = np.random.default_rng(len(kind) * 31 + kernel_shape[1])
    for model, find_r2, thresh in _configs():
        if model == 'gain-offset' and kernel_shape == (1, 1):
            continue
        norm = onp.fit_block_norm(src, np.nan, ref, np.nan) if model == 'gain-blk-offset' else None
        enc = ew.enclose(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm)
        what = f'{kind} {model} {kernel_shape} r2={find_r2}'
        for trial in range(2):
            p, c = emulate(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm,
                           _starts(rng, SHAPE[0], trial * 3 + 1))
            _in_enclosure(enc, p, c, f'{what} emulator', pass_only=thresh is not None)
        exp_p, aux = onp.fit(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm)
        c_p, c_corr, c_fail = oc.fit_apply(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm)
        _in_enclosure(enc, exp_p, onp.apply(src, exp_p), f'{what} oracle_np')
        _in_enclosure(enc, c_p, c_corr, f'{what} C oracle')
        if thresh is not None:
            n_cf, n_und = int(enc.certain_fail.sum()), int(enc.undecided.sum())
            assert n_cf <= aux <= n_cf + n_und and n_cf <= c_fail <= n_cf + n_und, what


MUTATIONS = ('s2-f32', 'den-f64-ss', 'np-unrounded', 'leave-off-by-one')


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_enclosures_reject_contract_mutations(mutation):
    """ Tightness: each mutation of the kernel's arithmetic puts some output outside the enclosure on at least one kind. """
    caught = []
    for kind in ('bright-1e4', 'dn-saturated', 'flat-dn', 'marginal', 'narrow', 'integer'):
        src, ref = ew.raster_pair(kind, SHAPE, seed=3)
        enc = ew.enclose('gain-offset', src, None, ref, None, (5, 5), True, None)
        p, c = emulate('gain-offset', src, None, ref, None, (5, 5), True, None, None, [30], mutation=mutation)
        ok = np.ones(SHAPE, bool)
        for i in range(3):
            ok &= enc.params[i].contains(p[i])
        ok &= enc.corr.contains(c)
        if not ok.all():
            caught.append(kind)
    assert caught, f'{mutation} is not rejected on any kind'


@pytest.mark.parametrize('kind, kernel_shape', [('integer', (5, 5)), ('integer', (3, 7)), ('integer', (15, 15)), ('narrow', (5, 5)),
                                                 ('narrow', (3, 7)), ('narrow', (7, 3))])
def test_exact_data_give_single_values_equal_to_the_oracle(kind, kernel_shape):
    """ Integer and narrow-range rasters: every window sum is exact, so every enclosure is one value -- oracle_np's.  (Values in
    [1, 2) have squares on a 2^-46 grid: their float64 sums stay exact while a window holds less than 2^7, i.e. up to 25 pixels.) """
    src, ref = ew.raster_pair(kind, SHAPE, seed=11)
    src[10:13, 10:14] = np.nan
    for model, find_r2, thresh in _configs():
        norm = np.array([1.0, 0.0]) if model == 'gain-blk-offset' else None   # (keeps the normalised sums exact)
        enc = ew.enclose(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm)
        exp_p, aux = onp.fit(model, src, np.nan, ref, np.nan, kernel_shape, find_r2, thresh, norm)
        for k, iv in enc.sums.items():
            assert iv.point.all(), (kind, model, k)
        for i in range(exp_p.shape[0]):
            assert enc.params[i].point.all(), (kind, model, i)
            assert enc.params[i].contains(exp_p[i]).all(), (kind, model, i)
        if thresh is not None:
            assert not enc.undecided.any()
            assert int(enc.certain_fail.sum()) == aux
        else:
            assert enc.corr.point.all() and enc.corr.contains(onp.apply(src, exp_p)).all()


def test_inexact_kinds_are_not_single_values():
    """ The data kinds of the GPU test make the sums of squares inexact -- the enclosures are honest intervals there. """
    for kind in ('bright-65535', 'tiny', 'log-uniform'):
        src, ref = ew.raster_pair(kind, SHAPE, seed=1)
        enc = ew.enclose('gain-offset', src, None, ref, None, (5, 5), True, None)
        assert not enc.sums['S2'].point.all(), kind
