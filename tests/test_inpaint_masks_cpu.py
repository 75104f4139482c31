"""
CPU tests of the chosen in-painting masks (tests/_inpaint_masks.py): the two oracles agree on them bit for bit, every family
holds what it was built for -- judged by brute-force quadrant distances, never by a kernel or by the oracles -- and wherever
those distances decide a target's value on their own, the oracle's value is the inverse-distance mean recomputed from them.
tests/test_gpu_inpaint_exact.py then holds the kernels to the C oracle on the same planes.
"""
import numpy as np
import pytest

import _inpaint_masks as M
from oracle import oracle_np as onp

CASES = M.cases()
NONE = M.NONE


@pytest.fixture(scope='module')
def oc():
    from homonim_amd import build
    build.build_oracle(verbose=False)
    from oracle import oracle_c
    assert oracle_c.available()
    return oracle_c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the two oracles agree --------------------------------------------------------------------------------------------
# oracle_np is plain loops: the large planes go through it as crops that keep the family's effect (a crop is a raster of its
# own; both oracles get the same one)
def _crops(name):
    img, flags = CASES[name]
    h, w = flags.shape
    fam = M.family(name)
    if name == 'reach':
        return [np.s_[:, 97:108], np.s_[97:108, :]]
    if fam == 'circle':
        c = h // 2
        return [np.s_[:, :]] if h <= 80 else [np.s_[:c + 2, :c + 2]]   # (the centre with its whole top-left quadrant)
    if name == 'lattice':
        return [np.s_[:, 120:200]]
    if fam == 'edges':
        return [{'col0': np.s_[90:, :104], 'lastcol': np.s_[90:, -104:], 'row0': np.s_[:104, 300:], 'lastrow': np.s_[-104:, 300:]}[
            name[6:-1]]]
    if fam == 'dense':
        return [np.s_[:64, w - 64:]]
    if name == 'holes':
        return [np.s_[20:70, 90:150]]
    return [np.s_[:, :]]


@pytest.mark.parametrize('name', [n for n in CASES if _crops(n)])
def test_c_oracle_equals_numpy_oracle(oc, name):
    img, flags = CASES[name]
    for crop in _crops(name):
        i, f = np.ascontiguousarray(img[crop]), np.ascontiguousarray(flags[crop])
        assert f.size <= 142 * 142
        a, b = oc.fill_nodata(i, f == 1), onp.fill_nodata(i, f == 1)
        keep = f != 2   # (flag 2 is a target to the oracles and nothing to the kernels: outside the comparison set)
        assert (_bits(a)[keep] == _bits(b)[keep]).all(), (name, np.argwhere(keep & (_bits(a) != _bits(b)))[:5])
        assert (_bits(a)[f == 1] == _bits(i)[f == 1]).all()


def test_the_flag_route_planes_hold_every_special_value(oc):
    img, gain, r2, thresh = M.flag_route_planes()
    t = np.float32(thresh)
    assert np.isnan(gain).sum() > 100 and np.isnan(r2).sum() > 100
    assert (r2 == t).sum() > 100 and (r2 == np.nextafter(t, np.float32(1))).sum() > 100
    assert ((gain == 0) & ~np.signbit(gain)).sum() > 100 and ((gain == 0) & np.signbit(gain)).sum() > 100
    assert np.isposinf(r2).sum() > 100 and np.isneginf(r2).sum() > 100 and (gain < 0).sum() > 100
    src = (r2 > t) & (gain > 0)
    assert 0.2 < src.mean() < 0.8
    a, b = oc.fill_nodata(img[:, :120], src[:, :120]), onp.fill_nodata(img[:, :120], src[:, :120])
    assert (_bits(a) == _bits(b)).all()


# ---- every family holds what it promises ------------------------------------------------------------------------------
def test_tie_distances_beyond_the_packed_range():
    on, off = M.tie_candidates(M.FTAB_N, M.MAX_DIST ** 2)
    assert (len(on), len(off)) == (234, 722)
    big = [n for n in M.CIRCLE_N if n >= M.FTAB_N]
    assert all(n in on or n in off for n in big)
    assert any(n in on for n in big) and any(n in off for n in big)
    assert any(n < M.FTAB_N for n in M.CIRCLE_N) and M.FTAB_N in M.CIRCLE_N and M.MAX_DIST ** 2 in M.CIRCLE_N
    print(f'[masks] tie distances in {M.FTAB_N}..{M.MAX_DIST ** 2}: {len(on)} set, {len(off)} clear; circles: '
          + ', '.join(f'{n}{"t" if M.tie_bit(n) else ""}' for n in M.CIRCLE_N))


def test_reach_family(oc):
    img, flags = CASES['reach']
    d2 = M.distances('reach')[0]
    got = oc.fill_nodata(img, flags == 1)
    filled = _bits(got) != _bits(img)
    sy = sx = 102
    # exactly 100 and exactly 101 away in the four directions, and the 60-80-100 triangle with one more column
    for (y, x), q, n in (((sy + 100, sx), 0, 10000), ((sy - 100, sx), 1, 10000), ((sy, sx + 100), 0, 10000), ((sy, sx - 100), 2, 10000),
                         ((sy + 60, sx + 80), 0, 10000), ((sy + 80, sx - 60), 2, 10000), ((sy - 60, sx + 80), 1, 10000),
                         ((sy - 80, sx - 60), 3, 10000)):
        assert flags[y, x] == 0 and d2[q, y, x] == n and (d2[:, y, x] != NONE).sum() == 1, (y, x)
        assert filled[y, x] and got[y, x] == img[sy, sx]
    for y, x in ((sy + 101, sx), (sy - 101, sx), (sy, sx + 101), (sy, sx - 101), (sy + 61, sx + 80), (sy + 80, sx - 61),
                 (sy - 61, sx + 80), (sy - 80, sx - 61)):
        assert flags[y, x] == 0 and (d2[:, y, x] == NONE).all() and not filled[y, x], (y, x)
    # the own row belongs to the top quadrants, the own column to the left ones
    assert d2[0, sy, sx + 5] == 25 and d2[1, sy, sx + 5] == NONE and d2[2, sy, sx - 5] == 25 and d2[3, sy, sx - 5] == NONE
    assert d2[0, sy + 5, sx] == 25 and d2[2, sy + 5, sx] == NONE and d2[1, sy - 5, sx] == 25 and d2[3, sy - 5, sx] == NONE
    n100 = int(((d2 == 10000).any(axis=0) & (flags == 0)).sum())
    print(f'[masks] reach: {n100} targets at distance exactly 100, {int(filled.sum())} filled, '
          f'{int(((flags == 0) & ~filled).sum())} out of reach')
    assert n100 == 20 and ((d2 != NONE).any(axis=0) & (flags == 0) == filled).all()


def test_words_family(oc):
    img, flags = CASES['words']
    d2 = M.distances('words')[0]
    got = oc.fill_nodata(img, flags == 1)
    src = dict(M.WORDS_SOURCES)   # row -> column
    for row, col in src.items():
        assert flags[row, col] == 1 and flags[:, col].sum() == 1
    assert {1, 3, 5, 7} == {x for x in range(9) if flags[:, x].sum() == 0}
    # (target row, source row, quadrant of the target's own column, in reach?): one and two 64-row words apart, both directions
    pairs = [(163, 63, 0, True), (164, 63, 0, False), (0, 64, 1, True), (164, 64, 0, True), (300, 200, 0, True), (301, 200, 0, False),
             (150, 200, 1, True), (100, 200, 1, True), (99, 200, 1, False), (229, 329, 1, True), (228, 329, 1, False),
             (270, 329, 1, True), (100, 0, 0, True), (101, 0, 0, False)]
    for ty, sy, q, reach in pairs:
        x = src[sy]
        assert abs(ty // 64 - sy // 64) in (1, 2) and flags[ty, x] == 0
        if reach and (ty, sy) == (0, 64):   # in reach, but the source at row 63 two columns to the left is nearer: 63^2 + 2^2 < 64^2
            assert d2[q, ty, x] == 63 ** 2 + 2 ** 2 and got[ty, x] != img[ty, x]
        elif reach:   # the pair decides the quadrant: a wrong seed of the column table shows in the value
            assert d2[q, ty, x] == (ty - sy) ** 2 and got[ty, x] != img[ty, x], (ty, sy)
        else:
            assert d2[q, ty, x] != (ty - sy) ** 2, (ty, sy)
    # the source at row 64 seeds word 0 of its column from the word below: it decides the bottom-right quadrant of the targets one
    # column to its left (in its own column the source at (63, 2) is nearer, above)
    assert flags[0, 3] == 0 and d2[3, 0, 3] == 64 ** 2 + 1 and d2[3, 10, 3] == 54 ** 2 + 1 and M.distances('words')[1][3, 0, 3] == 1
    assert (M.distances('words')[2][3, 0, 3], M.distances('words')[3][3, 0, 3]) == (64, 4)
    assert flags[329].sum() == 1 and (d2[1, 329] == NONE).all() and (d2[3, 329] == NONE).all()   # the last row: nothing below
    print(f'[masks] words: {len(pairs)} source/target pairs across one and two words, '
          f'{int((flags == 0).sum())} targets, {int(((d2 == NONE).all(axis=0) & (flags == 0)).sum())} out of reach')


@pytest.mark.parametrize('n', M.CIRCLE_N)
def test_circle_family(oc, n):
    name = f'circle[{n}]'
    img, flags = CASES[name]
    dist = M.distances(name)
    d2, cnt = dist[0], dist[1]
    c = flags.shape[0] // 2
    assert flags[c, c] == 0 and (d2[:, c, c] == n).all()
    assert (cnt[:, c, c] >= 2).any(), 'no quadrant of the centre holds two sources at the same distance'
    got = oc.fill_nodata(img, flags == 1)
    rule, wrong = M.mean_with_tie_rule(img, flags, dist, c, c), M.mean_with_tie_rule(img, flags, dist, c, c, invert=True)
    assert _bits(rule) != _bits(wrong), 'the two choices cannot be told apart on this image'
    assert _bits(got[c, c]) == _bits(rule), f'tie bit of {n} is {M.tie_bit(n)}: the oracle took the other candidate'
    print(f'[masks] {name}: tie bit {int(M.tie_bit(n))}, sources per quadrant of the centre {cnt[:, c, c].tolist()}, '
          f'{int(((cnt > 1).any(axis=0) & (flags == 0)).sum())} targets with a tie')


def test_lattice_family():
    img, flags = CASES['lattice']
    dist = M.distances('lattice')
    d2 = dist[0]
    settled = M.settled_by_packed_search(dist, flags)
    left = (flags == 0) & ~settled
    assert settled.sum() >= 100 and left.sum() >= 100
    # the waves that take the INTERIOR build of the general search (x0 = 128, 192 of a 384-column raster) hold long searches:
    # targets with an empty quadrant walk all the columns in reach
    interior = np.zeros(flags.shape, bool)
    interior[:, 128:256] = True
    long_search = left & (d2 == NONE).any(axis=0)
    assert flags.shape[1] == 384 and (long_search & interior).sum() >= 100 and (settled & interior).sum() >= 100
    print(f'[masks] lattice: {int(settled.sum())} targets for the packed search, {int(left.sum())} for the general one '
          f'({int((long_search & interior).sum())} of them with an empty quadrant in the interior waves)')


def test_lattice_settled_set_is_the_packed_model_s(oc):
    """ the brute-force account of what the packed search settles against the numpy model of the search itself """
    img, flags = CASES['lattice']
    crop = np.s_[:40, 300:]   # (keeps the raster's last column)
    i, f = np.ascontiguousarray(img[crop]), np.ascontiguousarray(flags[crop])
    got, settled = M.packed_fill(i, f == 1)
    dist = M.quadrant_distances(f)
    assert (settled == M.settled_by_packed_search(dist, f)).all() and settled.sum() >= 50
    exp = oc.fill_nodata(i, f == 1)
    assert (_bits(got)[settled] == _bits(exp)[settled]).all()


def test_edges_family():
    none_in_reach = one_quadrant = 0
    for name in CASES:
        if M.family(name) != 'edges':
            continue
        flags = CASES[name][1]
        d2 = M.distances(name)[0]
        n_q = ((d2 != NONE) & (flags == 0)).sum(axis=0)
        a, b = int(((n_q == 0) & (flags == 0)).sum()), int((n_q == 1).sum())
        print(f'[masks] {name}: {a} targets with no source in reach, {b} with exactly one non-empty quadrant')
        assert a >= 100
        none_in_reach, one_quadrant = none_in_reach + a, one_quadrant + b
    assert none_in_reach >= 100 and one_quadrant >= 100


def test_narrow_dense_holes_families():
    for name in CASES:
        fam = M.family(name)
        img, flags = CASES[name]
        if fam == 'narrow':
            assert flags.shape in M.NARROW
        elif fam == 'dense':
            h, w, d = next(c for c in M.DENSE if name == f'dense[{c[0]}x{c[1]},{c[2]}]')
            assert abs((flags == 1).mean() - d) < 0.02 and (flags == 0).any() and (flags == 1).any()
        elif fam == 'holes':
            assert (flags[30:50, 100:140] == 2).all() and (flags == 2).sum() > 800 + 300 and set(np.unique(flags)) == {0, 1, 2}
    assert np.abs(CASES['dense[130x301,0.5]'][0]).max() > 1e15 and 0 < np.abs(CASES['dense[130x301,0.5]'][0]).min() < 1e-15
    assert (CASES['none'][1] == 0).all() and (CASES['all'][1] == 1).all()
    # narrow rasters: both clamps at once -- in width 1 every target's four quadrants are its own column's two
    d2, tgt = M.distances('narrow[130x1]')[0], CASES['narrow[130x1]'][1] == 0
    assert (d2[0] == d2[2])[tgt].all() and (d2[1] == d2[3])[tgt].all() and (d2[0] != NONE)[tgt].any()


# ---- the oracle against means recomputed from the brute-force distances -------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_oracle_equals_the_mean_of_the_brute_force_sources(oc, name):
    img, flags = CASES[name]
    dist = M.distances(name)
    exp, decided = M.expected_without_ties(img, flags, dist)
    got = oc.fill_nodata(img, flags == 1)
    bad = decided & (_bits(got) != _bits(exp))
    assert not bad.any(), [M.describe(flags, dist, y, x) + f' oracle {got[y, x]!r} brute force {exp[y, x]!r}'
                           for y, x in np.argwhere(bad)[:5]]
    out_of_reach = (flags == 0) & (dist[0] == NONE).all(axis=0)
    assert (_bits(got)[out_of_reach] == _bits(img)[out_of_reach]).all()
    assert (_bits(got)[flags == 1] == _bits(img)[flags == 1]).all()
    # ... and a sample of the targets with ties, through the tie rule
    ties = np.argwhere((flags == 0) & (dist[1] > 1).any(axis=0))
    for y, x in ties[:: max(1, len(ties) // 40)]:
        assert _bits(got[y, x]) == _bits(M.mean_with_tie_rule(img, flags, dist, y, x)), M.describe(flags, dist, y, x)
    n_t = int((flags == 0).sum())
    print(f'[masks] {name}: {n_t} targets, {int(decided.sum())} decided without a tie, {len(ties)} with one, '
          f'{int(out_of_reach.sum())} out of reach')
