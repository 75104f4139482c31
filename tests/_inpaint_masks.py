"""
Chosen source masks for the in-painting step (hk_inpaint.hip), and an independent account of what a search must find on them.
Not a test: tests/test_inpaint_masks_cpu.py checks that every family holds what it is built for, tests/test_gpu_inpaint_exact.py
runs the kernels on them.

A case is (image float32, flags uint8): flag 1 = source, 0 = target, 2 = neither (what the fit kernel writes for invalid
pixels).  The image is normal noise with a fixed seed, so that a wrong source shows in the bits of the filled value.

`quadrant_distances` is a brute force over the offsets a search can accept -- it knows nothing of column tables, steps or
keys.  Quadrant membership as in the header comment of hk_inpaint.hip: the top quadrants hold the sources at or above the
target's row, the bottom ones those strictly below; the left quadrants include the target's own column, the right ones do not --
except in the raster's last column, where GDAL's clamp makes the own column the right-hand candidate as well (distance 0 in x).
A source is accepted up to distance max_dist = 100, so at most 101 x 101 (top) and 101 x 100 (bottom) offsets per side.
"""
import math
import os
import re

import numpy as np

NONE = np.iinfo(np.int32).max  # squared distance of a quadrant without a source in reach

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'homonim_amd', 'csrc', 'hk_inpaint.hip')


def kernel_const(name):
    """ an integer constant of hk_inpaint.hip, read from the source so that the models cannot drift from it """
    text = open(_SRC).read()
    m = re.search(r'constexpr\s+(?:int|unsigned)\s+' + name + r'\s*=\s*(\w+)\s*;', text)
    assert m, name
    val = m.group(1)
    if re.fullmatch(r'0x[0-9a-fA-F]+u?|\d+u?', val):
        return int(val.rstrip('u'), 0)
    m2 = re.search(r'#define\s+' + val + r'\s+(\d+)', text)  # defined through a macro with a default
    assert m2, val
    return int(m2.group(1))


MAX_DIST = kernel_const('FILL_MAX_DIST')
FAST_LAST = kernel_const('FAST_LAST')
FTAB_N = (FAST_LAST + 1) ** 2   # a quadrant the packed search settles has a squared distance below this


# ---- the tie rule ---------------------------------------------------------------------------------------------------------
def tie_bit(n: int) -> bool:
    """ GDAL compares a candidate's squared distance n with the ROUNDED square of the holder's distance: a candidate at the
    same n replaces the holder exactly when fl(fl(sqrt(n))^2) > n in float64 -- the LAST candidate met wins, else the first. """
    q = np.sqrt(np.float64(n))
    return bool(q * q > np.float64(n))


def representations(n: int):
    """ [(dy, dx)] with dy, dx >= 0 and dy^2 + dx^2 == n """
    out = []
    for dy in range(math.isqrt(n) + 1):
        dx = math.isqrt(n - dy * dy)
        if dx * dx + dy * dy == n:
            out.append((dy, dx))
    return out


def tie_candidates(lo=FTAB_N, hi=MAX_DIST * MAX_DIST):
    """ ([n with the tie bit set], [n with it clear]) among the squared distances lo..hi with several representations as a
    sum of two squares (the order of the two not counted): sources of ONE quadrant, one candidate per column, can share such
    a distance in more ways than the mirror pair (a, b) / (b, a) """
    on, off = [], []
    for n in range(lo, hi + 1):
        if len({tuple(sorted(r)) for r in representations(n)}) >= 2:
            (on if tie_bit(n) else off).append(n)
    return on, off


# ---- brute-force quadrant distances ------------------------------------------------------------------------------------
# quadrant q: 0 top-left, 1 bottom-left, 2 top-right, 3 bottom-right (the kernel's numbering)
def _offsets(q):
    """ (dy, dx) of a source relative to the target, for every offset quadrant q can accept """
    dxs = range(0, MAX_DIST + 1) if q < 2 else range(1, MAX_DIST + 1)
    dys = range(1, MAX_DIST + 1) if q & 1 else range(0, MAX_DIST + 1)
    sx, sy = (-1 if q < 2 else 1), (1 if q & 1 else -1)
    return [(sy * dy, sx * dx) for dy in dys for dx in dxs if dy * dy + dx * dx <= MAX_DIST * MAX_DIST and (dy or dx)]


def quadrant_distances(flags):
    """ -> (d2, cnt, sy, sx), each (4, h, w): per pixel and quadrant the squared distance of the nearest source (NONE without
    one in reach), how many sources lie at that distance, and the position of one of them (the only one where cnt == 1). """
    src = np.asarray(flags) == 1
    h, w = src.shape
    d2 = np.full((4, h, w), NONE, np.int32)
    cnt = np.zeros((4, h, w), np.int32)
    py = np.full((4, h, w), -1, np.int32)
    px = np.full((4, h, w), -1, np.int32)
    ys, xs = np.nonzero(src)
    if ys.size <= 2500:
        _by_source(src, ys, xs, d2, cnt, py, px)
    else:
        _by_offset(src, d2, cnt, py, px)
    # the last column is its own right-hand candidate (GDAL clamps x + step to the raster and checks that column again)
    for q in (2, 3):
        own = _own_column(src, q & 1)
        col = w - 1
        better = own[0] < d2[q, :, col]
        equal = (own[0] == d2[q, :, col]) & (own[0] != NONE)
        cnt[q, :, col] = np.where(better, 1, cnt[q, :, col] + equal)
        py[q, :, col] = np.where(better, own[1], py[q, :, col])
        px[q, :, col] = np.where(better, col, px[q, :, col])
        d2[q, :, col] = np.where(better, own[0], d2[q, :, col])
    return d2, cnt, py, px


def _own_column(src, below):
    """ last column only: (squared distance, row) of the nearest source at-or-above / strictly below in that column """
    h = src.shape[0]
    col = src[:, -1]
    rows = np.nonzero(col)[0]
    best = np.full(h, NONE, np.int32)
    at = np.full(h, -1, np.int32)
    for y in range(h):
        cand = rows[(rows > y) & (rows - y <= MAX_DIST)] if below else rows[(rows <= y) & (y - rows <= MAX_DIST)]
        if cand.size:
            r = cand.min() if below else cand.max()
            best[y], at[y] = (r - y) ** 2, r
    return best, at


def _by_source(src, ys, xs, d2, cnt, py, px):
    """ few sources: every source offers itself to the pixels of its window """
    h, w = src.shape
    for q in range(4):
        for sy, sx in zip(ys.tolist(), xs.tolist()):
            # targets of quadrant q that can see (sy, sx): left quadrants x >= sx, right x > sx; top y >= sy, bottom y < sy
            x0, x1 = (sx, min(w, sx + MAX_DIST + 1)) if q < 2 else (max(0, sx - MAX_DIST), sx)
            y0, y1 = (max(0, sy - MAX_DIST), sy) if q & 1 else (sy, min(h, sy + MAX_DIST + 1))
            if x0 >= x1 or y0 >= y1:
                continue
            yy = np.arange(y0, y1, dtype=np.int32)[:, None] - sy
            xx = np.arange(x0, x1, dtype=np.int32)[None, :] - sx
            n = yy * yy + xx * xx
            n = np.where((n <= MAX_DIST * MAX_DIST) & (n > 0), n, NONE)
            win = (q, slice(y0, y1), slice(x0, x1))
            better = n < d2[win]
            equal = (n == d2[win]) & (n != NONE)
            cnt[win] = np.where(better, 1, cnt[win] + equal)
            py[win] = np.where(better, sy, py[win])
            px[win] = np.where(better, sx, px[win])
            d2[win] = np.where(better, n, d2[win])


def _by_offset(src, d2, cnt, py, px):
    """ many sources: the open (pixel, quadrant) pairs try the offsets in the order of their length and close at the first hit """
    h, w = src.shape
    for q in range(4):
        groups = {}
        for dy, dx in _offsets(q):
            groups.setdefault(dy * dy + dx * dx, []).append((dy, dx))
        oy, ox = np.nonzero(np.ones((h, w), bool))
        for n in sorted(groups):
            if oy.size == 0:
                break
            hits = np.zeros(oy.size, np.int32)
            for dy, dx in groups[n]:
                ty, tx = oy + dy, ox + dx
                ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                hit = np.zeros(oy.size, bool)
                hit[ok] = src[ty[ok], tx[ok]]
                hits += hit
                py[q, oy[hit], ox[hit]] = ty[hit]
                px[q, oy[hit], ox[hit]] = tx[hit]
            found = hits > 0
            d2[q, oy[found], ox[found]] = n
            cnt[q, oy[found], ox[found]] = hits[found]
            oy, ox = oy[~found], ox[~found]
            # a pixel near the raster's edge whose quadrant holds no in-raster offset longer than this has tried them all
            far_y = ((h - 1 - oy) if q & 1 else oy).astype(np.int64)
            far_x = (ox if q < 2 else (w - 1 - ox)).astype(np.int64)
            keep = far_y * far_y + far_x * far_x > n
            oy, ox = oy[keep], ox[keep]


def weighted_mean(image, d2, py, px, y, x):
    """ the inverse-distance mean of the quadrants' sources of target (y, x) as GDAL forms it: float64 sums over the quadrants
    in order, weights 1 / sqrt(d2), cast to float32; None when no quadrant holds a source """
    wsum, vsum, has = np.float64(0), np.float64(0), False
    for q in range(4):
        if d2[q, y, x] != NONE:
            wgt = np.float64(1) / np.sqrt(np.float64(d2[q, y, x]))
            wsum = wsum + wgt
            vsum = vsum + np.float64(image[py[q, y, x], px[q, y, x]]) * wgt
            has = True
    return np.float32(vsum / wsum) if has else None


def expected_without_ties(image, flags, dist=None):
    """ -> (expected image, decided mask): the fill of every target whose quadrants each hold ONE nearest source (or none),
    recomputed from the brute-force distances alone; `decided` marks those targets.  Vectorised form of weighted_mean. """
    d2, cnt, py, px = dist if dist is not None else quadrant_distances(flags)
    h, w = flags.shape
    target = np.asarray(flags) == 0
    decided = target & (cnt <= 1).all(axis=0)
    wsum = np.zeros((h, w), np.float64)
    vsum = np.zeros((h, w), np.float64)
    has = np.zeros((h, w), bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for q in range(4):
            ok = d2[q] != NONE
            wgt = np.where(ok, np.float64(1) / np.sqrt(np.where(ok, d2[q], 1).astype(np.float64)), 0.0)
            val = image[np.clip(py[q], 0, h - 1), np.clip(px[q], 0, w - 1)].astype(np.float64)
            wsum = np.where(ok, wsum + wgt, wsum)
            vsum = np.where(ok, vsum + val * wgt, vsum)
            has |= ok
        filled = (vsum / wsum).astype(np.float32)
    out = np.where(decided & has, filled, image).astype(np.float32)
    return out, decided


def describe(flags, dist, y, x):
    """ one line about a pixel for failure messages: its flag and its brute-force quadrant distances """
    d2, cnt = dist[0], dist[1]
    parts = []
    for q, name in enumerate(('TL', 'BL', 'TR', 'BR')):
        n = int(d2[q, y, x])
        parts.append(f'{name} -' if n == NONE else f'{name} {n}x{int(cnt[q, y, x])}{"t" if tie_bit(n) else ""}')
    return f'({y}, {x}) flag {int(flags[y, x])}: ' + ', '.join(parts)


# ---- the families -----------------------------------------------------------------------------------------------------
CIRCLE_N = (25, 325, 625, 629, 1105, 4225, 5525, 9425, 10000)   # below, at and above FTAB_N; tie bit set and clear
NARROW = [(h, w) for w in (1, 2, 3, 5) for h in (1, 8, 65, 130)]
DENSE = [(h, w, d) for h, w in ((70, 257), (130, 301)) for d in (0.9, 0.5, 0.1, 0.01)]
WORDS_SOURCES = ((0, 0), (63, 2), (64, 4), (200, 6), (329, 8))   # (row, column); columns 1, 3, 5, 7 hold none
LATTICE_PITCH, LATTICE_ORIGIN = (29, 31), (7, 5)


def _image(shape, seed, mixed=False):
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 1, shape)
    if mixed:  # magnitudes between 1e-20 and 1e20: a sum in the wrong order or precision shows
        img = img * 10.0 ** rng.uniform(-20, 20, shape)
    return img.astype(np.float32)


def _random_flags(shape, density, seed):
    return (np.random.default_rng(seed).uniform(size=shape) < density).astype(np.uint8)


def circle(n):
    r = math.isqrt(n - 1) + 1 if n > 0 else 0   # ceil(sqrt(n))
    side, c = 2 * r + 7, r + 3
    yy, xx = np.mgrid[0:side, 0:side]
    flags = ((yy - c) ** 2 + (xx - c) ** 2 == n).astype(np.uint8)
    return _image((side, side), 1000 + n), flags


def _build():
    cases = {}
    f = np.zeros((205, 205), np.uint8)
    f[102, 102] = 1
    cases['reach'] = (_image(f.shape, 11), f)
    f = np.zeros((330, 9), np.uint8)
    for y, x in WORDS_SOURCES:
        f[y, x] = 1
    cases['words'] = (_image(f.shape, 12), f)
    for n in CIRCLE_N:
        cases[f'circle[{n}]'] = circle(n)
    f = np.zeros((72, 384), np.uint8)
    f[LATTICE_ORIGIN[0]::LATTICE_PITCH[0], LATTICE_ORIGIN[1]::LATTICE_PITCH[1]] = 1
    cases['lattice'] = (_image(f.shape, 13), f)
    for k, name in enumerate(('col0', 'lastcol', 'row0', 'lastrow')):
        f = np.zeros((120, 330), np.uint8)
        f[(slice(None), 0) if k == 0 else (slice(None), -1) if k == 1 else (0, slice(None)) if k == 2 else (-1, slice(None))] = 1
        cases[f'edges[{name}]'] = (_image(f.shape, 20 + k), f)
    for h, w in NARROW:
        cases[f'narrow[{h}x{w}]'] = (_image((h, w), 100 * h + w), _random_flags((h, w), 0.3, 7 * h + w))
    for h, w, d in DENSE:
        seed = int(1000 * d) + h
        cases[f'dense[{h}x{w},{d}]'] = (_image((h, w), seed, mixed=h == 130), _random_flags((h, w), d, seed + 1))
    cases['none'] = (_image((40, 70), 31), np.zeros((40, 70), np.uint8))
    cases['all'] = (_image((40, 70), 32), np.ones((40, 70), np.uint8))
    f = _random_flags((90, 300), 0.5, 41)
    f[30:50, 100:140] = 2
    f[np.random.default_rng(42).uniform(size=f.shape) < 0.03] = 2
    cases['holes'] = (_image(f.shape, 43), f)
    return cases


_CASES = None


def cases():
    """ {name: (image, flags)}, built once; callers must not write into the arrays """
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for img, f in _CASES.values():
            img.setflags(write=False)
            f.setflags(write=False)
    return _CASES


def family(name):
    return name.split('[')[0]


def flag_route_planes():
    """ (image, gain, r2, thresh) of the `flag-route` family: the source flags come from (r2 > thresh) & (gain > 0) on the
    device (inpaint_flag_kernel); every way a comparison can go wrong sits in the planes several times """
    h, w, thresh = 64, 300, np.float32(0.25)
    rng = np.random.default_rng(51)
    gain = rng.normal(0.6, 1.0, (h, w)).astype(np.float32)
    r2 = rng.uniform(0, 0.6, (h, w)).astype(np.float32)
    pick = rng.integers(0, 12, (h, w))
    gain[pick == 0] = np.nan
    r2[pick == 1] = np.nan
    r2[pick == 2] = thresh                                   # not above the threshold
    r2[pick == 3] = np.nextafter(thresh, np.float32(1))      # just above
    gain[pick == 4] = 0.0
    gain[pick == 5] = -0.0
    r2[pick == 6] = np.inf
    gain[pick == 7] = -np.abs(gain[pick == 7])
    gain[pick == 8] = np.float32(1e-45)                      # the smallest subnormal is positive
    r2[pick == 9] = -np.inf
    return _image((h, w), 52), gain, r2, float(thresh)


# ---- the packed search as a numpy model (tests/test_inpaint_packed_cpu.py) ----------------------------------------------
def settled_by_packed_search(dist, flags):
    """ the targets the packed search settles: all four quadrants hold a source closer than FAST_LAST + 1 -- each is then
    found within FAST_LAST columns and beats every clipped or farther candidate (hk_inpaint.hip, "SETTLED").  The last
    column never settles: its right quadrants see no staged column. """
    d2 = dist[0]
    ok = (np.asarray(flags) == 0) & (d2 < FTAB_N).all(axis=0)
    ok[:, -1] = False
    return ok


_DIST = {}


def distances(name):
    """ quadrant_distances of a named case, computed once """
    if name not in _DIST:
        _DIST[name] = quadrant_distances(cases()[name][1])
    return _DIST[name]


def tied_sources(flags, y, x, q, n):
    """ [(sy, sx)] of the sources of quadrant q of target (y, x) at squared distance n, by ascending column distance -- the
    order in which a search meets them (one candidate per column) """
    src = np.asarray(flags) == 1
    h, w = src.shape
    out = []
    for dy, dx in representations(n):
        if (q & 1 and dy == 0) or (q >= 2 and dx == 0 and x != w - 1):
            continue
        sy, sx = (y + dy if q & 1 else y - dy), (x + dx if q >= 2 else x - dx)
        if 0 <= sy < h and 0 <= sx < w and src[sy, sx]:
            out.append((sy, sx))
    return sorted(out, key=lambda p: abs(p[1] - x))


def mean_with_tie_rule(image, flags, dist, y, x, invert=False):
    """ weighted_mean where a quadrant's several nearest sources are resolved by the tie bit of their squared distance: set --
    the last one met (largest column distance), clear -- the first.  `invert`: the opposite choice (what a wrong rule gives). """
    d2 = dist[0]
    py, px = dist[2].copy(), dist[3].copy()
    for q in range(4):
        n = int(d2[q, y, x])
        if n != NONE and dist[1][q, y, x] > 1:
            tied = tied_sources(flags, y, x, q, n)
            assert len(tied) == dist[1][q, y, x]
            py[q, y, x], px[q, y, x] = tied[-1] if tie_bit(n) != invert else tied[0]
    return weighted_mean(image, d2, py, px, y, x)


# ---- the packed search itself, restated (constants read from the kernel source) ------------------------------------------
FAST_CLIP, NONE_SQ = kernel_const('FAST_CLIP'), kernel_const('NONE_SQ')


def column_tables(src_mask, max_dist=MAX_DIST):
    """ squared row distances to the nearest source at-or-above / strictly below, NONE_SQ beyond max_dist (inpaint_table_kernel) """
    h, w = src_mask.shape
    up = np.full((h, w), NONE_SQ, np.int64)
    dn = np.full((h, w), NONE_SQ, np.int64)
    for x in range(w):
        last = None
        for y in range(h):
            if src_mask[y, x]:
                last = y
            if last is not None and y - last <= max_dist:
                up[y, x] = (y - last) ** 2
        last = None
        for y in range(h - 1, -1, -1):
            if last is not None and last - y <= max_dist + 1:
                dn[y, x] = (last - y) ** 2
            if src_mask[y, x]:
                last = y
    return up, dn


def packed_fill(image, src_mask):
    """ (filled image, settled mask): the packed search of every target; unsettled targets keep their value """
    h, w = image.shape
    up, dn = column_tables(src_mask)
    out = image.copy()
    settled = np.zeros((h, w), bool)
    clip = lambda sq: min(int(sq), FAST_CLIP) << 5  # noqa: E731  (fast_stage_word)
    for y in range(h):
        for x in range(w):
            if src_mask[y, x]:
                continue
            kf = [0xffff] * 4  # quadrants: 0 up-left, 1 down-left (both with the own column), 2 up-right, 3 down-right
            kl = [0xffff] * 4
            ok = False
            for k in range(FAST_LAST + 1):
                cf, cl = (k * k << 5) + k, (k * k << 5) + 31 - k
                for side, xs in ((0, x - k), (2, x + k)):
                    if (side == 2 and k == 0) or xs < 0 or xs >= w:   # outside the raster: no source (GDAL re-checks the edge column)
                        continue
                    for q, sq in ((side, up[y, xs]), (side + 1, dn[y, xs])):
                        kf[q] = min(kf[q], clip(sq) + cf)
                        kl[q] = min(kl[q], clip(sq) + cl)
                        assert clip(sq) + cl <= 0xffff
                if k >= 4 and k % 4 == 0 and max(kf) >> 5 < (k + 1) ** 2:
                    ok = True
                    break
            if not ok:
                continue
            wsum, vsum = np.float64(0), np.float64(0)
            for q in range(4):
                n = kf[q] >> 5
                assert n == kl[q] >> 5 and 0 < n < (FAST_LAST + 1) ** 2
                root = np.sqrt(np.float64(n))
                tie = root * root > n                                  # GDAL's QUAD_CHECK on an equal squared distance
                dx = 31 - (kl[q] & 31) if tie else kf[q] & 31
                dy = int(round(np.sqrt(n - dx * dx)))
                assert dy * dy + dx * dx == n
                sy, sx = (y + dy if q & 1 else y - dy), (x + dx if q >= 2 else x - dx)
                assert src_mask[sy, sx]
                wgt = np.float64(1) / root
                wsum = wsum + wgt
                vsum = vsum + np.float64(image[sy, sx]) * wgt
            out[y, x] = np.float32(vsum / wsum)
            settled[y, x] = True
    return out, settled
