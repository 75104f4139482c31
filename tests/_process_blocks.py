""" The block loop of RasterFuse.process / RasterCompare.process on two different grids, held to references that the tests build
themselves (tests/test_process_blocks_cpu.py on the host, tests/test_gpu_process_blocks.py on the device).  Plain numpy,
``fractions.Fraction`` and the oracle; of homonim_amd/fuse.py only ``block_pairs_multires`` is used -- pinned by the goldens
(tests/test_fuse_cpu.py) and by the rational window checks below -- and of the package the geometry carriers and model classes.

Geometries
----------
North-up pairs in one CRS, every transform entry a multiple of 1/8: double arithmetic on the coordinates is exact, every floor /
ceil / round-half-even is unambiguous, and ``Fraction`` of a coefficient is the coefficient.  ``CASES`` lists them: the reference
2.5 x, 3 x and 2 x coarser than a 70 x 90 source, coarser along one axis only, flush with the source on two sides (top and right), and
-- under ``proc_crs=src`` -- a 12 m reference under a 24 x 40 source of 30 m pixels and the 2.5 x pair again.  No geometry had to be
dropped: in every one of them each source pixel lies in exactly one source out-window (``check_block_windows`` asserts it; two
neighbouring out-blocks round the SAME boundary coordinate, so the rounded windows cannot gap or overlap while that coordinate is
computed exactly, which is what the multiples of 1/8 ensure).

Window rule, in rationals (``check_block_windows``)
--------------------------------------------------
Blocks are cut on the processing grid inside the processing window (the reference window that covers the source, or the source
window that covers that): the out-blocks tile it exactly once, each in-block is its out-block grown by the overlap and clipped to
the window; the other grid's in-window is the smallest whole-pixel window containing the in-block's bounds (floor / ceil of the
edges), its out-window has the out-block's edges rounded half to even.

Reference (A): placement (``expected_by_blocks``)
-------------------------------------------------
What ``process`` must return, bit for bit, from one ``fit_apply`` call per block that the test makes itself: the helper's own
boundless reader (``read_window``: outside is NaN as float32 when the raster's nodata is None or NaN, else the nodata value in the
raster's own dtype), its own translation of the two transforms by the IN-windows (``shifted``), its own placement (``place``: the
out-window clipped to the raster, copied from the same offsets inside the in-window; parameter band ``pi`` of source band ``b`` in
plane ``pi * n_src + b``; the corrected planes start as the output nodata, the parameter planes as NaN).

Reference (B): a closed form (``closed_form_pair`` / ``closed_form_expected``)
------------------------------------------------------------------------------
Model ``gain``, kernel (1, 1), a source of ones with two NaN holes, a reference of position codes ``r * ref_width + c + 1`` (below
2^24: exact in float32), ``upsampling=nearest`` (and ``downsampling=nearest`` under ``proc_crs=src``; under ``proc_crs=ref`` the
average of ones is exactly 1).  Then the corrected pixel is the code of the reference pixel that holds its centre, NaN in the holes;
under ``proc_crs=ref`` gain band 0 is the reference itself wherever the footprint of the reference pixel holds a valid source pixel
and NaN elsewhere; under ``proc_crs=src`` the gain plane is the corrected plane.

RasterCompare (``compare_pair`` / ``compare_exact_sums``)
---------------------------------------------------------
Small integer codes in both rasters (every float32 product and squared difference exact, every sum an integer below 2^53), a hole
in each, ``nearest`` both ways: the seven sums over the WHOLE image in integer arithmetic, which every partition must return.

Guard (``centre_index``)
------------------------
A destination pixel centre that lies within 1e-9 of a source pixel edge WITHOUT lying on it could have its ``floor`` moved by the
1e-10 nudge of ``nearest``: such a case is mis-designed and ``centre_index`` raises.  A centre exactly ON an edge is allowed: the
double coordinate is then off by a few 2^-53 at most, the nudge brings it to the upper pixel, which is the exact ``floor`` (the
3 x pair has such a row: its reference origin lies half a reference pixel above the source, so the centre of source row 1 is the edge
between reference rows 0 and 1; the aligned 2 x pair has every reference centre on a source pixel corner). """
import functools
import math
import warnings
from fractions import Fraction as Fr
from typing import NamedTuple, Optional, Tuple

import numpy as np

from homonim_amd import Affine, CRS, RasterArray
from homonim_amd import fuse
from homonim_amd.enums import Resampling
from oracle import oracle_np as onp

SRC_X0, SRC_Y0 = 1000., 5000.
OVERLAPS = ((1, 1), (3, 3), (2, 4))
NEAR = Fr(1, 10 ** 9)


class Case(NamedTuple):
    name: str
    src_shape: Tuple[int, int]
    src_res: float
    ref_res: Tuple[float, float]    # (x, y)
    ref_out: Tuple[float, float]    # the reference origin lies this many reference pixels (x, y) outside the source's
    ref_shape: Tuple[int, int]
    proc_crs: str

    @property
    def src_tf(self) -> Affine:
        return Affine(self.src_res, 0., SRC_X0, 0., -self.src_res, SRC_Y0)

    @property
    def ref_tf(self) -> Affine:
        (rx, ry), (fx, fy) = self.ref_res, self.ref_out
        return Affine(rx, 0., SRC_X0 - fx * rx, 0., -ry, SRC_Y0 + fy * ry)

    @property
    def grids(self):
        return fuse.Grid(self.src_tf, *self.src_shape), fuse.Grid(self.ref_tf, *self.ref_shape)


CASES = {c.name: c for c in (
    Case('2.5x-ref', (70, 90), 10., (25., 25.), (0.75, 1.25), (31, 38), 'ref'),
    Case('3x-ref', (70, 90), 10., (30., 30.), (0.25, 0.5), (25, 32), 'ref'),
    Case('2x-aligned-ref', (70, 90), 10., (20., 20.), (1., 1.), (37, 47), 'ref'),
    Case('x-only-ref', (70, 90), 10., (25., 10.), (0.75, 1.), (72, 38), 'ref'),
    Case('12-under-30-src', (24, 40), 30., (12., 12.), (0.625, 0.875), (62, 102), 'src'),
    Case('2.5x-src', (70, 90), 10., (25., 25.), (0.75, 1.25), (31, 38), 'src'),
    Case('2x-flush-ref', (70, 90), 10., (20., 20.), (1., 0.), (36, 46), 'ref'),      # flush with the source at the top and on the right
)}
REF_CASES = [n for n, c in CASES.items() if c.proc_crs == 'ref']
SRC_CASES = [n for n, c in CASES.items() if c.proc_crs == 'src']


# -- rationals ------------------------------------------------------------------------------------------------------------------
class FrGrid(NamedTuple):
    x: Tuple[Fr, Fr]   # (origin, step) of the columns
    y: Tuple[Fr, Fr]   # (origin, step) of the rows (the step is negative: north-up)
    height: int
    width: int


def fr_grid(grid) -> FrGrid:
    t = grid.transform
    for v in (t.a, t.c, t.e, t.f):
        assert Fr(v).denominator <= 8, f'{v!r} is no multiple of 1/8'
    return FrGrid((Fr(t.c), Fr(t.a)), (Fr(t.f), Fr(t.e)), int(grid.height), int(grid.width))


def is_dyadic_grid(grid) -> bool:
    t = grid.transform
    return all(Fr(v).denominator <= 8 for v in (t.a, t.c, t.e, t.f))


def _to_pix(axis, world):
    return (world - axis[0]) / axis[1]


def _to_world(axis, pix):
    return axis[0] + pix * axis[1]


def _corners(win):
    """ (col0, row0, col1, row1) """
    return (win.col_off, win.row_off, win.col_off + win.width, win.row_off + win.height)


def _covering(grid: FrGrid, other: FrGrid, corners):
    """ the smallest whole-pixel window of `grid` that contains the pixel window `corners` of `other` """
    c0, r0, c1, r1 = corners
    return (math.floor(_to_pix(grid.x, _to_world(other.x, c0))), math.floor(_to_pix(grid.y, _to_world(other.y, r0))),
            math.ceil(_to_pix(grid.x, _to_world(other.x, c1))), math.ceil(_to_pix(grid.y, _to_world(other.y, r1))))


def _rounded(grid: FrGrid, other: FrGrid, corners):
    """ the pixel window `corners` of `other` on `grid`, edges rounded half to even (``round`` of a Fraction does that) """
    c0, r0, c1, r1 = corners
    return (round(_to_pix(grid.x, _to_world(other.x, c0))), round(_to_pix(grid.y, _to_world(other.y, r0))),
            round(_to_pix(grid.x, _to_world(other.x, c1))), round(_to_pix(grid.y, _to_world(other.y, r1))))


def exact_pair_windows(src: FrGrid, ref: FrGrid):
    """ (source window, reference window) as corners: the reference window is the smallest that covers the source, the source
    window the smallest that covers that """
    ref_win = _covering(ref, src, (0, 0, src.width, src.height))
    return _covering(src, ref, ref_win), ref_win


def check_block_windows(src_grid, ref_grid, proc_crs: str, n_bands: int, overlap, bps, src_once: bool = True):
    """ Assert the window rule of the module docstring on a block list, in rationals; with `src_once` also that every source
    pixel lies in exactly one source out-window clipped to the raster.  -> (block rows, block columns) of a band """
    S, R = fr_grid(src_grid), fr_grid(ref_grid)
    src_win, ref_win = exact_pair_windows(S, R)
    proc_is_ref = str(proc_crs) == 'ref'
    P, O = (R, S) if proc_is_ref else (S, R)
    p_c0, p_r0, p_c1, p_r1 = ref_win if proc_is_ref else src_win
    ov_r, ov_c = overlap
    assert sorted({bp.band_i for bp in bps}) == list(range(n_bands))
    counts = None
    for band in range(n_bands):
        band_bps = [bp for bp in bps if bp.band_i == band]
        tiles = np.zeros((p_r1 - p_r0, p_c1 - p_c0), int)
        src_hits = np.zeros((S.height, S.width), int)
        row_offs, col_offs = set(), set()
        for bp in band_bps:
            if proc_is_ref:
                p_in, p_out, o_in, o_out = bp.ref_in_block, bp.ref_out_block, bp.src_in_block, bp.src_out_block
            else:
                p_in, p_out, o_in, o_out = bp.src_in_block, bp.src_out_block, bp.ref_in_block, bp.ref_out_block
            c0, r0, c1, r1 = _corners(p_out)
            assert p_c0 <= c0 < c1 <= p_c1 and p_r0 <= r0 < r1 <= p_r1, (bp, 'out-block outside the processing window')
            tiles[r0 - p_r0:r1 - p_r0, c0 - p_c0:c1 - p_c0] += 1
            row_offs.add(r0)
            col_offs.add(c0)
            grown = (max(c0 - ov_c, p_c0), max(r0 - ov_r, p_r0), min(c1 + ov_c, p_c1), min(r1 + ov_r, p_r1))
            assert _corners(p_in) == grown, (bp, 'in-block is not the out-block grown by the overlap')
            assert _corners(o_in) == _covering(O, P, grown), (bp, 'other in-window is not the smallest cover')
            assert _corners(o_out) == _rounded(O, P, (c0, r0, c1, r1)), (bp, 'other out-window is not the rounded out-block')
            assert bp.outer == (grown[0] == p_c0 or grown[1] == p_r0 or grown[2] == p_c1 or grown[3] == p_r1), bp
            sc0, sr0, sc1, sr1 = _corners(bp.src_out_block)
            src_hits[max(sr0, 0):max(min(sr1, S.height), 0), max(sc0, 0):max(min(sc1, S.width), 0)] += 1
        assert (tiles == 1).all(), f'band {band}: the out-blocks do not tile the processing window exactly once'
        if src_once:
            assert (src_hits == 1).all(), (f'band {band}: {int((src_hits == 0).sum())} source pixels unwritten, '
                                           f'{int((src_hits > 1).sum())} written more than once')
        assert counts in (None, (len(row_offs), len(col_offs)))
        counts = (len(row_offs), len(col_offs))
        assert len(band_bps) == counts[0] * counts[1]
    return counts


def centre_index(n_dst: int, k: Fr, o: Fr, what: str = '') -> np.ndarray:
    """ ``floor(k * (j + 1/2) + o)`` for j in range(n_dst): the source pixel that holds destination pixel j's centre (may lie outside
    the source).  Raises when a centre lies within 1e-9 of a pixel edge without lying on it (the guard of the module docstring). """
    out = np.empty(n_dst, np.int64)
    for j in range(n_dst):
        s = k * (j + Fr(1, 2)) + o
        d = abs(s - round(s))
        if 0 < d < NEAR:
            raise AssertionError(f'mis-designed case {what}: centre {j} lies {float(d)!r} from a pixel edge')
        out[j] = math.floor(s)
    return out


def centre_indices(dst_grid, src_grid, what: str = ''):
    """ (rows, cols): for every destination row / column the source row / column that holds its centre, in rationals """
    D, S = fr_grid(dst_grid), fr_grid(src_grid)
    rows = centre_index(D.height, D.y[1] / S.y[1], (D.y[0] - S.y[0]) / S.y[1], f'{what} rows')
    cols = centre_index(D.width, D.x[1] / S.x[1], (D.x[0] - S.x[0]) / S.x[1], f'{what} columns')
    return rows, cols


def _footprint_ranges(n_dst: int, k: Fr, o: Fr, n_src: int):
    """ for every destination pixel the half-open range of source pixels that share length with it, clipped to the source """
    out = []
    for j in range(n_dst):
        lo, hi = max(k * j + o, Fr(0)), min(k * (j + 1) + o, Fr(n_src))
        out.append((math.floor(lo), math.ceil(hi)) if hi > lo else (0, 0))
    return out


# -- blocks -----------------------------------------------------------------------------------------------------------------------
def blocks_of(case: Case, n_bands: int, overlap, max_block_mem: float, proc_crs: Optional[str] = None):
    sg, rg = case.grids
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')       # the small-block ConfigWarning
        return list(fuse.block_pairs_multires(sg, rg, proc_crs or case.proc_crs, n_bands, tuple(overlap), max_block_mem))


def _grid_counts(bps, proc_crs: str):
    outs = [(bp.ref_out_block if proc_crs == 'ref' else bp.src_out_block) for bp in bps if bp.band_i == 0]
    return len({w.row_off for w in outs}), len({w.col_off for w in outs})


@functools.lru_cache(maxsize=None)
def block_mem(case_name: str, overlap, min_side: int = 3) -> float:
    """ the largest ``max_block_mem`` of 0.01 / 2^n that cuts the case into at least `min_side` x `min_side` blocks per band """
    case, mem = CASES[case_name], 0.01
    while min(_grid_counts(blocks_of(case, 1, overlap, mem), case.proc_crs)) < min_side:
        mem /= 2
    return mem


@functools.lru_cache(maxsize=None)
def compare_mem(case_name: str, proc_crs: str, at_least: int) -> float:
    """ ``max_block_mem`` for RasterCompare (overlap 0): 512 (one block) or the largest 0.05 / 2^n giving `at_least` blocks """
    case, mem = CASES[case_name], 512.
    if at_least > 1:
        mem = 0.05
        while len(blocks_of(case, 1, (0, 0), mem, proc_crs)) < at_least:
            mem /= 2
    return mem


# -- reader, translation, placement ---------------------------------------------------------------------------------------------
def _is_nan(v) -> bool:
    return v is not None and v != v


def read_window(band: np.ndarray, nodata, win):
    """ -> (array, nodata) of a window that may hang over the band or miss it: a window inside comes back as a view with the raster's
    nodata; otherwise the outside is NaN in a float32 array when the nodata is None or NaN, else the nodata value in an array of the
    band's dtype, and the nodata that comes back is that fill """
    h, w = band.shape
    rows = np.arange(win.row_off, win.row_off + win.height)
    cols = np.arange(win.col_off, win.col_off + win.width)
    r_in, c_in = (rows >= 0) & (rows < h), (cols >= 0) & (cols < w)
    if r_in.all() and c_in.all():
        return band[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1], nodata
    if nodata is None or _is_nan(nodata):
        out, fill = np.full((win.height, win.width), np.nan, np.float32), float('nan')
    else:
        out, fill = np.full((win.height, win.width), nodata, band.dtype), nodata
    if r_in.any() and c_in.any():
        out[np.ix_(r_in, c_in)] = band[np.ix_(rows[r_in], cols[c_in])]
    return out, fill


def shifted(tf: Affine, win) -> Affine:
    """ the geo-transform of a window of a north-up raster """
    return Affine(tf.a, 0., tf.c + win.col_off * tf.a, 0., tf.e, tf.f + win.row_off * tf.e)


def place(dst: np.ndarray, block: np.ndarray, in_win, out_win):
    """ the out-window, clipped to `dst`, copied from the same raster positions inside the block that was read as `in_win` """
    rows = [r for r in range(out_win.row_off, out_win.row_off + out_win.height) if 0 <= r < dst.shape[0]]
    cols = [c for c in range(out_win.col_off, out_win.col_off + out_win.width) if 0 <= c < dst.shape[1]]
    if rows and cols:
        dst[np.ix_(rows, cols)] = block[np.ix_([r - in_win.row_off for r in rows], [c - in_win.col_off for c in cols])]


def own_shard(items, rank: int, world: int, contiguous: bool):
    n = len(items)
    if contiguous:
        return [items[i] for i in range(n) if rank * n // world <= i < (rank + 1) * n // world]
    return [items[i] for i in range(n) if i % world == rank]


def written_mask(case: Case, bps) -> np.ndarray:
    """ the source pixels inside the source out-windows of `bps` (band 0) """
    m = np.zeros(case.src_shape, bool)
    for bp in bps:
        if bp.band_i == 0:
            place(m, np.ones((bp.src_in_block.height, bp.src_in_block.width), bool), bp.src_in_block, bp.src_out_block)
    return m


def expected_by_blocks(src, ref, src_nodata, ref_nodata, src_tf, ref_tf, proc_crs: str, bps, block_fn, n_param: int = 0,
                       out_dtype='float32', out_nodata=float('nan')):
    """ Reference (A).  `src`, `ref`: (bands, H, W); `bps`: the block pairs; ``block_fn(src_block, src_nodata, src_transform, ref_block,
    ref_nodata, ref_transform) -> (corrected block on the source in-window, parameter block (n_param, h, w) on the processing
    grid's in-window or None)``; `n_param`: parameter bands per source band, 0 = no parameters.  -> (corrected, params | None) """
    n_src = src.shape[0]
    out_dtype = np.dtype(out_dtype)
    fill = (np.nan if out_dtype.kind == 'f' else 0) if out_nodata is None else out_nodata
    corr = np.full(src.shape, fill, out_dtype)
    param_shape = ref.shape[-2:] if proc_crs == 'ref' else src.shape[-2:]
    params = np.full((n_param * n_src, *param_shape), np.nan, np.float32) if n_param else None
    for bp in bps:
        s_arr, s_nd = read_window(src[bp.band_i], src_nodata, bp.src_in_block)
        r_arr, r_nd = read_window(ref[bp.band_i], ref_nodata, bp.ref_in_block)
        corr_blk, param_blk = block_fn(s_arr, s_nd, shifted(src_tf, bp.src_in_block), r_arr, r_nd, shifted(ref_tf, bp.ref_in_block))
        assert corr_blk.shape == s_arr.shape and corr_blk.dtype == out_dtype
        place(corr[bp.band_i], corr_blk, bp.src_in_block, bp.src_out_block)
        if n_param:
            p_in, p_out = (bp.ref_in_block, bp.ref_out_block) if proc_crs == 'ref' else (bp.src_in_block, bp.src_out_block)
            assert param_blk.shape == (n_param, p_in.height, p_in.width)
            for pi in range(n_param):
                place(params[pi * n_src + bp.band_i], param_blk[pi], p_in, p_out)
    return corr, params


def model_block_fn(model, want_params: bool, out_dtype='float32', out_nodata=float('nan')):
    """ `block_fn` of ``expected_by_blocks``: one ``fit_apply`` of a RefSpaceModel / SrcSpaceModel per block """
    def fn(s_arr, s_nd, s_tf, r_arr, r_nd, r_tf):
        corr_ra, param_ra = model.fit_apply(RasterArray(s_arr, CRS(), s_tf, nodata=s_nd), RasterArray(r_arr, CRS(), r_tf, nodata=r_nd),
                                            want_params=want_params, out_dtype=np.dtype(out_dtype).name, out_nodata=out_nodata)
        return corr_ra.array, (param_ra.array if want_params else None)
    return fn


def _tf6(tf):
    return tuple(tf)[:6]


def oracle_gain_block_fn(proc_crs: str):
    """ `block_fn` of ``expected_by_blocks`` from the oracle, for reference (B): model gain, kernel (1, 1), nearest up-sampling
    (``proc_crs=ref``: average down, fit on the reference grid, gains and offsets back up; ``proc_crs=src``: the reference brought
    to the source grid by nearest, fit there); parameters masked by the source mask, then ``apply`` """
    def fn(s_arr, s_nd, s_tf, r_arr, r_nd, r_tf):
        s_mask = onp.mask_of(np.asarray(s_arr, np.float32), s_nd)
        if proc_crs == 'ref':
            src_ds = onp.reproject(s_arr, s_nd, onp.grid_mapping(_tf6(s_tf), _tf6(r_tf)), r_arr.shape, np.nan, 'average')
            params, _ = onp.fit('gain', src_ds, np.nan, r_arr, r_nd, (1, 1), False)
            up = onp.grid_mapping(_tf6(r_tf), _tf6(s_tf))
            params_us = np.stack([onp.reproject(p, np.nan, up, s_arr.shape, np.nan, 'nearest') for p in params[:2]])
        else:
            ref_us = onp.reproject(r_arr, r_nd, onp.grid_mapping(_tf6(r_tf), _tf6(s_tf)), s_arr.shape, np.nan, 'nearest')
            params, _ = onp.fit('gain', s_arr, s_nd, ref_us, np.nan, (1, 1), False)
            params_us = params.copy()
        params_us[:, ~s_mask] = np.nan
        params = params if proc_crs == 'ref' else params_us
        return onp.apply(s_arr, params_us), params
    return fn


# -- reference (B) ------------------------------------------------------------------------------------------------------------------
def _holes(shape):
    """ two holes: one pixel, and a square that swallows whole reference footprints (8 pixels a side; 3 in the small source) """
    h, w = shape
    n = 8 if h >= 60 else 3
    return (slice(h // 3, h // 3 + 1), slice(w // 4, w // 4 + 1)), (slice(h // 2, h // 2 + n), slice(w // 2 + 1, w // 2 + 1 + n))


@functools.lru_cache(maxsize=None)
def closed_form_pair(case_name: str, n_src: int = 1, n_ref: int = 1):
    """ -> (src (n_src, H, W) of ones with two NaN holes, ref (n_ref, h, w) of position codes, band b starting at b * h * w + 1),
    float32, read-only """
    case = CASES[case_name]
    src = np.ones((n_src, *case.src_shape), np.float32)
    for hole in _holes(case.src_shape):
        src[(slice(None), *hole)] = np.nan
    rh, rw = case.ref_shape
    ref = (np.arange(n_ref * rh * rw, dtype=np.float32).reshape(n_ref, rh, rw) + 1)
    assert ref.max() < 2 ** 24
    src.setflags(write=False)
    ref.setflags(write=False)
    return src, ref


@functools.lru_cache(maxsize=None)
def closed_form_expected(case_name: str, n_src: int = 1):
    """ -> (corrected (n_src, H, W), gain planes (n_src, h, w) on the processing grid), float32: reference (B) of the module
    docstring, band b against reference band b """
    case = CASES[case_name]
    src, ref = closed_form_pair(case_name, n_src, n_src)
    sg, rg = case.grids
    rows, cols = centre_indices(sg, rg, case_name)               # the reference pixel that holds each source centre
    assert rows.min() >= 0 and rows.max() < rg.height and cols.min() >= 0 and cols.max() < rg.width   # the reference covers the source
    corr = np.stack([ref[b][np.ix_(rows, cols)] for b in range(n_src)])
    corr[np.isnan(src)] = np.nan
    if case.proc_crs == 'src':
        gain = corr.copy()
    else:
        S, R = fr_grid(sg), fr_grid(rg)
        valid = ~np.isnan(src[0])
        r_rng = _footprint_ranges(R.height, R.y[1] / S.y[1], (R.y[0] - S.y[0]) / S.y[1], S.height)
        c_rng = _footprint_ranges(R.width, R.x[1] / S.x[1], (R.x[0] - S.x[0]) / S.x[1], S.width)
        gain = np.full((n_src, *case.ref_shape), np.nan, np.float32)
        for r, (a0, a1) in enumerate(r_rng):
            for c, (b0, b1) in enumerate(c_rng):
                if valid[a0:a1, b0:b1].any():
                    gain[:, r, c] = ref[:n_src, r, c]
    corr.setflags(write=False)
    gain.setflags(write=False)
    return corr, gain


CLOSED_FORM_CONFIG = {'ref': dict(upsampling=Resampling.nearest),
                      'src': dict(upsampling=Resampling.nearest, downsampling=Resampling.nearest)}


# -- RasterCompare ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compare_pair(case_name: str):
    """ -> (src (1, H, W), ref (1, h, w)) float32 of small integer codes with one NaN hole each, read-only """
    case = CASES[case_name]
    (sh, sw), (rh, rw) = case.src_shape, case.ref_shape
    y, x = np.mgrid[0:sh, 0:sw]
    r, c = np.mgrid[0:rh, 0:rw]
    src = ((7 * y + 3 * x) % 4001 + 1).astype(np.float32)[None]
    ref = ((5 * r + 11 * c) % 3989 + 1).astype(np.float32)[None]
    src[0, sh // 4:sh // 4 + 3, sw // 3:sw // 3 + 5] = np.nan
    ref[0, rh // 2:rh // 2 + 2, rw // 5:rw // 5 + 3] = np.nan
    src.setflags(write=False)
    ref.setflags(write=False)
    return src, ref


@functools.lru_cache(maxsize=None)
def compare_exact_sums(case_name: str, proc_crs: str):
    """ the seven sums of RasterCompare over the whole image in integer arithmetic, `nearest` both ways, as floats in the order of
    ``oracle_np.COMPARE_KEYS``: on the processing grid a pixel counts when it is valid and its centre falls in a valid pixel of the
    other raster """
    case = CASES[case_name]
    src, ref = compare_pair(case_name)
    sg, rg = case.grids
    dst, other, dst_grid, other_grid = (ref[0], src[0], rg, sg) if proc_crs == 'ref' else (src[0], ref[0], sg, rg)
    rows, cols = centre_indices(dst_grid, other_grid, f'{case_name} {proc_crs}')
    r_ok, c_ok = (rows >= 0) & (rows < other.shape[0]), (cols >= 0) & (cols < other.shape[1])
    picked = other[np.ix_(np.clip(rows, 0, other.shape[0] - 1), np.clip(cols, 0, other.shape[1] - 1))]
    ok = r_ok[:, None] & c_ok[None, :] & ~np.isnan(picked) & ~np.isnan(dst)
    d = [int(v) for v in dst[ok]]
    o = [int(v) for v in picked[ok]]
    s, r = (o, d) if proc_crs == 'ref' else (d, o)
    sums = (sum(s), sum(r), sum(v * v for v in s), sum(v * v for v in r), sum(a * b for a, b in zip(s, r)),
            sum((b - a) ** 2 for a, b in zip(s, r)), len(s))
    assert all(v < 2 ** 53 for v in sums) and max(max(s), max(r)) ** 2 < 2 ** 24 and len(s) > 100
    return dict(zip(onp.COMPARE_KEYS, (float(v) for v in sums)))


def band_stats(src_sum, ref_sum, src2_sum, ref2_sum, src_ref_sum, res2_sum, mask_sum) -> dict:
    """ r2, RMSE, rRMSE and N from the seven sums, float64 operation by operation as the reference's compare.py:145-163 """
    n = np.float64(mask_sum)
    src_mean, ref_mean = np.float64(src_sum) / n, np.float64(ref_sum) / n
    pcc_num = src_ref_sum - (n * src_mean * ref_mean)
    pcc_den = np.sqrt(src2_sum - (n * (src_mean ** 2))) * np.sqrt(ref2_sum - (n * (ref_mean ** 2)))
    rmse = np.sqrt(np.float64(res2_sum) / n)
    return dict(r2=float((pcc_num / pcc_den) ** 2), rmse=float(rmse), rrmse=float(rmse / ref_mean), n=int(mask_sum))


def f32_term_sums(src_arr: np.ndarray, src_nodata, ref_arr: np.ndarray, ref_nodata) -> np.ndarray:
    """ float64 sums of the float32 per-pixel terms of compare.py:243-255 over the jointly valid pixels of two arrays on one grid """
    s, r = np.asarray(src_arr, np.float32), np.asarray(ref_arr, np.float32)
    ok = onp.mask_of(s, src_nodata) & onp.mask_of(r, ref_nodata)
    s, r = s[ok], r[ok]
    terms = (s, r, s * s, r * r, s * r, (r - s) * (r - s))
    return np.array([t.astype(np.float64).sum() for t in terms] + [float(ok.sum())])


def compare_by_blocks(case_name: str, proc_crs: str, max_block_mem: float, reproject_fn, sums_fn):
    """ RasterCompare's sums of band 0 accumulated in block order from the helper's own windows: ``reproject_fn(array, nodata, its
    transform, target transform, target shape, down: bool) -> float32 array with NaN nodata`` brings the other raster's block onto
    the processing grid (`down`: onto coarser pixels), ``sums_fn(src, src_nodata, ref, ref_nodata) -> 7 sums`` """
    case = CASES[case_name]
    src, ref = compare_pair(case_name)
    acc = np.zeros(7)
    src_area, ref_area = case.src_res ** 2, case.ref_res[0] * case.ref_res[1]
    for bp in blocks_of(case, 1, (0, 0), max_block_mem, proc_crs):
        s_arr, s_nd = read_window(src[0], float('nan'), bp.src_in_block)
        r_arr, r_nd = read_window(ref[0], float('nan'), bp.ref_in_block)
        s_tf, r_tf = shifted(case.src_tf, bp.src_in_block), shifted(case.ref_tf, bp.ref_in_block)
        if proc_crs == 'ref':
            s_arr, s_nd = reproject_fn(s_arr, s_nd, s_tf, r_tf, r_arr.shape, src_area <= ref_area), float('nan')
        else:
            r_arr, r_nd = reproject_fn(r_arr, r_nd, r_tf, s_tf, s_arr.shape, ref_area <= src_area), float('nan')
        acc += np.asarray(sums_fn(s_arr, s_nd, r_arr, r_nd), np.float64)
    return dict(zip(onp.COMPARE_KEYS, (float(v) for v in acc)))


def oracle_nearest(arr, nodata, tf, dst_tf, dst_shape, down):
    return onp.reproject(np.asarray(arr, np.float32), nodata, onp.grid_mapping(_tf6(tf), _tf6(dst_tf)), dst_shape, np.nan, 'nearest')


# -- data for reference (A) -------------------------------------------------------------------------------------------------------
NODATA = {'nan': float('nan'), 'numeric': 0., 'none': None}


@functools.lru_cache(maxsize=None)
def kernel_pair(case_name: str, nodata_key: str, n_src: int = 1, n_ref: int = 1, typed: Optional[str] = None):
    """ -> (src (n_src, H, W), ref (n_ref, h, w)), read-only: positive data with a smooth gain / offset between paired bands, a stretch
    of reference columns that is noise (the fit cannot explain it: it fails the r2 mask, so gain-offset in-paints there) and, when
    the rasters have a nodata value, holes in both.  `typed`: None -- float32; 'uint16' -- both x 10 as uint16; 'uint8' -- both as
    uint8 (the reference scaled to fit) """
    case = CASES[case_name]
    (sh, sw), (rh, rw) = case.src_shape, case.ref_shape
    sg, rg = case.grids
    rows, cols = centre_indices(rg, sg, case_name)       # the source pixel under each reference centre
    si, sj = np.clip(rows, 0, sh - 1)[:, None], np.clip(cols, 0, sw - 1)[None, :]
    rng = np.random.default_rng(sum(map(ord, case_name)) + 7 * n_src)
    src = rng.uniform(50., 200., (n_src, sh, sw)).astype(np.float32)
    ref = np.empty((n_ref, rh, rw), np.float32)
    for b in range(n_ref):
        gain = 1.2 + 0.05 * b + 0.3 * np.sin(sj / 17.) * np.cos(si / 5.)
        ref[b] = (gain * src[b % n_src][si, sj] + 20. + 3. * b + rng.normal(0., 1., (rh, rw))).astype(np.float32)
        noise = slice(rw // 2 - max(rw // 10, 2), rw // 2 + max(rw // 10, 2))
        ref[b, :, noise] = rng.uniform(50., 250., ref[b, :, noise].shape).astype(np.float32)
    if typed == 'uint16':
        src, ref = np.round(src * 10).astype(np.uint16), np.round(ref * 10).astype(np.uint16)
    elif typed == 'uint8':
        src, ref = np.round(src).astype(np.uint8), np.clip(np.round(ref * 0.8), 1, 255).astype(np.uint8)
    nodata = NODATA[nodata_key]
    if nodata is not None:
        src[:, sh // 7:sh // 7 + 2, sw // 4:sw // 4 + 3] = nodata
        src[:, sh - 2, sw // 2] = nodata
        src[:, 0, 0] = nodata
        ref[:, rh // 3:rh // 3 + 3, rw // 4:rw // 4 + 4] = nodata
        ref[:, rh - 3, rw // 3] = nodata
    src.setflags(write=False)
    ref.setflags(write=False)
    return src, ref
