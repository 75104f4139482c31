""" The references of tests/_process_blocks.py, checked on the host before a GPU sees them: the window rule in rationals against
``fuse.block_pairs_multires`` (on the helper's geometries and on the dyadic cases of tests/golden/block_pairs_multires.json), reference
(B) and the RasterCompare closed form against the oracle's own per-block composition over the helper's reader and placement,
``RasterFuse._read_boundless`` against the helper's reader, and the pool of the block loop (``RasterFuse._run_blocks``) on a fake ``fn``. """
import json
import os
import warnings

import numpy as np
import pytest

import _process_blocks as pb
from conftest import GOLDEN_DIR, assert_same_f32
from homonim_amd import fuse
from homonim_amd.geo import Affine, Window
from oracle import oracle_np as onp


# -- the window rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('overlap', pb.OVERLAPS, ids=lambda o: f'ov{o[0]}x{o[1]}')
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_block_windows_follow_the_rule_in_rationals(case_name, overlap):
    case = pb.CASES[case_name]
    mem = pb.block_mem(case_name, overlap)
    bps = pb.blocks_of(case, 2, overlap, mem)
    sg, rg = case.grids
    n_rows, n_cols = pb.check_block_windows(sg, rg, case.proc_crs, 2, overlap, bps, src_once=True)
    assert n_rows >= 3 and n_cols >= 3
    # the overlap is real: some in-block is larger than its out-block on every side
    ins, outs = ('ref_in_block', 'ref_out_block') if case.proc_crs == 'ref' else ('src_in_block', 'src_out_block')
    assert any(getattr(bp, ins).height == getattr(bp, outs).height + 2 * overlap[0] and
               getattr(bp, ins).width == getattr(bp, outs).width + 2 * overlap[1] for bp in bps)


def test_some_geometry_reads_beyond_the_source_and_some_block_inside():
    """ the typed pairs of reference (A) need a case whose edge blocks are boundless and whose interior blocks are not """
    for name in ('2.5x-ref', '2.5x-src'):
        case = pb.CASES[name]
        bps = pb.blocks_of(case, 1, (3, 3), pb.block_mem(name, (3, 3)))
        h, w = case.src_shape
        inside = [0 <= bp.src_in_block.col_off and 0 <= bp.src_in_block.row_off and bp.src_in_block.col_off + bp.src_in_block.width <= w
                  and bp.src_in_block.row_off + bp.src_in_block.height <= h for bp in bps]
        assert any(inside) and not all(inside), name


def _dyadic_goldens():
    with open(os.path.join(GOLDEN_DIR, 'block_pairs_multires.json')) as f:
        cases = json.load(f)['cases']
    mk = lambda g: fuse.Grid(Affine(g['res'], 0., g['origin'][0], 0., -g['res'], g['origin'][1]), g['height'], g['width'])   # noqa: E731
    out = [(c, mk(c['src']), mk(c['ref'])) for c in cases]
    return [t for t in out if pb.is_dyadic_grid(t[1]) and pb.is_dyadic_grid(t[2])]


def test_the_goldens_hold_dyadic_cases():
    assert len(_dyadic_goldens()) >= 4


@pytest.mark.parametrize('case, src, ref', _dyadic_goldens(),
                         ids=lambda v: f"src{v['src']['res']}-ref{v['ref']['res']}-{v['proc_crs']}" if isinstance(v, dict) else '')
def test_dyadic_golden_partitions_follow_the_rule(case, src, ref):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bps = list(fuse.block_pairs_multires(src, ref, case['proc_crs'], case['n_bands'], case['overlap'], case['max_block_mem']))
    assert len(bps) == case['n_blocks']
    pb.check_block_windows(src, ref, case['proc_crs'], case['n_bands'], tuple(case['overlap']), bps, src_once=True)


def test_the_window_check_sees_a_shifted_block():
    """ the rational check is not vacuous: a block list with one window moved by a pixel fails it """
    case = pb.CASES['2.5x-ref']
    bps = pb.blocks_of(case, 1, (1, 1), pb.block_mem('2.5x-ref', (1, 1)))
    sg, rg = case.grids
    for field in ('src_in_block', 'src_out_block', 'ref_in_block', 'ref_out_block'):
        bad = list(bps)
        win = getattr(bad[5], field)
        bad[5] = bad[5]._replace(**{field: Window(win.col_off, win.row_off + 1, win.width, win.height)})
        with pytest.raises(AssertionError):
            pb.check_block_windows(sg, rg, 'ref', 1, (1, 1), bad)


def test_the_guard_refuses_a_centre_next_to_an_edge():
    from fractions import Fraction as Fr
    pb.centre_index(4, Fr(1, 3), Fr(1, 2))                       # centre 1 lies ON an edge: allowed
    with pytest.raises(AssertionError, match='mis-designed'):
        pb.centre_index(4, Fr(1, 3), Fr(1, 2) + Fr(1, 10 ** 10))


# -- reference (B) against the oracle's per-block composition ---------------------------------------------------------------------
@pytest.mark.parametrize('case_name, n_src, n_ref', [(n, 1, 1) for n in pb.CASES] + [('3x-ref', 2, 3), ('12-under-30-src', 2, 3)])
def test_closed_form_equals_the_oracle_composed_over_blocks(case_name, n_src, n_ref):
    case = pb.CASES[case_name]
    src, ref = pb.closed_form_pair(case_name, n_src, n_ref)
    exp_corr, exp_gain = pb.closed_form_expected(case_name, n_src)
    bps = pb.blocks_of(case, n_src, (1, 1), pb.block_mem(case_name, (1, 1)))
    assert len(bps) >= 9 * n_src
    corr, params = pb.expected_by_blocks(src, ref, float('nan'), float('nan'), case.src_tf, case.ref_tf, case.proc_crs, bps,
                                         pb.oracle_gain_block_fn(case.proc_crs), n_param=2)
    assert_same_f32(corr, exp_corr, f'{case_name} corrected')
    assert_same_f32(params[:n_src], exp_gain, f'{case_name} gains')
    assert_same_f32(params[n_src:], np.where(np.isnan(exp_gain), np.nan, 0).astype(np.float32), f'{case_name} offsets')
    # the case shows what it is meant to: holes in the corrected raster, codes from many reference pixels, and -- proc_crs=ref -- a
    # reference pixel inside the source whose whole footprint is a hole
    assert np.isnan(exp_corr[0]).sum() >= 10 and len(np.unique(exp_corr[~np.isnan(exp_corr)])) > 500 * n_src
    if case.proc_crs == 'ref':
        rows, cols = pb.centre_indices(case.grids[0], case.grids[1])
        inner = exp_gain[0][np.ix_(np.unique(rows), np.unique(cols))]
        assert np.isnan(inner).sum() >= 1 and np.isfinite(inner).sum() > 500


# -- the compare closed form against the oracle's per-block composition -------------------------------------------------------------
@pytest.mark.parametrize('at_least', [1, 4, 9])
@pytest.mark.parametrize('case_name, proc_crs', [('2.5x-ref', 'ref'), ('3x-ref', 'ref'), ('2x-aligned-ref', 'ref'),
                                                 ('x-only-ref', 'ref'), ('12-under-30-src', 'src'), ('2.5x-src', 'src')])
def test_compare_closed_form_equals_the_oracle_composed_over_blocks(case_name, proc_crs, at_least):
    mem = pb.compare_mem(case_name, proc_crs, at_least)
    n_blocks = len(pb.blocks_of(pb.CASES[case_name], 1, (0, 0), mem, proc_crs))
    assert n_blocks == 1 if at_least == 1 else n_blocks >= at_least
    exact = pb.compare_exact_sums(case_name, proc_crs)
    got = pb.compare_by_blocks(case_name, proc_crs, mem, pb.oracle_nearest, pb.f32_term_sums)
    assert got == exact
    # ... and the oracle's own statistics of those sums are the helper's
    stats = onp.compare_band_stats(**exact)
    assert {k: (int(v) if k == 'n' else float(v)) for k, v in stats.items()} == pb.band_stats(**exact)


# -- the boundless reader -----------------------------------------------------------------------------------------------------------
H, W = 6, 9
WINDOWS = {
    'inside': Window(2, 1, 4, 3), 'whole': Window(0, 0, W, H), 'left': Window(-2, 1, 5, 3), 'right': Window(6, 2, 5, 3),
    'top': Window(3, -3, 4, 5), 'bottom': Window(3, 4, 4, 5), 'top-left': Window(-1, -2, 4, 4), 'top-right': Window(7, -1, 4, 3),
    'bottom-left': Window(-3, 4, 5, 4), 'bottom-right': Window(7, 5, 3, 2), 'around': Window(-1, -1, W + 2, H + 2),
    'outside-left': Window(-5, 1, 4, 3), 'outside-below': Window(2, H, 3, 2), 'outside-corner': Window(W + 1, -4, 2, 3),
}
RASTERS = {
    'float32-nan': (np.float32, float('nan')), 'uint16-0': (np.uint16, 0), 'uint8-none': (np.uint8, None),
}


@pytest.mark.parametrize('raster', list(RASTERS))
@pytest.mark.parametrize('window', list(WINDOWS))
def test_read_boundless_against_the_helpers_reader(window, raster):
    dtype, nodata = RASTERS[raster]
    band = (np.arange(H * W).reshape(H, W) + 1).astype(dtype)
    win = WINDOWS[window]
    got, got_nd = fuse.RasterFuse._read_boundless(band, nodata, win)
    exp, exp_nd = pb.read_window(band, nodata, win)
    assert got.shape == (win.height, win.width) and got.dtype == exp.dtype
    assert np.array_equal(got, exp, equal_nan=got.dtype.kind == 'f')
    assert (got_nd is None and exp_nd is None) or (got_nd is not None and exp_nd is not None and
                                                   (got_nd == exp_nd or (got_nd != got_nd and exp_nd != exp_nd)))
    # ... and the helper's reader against the rule spelt out pixel by pixel
    inside = 0 <= win.col_off and 0 <= win.row_off and win.col_off + win.width <= W and win.row_off + win.height <= H
    nan_fill = nodata is None or nodata != nodata
    assert exp.dtype == (np.dtype(dtype) if inside or not nan_fill else np.float32)
    for r in range(win.height):
        for c in range(win.width):
            y, x = r + win.row_off, c + win.col_off
            if 0 <= y < H and 0 <= x < W:
                assert exp[r, c] == band[y, x]
            else:
                assert np.isnan(exp[r, c]) if nan_fill else exp[r, c] == nodata
    if inside:
        assert exp_nd is nodata or exp_nd == nodata or (exp_nd != exp_nd and nodata != nodata)
    else:
        assert (exp_nd != exp_nd) if nan_fill else exp_nd == nodata


# -- the pool ------------------------------------------------------------------------------------------------------------------------
class _FakeContext:
    device = 0      # (contexts on one device: no thread is bound to a NUMA node)


@pytest.mark.parametrize('threads', [1, 4])
def test_run_blocks_hands_the_results_back_in_block_order(threads):
    import threading
    third_done = threading.Event()

    def fn(bp, worker_i):
        if threads > 1 and bp == 0:      # with a pool the first block ends after the third: completion order is not block order
            assert third_done.wait(30), 'the pool does not run four blocks at a time'
        if bp == 2:
            third_done.set()
        return bp * 10, worker_i

    got = fuse.RasterFuse._run_blocks(list(range(8)), fn, [_FakeContext()], threads)
    assert got == [(bp * 10, 0) for bp in range(8)]


@pytest.mark.parametrize('threads', [1, 4])
def test_run_blocks_raises_what_a_worker_raised(threads):
    ran = []

    def fn(bp, worker_i):
        ran.append(bp)
        if bp == 2:                      # the third of eight
            raise KeyError('block 2')
        return bp

    with pytest.raises(KeyError, match='block 2'):
        fuse.RasterFuse._run_blocks(list(range(8)), fn, [_FakeContext()], threads)
    assert 2 in ran and (threads > 1 or ran == [0, 1, 2])


@pytest.mark.parametrize('threads', [1, 4])
def test_run_blocks_deals_the_blocks_round_robin_to_two_contexts(threads):
    got = fuse.RasterFuse._run_blocks(list(range(7)), lambda bp, worker_i: worker_i, [_FakeContext(), _FakeContext()], threads)
    assert got == [i % 2 for i in range(7)]
