"""
CPU test: the PACKED in-painting search of hk_inpaint.hip (fill_fast) as a numpy model against the oracle's restatement
of GDALFillNodata (oracle_np.fill_nodata; reference call site kernel_model.py:366).

The device search keeps 16-bit keys per quadrant -- (squared distance << 5) | column distance for the first candidate met at
the best distance, the complement of the column distance in the low bits for the last -- over row distances clipped at
FAST_CLIP, declares a quadrant SETTLED after step S when its best squared distance is below (S + 1)^2, and hands every
target with an unsettled quadrant after FAST_LAST to the general search.  The model (packed_fill in tests/_inpaint_masks.py)
restates exactly that (same constants, same order of the weighted sums); wherever it settles it must reproduce the oracle
bit for bit -- ties between columns at equal distance and GDAL's float comparison of them included -- and on dense source
masks it must settle nearly everywhere.  The constants are read from the kernel source so that the model cannot drift from
it.
"""
import numpy as np
import pytest

from _inpaint_masks import kernel_const, packed_fill
from oracle import oracle_np as onp

FAST_LAST, FAST_CLIP, MAX_DIST = kernel_const('FAST_LAST'), kernel_const('FAST_CLIP'), kernel_const('FILL_MAX_DIST')


def test_constants_of_the_packed_search():
    assert (FAST_CLIP + FAST_LAST ** 2) * 32 + 31 <= 0xffff          # a key fits its half
    assert FAST_CLIP > (FAST_LAST + 1) ** 2                           # a clipped candidate cannot settle a quadrant
    assert FAST_LAST <= 31 and FAST_LAST % 4 == 0 and MAX_DIST == 100  # the column distance fits five bits; groups of four


@pytest.mark.parametrize('h, w, density, seed', [(40, 70, 0.65, 1), (40, 70, 0.3, 2), (48, 64, 0.06, 3), (30, 90, 0.9, 4),
                                                 (64, 64, 0.02, 5)])
def test_packed_search_equals_the_restatement_where_it_settles(h, w, density, seed):
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 1, (h, w)).astype(np.float32)
    src = rng.uniform(size=(h, w)) < density
    exp = onp.fill_nodata(img, src)
    got, settled = packed_fill(img, src)
    assert (got[settled] == exp[settled]).all(), np.argwhere(settled & (got != exp))[:5]
    assert (got[src] == img[src]).all()
    inner = np.zeros((h, w), bool)
    inner[8:-8, 8:-8] = True
    if density >= 0.3:   # dense sources: everything away from the raster's edges settles
        assert settled[inner & ~src].all()
    assert settled.sum() > 0


def test_packed_search_ties_between_columns():
    """ sources placed so that several columns offer the same squared distance (5-12-13 and 3-4-5 triangles, diagonals): the tie
    rule of GDAL's float comparison decides which source's value is taken """
    h, w = 41, 61
    img = np.arange(h * w, dtype=np.float32).reshape(h, w)
    src = np.zeros((h, w), bool)
    cy, cx = 20, 30
    for dy, dx in ((3, 4), (4, 3), (5, 0), (0, 5), (5, 12), (12, 5), (13, 0), (1, 7), (7, 1), (5, 5), (2, 2), (2, 11), (10, 5), (11, 2)):
        for sy, sx in ((cy - dy, cx - dx), (cy - dy, cx + dx), (cy + dy, cx - dx), (cy + dy, cx + dx)):
            src[sy, sx] = True
    src[cy, cx] = False
    exp = onp.fill_nodata(img, src)
    got, settled = packed_fill(img, src)
    assert settled[cy, cx]
    assert (got[settled] == exp[settled]).all()
    assert settled.sum() > 300
