""" The predictor-3 images of tests/test_predictor3_cpu.py and tests/test_gpu_predictor3.py: the smallest layouts at which undoing the
floating-point predictor behind a block decoder can go wrong, filled with random BIT PATTERNS viewed as floats (NaN payloads,
infinities, -0.0 and denormals among them: the undo is byte arithmetic and has to keep every bit).  The blocks and the files are
built by tests/_lzw_streams.py, which shares no code with the package; every array and every list of streams is made once per
process and must be left unchanged. """
import functools
import zlib

import numpy as np

import _lzw_streams as st

# (dtype, spp, height, width, tile, rows_per_strip, separate, predictor)
LAYOUTS = (
    st.Layout('t16-f4', 'f4', 1, 37, 45, 16, 0, 0, 3),              # bw < 64; edge tiles with cols < bw in both directions
    st.Layout('t16-contig3-f4', 'f4', 3, 40, 41, 16, 0, 0, 3),      # the distance cspp = 3; the plane stride bw * cspp
    st.Layout('t48-sep-f8', 'f8', 2, 100, 70, 48, 0, 1, 3),         # es = 8; planes of blocks
    st.Layout('t80-f4', 'f4', 1, 90, 200, 80, 0, 0, 3),             # more than one 64-sample step with a carry; a ragged last step
    st.Layout('strips-short-f4', 'f4', 1, 50, 33, 0, 16, 0, 3),     # a short last strip
    st.Layout('strips-contig3-f8', 'f8', 3, 41, 29, 0, 7, 0, 3),    # es = 8 with cspp = 3
    st.Layout('strips-sep-f4-w1', 'f4', 2, 19, 1, 0, 5, 1, 3),      # a one-pixel row: the planes are one byte each
    st.Layout('strip-wide-f4', 'f4', 1, 3, 5000, 0, 2, 0, 3),       # a row far wider than a wave step: 20 000-byte rows
)
BY_NAME = {lay.name: lay for lay in LAYOUTS}


def random_bits(shape, dtype, seed):
    """ random bit patterns as little-endian floats of ``dtype`` ('f4' or 'f8') """
    rng = np.random.default_rng(seed)
    es = np.dtype(dtype).itemsize
    u = rng.integers(0, 2 ** (8 * es), shape, dtype=f'u{es}', endpoint=False)
    return u.astype(f'<u{es}').view(f'<f{es}')


@functools.lru_cache(maxsize=None)
def case(name):
    """ -> (layout, the (spp, height, width) array, the raw bytes of every block in TIFF order) """
    lay = BY_NAME[name]
    a = random_bits((lay.spp, lay.height, lay.width), lay.dtype, 1000 + LAYOUTS.index(lay))
    a.setflags(write=False)
    return lay, a, tuple(st.raw_blocks(a, lay))


@functools.lru_cache(maxsize=None)
def lzw_streams(name):
    return tuple(st.encode(b) for b in case(name)[2])


@functools.lru_cache(maxsize=None)
def deflate_streams(name):
    return tuple(zlib.compress(b) for b in case(name)[2])


def tiff_bytes(name, compression):
    """ the layout as a classic little-endian TIFF file: ``compression`` 5 (LZW) or 8 (DEFLATE) """
    lay, a, _ = case(name)
    return st.build_tiff(a, lay, compression=compression, streams=list(lzw_streams(name) if compression == 5 else deflate_streams(name)))


def block_geometry(lay):
    """ per block in TIFF order: (rows, cols) -- the rows its stream holds and the pixels of a row that lie inside the image """
    bw, bh = (lay.tile, lay.tile) if lay.tile else (lay.width, min(lay.rows_per_strip, lay.height))
    out = []
    for _ in range(lay.spp if lay.separate else 1):
        for y0 in range(0, lay.height, bh):
            for x0 in range(0, lay.width, bw):
                out.append((bh if lay.tile else min(bh, lay.height - y0), min(bw, lay.width - x0)))
    return out
