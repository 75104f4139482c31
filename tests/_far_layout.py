""" Layouts that put the bands, or the rows, of a device raster 2^32 + delta elements apart, inside one device arena, and the
arithmetic that checks the whole arena afterwards without moving it to the host (tests/test_gpu_far_planes.py; the arithmetic
itself is checked without a device in tests/test_far_layout_cpu.py).

The distance F = 2^32 + delta is chosen so that an offset narrowed anywhere on its way -- a term or the sum, to int32 or uint32
elements, or the byte offset to 32 bits -- is still a small non-negative number: the access lands delta-scale bytes into the arena,
on the canary or on another array, and shows as wrong bytes or a changed checksum, never as an access outside the allocation
(``narrowings`` lists those offsets; the CPU test asserts that every one of them lies inside the used part of the arena).

All arrays of a case share the layout: array k starts k * (delta // 8) elements behind the arena's base, its second band (or row)
F elements later, its third 2 F later.  Before a case the used part of the arena is set to the canary byte; ``ArenaModel`` keeps
what the host put there and what the case is expected to write, and gives the sum of the arena's 32-bit words modulo 2^64 that
``Context.checksum_dev`` must then return: no byte outside the expected pixels was written, and no input was changed. """
import numpy as np

GIB, MIB = 1 << 30, 1 << 20
ARENA_BYTES = 32 * GIB + 64 * MIB
DELTA_ALIGNED = 1 << 22          # every row and plane 16-byte aligned
DELTA_ODD = (1 << 22) + 3        # no far row or plane 16-byte aligned: the scalar paths
DELTAS = {'aligned': DELTA_ALIGNED, 'odd': DELTA_ODD}
CANARY = 0xC3
CANARY_WORD = 0xC3C3C3C3
ROW_WORDS = 65536                # the arena as rows of this many 32-bit words (checksum_dev takes int32 heights and widths)
ROW_BYTES = 4 * ROW_WORDS
MAX_ARRAYS = 8                   # slots of delta // 8 elements: all of them lie in front of the offset a narrowed F leaves
CHUNK = 4096                     # bytes per piece of the model


def far(delta):
    return (1 << 32) + delta


def slot(k, delta):
    """ element offset of array k of a case from the arena's base """
    assert 0 <= k < MAX_ARRAYS
    return k * (delta // 8)


class Layout:
    """ How the planes of every array of a case lie: 'compact' (the strides the caller gives), 'band' (bands F apart) or 'row'
    (one band, rows F apart).  ``delta`` also spaces the slots of the compact layout, so that the three agree on where array k
    starts. """

    def __init__(self, kind, delta=DELTA_ALIGNED):
        assert kind in ('compact', 'band', 'row')
        self.kind, self.delta = kind, delta

    def __repr__(self):
        return f'{self.kind}-{self.delta - DELTA_ALIGNED}'

    def strides(self, height, pitch, band_pad=0):
        """ -> (row stride, band stride) in elements of a raster of ``height`` rows whose compact row pitch is ``pitch`` """
        f = far(self.delta)
        if self.kind == 'band':
            return pitch, f
        if self.kind == 'row':
            return f, height * f
        return pitch, height * pitch + band_pad

    def extent(self, k, shape, pitch, band_pad=0):
        """ one element past the last one of array k of ``shape`` = (bands, height, width), from the arena's base """
        nb, h, w = shape
        stride, band_stride = self.strides(h, pitch, band_pad)
        assert self.kind != 'row' or nb == 1
        end = slot(k, self.delta) + (nb - 1) * band_stride + (h - 1) * stride + w
        if self.kind != 'row':   # every plane stays inside its slot
            assert (h - 1) * stride + w + (0 if self.kind == 'band' else (nb - 1) * band_stride) <= self.delta // 8, 'the array outgrows its slot'
        else:
            assert w <= self.delta // 8, 'the row outgrows its slot'
        return end


def used_bytes(end_bytes):
    """ the used part of the arena for arrays that end at ``end_bytes``: whole checksum rows """
    used = -(-end_bytes // ROW_BYTES) * ROW_BYTES
    assert used <= ARENA_BYTES, f'{used} bytes do not fit the arena'
    return used


def _narrow(v, how):
    if how == 'i32':
        v &= 0xffffffff
        return v - (1 << 32) if v >= (1 << 31) else v
    if how == 'u32':
        return v & 0xffffffff
    return v


def narrowings(base, band, band_stride, y, stride, x, itemsize):
    """ The byte offsets a kernel would reach for element ``base + band * band_stride + y * stride + x`` if it narrowed a product,
    the element sum or the byte offset to 32 bits, signed or unsigned: a set that holds the true byte offset as well. """
    out = set()
    hows = (None, 'i32', 'u32')
    for hb in hows:
        for hy in hows:
            for hs in hows:
                elems = _narrow(base + _narrow(band * band_stride, hb) + _narrow(y * stride, hy) + x, hs)
                for hbytes in hows:
                    out.add(_narrow(elems * itemsize, hbytes))
    return out


class ArenaModel:
    """ The bytes of the first ``used`` bytes of an arena that was set to the canary and then written at a few places, kept as
    the pieces that were written; ``checksum`` is the sum of its little-endian 32-bit words modulo 2^64. """

    def __init__(self, used, canary=CANARY):
        assert used % 4 == 0
        self.used, self.canary, self.chunks = used, canary, {}

    def write(self, offset, data):
        data = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8)
        assert 0 <= offset and offset + data.size <= self.used, 'a write outside the used part of the arena'
        pos = 0
        while pos < data.size:
            c, o = divmod(offset + pos, CHUNK)
            n = min(CHUNK - o, data.size - pos)
            if c not in self.chunks:
                self.chunks[c] = np.full(CHUNK, self.canary, np.uint8)
            self.chunks[c][o:o + n] = data[pos:pos + n]
            pos += n

    def read(self, offset, nbytes):
        out = np.full(nbytes, self.canary, np.uint8)
        pos = 0
        while pos < nbytes:
            c, o = divmod(offset + pos, CHUNK)
            n = min(CHUNK - o, nbytes - pos)
            if c in self.chunks:
                out[pos:pos + n] = self.chunks[c][o:o + n]
            pos += n
        return out

    def checksum(self):
        word = self.canary * 0x01010101
        held = 0   # words of the pieces inside the used part (the last piece may reach past it: what lies there was never written)
        total = 0
        for c, chunk in self.chunks.items():
            n = min(CHUNK, self.used - c * CHUNK) // 4
            held += n
            total += int(chunk[:4 * n].view('<u4').sum(dtype=np.uint64))
        return (total + (self.used // 4 - held) * word) % (1 << 64)


def row_runs(shape, itemsize, base, stride, band_stride):
    """ (byte offset, band, row) of every row of a raster, in order """
    nb, h, _ = shape
    return [((base + b * band_stride + y * stride) * itemsize, b, y) for b in range(nb) for y in range(h)]


class Arena:
    """ The device arena of a test module: one allocation, a canary fill and a model per case. """

    def __init__(self, ctx, nbytes=ARENA_BYTES):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx.dev_alloc(nbytes)
        self.model = None

    def free(self):
        if self.ptr:
            self.ctx.dev_free(self.ptr)
            self.ptr = None

    def begin(self, end_bytes):
        """ a new case whose arrays end ``end_bytes`` behind the base: canary over the used part, an empty model """
        used = used_bytes(end_bytes)
        assert used <= self.nbytes
        self.ctx.memset(self.ptr, CANARY, used)
        self.ctx.sync()   # (the fill is queued on the device's default stream: the uploads and the case's own streams do not wait for it)
        self.model = ArenaModel(used)
        return used

    def at(self, elem_offset, itemsize):
        return self.ptr + elem_offset * itemsize

    def _rows(self, arr, base, stride, band_stride):
        arr = np.asarray(arr)
        if arr.ndim == 2:
            arr = arr[None]
        return arr, row_runs(arr.shape, arr.dtype.itemsize, base, stride, band_stride)

    def put(self, arr, base, stride, band_stride=0):
        """ upload the rows of a (bands, h, w) or (h, w) array, and nothing between them; the rows must be the first thing put
        where they go (two arrays of a case that overlap are a mistake of the case) """
        arr, runs = self._rows(arr, base, stride, band_stride)
        for off, b, y in runs:
            row = np.ascontiguousarray(arr[b, y])
            assert (self.model.read(off, row.nbytes) == CANARY).all(), 'two arrays of the case overlap'
            self.ctx.h2d(self.ptr + off, row)
            self.model.write(off, row)

    def expect(self, arr, base, stride, band_stride=0):
        """ the rows the case is expected to write (the compact run's result): into the model only """
        arr, runs = self._rows(arr, base, stride, band_stride)
        for off, b, y in runs:
            self.model.write(off, np.ascontiguousarray(arr[b, y]))

    def get(self, shape, dtype, base, stride, band_stride=0):
        """ download the rows of a (bands, h, w) raster """
        out = np.empty(shape, dtype)
        for off, b, y in row_runs(shape, out.dtype.itemsize, base, stride, band_stride):
            row = np.empty(shape[2], dtype)
            self.ctx.d2h(row, self.ptr + off)
            out[b, y] = row
        return out

    def checksum(self):
        """ (the device's sum over the used part, the model's) """
        used = self.model.used
        return self.ctx.checksum_dev(self.ptr, ROW_WORDS, used // ROW_BYTES, ROW_WORDS), self.model.checksum()
