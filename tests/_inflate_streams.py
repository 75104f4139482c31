""" The zlib streams the inflate tests share (tests/test_inflate_cpu.py: the decoder core compiled for the host;
tests/test_gpu_inflate.py: the kernel).  Four sets, each built once:

a. what zlib writes in its modes -- levels 0, 1, 6, 9, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, a stream cut by a sync and a full flush --
   over the chosen content of tests/test_gpu_deflate.py (128 x 128 uint8 and float32) and its strict Fibonacci chunk, whose
   Z_HUFFMAN_ONLY stream has 15-bit codes;
b. hand-built streams: stored blocks of P random bytes, then one fixed-Huffman block with matches at distance 32768 (zlib itself
   never goes above 32506), overlapping copies and the longest length, for P that put them at different phases of a 64 KiB ring;
c. malformed streams derived from (b), each with the status the decoder has to give and zlib's own refusal;
d. a seeded sweep of 4096 blocks of 256 bytes.

A stream is a ``Stream(name, data, raw, status)``: ``raw`` are the bytes it has to inflate to -- for a malformed one the bytes of
the good stream it was derived from: their number is the block size the decoder is given -- and ``status`` the decoder's status
(an ``INFLATE_*`` of homonim_amd/_hk.py). """
import functools
import zlib
from typing import NamedTuple

import numpy as np

from test_gpu_deflate import CONTENTS, _content, _strict_fibonacci_chunk, _sweep_tile

OK, TRUNCATED, BAD_HEADER, BAD_BLOCK, BAD_STORED, BAD_CODE, BAD_SYMBOL, FAR, OVERRUN, SHORT, ADLER = range(11)


class Stream(NamedTuple):
    name: str
    data: bytes
    raw: bytes
    status: int


def _with(strategy):
    def f(raw):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
        return c.compress(raw) + c.flush()
    return f


def _flushed(raw):
    c = zlib.compressobj(6)
    a, b = len(raw) // 3, 2 * len(raw) // 3
    return (c.compress(raw[:a]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[a:b]) + c.flush(zlib.Z_FULL_FLUSH)
            + c.compress(raw[b:]) + c.flush())


MODES = {'level0': lambda r: zlib.compress(r, 0), 'level1': lambda r: zlib.compress(r, 1), 'level6': lambda r: zlib.compress(r, 6),
         'level9': lambda r: zlib.compress(r, 9), 'fixed': _with(zlib.Z_FIXED), 'huffman': _with(zlib.Z_HUFFMAN_ONLY),
         'rle': _with(zlib.Z_RLE), 'flushed': _flushed}


def block_types(stream):
    """ the BTYPE of a stream's first block """
    return (stream[2] >> 1) & 3


def max_code_length(stream):
    """ the longest literal/length code of the FIRST block of a stream, which has to be a dynamic one: its header decoded """
    bits = int.from_bytes(stream[2:], 'little')
    pos = 0

    def take(n):
        nonlocal pos
        v = (bits >> pos) & ((1 << n) - 1)
        pos += n
        return v

    take(1)
    assert take(2) == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = take(3)
    # canonical code of the code-length code, as {(length, code): symbol}
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, ln = 0, 0
        while (ln, c) not in codes:
            c, ln = (c << 1) | take(1), ln + 1
        s = codes[(ln, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    return max(lens[:hlit])


@functools.lru_cache(None)
def set_a():
    contents = [(f'{kind}-{dtype}', _content(kind, 128 * 128 * np.dtype(dtype).itemsize).tobytes())
                for kind in CONTENTS for dtype in ('uint8', 'float32')]
    contents.append(('strict-fibonacci', _strict_fibonacci_chunk(3).tobytes()))
    out = []
    for cname, raw in contents:
        for mode, f in MODES.items():
            out.append(Stream(f'{mode}:{cname}', f(raw), raw, OK))
    return out


# ---- (b) -------------------------------------------------------------------------------------------------------------
class BitWriter:
    """ bits LSB first, as DEFLATE packs them; Huffman codes go in from their most significant bit """
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, count):
        self.acc |= value << self.n
        self.n += count

    def code(self, value, count):
        for i in range(count - 1, -1, -1):
            self.bits((value >> i) & 1, 1)

    def align(self):
        self.n = -(-self.n // 8) * 8

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), 'little')


def _fixed_ll(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def _length_symbol(length):
    if length == 258:
        return 285, 0, 0
    for c in range(28):
        extra = 0 if c < 8 else (c >> 2) - 1
        base = 3 + c if c < 8 else 3 + ((4 + (c & 3)) << extra)
        if base <= length < base + (1 << extra):
            return 257 + c, extra, length - base
    raise ValueError(length)


def _distance_symbol(dist):
    for d in range(30):
        extra = 0 if d < 4 else (d >> 1) - 1
        base = 1 + d if d < 4 else 1 + ((2 + (d & 1)) << extra)
        if base <= dist < base + (1 << extra):
            return d, extra, dist - base
    raise ValueError(dist)


TOKENS = (('match', 258, 32768), ('match', 3, 1), ('lit', 0x5A), ('match', 258, 1), ('match', 10, 32768), ('match', 7, 3), ('end',))


def hand_built(p, tokens=TOKENS, btype=1, header=b'\x78\x9c', seed=0):
    """ -> (stream, raw bytes): stored blocks of ``p`` random bytes, then one final block of type ``btype`` with the fixed code's
    ``tokens``: ('lit', byte), ('match', length, distance), ('end',), ('ll', symbol) / ('dist', symbol): a bare symbol """
    prefix = np.random.default_rng(7000 + p + seed).integers(0, 256, p, dtype=np.uint8).tobytes()
    w = BitWriter()
    parts = [header]
    for o in range(0, p, 65535):
        n = min(65535, p - o)
        parts.append(bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + prefix[o:o + n])
    w.bits(1, 1), w.bits(btype, 2)
    raw = bytearray(prefix)
    for t in tokens:
        if t[0] == 'lit':
            _fixed_ll(w, t[1])
            raw.append(t[1])
        elif t[0] == 'match':
            sym, extra, value = _length_symbol(t[1])
            _fixed_ll(w, sym), w.bits(value, extra)
            sym, extra, value = _distance_symbol(t[2])
            w.code(sym, 5), w.bits(value, extra)
            for _ in range(t[1]):
                raw.append(raw[-t[2]] if t[2] <= len(raw) else 0)
        elif t[0] == 'll':
            _fixed_ll(w, t[1])
        elif t[0] == 'dist':
            w.code(t[1], 5)
        else:
            _fixed_ll(w, 256)
    parts.append(w.bytes())
    raw = bytes(raw)
    parts.append(zlib.adler32(raw).to_bytes(4, 'big'))
    return b''.join(parts), raw


PREFIXES = (32768, 65535, 65536, 65537, 98321)


@functools.lru_cache(None)
def set_b():
    out = []
    for p in PREFIXES:
        data, raw = hand_built(p)
        assert zlib.decompress(data) == raw and len(raw) == p + 258 + 3 + 1 + 258 + 10 + 7
        out.append(Stream(f'hand-built:{p}', data, raw, OK))
    return out


# ---- (c) -------------------------------------------------------------------------------------------------------------
def _dynamic(cl_lengths, symbols):
    """ a final dynamic block's header with HLIT = 257, HDIST = 1: ``cl_lengths`` in the header's order, then ``symbols``:
    (code, code length, extra value, extra bits) of the code-length code, as they come """
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(len(cl_lengths) - 4, 4)
    for v in cl_lengths:
        w.bits(v, 3)
    for code, n, value, extra in symbols:
        w.code(code, n), w.bits(value, extra)
    w.bits(0, 64)   # (whatever comes next is there)
    return b'\x78\x9c' + w.bytes()


def zlib_refusal(data):
    """ what zlib says to a stream: its error's text, 'eof False' for a stream that merely ends too soon, '' for one it accepts """
    d = zlib.decompressobj()
    try:
        d.decompress(data)
    except zlib.error as e:
        return str(e)
    return '' if d.eof else 'eof False'


@functools.lru_cache(None)
def set_c(p=32768):
    good, raw = hand_built(p)
    fixed_at = 2 + 5 * -(-p // 65535) + p    # the fixed block's first byte
    flip = lambda s, at, mask: s[:at] + bytes([s[at] ^ mask]) + s[at + 1:]
    out = [
        Stream('truncated', good[:-20], raw, TRUNCATED),
        Stream('adler', flip(good, len(good) - 1, 0xFF), raw, ADLER),
        Stream('block-type-3', flip(good, fixed_at, 0x04), raw, BAD_BLOCK),
        Stream('nlen', flip(good, 5, 0x10), raw, BAD_STORED),
        Stream('header', b'\x78\x9d' + good[2:], raw, BAD_HEADER),
        Stream('distance-30', hand_built(p, TOKENS[:1] + (('ll', 257), ('dist', 30)) + TOKENS[1:])[0], raw, BAD_SYMBOL),
        Stream('length-286', hand_built(p, TOKENS[:1] + (('ll', 286),) + TOKENS[1:])[0], raw, BAD_SYMBOL),
        Stream('match-first', hand_built(0, (('match', 3, 1), ('end',)))[0], raw, FAR),
        # three codes of one bit (16, 17, 18)
        Stream('over-subscribed', _dynamic([1, 1, 1, 0], []), raw, BAD_CODE),
        # the code-length code: 1 -> '0', 18 -> '1'; lengths 1 1, 255 zeros (138 + 117) up to and including symbol 256, distance 1
        Stream('no-end-of-block', _dynamic([0, 0, 1] + [0] * 14 + [1], [(0, 1, 0, 0), (0, 1, 0, 0), (1, 1, 127, 7), (1, 1, 106, 7),
                                                                         (0, 1, 0, 0)]), raw, BAD_CODE),
        # the code-length code: 16 -> '0', 17 -> '1'; the first length is a repeat of the one before
        Stream('repeat-first', _dynamic([1, 1, 0, 0], [(0, 1, 0, 2)]), raw, BAD_CODE),
        Stream('more', hand_built(p, TOKENS[:-1] + (('lit', 1), ('end',)))[0], raw, OVERRUN),
        Stream('fewer', hand_built(p, TOKENS[:-2] + (('end',),))[0], raw, SHORT),
        Stream('empty', b'', raw, TRUNCATED),
        Stream('trailing-garbage', good + b'\xde\xad', raw, OK),
    ]
    return out


# what zlib answers to the malformed streams whose refusal is a matter of the format (not of the block size, which zlib does not know)
ZLIB_SAYS = {'truncated': 'eof False', 'adler': 'incorrect data check', 'block-type-3': 'invalid block type',
             'nlen': 'invalid stored block lengths', 'header': 'incorrect header check', 'distance-30': 'invalid distance code',
             'length-286': 'invalid literal/length code', 'match-first': 'invalid distance too far back',
             'over-subscribed': 'invalid code lengths set', 'no-end-of-block': 'missing end-of-block',
             'repeat-first': 'invalid bit length repeat', 'empty': 'eof False', 'trailing-garbage': ''}


# ---- (d) -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def set_d():
    modes = (MODES['level0'], MODES['level1'], MODES['level6'], MODES['level9'], MODES['fixed'])
    out = []
    for i in range(4096):
        raw = _sweep_tile(i).tobytes()
        out.append(Stream(f'sweep:{i}', modes[i % 5](raw), raw, OK))
    return out
