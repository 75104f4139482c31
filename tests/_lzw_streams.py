""" LZW streams for the tests of the LZW reader (tests/test_lzw_cpu.py, tests/test_gpu_lzw.py): what Pillow's libtiff cannot be asked
for -- tiles, separate planes, chosen encoder behaviour, malformed streams.  Everything is built to the statement of DESIGN.md 5.6
and shares no code with ``homonim_amd.tiff``: an encoder with switches, a code-level tracer (Clears, KwKwK codes, widths, uses of
strings whose last appearance lies far back), the malformed set, and whole TIFF files packed with ``struct``. """
import struct
import zlib
from collections import namedtuple

import numpy as np

OK, TRUNCATED, OLD_STYLE, BAD_FIRST, BAD_CODE, SHORT = range(6)
STATUS_NAMES = ('OK', 'TRUNCATED', 'OLD_STYLE', 'BAD_FIRST', 'BAD_CODE', 'SHORT')
CLEAR, EOI = 256, 257

Stream = namedtuple('Stream', 'name data raw status')


class _Bits:
    """ codes packed most significant bit first """

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, width):
        self.acc, self.n = (self.acc << width) | code, self.n + width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def pack(codes, width=9):
    """ codes of one width as a stream (for the malformed set) """
    b = _Bits()
    for c in codes:
        b.put(c, width)
    return b.done()


def encode(raw, clear_at=4094, eoi=True, lead_clear=True, double_clear=False):
    """ ``raw`` as one TIFF LZW stream.  ``clear_at``: a Clear is emitted once the encoder's next entry is this one (4094: as
    libtiff); None: never, the table fills up and stays.  ``eoi``: end with code 257.  ``lead_clear``: begin with a Clear.
    ``double_clear``: every Clear twice.  The width of every code is the one the DECODER of the statement has when it reads it
    (``dn`` is its next free entry). """
    bits, table = _Bits(), {}
    en, dn, w, first = 258, 258, 9, True

    def clear():
        nonlocal en, dn, w, first
        for _ in range(2 if double_clear else 1):
            bits.put(CLEAR, w)
            w = 9
        table.clear()
        en, dn, first = 258, 258, True

    def data(code):
        nonlocal dn, w, first
        bits.put(code, w)
        if first:
            first = False
        elif dn < 4096:
            dn += 1
            if dn == (1 << w) - 1 and w < 12:
                w += 1

    if lead_clear:
        clear()
    raw = bytes(raw)
    if raw:
        cur = raw[0]
        for k in raw[1:]:
            key = (cur << 8) | k
            code = table.get(key)
            if code is not None:
                cur = code
                continue
            data(cur)
            if en < 4096:
                table[key] = en
                en += 1
            cur = k
            if clear_at is not None and en >= clear_at:
                clear()
        data(cur)
    if eoi:
        bits.put(EOI, w)
    out = bits.done()
    if not lead_clear and len(out) >= 2 and out[0] == 0 and out[1] & 1:
        # (a byte 0 and then a code with bit 1 set look like the pre-6.0 bit order to every reader: such data needs its Clear)
        return encode(raw, clear_at, eoi, True, double_clear)
    return out


def trace(stream, raw_size, history=28672):
    """ The codes of a good stream, followed as the statement says without building a string: -> dict(codes, clears, kwkwk,
    max_width, max_len, far, cut), ``far`` counting the uses of a string (code >= 258, below n) whose last appearance -- its
    creation or its last use -- starts more than ``history`` bytes back, ``cut`` the bytes of the last string that did not fit. """
    data, pos, acc, nacc = bytes(stream), 0, 0, 0
    length, last_at = [1] * 258 + [0] * (4096 - 258), [0] * 4096
    n, w, prev, out = 258, 9, None, 0
    rec = dict(codes=0, clears=0, kwkwk=0, max_width=9, max_len=1, far=0, cut=0)
    while out < raw_size:
        while nacc < w:
            acc, pos, nacc = (acc << 8) | (data[pos] if pos < len(data) else 0), pos + 1, nacc + 8
        nacc -= w
        assert 8 * pos - nacc <= 8 * len(data), 'the stream ends too soon'
        c, acc = acc >> nacc, acc & ((1 << nacc) - 1)
        rec['codes'] += 1
        rec['max_width'] = max(rec['max_width'], w)
        if c == CLEAR:
            rec['clears'] += 1
            n, w, prev = 258, 9, None
            continue
        assert c != EOI
        if prev is None:
            assert c < 256
            ln = 1
        else:
            assert c <= n
            if c == n:
                rec['kwkwk'] += 1
                ln = length[prev] + 1
            else:
                ln = length[c]
                if c >= 258 and out - last_at[c] > history:
                    rec['far'] += 1
            if n < 4096:
                length[n], last_at[n] = length[prev] + 1, prev_at
                n += 1
                if n == (1 << w) - 1 and w < 12:
                    w += 1
        if c >= 258:
            last_at[c] = out
        rec['max_len'] = max(rec['max_len'], ln)
        prev, prev_at, out = c, out, out + ln
    rec['cut'] = out - raw_size
    return rec


SWITCHES = (dict(), dict(clear_at=None), dict(eoi=False), dict(lead_clear=False), dict(double_clear=True),
            dict(clear_at=None, eoi=False, lead_clear=False), dict(clear_at=600, double_clear=True, eoi=False))
# The switches whose streams libtiff reads too.  It refuses a stream that goes on behind a full table, and one without a Clear at
# its start it reads differently (its first code adds an entry there): those two tolerances are the statement's own.
LIBTIFF_SWITCHES = tuple(kw for kw in SWITCHES if kw.get('lead_clear', True) and kw.get('clear_at', 4094) is not None)


def _chunks():
    """ (name, bytes): what the good streams hold """
    rng = np.random.default_rng(2025)
    y, x = np.mgrid[0:96, 0:96]
    smooth = ((np.sin(x / 9.0) + np.cos(y / 7.0)) * 40 + 128).astype(np.uint8)
    return [
        ('noise-96x96', rng.integers(0, 256, 96 * 96, dtype=np.uint8).tobytes()),          # widths 9..12 and a Clear
        ('smooth-96x96', smooth.tobytes()),
        ('flat-128x128', bytes([7]) * (128 * 128)),                                          # strings far longer than a wave
        ('flat-odd-10007', bytes([200]) * 10007),                                            # no multiple of 16, the last string cut
        ('runs', b''.join(bytes([int(v)]) * int(k) for v, k in zip(rng.integers(0, 4, 400), rng.integers(1, 90, 400)))),
        ('u16-ramp', (np.arange(5000) * 3 % 65536).astype('<u2').tobytes()),
        ('one-byte', b'\x42'),
        ('two-bytes', b'\x00\x01'),
        ('seventeen', bytes(range(17))),
    ]


def good_set():
    """ every chunk under every set of encoder switches; and two whose streams hold more than the block, so that the last string
    is cut: a long one of a constant block with an odd size, a short one of a smooth block """
    out = [Stream(f'{name}:{i}', encode(raw, **kw), raw, OK) for name, raw in _chunks() for i, kw in enumerate(SWITCHES)]
    smooth = dict(_chunks())['smooth-96x96']
    for i, kw in enumerate(SWITCHES):
        out.append(Stream(f'flat-cut-9875:{i}', encode(bytes([200]) * 10100, **kw), bytes([200]) * 9875, OK))   # (5 of a string of 141)
        out.append(Stream(f'smooth-cut-9001:{i}', encode(smooth, **kw), smooth[:9001], OK))
    return out


def malformed_set():
    """ one stream per status, each between good blocks (the good ones first and last) """
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    good = encode(noise)
    flat = bytes([9]) * 3000
    return [
        Stream('good-noise', good, noise, OK),
        Stream('cut-mid-code', good[:len(good) // 2], noise, TRUNCATED),
        Stream('good-flat', encode(flat), flat, OK),
        Stream('empty', b'', noise, TRUNCATED),
        Stream('old-style', b'\x00\x01' + good[2:], noise, OLD_STYLE),
        Stream('good-no-eoi', encode(noise, eoi=False), noise, OK),
        Stream('300-behind-clear', pack([CLEAR, 300, 65, 66, EOI]), bytes(3000), BAD_FIRST),
        Stream('code-n-plus-1', pack([CLEAR, 65, 66, 260, 65, EOI]), bytes(3000), BAD_CODE),
        Stream('early-eoi', pack([CLEAR, 65, 66, EOI]), bytes(3000), SHORT),
        Stream('good-last', encode(noise, lead_clear=False), noise, OK),
    ]


def sweep_set(count=2048, seed=11, pad_to=None):
    """ small blocks of 1..600 raw bytes, all encoder switches in turn, four kinds of content.  ``pad_to``: every block filled up
    with zeros to this many bytes -- the blocks of ONE image have one size, so this is how they share a call. """
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        size, kind = int(rng.integers(1, 601)), i % 4
        if kind == 0:
            raw = rng.integers(0, 256, size, dtype=np.uint8)
        elif kind == 1:
            raw = rng.integers(0, 3, size, dtype=np.uint8)
        elif kind == 2:
            raw = np.full(size, rng.integers(0, 256), np.uint8)
        else:
            raw = np.repeat(rng.integers(0, 256, size // 5 + 1, dtype=np.uint8), 5)[:size]
        raw = raw.tobytes() + bytes(0 if pad_to is None else pad_to - size)
        out.append(Stream(f'sweep{i}', encode(raw, **SWITCHES[i % len(SWITCHES)]), raw, OK))
    return out


def chain_walk_tile(history=28672):
    """ One 512 x 512 uint8 tile whose last rows repeat row patterns of its first KiB behind long constant stretches: strings made
    early are used again when their last appearance has long left any ring's history.  -> (raw bytes, stream, trace record) """
    rng = np.random.default_rng(99)
    a = np.full((512, 512), 17, np.uint8)
    first = rng.integers(0, 256, (2, 512), dtype=np.uint8)
    a[0:2] = first
    a[200] = 90                       # (another constant: the table keeps filling slowly, no Clear comes)
    a[508:510] = first
    a[510:512, :256] = first[:, 256:]
    raw = a.tobytes()
    data = encode(raw)
    return raw, data, trace(data, len(raw), history)


# ---- layouts and whole files --------------------------------------------------------------------------------------------------
Layout = namedtuple('Layout', 'name dtype spp height width tile rows_per_strip separate predictor')
LAYOUTS = (
    Layout('tiles16-u8', 'u1', 1, 37, 45, 16, 0, 0, 1),
    Layout('tiles48-separate-u16-pred2', 'u2', 2, 100, 70, 48, 0, 1, 2),
    Layout('tiles512-u8', 'u1', 1, 520, 515, 512, 0, 0, 1),
    Layout('tiles16-contig3-u16', 'u2', 3, 40, 41, 16, 0, 0, 1),
    Layout('tiles48-contig3-u8-pred2', 'u1', 3, 50, 97, 48, 0, 0, 2),
    Layout('strips-short-u32-pred2', 'u4', 1, 50, 33, 0, 16, 0, 2),
    Layout('strips-contig3-u8', 'u1', 3, 41, 29, 0, 7, 0, 1),
    Layout('strips-separate-u64', 'u8', 2, 19, 21, 0, 5, 1, 1),
    Layout('tiles16-separate-u32', 'u4', 2, 33, 31, 16, 0, 1, 1),
)


def layout_array(lay):
    """ the (spp, height, width) pixels of a layout: smooth with noise in the low bits, so that the streams have long and short
    strings """
    rng = np.random.default_rng(len(lay.name) * 1000 + lay.height)
    y, x = np.mgrid[0:lay.height, 0:lay.width]
    dt = np.dtype('<' + lay.dtype)
    bands = [((x // 5 + y // 3 + 11 * b) * (1 if dt.itemsize == 1 else 257) + rng.integers(0, 2, x.shape)) for b in range(lay.spp)]
    return np.stack(bands).astype(np.uint64).astype(dt)


def block_layout(lay):
    """ the nine fields of tiff.BlockLayout / hk_inflate_layout as a plain tuple """
    bw, bh = (lay.tile, lay.tile) if lay.tile else (lay.width, min(lay.rows_per_strip, lay.height))
    return (np.dtype(lay.dtype).itemsize, lay.spp, lay.height, lay.width, bw, bh, int(bool(lay.tile)), lay.separate, lay.predictor)


def _float_predict(rows):
    """ libtiff's floating-point predictor on (rows, pixels, cspp) little-endian floats -> (rows, bytes) """
    r, n, cspp = rows.shape
    es = rows.dtype.itemsize
    be = rows.astype(rows.dtype.newbyteorder('>')).view(np.uint8).reshape(r, n * cspp, es)
    planes = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(r, es * n * cspp)
    d = planes.copy()
    d[:, cspp:] = planes[:, cspp:] - planes[:, :-cspp]
    return d


def raw_blocks(array, lay, byteorder='<'):
    """ the raw bytes of every block of ``array`` (spp, height, width) in TIFF order: tiles padded with zeros, the last strip
    short, the predictor applied """
    spp, h, w = array.shape
    bw, bh = (lay.tile, lay.tile) if lay.tile else (w, min(lay.rows_per_strip, h))
    planes = [array[p:p + 1] for p in range(spp)] if lay.separate else [array]
    out = []
    for pl in planes:
        for y0 in range(0, h, bh):
            for x0 in range(0, w, bw):
                rows = bh if lay.tile else min(bh, h - y0)
                blk = np.zeros((rows, bw, pl.shape[0]), array.dtype)
                part = pl[:, y0:y0 + rows, x0:x0 + bw]
                blk[:part.shape[1], :part.shape[2]] = np.moveaxis(part, 0, 2)
                if lay.predictor == 2:
                    d = blk.copy()
                    d[:, 1:] = blk[:, 1:] - blk[:, :-1]
                    blk = d
                if lay.predictor == 3:
                    out.append(_float_predict(blk).tobytes())
                else:
                    out.append(blk.astype(blk.dtype.newbyteorder(byteorder)).tobytes())
    return out


def layout_streams(lay, switches=SWITCHES):
    """ -> (array, [stream per block]) of a layout; block k is encoded under ``switches[k mod len(switches)]`` """
    a = layout_array(lay)
    blocks = raw_blocks(a, lay)
    return a, [encode(b, **switches[k % len(switches)]) for k, b in enumerate(blocks)]


def build_tiff(array, lay, byteorder='<', compression=5, streams=None):
    """ A classic TIFF file of ``array`` laid out as ``lay`` with every block an LZW stream (or ``streams``), packed here with
    ``struct``: no code of the package under test is involved. """
    spp, h, w = array.shape
    dt = array.dtype
    if streams is None:
        streams = [encode(b) for b in raw_blocks(array, lay, byteorder)]
    bo = byteorder
    fmt = {'u': 1, 'i': 2, 'f': 3}[dt.kind]
    entries = [(256, 4, [w]), (257, 4, [h]), (258, 3, [8 * dt.itemsize] * spp), (259, 3, [compression]),
               (262, 3, [2 if spp == 3 and not lay.separate and dt.itemsize == 1 else 1]), (277, 3, [spp]),
               (284, 3, [2 if lay.separate else 1]), (339, 3, [fmt] * spp)]
    if spp > 1 and not (spp == 3 and not lay.separate and dt.itemsize == 1):
        entries.append((338, 3, [0] * (spp - 1)))
    if lay.predictor != 1:
        entries.append((317, 3, [lay.predictor]))
    if lay.tile:
        entries += [(322, 3, [lay.tile]), (323, 3, [lay.tile])]
        t_off, t_cnt = 324, 325
    else:
        entries.append((278, 3, [min(lay.rows_per_strip, h)]))
        t_off, t_cnt = 273, 279
    data_at = 8
    offsets, at = [], data_at
    for s in streams:
        offsets.append(at)
        at += len(s) + (len(s) & 1)
    entries += [(t_off, 4, offsets), (t_cnt, 4, [len(s) for s in streams])]
    entries.sort()
    ifd_at = at
    extra_at = ifd_at + 2 + 12 * len(entries) + 4
    ifd, extra = struct.pack(bo + 'H', len(entries)), b''
    for tag, typ, vals in entries:
        code = {3: 'H', 4: 'I'}[typ]
        payload = struct.pack(bo + code * len(vals), *vals)
        if len(payload) <= 4:
            field = payload.ljust(4, b'\0')
        else:
            field = struct.pack(bo + 'I', extra_at + len(extra))
            extra += payload + (b'\0' if len(payload) & 1 else b'')
        ifd += struct.pack(bo + 'HHI', tag, typ, len(vals)) + field
    ifd += struct.pack(bo + 'I', 0)
    body = b''.join(s + (b'\0' if len(s) & 1 else b'') for s in streams)
    return (b'II' if bo == '<' else b'MM') + struct.pack(bo + 'HI', 42, ifd_at) + body + ifd + extra


def lzw_copy(data, mapper=map):
    """ A classic little-endian TIFF with DEFLATE blocks (as ``write_tiff`` makes them) -> the same file with every block of every
    image re-coded as LZW: the directories are patched in place (compression, block offsets, byte counts), the new streams are
    appended; geo-referencing, nodata, metadata and predictor stay what they were.  ``mapper``: what applies ``encode`` to the raw
    blocks of an image (a process pool's ``map`` for large files). """
    buf = bytearray(data)
    assert buf[:4] == b'II*\0'
    (ifd,) = struct.unpack_from('<I', buf, 4)
    while ifd:
        (n,) = struct.unpack_from('<H', buf, ifd)
        ent = {struct.unpack_from('<H', buf, ifd + 2 + 12 * i)[0]: ifd + 2 + 12 * i for i in range(n)}

        def values(tag):
            at = ent[tag]
            _, typ, cnt = struct.unpack_from('<HHI', buf, at)
            code = {3: 'H', 4: 'I'}[typ]
            pos = at + 8 if cnt * struct.calcsize(code) <= 4 else struct.unpack_from('<I', buf, at + 8)[0]
            return pos, '<' + code * cnt, list(struct.unpack_from('<' + code * cnt, buf, pos))

        pos, fmt, comp = values(259)
        assert comp[0] in (8, 32946)
        struct.pack_into(fmt, buf, pos, 5)
        o_pos, o_fmt, offs = values(324 if 324 in ent else 273)
        c_pos, c_fmt, cnts = values(325 if 324 in ent else 279)
        streams = list(mapper(encode, [zlib.decompress(bytes(buf[o:o + c])) for o, c in zip(offs, cnts)]))
        for k, stream in enumerate(streams):
            if len(buf) & 1:
                buf.append(0)
            offs[k], cnts[k] = len(buf), len(stream)
            buf += stream
        struct.pack_into(o_fmt, buf, o_pos, *offs)
        struct.pack_into(c_fmt, buf, c_pos, *cnts)
        (ifd,) = struct.unpack_from('<I', buf, ifd + 2 + 12 * n)
    return bytes(buf)
