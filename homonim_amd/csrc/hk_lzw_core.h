// hk_lzw_core.h -- the TIFF LZW decoder of hk_lzw.hip as functions over ONE WAVE's shared state: one wave of 64 lanes decodes one
// stream (a tile or a strip of a GeoTIFF, compression 5).  A host program compiles the same functions as plain C++ (HKI_HOST, as
// hk_inflate_core.h, whose lane loop, 16-byte loads and stores and pointer types are used here): tests/c/lzw_core_host.cpp, and
// the library's own host decoder hk_lzw_image_host.
//
// THE STREAM.  Codes of 9 to 12 bits, most significant bit first.  0..255 bytes, 256 Clear, 257 end of information,
// entries from 258.  The state at the start is the state after a Clear: n = 258, width 9, no previous code.  A code c with a
// previous code p: c < n its string, c == n string(p) + first byte of string(p), c > n refused; then entry n = string(p) + first
// byte of string(c), n += 1, and the width grows once n == 2^width - 1 (libtiff's early change), up to 12.  At n == 4096 nothing
// is added any more.  The first code after a Clear is a byte and adds nothing; Clears behind a Clear are skipped.  Decoding ends
// when the block's raw size is there (a last string is cut; nothing behind it is looked at).
//
// WHAT IS UNIFORM.  The bit buffer, n, the width, the previous code, the positions and the status are the same in all lanes
// (`uni()`: scalar registers); lanes differ only where bytes move: the input window, a string's copy, the flush.
//
// MEMORY SAFETY.
//   * every table index is a code that was checked against n before use: the code just read (c <= n, and c == n never reads the
//     table), and the prefix of an entry, which was such a code when the entry was made and is smaller than the entry's index;
//     entries below n were all written since the last Clear.
//   * nothing is written past the raw size: a string is cut to raw - out before a byte of it moves, and the flush stores whole
//     16-byte groups into a slot of the raw size rounded up to 16.
//   * nothing is read outside the stream: aligned 16-byte groups wholly inside [in, in + size) are loaded as such, any other byte
//     by byte under bounds; bits past the end read as zero, and a code that takes a bit past 8 * size sets TRUNCATED before its
//     value is used.
//   * the ring: a string is copied from its last appearance only while that lies at most HISTORY = RING - 4096 bytes back, so the
//     at most 3839 bytes written by the step cannot land on what it reads; the unflushed part is at most FLUSH_AT + 15 + 3839
//     bytes, far below RING.  Global memory the kernel has written is never loaded.
//
// TERMINATION.  Every step of the loop takes `width` >= 9 bits of input or ends the block, `used` never decreases and a step that
// leaves used > 8 * size ends the block: at most 8 * size / 9 + 1 steps.  The loops inside a step are bounded by constants: 3839
// bytes of a string (the copy, and the walk down the prefix chain, whose length falls by one per link), FLUSH_AT + 3854 bytes of a
// flush.
#pragma once
#include "hk_inflate_core.h"

namespace hk {
namespace lzw {

using inflate::in_ptr;
using inflate::out_ptr;
using inflate::Quad;
using inflate::uni;
using inflate::WAVE;

constexpr unsigned RING = 32768, RING_MASK = RING - 1;   // the output ring (a power of two)
constexpr unsigned MAX_STRING = 3839;                     // entry 4095's string: an entry's string is at most index - 256 bytes
constexpr unsigned HISTORY = RING - 4096;                 // how far back a string's last appearance may lie to be copied
constexpr unsigned FLUSH_AT = 8192;                       // unflushed bytes at which the ring is flushed
constexpr int WIN_WORDS = 4 * WAVE;                       // the input window: one 16-byte group per lane
constexpr unsigned TABLE = 4096, CLEAR = 256, EOI = 257, FIRST = 258, NONE = 0xFFFFFFFFu;
constexpr long long MAX_STREAM = 1ll << 28;               // bytes of a stream that are looked at (bit counts stay below 2^31)
static_assert(MAX_STRING + 1 <= 4096 && FLUSH_AT + 15 + MAX_STRING <= HISTORY, "the ring's margins");

// (HK_LZW_* of include/homonim_hk.h)
enum Status { OK = 0, TRUNCATED = 1, OLD_STYLE = 2, BAD_FIRST = 3, BAD_CODE = 4, SHORT = 5 };

struct Shared {
    alignas(16) unsigned char ring[RING];
    alignas(16) unsigned in[WIN_WORDS];
    unsigned entry[TABLE];        // prefix code | string length << 12 | first byte << 24
    unsigned pos[TABLE];          // the output position at which the string was last produced
    unsigned char last[TABLE];    // its last byte
};   // 69 KiB

// what the wave carries in scalar registers
struct State {
    in_ptr in;              // the stream, and its first byte's place in its 16-byte group
    unsigned skew;
    unsigned size;          // its bytes (at most MAX_STREAM)
    out_ptr slot;           // the block's bytes in global memory
    unsigned raw;           // how many there have to be
    unsigned long long bb;  // the bit buffer: the next `nbits` bits of the stream are its lowest, the first one highest
    unsigned nbits;
    unsigned wpos;          // the next word to enter the bit buffer (a word index from the stream's aligned-down start)
    unsigned win0;          // first word of the window in LDS (a multiple of 4); 0xFFFFFFFF: none loaded
    unsigned used, limit;   // bits consumed; 8 * size
    unsigned out, flushed;  // bytes produced / of them in the slot
    unsigned n, width;      // the next free entry; bits of the next code
    unsigned prev;          // the previous code (NONE behind a Clear), its string's length and first byte, and where it stands
    unsigned plen, pfirst, ppos;
    unsigned status;
};

// ---- input ----------------------------------------------------------------------------------------------------------------
// the 64 groups from word `w0` (a multiple of 4) on into LDS (hk_inflate_core.h load_window, over this decoder's state)
HKI_FN void load_window(Shared& S, State& s, unsigned w0) {
    HKI_SYNC();   // (the window's last readers are done)
    HKI_FOR_LANES {
        const long long gs = 4ll * w0 + 16ll * lane - (long long)s.skew;   // the group's first byte within the stream
        Quad q = {{0, 0, 0, 0}};
        if (gs >= 0 && gs + 16 <= (long long)s.size) {
            q = inflate::load_quad(s.in + gs);
        } else if (gs > -16 && gs < (long long)s.size) {
HKI_UNROLL
            for (int j = 0; j < 16; ++j)
                if (gs + j >= 0 && gs + j < (long long)s.size) q.w[j >> 2] |= (unsigned)s.in[gs + j] << (8 * (j & 3));
        }
        S.in[4 * lane + 0] = q.w[0], S.in[4 * lane + 1] = q.w[1], S.in[4 * lane + 2] = q.w[2], S.in[4 * lane + 3] = q.w[3];
    }
    HKI_SYNC();
    s.win0 = w0;
}

// the next four bytes of the stream, the first one highest
HKI_FN unsigned next_word(Shared& S, State& s) {
    const unsigned w = s.wpos++;
    if (4ull * w >= (unsigned long long)s.skew + s.size) return 0;   // past the end: zero bits, no load
    if (s.win0 == 0xFFFFFFFFu || w - s.win0 >= (unsigned)WIN_WORDS) load_window(S, s, w & ~3u);
    return __builtin_bswap32(uni(S.in[w - s.win0]));
}

// the next w <= 16 bits; a bit past the end sets TRUNCATED (the caller looks at the status before the value)
HKI_FN unsigned take(Shared& S, State& s, unsigned w) {
    if (s.nbits < w) {
        s.bb = (s.bb << 32) | next_word(S, s);
        s.nbits += 32;
    }
    s.nbits -= w, s.used += w;
    if (s.used > s.limit && !s.status) s.status = TRUNCATED;
    return (unsigned)(s.bb >> s.nbits) & ((1u << w) - 1);
}

// ---- output ---------------------------------------------------------------------------------------------------------------
// Bytes [flushed, upto) of the block from the ring to the slot, 16 per lane and store (`flushed` is a multiple of 16; a last group
// that is not whole is stored whole: the slot is the raw size rounded up to 16).
HKI_FN void flush(Shared& S, State& s, unsigned upto) {
    const unsigned n = upto - s.flushed;
    if (n == 0) return;
    HKI_SYNC();
    HKI_FOR_LANES {
        for (unsigned g = 16u * lane; g < n; g += 16u * WAVE) {   // byte g of the flush
            const unsigned* const w = reinterpret_cast<const unsigned*>(&S.ring[(s.flushed + g) & RING_MASK]);
            const Quad q = {{w[0], w[1], w[2], w[3]}};
            inflate::store_quad(s.slot + s.flushed + g, q);
        }
    }
    s.flushed = upto;
}

HKI_FN void put_byte(Shared& S, const State& s, unsigned at, unsigned v) {
    HKI_FOR_LANES {
        if (lane == 0) S.ring[at & RING_MASK] = (unsigned char)v;
    }
}

// `len` bytes to the ring at `out` from the `avail` bytes at `from` (all in front of `out`, at most HISTORY back): byte k takes
// byte k of them, and byte `avail` -- the KwKwK case, len = avail + 1 -- their first.  No read is of a byte this step writes.
HKI_FN void copy_string(Shared& S, const State& s, unsigned from, unsigned avail, unsigned len) {
    HKI_FOR_LANES {
        for (unsigned k = (unsigned)lane; k < len; k += WAVE)
            S.ring[(s.out + k) & RING_MASK] = S.ring[(from + (k == avail ? 0u : k)) & RING_MASK];
    }
}

// The first `cut` bytes of string(c), c in [258, n), of `len` bytes, to the ring at `out`.  Where its last appearance is still in
// the history all lanes copy it from there; otherwise the prefix chain is walked backwards, wave-uniformly, one last byte per
// link, until an ancestor's last appearance is in the history (copied by all lanes) or the chain ends in a byte.
HKI_FN void put_string(Shared& S, const State& s, unsigned c, unsigned len, unsigned cut) {
    unsigned cur = c, k = len;   // string(cur) is bytes [0, k) of the string
    for (;;) {
        if (cur < 256) {         // (k == 1)
            put_byte(S, s, s.out, cur);
            return;
        }
        const unsigned q = uni(S.pos[cur]);
        if (s.out - q <= HISTORY) {
            copy_string(S, s, q, k, k < cut ? k : cut);
            return;
        }
        --k;
        if (k < cut) put_byte(S, s, s.out + k, uni(S.last[cur]));
        cur = uni(S.entry[cur]) & 4095u;
    }
}

// One stream into its slot: -> the status.  `size` bytes at `in`; `raw` bytes are expected; the slot has raw rounded up to 16.
HKI_FN unsigned lzw_stream(Shared& S, in_ptr in, long long size, out_ptr slot, unsigned raw) {
    State s;
    s.in = in, s.skew = (unsigned)((uintptr_t)in & 15u);
    s.size = (unsigned)(size < 0 ? 0 : size > MAX_STREAM ? MAX_STREAM : size);
    s.slot = slot, s.raw = raw;
    s.limit = 8 * s.size, s.used = 0, s.out = 0, s.flushed = 0, s.status = OK, s.win0 = 0xFFFFFFFFu;
    s.n = FIRST, s.width = 9, s.prev = NONE, s.plen = 0, s.pfirst = 0, s.ppos = 0;
    if (s.size == 0) return TRUNCATED;
    // the bit buffer starts at the stream's first byte: the bytes of its word in front of it are left out
    s.wpos = s.skew >> 2;
    s.bb = next_word(S, s), s.nbits = 32 - 8 * (s.skew & 3);
    if (s.size >= 2) {   // libtiff's test for the pre-6.0 bit order: first byte 0, bit 0 of the second set
        if (s.nbits < 16) s.bb = (s.bb << 32) | next_word(S, s), s.nbits += 32;
        const unsigned two = (unsigned)(s.bb >> (s.nbits - 16)) & 0xFFFFu;
        if ((two >> 8) == 0 && (two & 1u)) return OLD_STYLE;
    }
    while (s.out < s.raw) {
        const unsigned c = take(S, s, s.width);
        if (s.status) return s.status;
        if (c == CLEAR) {
            s.n = FIRST, s.width = 9, s.prev = NONE;
            continue;
        }
        if (c == EOI) return SHORT;
        if (s.prev == NONE) {
            if (c > 255) return BAD_FIRST;
            put_byte(S, s, s.out, c);
            HKI_SYNC();
            s.prev = c, s.plen = 1, s.pfirst = c, s.ppos = s.out;
            s.out += 1;
        } else {
            if (c > s.n) return BAD_CODE;
            const bool kwkwk = c == s.n;   // (then n < 4096: a code has 12 bits)
            unsigned len, first;
            if (kwkwk) {
                len = s.plen + 1, first = s.pfirst;
            } else if (c < 256) {
                len = 1, first = c;
            } else {
                const unsigned e = uni(S.entry[c]);
                len = (e >> 12) & 4095u, first = e >> 24;
            }
            const unsigned room = s.raw - s.out, cut = len < room ? len : room;
            if (kwkwk) copy_string(S, s, s.out - s.plen, s.plen, cut);   // (the previous string ends at `out`)
            else if (c < 256) put_byte(S, s, s.out, c);
            else put_string(S, s, c, len, cut);
            const bool add = s.n < TABLE;
            HKI_FOR_LANES {
                if (lane == 0) {
                    if (add) {
                        S.entry[s.n] = s.prev | ((s.plen + 1) << 12) | (s.pfirst << 24);
                        S.last[s.n] = (unsigned char)first;
                        S.pos[s.n] = kwkwk ? s.out : s.ppos;   // (string(p) and the first byte of this string behind it)
                    }
                    if (!kwkwk && c >= FIRST) S.pos[c] = s.out;
                }
            }
            HKI_SYNC();
            if (add) {
                s.n += 1;
                if (s.n == (1u << s.width) - 1 && s.width < 12) s.width += 1;
            }
            s.prev = c, s.plen = len, s.pfirst = first, s.ppos = s.out;
            s.out += cut;
        }
        if (s.out - s.flushed >= FLUSH_AT) flush(S, s, s.out & ~15u);
    }
    flush(S, s, s.out);
    return OK;
}

}  // namespace lzw
}  // namespace hk
